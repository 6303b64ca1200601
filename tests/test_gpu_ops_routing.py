"""GPU: which library entry point every split-precision op of svr_amd.ops takes, call by call.

A recorder wraps the launching `svr_*` attributes of the loaded library object (monkeypatch: undone after each test)
and notes the entry point's name and what the call did with the weight: "prepare" (no data operand: planes only), "W=NULL"
(ran on prepared planes) or "W" (the weight was passed).  The expected sequences are written out below, one table per
op, from the ops' dispatch chains: whoever reorganises those chains has this file to hold the routing still.

No numbers are asserted here: the numeric gates are the kernels' own tests.  `refused` in a table row: the exact-f32 entry
point the call is routed to refuses that shape or alignment itself (the cited SVR_CHECK), so the op raises AFTER the
recorded call; the routing is what is checked.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# position of the weight pointer in the entry points that have a PREPARE / RUN form (include/svr_hip.h)
_W_ARG = {"svr_linear_fwd_f16x3": 2, "svr_linear_bwd_data_bf16x3": 2, "svr_linear_bwd_data_f16x3": 2,
          "svr_conv3d_k3_fwd_f16x3": 1, "svr_conv3d_k3_fwd_f16x3_stats": 1, "svr_conv3d_k3_bwd_data_bf16x3": 1,
          "svr_conv3d_k3_bwd_data_f16x3": 1}
# the prepared-plane kind behind each of them
_KIND = {"svr_linear_fwd_f16x3": "lf", "svr_linear_bwd_data_bf16x3": "lb", "svr_linear_bwd_data_f16x3": "lbh",
         "svr_conv3d_k3_fwd_f16x3": "cf", "svr_conv3d_k3_bwd_data_bf16x3": "cb", "svr_conv3d_k3_bwd_data_f16x3": "cbh"}


def _null(a):
    if isinstance(a, C.c_void_p):
        a = a.value
    return not a


@pytest.fixture
def calls(monkeypatch):
    """[(entry point, "prepare" | "W=NULL" | "W" | None), ...] of every launching svr_* call made during the test."""
    from svr_amd import _lib, ops
    l = _lib.lib()
    rec = []

    def wrap(name, fn):
        wi = _W_ARG.get(name)

        def recorder(*args):
            how = None
            if wi is not None:
                how = "prepare" if _null(args[0]) else ("W=NULL" if _null(args[wi]) else "W")
            rec.append((name, how))
            return fn(*args)
        return recorder

    for name in _lib.SIGNATURES:
        if name.endswith("_workspace") or name.endswith("_stats_blocks") or name in ("svr_last_error", "svr_version"):
            continue                        # host-side size queries: not part of the routing
        monkeypatch.setattr(l, name, wrap(name, getattr(l, name)))
    monkeypatch.setattr(ops, "_prepared", None)
    return rec


def _run(calls, fn, refused=False):
    del calls[:]
    if refused:
        with pytest.raises(RuntimeError, match="libsvr_hip"):
            fn()
        return None, list(calls)
    out = fn()
    return out, list(calls)


def _via(monkeypatch, ops, via, names, mode):
    """mode through the argument ("arg") or through the module globals `names` ("global")."""
    if via == "arg":
        return mode
    for n in names:
        monkeypatch.setattr(ops, n, mode)
    return None


def _dev(*shape):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(*shape, generator=g).cuda()


AMAX = ("svr_amax_f32", None)
VIA = ("arg", "global")

# ---- linear_fwd, M = 8, N = 32 ---------------------------------------------------------------------------------------
# (K, mode) -> sequence, refused by svr_linear_fwd itself (gemm.hip:379: K % 16)
LINEAR_FWD = [
    (16, "f16x3", [("svr_linear_fwd_f16x3", "W")], False),
    (16, "bf16x6", [("svr_linear_fwd_bf16x6", None)], False),
    (16, "f32", [("svr_linear_fwd", None)], False),
    (12, "f16x3", [("svr_linear_fwd", None)], True),
]


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("K,mode,want,refused", LINEAR_FWD)
def test_linear_fwd(calls, monkeypatch, via, K, mode, want, refused):
    from svr_amd import ops
    x, w, b = _dev(8, K), _dev(32, K), _dev(32)
    m = _via(monkeypatch, ops, via, ("FORWARD_GEMM",), mode)
    out, got = _run(calls, lambda: ops.linear_fwd(x, w, b, mode=m), refused)
    assert got == want
    assert refused or tuple(out.shape) == (8, 32)


# ---- linear_bwd_data, M = 8, K = 16 ----------------------------------------------------------------------------------
F16_BWD = [AMAX, ("svr_linear_bwd_data_f16x3", "W")]
F32_BWD = [("svr_linear_bwd_data", None)]
# (N, mode) -> sequence, refused by svr_linear_bwd_data itself (gemm.hip:394: N % 16)
LINEAR_BWD_DATA = [
    (32, "f16x3s", F16_BWD, False),
    (32, "bf16x3", [("svr_linear_bwd_data_bf16x3", "W")], False),
    (32, "f32", F32_BWD, False),
    (16, "f16x3s", F16_BWD, False),
    (16, "bf16x3", F32_BWD, False),
    (24, "f16x3s", F32_BWD, True),
    (24, "bf16x3", F32_BWD, True),
]


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("N,mode,want,refused", LINEAR_BWD_DATA)
def test_linear_bwd_data(calls, monkeypatch, via, masked, N, mode, want, refused):
    from svr_amd import ops
    dy, w = _dev(8, N), _dev(N, 16)
    mask = _dev(8, 16) if masked else None
    m = _via(monkeypatch, ops, via, ("BACKWARD_GEMM",), mode)
    out, got = _run(calls, lambda: ops.linear_bwd_data(dy, w, mask=mask, mode=m), refused)
    assert got == want
    assert refused or tuple(out.shape) == (8, 16)


def test_linear_bwd_data_strided_dy_f16x3s(calls):
    """dy a column slice of an (8, 33) matrix: the f16x3s chain tests the row stride and takes exact f32, which refuses it
    itself (gemm.hip:395).  (Under "bf16x3" the same dy, K % 4 != 0, and an x of row stride 18 in linear_fwd still reach the
    split kernel and are refused there: gemm_bf16x3.hip:790 / :798, gemm_f16x3.hip:345.)"""
    from svr_amd import ops
    dy, w = _dev(8, 33)[:, :32], _dev(32, 16)
    _, got = _run(calls, lambda: ops.linear_bwd_data(dy, w, mode="f16x3s"), refused=True)
    assert got == F32_BWD


# ---- linear_bwd_weight, M = 8 ----------------------------------------------------------------------------------------
# (N, K, mode) -> sequence, refused by svr_linear_bwd_weight itself (gemm.hip:414: N, K % 4)
LINEAR_BWD_WEIGHT = [
    (8, 8, "f16x3s", [AMAX, ("svr_linear_bwd_weight_f16x3", None)], False),
    (8, 8, "bf16x3", [("svr_linear_bwd_weight_bf16x3", None)], False),
    (8, 8, "f32", [("svr_linear_bwd_weight", None)], False),
    (6, 8, "f16x3s", [("svr_linear_bwd_weight", None)], True),
    (8, 6, "f16x3s", [("svr_linear_bwd_weight", None)], True),
]


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("N,K,mode,want,refused", LINEAR_BWD_WEIGHT)
def test_linear_bwd_weight(calls, monkeypatch, via, N, K, mode, want, refused):
    from svr_amd import ops
    dy, x = _dev(8, N), _dev(8, K)
    m = _via(monkeypatch, ops, via, ("BACKWARD_GEMM",), mode)
    out, got = _run(calls, lambda: ops.linear_bwd_weight(dy, x, mode=m), refused)
    assert got == want
    assert refused or (tuple(out[0].shape) == (N, K) and tuple(out[1].shape) == (N,))


# ---- conv3d_k3_fwd, B = 1, 4^3 ---------------------------------------------------------------------------------------
PACK_K3 = [("svr_conv3d_pack_weight", None), ("svr_conv3d_k3", None)]
# (Ci, mode, want_stats) -> sequence, refused by svr_conv3d_k3 itself (conv3d.hip:886: Ci % 16)
CONV_FWD = [
    (16, "f16x3", False, [("svr_conv3d_k3_fwd_f16x3", "W")], False),
    (16, "f16x3", True, [("svr_conv3d_k3_fwd_f16x3_stats", "W")], False),
    (16, "bf16x6", False, [("svr_conv3d_k3_fwd_bf16x6", None)], False),
    (16, "f32", False, PACK_K3, False),
    (16, "f32", True, PACK_K3, False),
    (2, "f16x3", False, PACK_K3, True),
    (2, "f16x3", True, PACK_K3, True),
    # Ci = 1: the f16x3 kernel does not take it (conv3d_bf16.hip:925), svr_conv3d_k3 does (conv3d.hip:863-870)
    (1, "f16x3", False, PACK_K3, False),
    (1, "f16x3", True, PACK_K3, False),
]


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("Ci,mode,want_stats,want,refused", CONV_FWD)
def test_conv3d_k3_fwd(calls, monkeypatch, via, Ci, mode, want_stats, want, refused):
    from svr_amd import ops
    x, w, b = _dev(1, 4, 4, 4, Ci), _dev(16, Ci, 3, 3, 3), _dev(16)
    m = _via(monkeypatch, ops, via, ("FORWARD_CONV",), mode)
    out, got = _run(calls, lambda: ops.conv3d_k3_fwd(x, w, b, mode=m, want_stats=want_stats), refused)
    assert got == want
    if refused:
        return
    if want_stats:          # statistics only where the f16x3 kernel ran: every other path hands back (out, None)
        out, stats = out
        assert (stats is not None) == (want[-1][0] == "svr_conv3d_k3_fwd_f16x3_stats")
    assert tuple(out.shape) == (1, 4, 4, 4, 16)


# ---- conv3d_k3_bwd_data ----------------------------------------------------------------------------------------------
# (Co, mode) -> sequence (Ci = 2), refused by svr_conv3d_k3 itself (conv3d.hip:886: its input channels, Co here, % 16)
CONV_BWD_DATA = [
    (16, "f16x3s", [AMAX, ("svr_conv3d_k3_bwd_data_f16x3", "W")], False),
    (16, "bf16x3", [("svr_conv3d_k3_bwd_data_bf16x3", "W")], False),
    (8, "f16x3s", PACK_K3, True),
    (8, "bf16x3", PACK_K3, True),
]


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("Co,mode,want,refused", CONV_BWD_DATA)
def test_conv3d_k3_bwd_data(calls, monkeypatch, via, masked, Co, mode, want, refused):
    from svr_amd import ops
    dout, w = _dev(1, 4, 4, 4, Co), _dev(Co, 2, 3, 3, 3)
    mask = _dev(1, 4, 4, 4, 2) if masked else None
    m = _via(monkeypatch, ops, via, ("BACKWARD_CONV",), mode)
    out, got = _run(calls, lambda: ops.conv3d_k3_bwd_data(dout, w, mask=mask, mode=m), refused)
    assert got == want
    assert refused or tuple(out.shape) == (1, 4, 4, 4, 2)


# ---- conv3d_k3_bwd_weight, Co = 16 -----------------------------------------------------------------------------------
F32_WGRAD = ("svr_conv3d_k3_bwd_weight", None)
UNPACK = ("svr_conv3d_unpack_wgrad", None)
# (Ci, mode, param_layout) -> sequence, refused by svr_conv3d_k3_bwd_weight itself (conv3d.hip:953: Ci % 4; the unpack
# behind it is then never reached)
CONV_BWD_WEIGHT = [
    (4, "f16x3s", False, [AMAX, ("svr_conv3d_k3_bwd_weight_f16x3", None)], False),
    (4, "f16x3s", True, [AMAX, ("svr_conv3d_k3_bwd_weight_f16x3", None)], False),
    (4, "bf16x3", False, [("svr_conv3d_k3_bwd_weight_bf16x3", None)], False),
    (4, "bf16x3", True, [("svr_conv3d_k3_bwd_weight_bf16x3_param", None)], False),
    (4, "f32", False, [F32_WGRAD], False),
    (4, "f32", True, [F32_WGRAD, UNPACK], False),
    (2, "f16x3s", False, [F32_WGRAD], True),
    (2, "f16x3s", True, [F32_WGRAD], True),
    (2, "bf16x3", False, [F32_WGRAD], True),
    (2, "bf16x3", True, [F32_WGRAD], True),
    (2, "f32", False, [F32_WGRAD], True),
    (2, "f32", True, [F32_WGRAD], True),
    # Ci = 1: no split kernel takes it (conv3d_bwdw_bf16.hip:652), svr_conv3d_k3_bwd_weight does (conv3d.hip:928-951)
    (1, "f16x3s", False, [F32_WGRAD], False),
    (1, "f16x3s", True, [F32_WGRAD, UNPACK], False),
    (1, "bf16x3", True, [F32_WGRAD, UNPACK], False),
]


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("Ci,mode,param_layout,want,refused", CONV_BWD_WEIGHT)
def test_conv3d_k3_bwd_weight(calls, monkeypatch, via, Ci, mode, param_layout, want, refused):
    from svr_amd import ops
    x, dout = _dev(1, 4, 4, 4, Ci), _dev(1, 4, 4, 4, 16)
    m = _via(monkeypatch, ops, via, ("BACKWARD_CONV_WEIGHT",), mode)
    out, got = _run(calls, lambda: ops.conv3d_k3_bwd_weight(x, dout, mode=m, param_layout=param_layout), refused)
    assert got == want
    assert refused or (tuple(out[0].shape) == ((16, Ci, 3, 3, 3) if param_layout else (27, Ci, 16)) and tuple(out[1].shape) == (16,))


# ---- prepared planes -------------------------------------------------------------------------------------------------
# backward mode -> the prepare launches of add_linear(32 x 32) + add_conv(16 -> 16), in order, and the kinds they leave
PREPARED = {
    "f16x3s": ([("svr_linear_fwd_f16x3", "prepare"), ("svr_linear_bwd_data_f16x3", "prepare"),
                ("svr_conv3d_k3_fwd_f16x3", "prepare"), ("svr_conv3d_k3_bwd_data_f16x3", "prepare")], {"lf", "lbh", "cf", "cbh"}),
    "bf16x3": ([("svr_linear_fwd_f16x3", "prepare"), ("svr_linear_bwd_data_bf16x3", "prepare"),
                ("svr_conv3d_k3_fwd_f16x3", "prepare"), ("svr_conv3d_k3_bwd_data_bf16x3", "prepare")], {"lf", "lb", "cf", "cb"}),
    "f32": ([("svr_linear_fwd_f16x3", "prepare"), ("svr_conv3d_k3_fwd_f16x3", "prepare")], {"lf", "cf"}),
}


def _backward(monkeypatch, ops, mode):
    for n in ("BACKWARD_GEMM", "BACKWARD_CONV", "BACKWARD_CONV_WEIGHT"):
        monkeypatch.setattr(ops, n, mode)
    assert ops.FORWARD_GEMM == "f16x3" and ops.FORWARD_CONV == "f16x3"


@pytest.mark.parametrize("bwd", sorted(PREPARED))
def test_prepared_kinds_are_the_ops_null_weight_calls(calls, monkeypatch, bwd):
    from svr_amd import ops
    _backward(monkeypatch, ops, bwd)
    launches, kinds = PREPARED[bwd]
    wl, wc = _dev(32, 32), _dev(16, 16, 3, 3, 3)
    p = ops.PreparedWeights()
    p.begin()
    del calls[:]
    p.add_linear(wl)
    p.add_conv(wc)
    assert list(calls) == launches
    p.finish(torch.cuda.current_stream())
    assert {k for k, _ in p._valid} == kinds
    monkeypatch.setattr(ops, "_prepared", p)
    del calls[:]
    ops.linear_fwd(_dev(8, 32), wl, _dev(32))
    ops.linear_bwd_data(_dev(8, 32), wl)
    ops.conv3d_k3_fwd(_dev(1, 4, 4, 4, 16), wc, _dev(16))
    ops.conv3d_k3_bwd_data(_dev(1, 4, 4, 4, 16), wc)
    assert {_KIND[n] for n, how in calls if how == "W=NULL"} == kinds
    assert not [n for n, how in calls if how == "prepare"]
    p.invalidate()


@pytest.mark.parametrize("bwd", sorted(PREPARED))
def test_refused_weights_make_no_prepare_launch(calls, monkeypatch, bwd):
    """(24, 12): K % 16, N % 16 and N % 32 all fail; 3 -> 8 channels: Ci % 16, Ci % 2 and Co % 16 all fail."""
    from svr_amd import ops
    _backward(monkeypatch, ops, bwd)
    p = ops.PreparedWeights()
    p.begin()
    del calls[:]
    p.add_linear(_dev(24, 12))
    p.add_conv(_dev(8, 3, 3, 3, 3))
    assert list(calls) == [] and not p._valid
