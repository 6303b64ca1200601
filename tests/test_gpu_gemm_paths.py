"""Every branch the linear launchers of csrc/gemm.hip, gemm_f16x3.hip, gemm_bf16x3.hip and gemm_bf16x6.hip can take, and the tile
edges of their kernels, against an f64 reference: the two-wave 128 x 64 forward tile, the float4 and the per-lane epilogue at
partial column tiles, one and an odd number of k-steps, the forward kernel reused for the data gradient, linear_nn_x3_kernel on
column slices, both weight-gradient paths of bf16x3 (transposing LDS reads, and the dY pre-pass for an X that is not float4-able),
1 / 2 / 35 reduction splits, both column-sum kernels, fc_out's two backward kernels and the BCE loss past one grid of blocks.
Each case first ASSERTS, through ops.linear_variant (svr_linear_variant: the function the launchers call), that it runs the
kernel it is named for (tests/_gemm_cases.py; the CPU test test_linear_variant_table_and_every_launcher_branch_is_reached checks
that the cases reach every variant).  Where the query reports a refusal the op must raise.

Inputs are seeded from the case name: x is a ReLU output (exact zeros for the mask), w is scaled 1 / sqrt(K), dy is gradient-like
(magnitude 1 or 1e-6, rows spread over e^(+-3 sigma): f16 would overflow or flush without the kernels' scale).  Operands that the
table places in a wider buffer are surrounded by NaN (inputs) or by a sentinel (outputs): rows >= M and columns outside the slice
must hold the sentinel bit for bit afterwards.  The reference is an f64 product with stock torch ops on the device, computed once
per case and shared by the modes.  Errors are tests._golden.rel_err (max |a - b| / max |b|), evaluated on the device.  Gates
(those of test_linear_fwd_bwd, test_linear_backward_at_f32_level_f16x3s and test_fc_out_and_bce in tests/test_gpu_kernels.py):
2e-6 for f32 / f16x3 / bf16x6 / f16x3s, f16x3s also <= 3 x the exact-f32 kernel's error on the same operands + 1e-7, 5e-5 for
bf16x3, 2e-6 for db, 1e-6 for fc_out, 1e-5 for the BCE loss and gradient.

Wall time of the file on one MI355X: 4 s for its 90 tests (the first one pays 0.8 s for loading the library; every other test
stays under 0.1 s).  Measured errors per variant: DESIGN.md section 4."""
import ctypes as C
import functools
import os
import sys
import zlib

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _gemm_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu

GATE = {"f32": 2e-6, "f16x3": 2e-6, "bf16x6": 2e-6, "f16x3s": 2e-6, "bf16x3": 5e-5}      # by the arithmetic of the entry point reached
SENT = -123456.75      # what every output buffer holds before the call
EXTRA_ROWS = 3         # rows of every buffer below the operand


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _rel_err(a, ref):
    """tests._golden.rel_err on the device: max |a - ref| / max |ref|, in f64"""
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _seed(name):
    return zlib.crc32(name.encode())


def _place(t, rows, cols, lay, fill):
    """(buffer, view): a (rows + EXTRA_ROWS, ld) buffer of `fill` and its [:rows, col0:col0 + cols] view, holding t (if given)"""
    ld, col0 = lay if lay is not None else (cols, 0)
    buf = torch.full((rows + EXTRA_ROWS, ld), fill, device="cuda", dtype=torch.float32)
    view = buf[:rows, col0:col0 + cols]
    if t is not None:
        view.copy_(t)
    return buf, view


def _untouched(buf, view):
    """every element of buf outside view still holds the sentinel, bit for bit"""
    own = torch.zeros_like(buf, dtype=torch.bool)
    own[:view.shape[0], view.storage_offset() % buf.stride(0):view.storage_offset() % buf.stride(0) + view.shape[1]] = True
    return bool((buf[~own].view(torch.int32) == torch.tensor(SENT).view(torch.int32).item()).all())


@functools.lru_cache(maxsize=None)
def _data(name):
    """the case's operands (made once, never modified) and its f64 references"""
    _, kind, M, N, K, _, opt, _ = GC.by_name(name)
    g = torch.Generator().manual_seed(_seed(name))
    x = torch.randn(M, K, generator=g).relu_().cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    dy = (torch.randn(M, N, generator=g) * opt.get("gscale", 1.0) * torch.exp(3 * torch.randn(M, 1, generator=g))).cuda()
    d = {"x": x, "w": w, "b": b, "dy": dy}
    if kind == "fwd":
        d["z"] = x.double() @ w.double().t()
    elif kind == "bwd_data":
        d["mask"] = -x if opt.get("zero_mask") else x      # (zero_mask: <= 0 everywhere, exact zeros and negative values)
        d["dx"] = dy.double() @ w.double()
    else:
        d["dw"] = dy.double().t() @ x.double()
        d["db"] = dy.double().sum(0)
    return d


def _operands(case, contiguous=False, pad_k=0):
    """{"a", "b", "mask"}: the input operands of the case in the layouts of the table (NaN around them), or contiguous; pad_k:
    w and the mask widened by zero columns (the exact-f32 kernel on a K it refuses)"""
    name, kind, M, N, K, lays, _, _ = case
    d = _data(name)
    lay = (lambda o: None) if contiguous else lays.get
    nan = float("nan")
    if kind == "fwd":
        return {"a": _place(d["x"], M, K, lay("a"), nan)[1], "b": _place(d["w"], N, K, lay("b"), nan)[1]}
    if kind == "bwd_data":
        w, mask = d["w"], d["mask"]
        if pad_k:
            w, mask = torch.nn.functional.pad(w, (0, pad_k)), torch.nn.functional.pad(mask, (0, pad_k))
        return {"a": _place(d["dy"], M, N, lay("a"), nan)[1], "b": _place(w, N, K + pad_k, lay("b"), nan)[1],
                "mask": _place(mask, M, K + pad_k, lay("mask"), nan)[1]}
    return {"a": _place(d["dy"], M, N, lay("a"), nan)[1], "b": _place(d["x"], M, K, lay("b"), nan)[1]}


def _check_layouts(ops, case, t, out=None):
    """the tensors really have the (leading dimension, address bits) the table -- and so the CPU reach test -- assumes"""
    _, kind, M, N, K, _, _, _ = case
    cols = {"fwd": (K, K, N, None), "bwd_data": (N, K, K, K), "bwd_weight": (N, K, K, None)}[kind]
    for o, c, ten in zip(("a", "b", "out", "mask"), cols, (t["a"], t["b"], out, t.get("mask"))):
        if ten is not None:
            assert ops.operand_layout(ten) == GC.layout(case, o, c), (case[0], o)


# ---- forward ----------------------------------------------------------------------------------------------------------------
EPILOGUES = ("bias_relu", "bias", "none")


def _ref_fwd(d, epi):
    z = d["z"] if epi == "none" else d["z"] + d["b"].double()
    return z.relu() if epi == "bias_relu" else z


def _run_fwd(ops, case, mode, epi, contiguous=False):
    name, _, M, N, K, lays, _, _ = case
    t = _operands(case, contiguous)
    buf, out = _place(None, M, N, None if contiguous else lays.get("out"), SENT)
    if not contiguous:
        _check_layouts(ops, case, t, out)
    y = ops.linear_fwd(t["a"], t["b"], None if epi == "none" else _data(name)["b"], relu=epi == "bias_relu", out=out, mode=mode)
    assert y is out and _untouched(buf, out), (name, mode, epi, "wrote outside its rows / columns")
    return out


@functools.lru_cache(maxsize=None)
def _f32_err_fwd(name, epi):
    return _rel_err(_run_fwd(_ops(), GC.by_name(name), "f32", epi), _ref_fwd(_data(name), epi))


@pytest.mark.parametrize("mode", GC.FWD_MODES)
@pytest.mark.parametrize("name", [c[0] for c in GC.CASES if c[1] == "fwd"])
def test_forward(name, mode):
    ops = _ops()
    case = GC.by_name(name)
    v = GC.query(ops, case, mode)
    assert GC.tag("fwd", v) == case[7][mode], (name, mode, v)
    for epi in EPILOGUES:
        if v["status"] != 0:
            with pytest.raises(RuntimeError):
                _run_fwd(ops, case, mode, epi)
            continue
        y = _run_fwd(ops, case, mode, epi)
        err, e32 = _rel_err(y, _ref_fwd(_data(name), epi)), _f32_err_fwd(name, epi)
        print(f"GEMM fwd {name} {mode} {epi} {v['kernel']}/{'coal' if v['coalesced'] else 'lane'} err={err:.2e} f32={e32:.2e}")
        assert err < GATE[v["op"].split("_")[-1]], (name, mode, epi, err)
        vc = GC.query(ops, case, mode, contiguous=True)
        if case[5] and (vc["kernel"], vc["coalesced"]) == (v["kernel"], v["coalesced"]):      # same kernel and epilogue: same bits
            assert torch.equal(_run_fwd(ops, case, mode, epi, contiguous=True), y), (name, mode, epi)


# ---- backward-data ----------------------------------------------------------------------------------------------------------
def _ref_bwd_data(d, masked):
    return d["dx"] * (d["mask"] > 0) if masked else d["dx"]


def _run_bwd_data(ops, case, mode, masked, contiguous=False, pad_k=0):
    name, _, M, N, K, lays, _, _ = case
    t = _operands(case, contiguous, pad_k)
    buf, out = _place(None, M, K + pad_k, None if contiguous else lays.get("out"), SENT)
    if not contiguous and not pad_k:
        _check_layouts(ops, case, t, out)
    dx = ops.linear_bwd_data(t["a"], t["b"], mask=t["mask"] if masked else None, out=out, mode=mode)
    assert dx is out and _untouched(buf, out), (name, mode, masked, "wrote outside its rows / columns")
    return out


@functools.lru_cache(maxsize=None)
def _f32_err_bwd_data(name, masked):
    """the exact-f32 kernel's own error on the case's operands (a K it refuses: on w and the mask widened by zero columns)"""
    ops, case = _ops(), GC.by_name(name)
    K = case[4]
    if GC.query(ops, case, "f32", masked=masked)["status"] == 0:
        dx = _run_bwd_data(ops, case, "f32", masked)
    else:
        dx = _run_bwd_data(ops, case, "f32", masked, contiguous=True, pad_k=-K % 4)[:, :K]
    return _rel_err(dx, _ref_bwd_data(_data(name), masked))


@pytest.mark.parametrize("mode", GC.BWD_MODES)
@pytest.mark.parametrize("name", [c[0] for c in GC.CASES if c[1] == "bwd_data"])
def test_backward_data(name, mode):
    ops = _ops()
    case = GC.by_name(name)
    assert GC.tag("bwd_data", GC.query(ops, case, mode)) == case[7][mode], (name, mode)
    for masked in (True, False):
        v = GC.query(ops, case, mode, masked=masked)
        if v["status"] != 0:
            with pytest.raises(RuntimeError):
                _run_bwd_data(ops, case, mode, masked)
            continue
        dx = _run_bwd_data(ops, case, mode, masked)
        arith = v["op"].split("_")[-1]
        if arith == "f16x3s":      # the |max| the kernel leaves for the next layer's scale is the tensor's, exactly
            assert float(dx._svr_amax.view(torch.float32)) == float(dx.abs().max()), (name, mode, masked, v["kernel"])
        if masked and case[6].get("zero_mask"):
            assert not dx.any(), (name, mode)
            if arith == "f16x3s":
                assert int(dx._svr_amax) == 0
            continue
        err, e32 = _rel_err(dx, _ref_bwd_data(_data(name), masked)), _f32_err_bwd_data(name, masked)
        print(f"GEMM bwd_data {name} {mode} {'mask' if masked else 'nomask'} {v['kernel']}/{'coal' if v['coalesced'] else 'lane'} "
              f"err={err:.2e} f32={e32:.2e}")
        assert err < GATE[arith], (name, mode, masked, err)
        if arith == "f16x3s":
            assert err <= 3 * e32 + 1e-7, (name, masked, err, e32)
        vc = GC.query(ops, case, mode, masked=masked, contiguous=True)
        if case[5] and vc["status"] == 0 and (vc["op"], vc["kernel"], vc["coalesced"]) == (v["op"], v["kernel"], v["coalesced"]):
            assert torch.equal(_run_bwd_data(ops, case, mode, masked, contiguous=True), dx), (name, mode, masked)


# ---- backward-weight --------------------------------------------------------------------------------------------------------
def _run_bwd_weight(ops, case, mode, want_bias, contiguous=False):
    t = _operands(case, contiguous)
    if not contiguous:
        _check_layouts(ops, case, t)
    return ops.linear_bwd_weight(t["a"], t["b"], want_bias=want_bias, mode=mode)


@functools.lru_cache(maxsize=None)
def _f32_err_bwd_weight(name):
    ops, case = _ops(), GC.by_name(name)
    if GC.query(ops, case, "f32")["status"] != 0:
        return None
    return _rel_err(_run_bwd_weight(ops, case, "f32", False)[0], _data(name)["dw"])


@pytest.mark.parametrize("name,mode", [(c[0], m) for c in GC.CASES if c[1] == "bwd_weight" for m in GC.modes(c)])
def test_backward_weight(name, mode):
    """w_1x4x4 is what moved the 2^-11 of linear_tn_x3_tr_kernel's f16 split from hi(x) to lo'(dY): with ONE row every element of
    dW is a single product, x = 0.087 made hi(x) 2^-11 a subnormal f16, and the case measured 2.28e-7 against 1.44e-8 for the
    exact-f32 kernel on the same operands -- over 3 x 1.44e-8 + 1e-7.  dY is scaled into [2^13, 2^14), so its halves stay normal."""
    ops = _ops()
    case = GC.by_name(name)
    d = _data(name)
    biases = case[6].get("bias", (True, False))
    assert GC.tag("bwd_weight", GC.query(ops, case, mode, want_bias=biases[0])) == case[7][mode], (name, mode)
    for want_bias in biases:
        v = GC.query(ops, case, mode, want_bias=want_bias)
        if v["status"] != 0:
            with pytest.raises(RuntimeError):
                _run_bwd_weight(ops, case, mode, want_bias)
            continue
        dw, db = _run_bwd_weight(ops, case, mode, want_bias)
        dw2, db2 = _run_bwd_weight(ops, case, mode, want_bias)
        assert torch.equal(dw, dw2), (name, mode, "the slabs are summed in a fixed order")
        arith = v["op"].split("_")[-1]
        err, e32 = _rel_err(dw, d["dw"]), _f32_err_bwd_weight(name)
        print(f"GEMM bwd_weight {name} {mode} {v['kernel']}/{v['bias']} splits={v['splits']} err={err:.2e} "
              f"f32={'-' if e32 is None else format(e32, '.2e')}" + (f" db={_rel_err(db, d['db']):.2e}" if want_bias else ""))
        assert err < GATE[arith], (name, mode, want_bias, err)
        if arith == "f16x3s":
            assert err <= 3 * e32 + 1e-7, (name, err, e32)
        if want_bias:
            assert torch.equal(db, db2) and _rel_err(db, d["db"]) < 2e-6, (name, mode, _rel_err(db, d["db"]))
        else:
            assert db is None
        vc = GC.query(ops, case, mode, want_bias=want_bias, contiguous=True)
        if case[5] and (vc["op"], vc["kernel"]) == (v["op"], v["kernel"]):
            dwc, dbc = _run_bwd_weight(ops, case, mode, want_bias, contiguous=True)
            assert torch.equal(dwc, dw) and (not want_bias or torch.equal(dbc, db)), (name, mode)


@pytest.mark.parametrize("mode", GC.BWD_MODES)
def test_backward_weight_into_a_wider_dw(mode):
    """lddw > K (the entry points take it, ops always passes a contiguous dW): the reduce kernels write N rows of K columns at
    a stride of lddw -- the same bits as into a contiguous dW, the sentinel everywhere else."""
    ops = _ops()
    from svr_amd import _lib
    l = _lib.lib()
    case = GC.by_name("w_33x8x36")
    _, _, M, N, K, _, _, _ = case
    t = _operands(case)
    dy, x = t["a"], t["b"]
    dw_ref, db_ref = ops.linear_bwd_weight(dy, x, mode=mode)
    buf, dw = _place(None, N, K, (K + 4, 0), SENT)
    db = torch.empty(N, device="cuda")
    p = lambda ten: C.c_void_p(ten.data_ptr())      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if mode == "f32":
        ws = torch.empty(l.svr_linear_bwd_weight_workspace(M, N, K), device="cuda", dtype=torch.uint8)
        rc = l.svr_linear_bwd_weight(p(dy), N, p(x), K, p(dw), K + 4, p(db), M, N, K, p(ws), s)
    elif mode == "bf16x3":
        ws = torch.empty(l.svr_linear_bwd_weight_bf16x3_workspace(M, N, K), device="cuda", dtype=torch.uint8)
        rc = l.svr_linear_bwd_weight_bf16x3(p(dy), N, p(x), K, p(dw), K + 4, p(db), M, N, K, p(ws), s)
    else:
        ws = torch.empty(l.svr_linear_bwd_weight_f16x3_workspace(M, N, K), device="cuda", dtype=torch.uint8)
        rc = l.svr_linear_bwd_weight_f16x3(p(dy), N, p(x), K, p(dw), K + 4, p(db), M, N, K, p(ops.amax_of(dy)), p(ws), s)
    assert rc == 0
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref) and _untouched(buf, dw)


# ---- fc_out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_map", (False, True))
@pytest.mark.parametrize("K,M", [(64, 1), (64, 513), (64, 700), (256, 1), (256, 511)])
def test_fc_out(K, M, with_map, monkeypatch):
    """fc_out_bwd_kernel (K != 256) and fc_out_bwd_k256_kernel at one row, a partial block and a second block of one / 188 rows.
    db is ONE number, the plain sum of dlogits, and max |a - b| / max |b| of one number is its relative error: dlogits has a mean
    of 0.5 so that the sum is well conditioned (sum |g| / |sum g| ~ 1.6) -- with a zero mean the reference itself can land
    anywhere near 0 and the gate would measure the seed.  (The workgroups' partial sums are stored as f32: 2^-24 of their
    magnitude is the floor.)"""
    ops = _ops()
    monkeypatch.setattr(ops, "BACKWARD_GEMM", "f16x3s")      # fc_out_bwd then leaves |max| of dH on the tensor
    g = torch.Generator().manual_seed(_seed(f"fc_out_{K}_{M}_{with_map}"))
    h = torch.randn(M, K, generator=g).relu_().cuda()
    w = (torch.randn(K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(1, generator=g).cuda()
    dz = (0.5 + torch.randn(M, generator=g)).cuda()
    perm = torch.randperm(M, generator=g).to(torch.int32).cuda() if with_map else None
    z_ref = h.double() @ w.double() + b.double()
    gm = dz.double()
    if with_map:      # logits / dlogits live in the caller's order: row m is element perm[m]
        z_ref = torch.empty_like(z_ref).scatter_(0, perm.long(), z_ref)
        gm = gm[perm.long()]
    z = ops.fc_out_fwd(h, w, b, perm)
    dh, dw, db = ops.fc_out_bwd(h, w, dz, perm)
    errs = {"logits": _rel_err(z, z_ref), "dH": _rel_err(dh, gm[:, None] * w.double()[None, :] * (h > 0)),
            "dw": _rel_err(dw, gm @ h.double()), "db": _rel_err(db, gm.sum().reshape(1))}
    print(f"GEMM fc_out K={K} M={M} map={with_map} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(e < 1e-6 for e in errs.values()), errs
    assert float(dh._svr_amax.view(torch.float32)) == float(dh.abs().max())


# ---- BCE with logits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", (False, True))
@pytest.mark.parametrize("B,N", [(2, 16500), (3, 1)])
def test_bce(B, N, ordered):
    """N > 64 x 256: every block walks more than one grid stride; gscale != 1; want_grad=False; saturated logits (+-100, with
    both targets) in the large shape.  The three logits of (3, 1) are not saturated: sigmoid(z) - t in f32 is exact to 2^-24 of
    ONE, not of the difference, so a tensor whose every |sigmoid(z) - t| is below 2^-24 / 1e-5 = 6e-3 has no value the 1e-5
    gate (relative to the largest gradient) could be held against -- +-100 in two of three slots left exactly that."""
    ops = _ops()
    g = torch.Generator().manual_seed(_seed(f"bce_{B}_{N}"))
    z = (3 * torch.randn(B, N, generator=g)).cuda()
    if N > 4:
        z[0, 0], z[B - 1, N - 1], z[1, 3], z[0, N - 2] = 100.0, -100.0, -100.0, 100.0
    t = (torch.rand(B, N, generator=g) < 0.5).float().cuda()
    if N > 4:
        t[0, 0], t[B - 1, N - 1], t[1, 3], t[0, N - 2] = 0.0, 1.0, 0.0, 1.0      # a loss of 100 twice, of e^-100 twice
    zd, td = z.double(), t.double()
    ref = (zd.clamp_min(0) - zd * td + torch.log1p(torch.exp(-zd.abs()))).sum(1).mean()      # the softplus form, f64
    gref = (torch.sigmoid(zd) - td) * 0.25 / B
    loss, dz = ops.bce_logits_sum_mean(z, t, gscale=0.25, ordered=ordered)
    loss2, none = ops.bce_logits_sum_mean(z, t, want_grad=False, gscale=0.25, ordered=ordered)
    print(f"GEMM bce B={B} N={N} ordered={ordered} loss={abs(loss.item() - ref.item()) / abs(ref.item()):.2e} grad={_rel_err(dz, gref):.2e}")
    assert none is None and torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    assert torch.isfinite(loss).all() and abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert _rel_err(dz, gref) < 1e-5
