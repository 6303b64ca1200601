"""GPU: the fused point-MLP tail (csrc/mlp_tail.hip: fc_1 + ReLU, fc_2 + ReLU, fc_out in one kernel) against the three ops it
replaces -- EXACT equality, because the kernel issues linear_nt_h3_kernel's accumulation sequence on the same operands and
fc_out_fwd_kernel's sum in the same order.  One differing bit means the sequence is not that one.

Shapes: hidden 256; M in {1, 63, 64, 65, 130, 1000} for the kernel's 64-row tile (one partial tile, an exact tile, one row
over, several tiles with a partial last one).  Inputs: h0 a ReLU output (half zeros, all-zero rows, one row with entries near
6e4 -- inside the f16 split's |x| < 65504 domain; few enough of them that h1 stays inside it too), contiguous and as the left
256 columns of a 320-wide buffer; weights 1/sqrt(256)-scaled normals, one case with a zero column in W2, one with biases that
drive a whole column negative; row_map None and a permutation; planes prepared ahead and in the call.  Outputs start as NaN,
the rows behind M and 4096 guard bytes behind every output and the workspace carry a pattern that has to survive."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 256
GUARD, PATTERN, NAN_BYTE = 4096, 0xA5, 0xFF       # four 0xFF bytes are a float32 NaN
SPARE_ROWS = 3                                     # rows behind M in h1 / h2 that must stay untouched
MS = (1, 63, 64, 65, 130, 1000)
CASES = ("plain", "zero_column", "negative_column")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@functools.lru_cache(maxsize=None)
def _case(M, case):
    """Inputs and the three-op reference of one (M, case), made once: (h0, w1, b1, w2, b2, wo, bo, perm, h1, h2, logits, logits_perm)."""
    from svr_amd import ops
    g = torch.Generator().manual_seed(1000 * M + CASES.index(case))
    h0 = torch.relu(torch.randn(M, H, generator=g))
    h0[torch.arange(M) % 7 == 3] = 0.0                                  # all-zero rows
    big = M // 2
    h0[big, :8] = 5.5e4 + 9.0e3 * torch.rand(8, generator=g)           # near the top of the f16 range: up to 6.4e4
    w1, w2 = torch.randn(H, H, generator=g) / 16.0, torch.randn(H, H, generator=g) / 16.0
    b1, b2 = 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    wo, bo = torch.randn(H, generator=g) / 16.0, torch.randn(1, generator=g)
    if case == "zero_column":
        w2[:, 5] = 0.0
    if case == "negative_column":
        b1[7] = -1.0e6
        b2[9] = -1.0e6
    perm = torch.randperm(M, generator=g).to(torch.int32)
    dev = [t.cuda() for t in (h0, w1, b1, w2, b2, wo, bo, perm)]
    h0, w1, b1, w2, b2, wo, bo, perm = dev
    h1 = ops.linear_fwd(h0, w1, b1, relu=True)
    h2 = ops.linear_fwd(h1, w2, b2, relu=True)
    ref = (h1, h2, ops.fc_out_fwd(h2, wo, bo), ops.fc_out_fwd(h2, wo, bo, perm))
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    if case == "negative_column":
        assert float(h1[:, 7].max()) == 0.0 and float(h2[:, 9].max()) == 0.0
    return tuple(dev) + ref


def _guarded(nbytes, spare=0):
    """nbytes of NaN, then `spare` + GUARD pattern bytes"""
    buf = torch.empty(nbytes + spare + GUARD, dtype=torch.uint8, device="cuda")
    buf[:nbytes] = NAN_BYTE
    buf[nbytes:] = PATTERN
    return buf


def _tail_intact(buf, nbytes):
    return bool((buf[nbytes:] == PATTERN).all())


def _fused(M, case, wide, use_map, prepared):
    """One run of svr_mlp_tail_fwd on guarded buffers -> (h1, h2, logits); asserts that nothing outside the outputs was written."""
    from svr_amd import _lib
    l = _lib.lib()
    h0, w1, b1, w2, b2, wo, bo, perm = _case(M, case)[:8]
    if wide:
        buf = torch.full((M, 320), float("nan"), device="cuda")
        buf[:, :H] = h0
        h0 = buf[:, :H]
    row_bytes = H * 4
    h1b, h2b = _guarded(M * row_bytes, SPARE_ROWS * row_bytes), _guarded(M * row_bytes, SPARE_ROWS * row_bytes)
    zb = _guarded(M * 4)
    wsn = l.svr_mlp_tail_fwd_workspace(H)
    ws = _guarded(wsn)
    z = C.c_void_p(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rm = perm if use_map else None
    if prepared:
        assert l.svr_mlp_tail_fwd(z, 0, _p(w1), z, _p(w2), z, z, z, z, 0, z, 0, z, z, 0, H, _p(ws), s) == 0
        wp1, wp2 = z, z
    else:
        wp1, wp2 = _p(w1), _p(w2)
    rc = l.svr_mlp_tail_fwd(_p(h0), h0.stride(0), wp1, _p(b1), wp2, _p(b2), _p(wo), _p(bo), _p(h1b), H, _p(h2b), H, _p(zb), _p(rm), M, H,
                            _p(ws), s)
    assert rc == 0, l.svr_last_error()
    torch.cuda.synchronize()
    assert _tail_intact(h1b, M * row_bytes) and _tail_intact(h2b, M * row_bytes), "rows behind M or the guard were written"
    assert _tail_intact(zb, M * 4) and _tail_intact(ws, wsn), "guard behind the logits or the workspace was written"
    f = lambda b, n: b[:n].view(torch.float32)      # noqa: E731
    return f(h1b, M * row_bytes).view(M, H), f(h2b, M * row_bytes).view(M, H), f(zb, M * 4)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("M", MS)
def test_fused_tail_returns_the_bits_of_the_three_ops(M, case):
    ref_h1, ref_h2, ref_z, ref_zp = _case(M, case)[8:]
    for wide in (False, True):
        for use_map in (False, True):
            for prepared in (True, False):
                h1, h2, z = _fused(M, case, wide, use_map, prepared)
                tag = f"M={M} {case} wide={wide} row_map={use_map} prepared={prepared}"
                assert not bool(torch.isnan(h1).any() | torch.isnan(h2).any() | torch.isnan(z).any()), tag + ": an element was not written"
                assert torch.equal(h1, ref_h1), f"{tag}: h1 differs in {int((h1 != ref_h1).sum())} elements"
                assert torch.equal(h2, ref_h2), f"{tag}: h2 differs in {int((h2 != ref_h2).sum())} elements"
                want = ref_zp if use_map else ref_z
                assert torch.equal(z, want), f"{tag}: logits differ in {int((z != want).sum())} rows, max {float((z - want).abs().max()):.3e}"


@pytest.fixture
def tail_calls(monkeypatch):
    """["prepare" | "W=NULL" | "W", ...] of every svr_mlp_tail_fwd call the binding makes during the test."""
    from svr_amd import _lib, ops
    l = _lib.lib()
    rec, fn = [], l.svr_mlp_tail_fwd

    def recorder(*args):
        null = lambda a: not (a.value if isinstance(a, C.c_void_p) else a)      # noqa: E731
        rec.append("prepare" if null(args[0]) else ("W=NULL" if null(args[2]) else "W"))
        return fn(*args)
    monkeypatch.setattr(l, "svr_mlp_tail_fwd", recorder)
    monkeypatch.setattr(ops, "_prepared", None)
    return rec


def _three_ops(ops, h0, w1, b1, w2, b2, wo, bo, rm):
    h1 = ops.linear_fwd(h0, w1, b1, relu=True)
    h2 = ops.linear_fwd(h1, w2, b2, relu=True)
    return h1, h2, ops.fc_out_fwd(h2, wo, bo, rm)


def test_binding_takes_the_fused_kernel_and_finds_prepared_planes(tail_calls, monkeypatch):
    from svr_amd import ops
    h0, w1, b1, w2, b2, wo, bo, perm, ref_h1, ref_h2, _, ref_zp = _case(130, "plain")
    out = ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, perm)
    assert tail_calls == ["W"]      # a miss prepares in place
    assert all(torch.equal(a, b) for a, b in zip(out, (ref_h1, ref_h2, ref_zp)))
    p = ops.PreparedWeights()
    p.begin()
    assert p.add_mlp_tail(w1, w2)
    p.finish(torch.cuda.current_stream())
    monkeypatch.setattr(ops, "_prepared", p)
    del tail_calls[:]
    out = ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, perm)
    assert tail_calls == ["W=NULL"]
    assert all(torch.equal(a, b) for a, b in zip(out, (ref_h1, ref_h2, ref_zp)))
    # planes made with another second matrix are not this pair's planes; a parameter changed in place is a miss
    del tail_calls[:]
    ops.mlp_tail_fwd(h0, w1, b1, w2.clone(), b2, wo, bo, perm)
    w1.add_(0.0)
    ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, perm)
    p.invalidate()
    ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, perm)
    assert tail_calls == ["W", "W", "W"]


def test_shapes_and_layouts_the_kernel_does_not_take_reach_the_three_ops(tail_calls, monkeypatch):
    from svr_amd import ops
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).cuda()      # noqa: E731
    # hidden 128
    h0, w1, b1, w2, b2, wo, bo = torch.relu(r(70, 128)), r(128, 128) / 11, r(128), r(128, 128) / 11, r(128), r(128) / 11, r(1)
    got, want = ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo), _three_ops(ops, h0, w1, b1, w2, b2, wo, bo, None)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a weight matrix that is a column slice of a wider one (the entry point takes contiguous matrices)
    h0, w1, b1, w2, b2, wo, bo, perm, ref_h1, ref_h2, _, ref_zp = _case(65, "plain")
    w1s = torch.cat([w1, w1], dim=1)[:, :H]
    assert not w1s.is_contiguous()
    got = ops.mlp_tail_fwd(h0, w1s, b1, w2, b2, wo, bo, perm)
    assert all(torch.equal(a, b) for a, b in zip(got, (ref_h1, ref_h2, ref_zp)))
    # the default arithmetic switched off
    monkeypatch.setattr(ops, "FORWARD_GEMM", "bf16x6")
    got, want = ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, perm), _three_ops(ops, h0, w1, b1, w2, b2, wo, bo, perm)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    monkeypatch.setattr(ops, "FORWARD_GEMM", "f16x3")
    # h0 at a 4-byte offset: the three-op path is reached and answers as it always has -- its first GEMM refuses the operand
    mis = torch.zeros(65, 260, device="cuda")[:, 1:1 + H]
    mis.copy_(h0)
    assert mis.data_ptr() % 16 == 4
    for call in (lambda: ops.mlp_tail_fwd(mis, w1, b1, w2, b2, wo, bo, perm), lambda: _three_ops(ops, mis, w1, b1, w2, b2, wo, bo, perm)):
        with pytest.raises(RuntimeError, match="linear_fwd_f16x3: X must be 16-byte aligned"):
            call()
    assert tail_calls == []


@pytest.mark.parametrize("headless", (True, False))
def test_point_mlp_function_end_to_end_matches_the_three_op_form(tail_calls, monkeypatch, headless):
    """_PointMLPFn at M = 130, fused tail against the three ops: logits, saved activations and every gradient bit for bit."""
    from svr_amd import ops
    from svr_amd.model import ifnet
    h0, w1, b1, w2, b2, wo, bo, perm = _case(130, "plain")[:8]
    g = torch.Generator().manual_seed(77)
    feat0 = h0 if headless else torch.randn(130, 64, generator=g).cuda()
    w0p0, b00 = (None, None) if headless else ((torch.randn(H, 64, generator=g) / 8).cuda(), (0.1 * torch.randn(H, generator=g)).cuda())
    dz = torch.randn(130, generator=g).cuda()

    def run():
        leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)      # noqa: E731
        args = [leaf(feat0), perm, leaf(w0p0), leaf(b00)] + [leaf(t) for t in (w1, b1, w2, b2, wo, bo)]
        z = ifnet._PointMLPFn.apply(*args)
        saved = [t.clone() for t in z.grad_fn.saved_tensors]
        z.backward(dz)
        return z.detach(), saved, [a.grad for a in args if a is not None and a.requires_grad]

    z_f, saved_f, grads_f = run()
    assert tail_calls == ["W"]
    monkeypatch.setattr(ops, "_mlp_tail_op", lambda *a, **k: "three_ops")
    z_3, saved_3, grads_3 = run()
    assert tail_calls == ["W"]
    assert torch.equal(z_f, z_3)
    assert len(saved_f) == len(saved_3) and all(torch.equal(a, b) for a, b in zip(saved_f, saved_3))
    assert len(grads_f) == len(grads_3) == (7 if headless else 9)      # feat [, w0p, b0], w1, b1, w2, b2, wo, bo
    for i, (a, b) in enumerate(zip(grads_f, grads_3)):
        assert a is not None and torch.equal(a, b), f"gradient {i} differs"
