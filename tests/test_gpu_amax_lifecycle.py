"""GPU: does the |max| word of the "f16x3s" backward kernels still describe the gradient tensor when a kernel reads it?

Every gradient operand of the scaled f16 split is multiplied by a power of two taken from its |max|, a one-word device tensor
that travels on the tensor object (`_svr_amax`: left by the producing kernel, or computed once by ops.amax_of and remembered).
The other suites pin the kernels that consume the word and the kernels that produce it; this one pins the time in between:
tensors that are refilled in place, changed between their two consumers, changed through a view, accumulated into by
autograd, or written by an op through a raw pointer.  A stale word is no error anywhere: a tensor that grew overflows f16
(inf / NaN out), one that shrank loses its mantissa or flushes to zero (a wrong finite number out).

Every result is compared with the float64 product of the same operands on the CPU, at the gates the project already holds
these kernels to: 2e-6 for the linear dX / dW (test_linear_backward_at_f32_level_f16x3s), 3e-6 for the 3x3x3 convolution
(test_conv3d_backward_at_f32_level_f16x3s), 5e-6 for the implicit-GEMM 2-D convolution (test_conv_block_forward_backward).
Refills are by powers of two (2^10 up, 2^-40 down), so the reference of a refilled tensor is an exact rescale.  The shapes are
the smallest ones those tests already route to the f16x3s kernels; the route is asserted here as well.  The host-side rule
(ops.amax_cached) is tests/test_amax_cache_cpu.py.  Graph capture is not touched: its words come from torch.zeros
(test_whole_step_hip_graph_replays_the_eager_step)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _golden as G

pytestmark = pytest.mark.gpu

GROW, SHRINK = 2.0 ** 10, 2.0 ** -40
LIN_GATE, CONV3_GATE, CONV2_GATE = 2e-6, 3e-6, 5e-6
LINEAR_SHAPES = [(520, 256, 36), (130, 512, 64)]
CONV2_SHAPE = (2, 7, 5, 20, 12, 72, 4, 2)            # B, H, W, C0, C1, Cout, k, stride: dy (2, 3, 2, 72)
# (f) a layer that is not `small` whose dy has an element count that is no multiple of 4: _amax_any's abs().max() branch.
# Cout = 6 is outside 1..4, and B Ho Wo = 1 * 3 * 3 is odd: 54 elements.  The library takes the shape (any Cout > 0).
CONV2_ODD_SHAPE = (1, 7, 6, 20, 12, 6, 4, 2)


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _word(a):
    return float(a.view(torch.float32))


def _amax_is(ops, t):
    """ops' word for t (amax_of, or _amax_any's branch for element counts that are no multiple of 4) == t.abs().max(), bit for bit"""
    a = ops.amax_of(t) if t.numel() % 4 == 0 else ops._amax_any(t)
    return _word(a) == float(t.abs().max())


def _errs(outs, refs, factor=1.0):
    """[(finite, max|out - ref f| / max|ref f|)] per output; refs are float64 CPU tensors in the outputs' layout"""
    return [(bool(torch.isfinite(o).all()), G.rel_err(o.detach().cpu().double().numpy(), (r * factor).numpy())) for o, r in zip(outs, refs)]


def _assert_errs(errs, gate, what):
    print("amax_lifecycle", what, [(f, f"{e:.2e}") for f, e in errs])
    for finite, e in errs:
        assert finite, (what, "inf / NaN in the output")
        assert e < gate, (what, e, gate)


class _Consumer:
    """One op that reads the word of its gradient operand: dy0 (CPU, the op's layout), run(ops, dy on the GPU) -> outputs,
    refs: their float64 values for dy0 (linear in dy: the reference of f * dy0 is f * refs)."""

    def __init__(self, dy0, run, refs, gate):
        self.dy0, self.run, self.refs, self.gate = dy0, run, refs, gate


@functools.lru_cache(maxsize=None)
def _linear_operands(M, N, K):
    g = torch.Generator().manual_seed(M + K)
    x = F.relu(torch.randn(M, K, generator=g)) * torch.exp(torch.randn(M, 1, generator=g))
    w = torch.randn(N, K, generator=g) / K ** 0.5
    dy0 = torch.randn(M, N, generator=g) * torch.exp(2 * torch.randn(M, 1, generator=g))
    dx = dy0.double() @ w.double()
    return {"x": x, "w": w, "dy0": dy0, "xc": x.cuda(), "wc": w.cuda(), "dx": dx, "dxm": dx * (x.double() > 0),
            "dw": dy0.double().t() @ x.double()}


def _linear_consumer(kind, M, N, K):
    ops = _ops()
    o = _linear_operands(M, N, K)
    if kind == "weight":
        assert ops.linear_variant("bwd_weight", "f16x3s", M, N, K)["op"] == "bwd_weight_f16x3s"
        return _Consumer(o["dy0"], lambda ops, dy: [ops.linear_bwd_weight(dy, o["xc"], mode="f16x3s")[0]], [o["dw"]], LIN_GATE)
    masked = kind == "data_masked"
    assert ops.linear_variant("bwd_data", "f16x3s", M, N, K, mask=(K, 0, True) if masked else None)["op"] == "bwd_data_f16x3s"

    def run(ops, dy):
        dx = ops.linear_bwd_data(dy, o["wc"], mask=o["xc"] if masked else None, mode="f16x3s")
        assert hasattr(dx, "_svr_amax"), "the f16x3s kernel did not run"
        return [dx]
    return _Consumer(o["dy0"], run, [o["dxm" if masked else "dx"]], LIN_GATE)


def _splitk_consumer(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    dy0 = torch.randn(M, N, generator=g) * torch.exp(2 * torch.randn(M, 1, generator=g))
    wt = torch.randn(K, N, generator=g) / N ** 0.5
    wtc = wt.cuda()

    def run(ops, dy):
        dx = ops.linear_bwd_data_splitk(dy, wtc)
        assert hasattr(dx, "_svr_amax")
        return [dx]
    return _Consumer(dy0, run, [dy0.double() @ wt.double().t()], LIN_GATE)


@functools.lru_cache(maxsize=None)
def _conv3_operands(B=1, D=8, Ci=32, Co=32):
    g = torch.Generator().manual_seed(Ci * 1000 + Co + 11)
    x = F.relu(torch.randn(B, Ci, D, D, D, generator=g))
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g) / (27 * Ci) ** 0.5
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    pre = F.conv3d(xd, wd, None, padding=1)
    dy = torch.randn(pre.shape, generator=g) * torch.exp(2 * torch.randn(B, 1, D, D, D, generator=g))
    return {"x": x, "w": w, "xc": x.permute(0, 2, 3, 4, 1).contiguous().cuda(), "wc": w.cuda(),
            "dy0": dy.permute(0, 2, 3, 4, 1).contiguous()}


def _conv3_refs(o, dy_cl):
    """float64 gradients (NCDHW input gradient, parameter-layout weight gradient) of conv3d for a channels-last CPU dy"""
    xd, wd = o["x"].double().requires_grad_(True), o["w"].double().requires_grad_(True)
    pre = F.conv3d(xd, wd, None, padding=1)
    gx, gw = torch.autograd.grad(pre, (xd, wd), dy_cl.double().permute(0, 4, 1, 2, 3))
    return gx, gw


def _conv3_run(ops, o, dy, which):
    if which == "data":
        din = ops.conv3d_k3_bwd_data(dy, o["wc"], mode="f16x3s")
        assert hasattr(din, "_svr_amax"), "the f16x3s kernel did not run"
        return [din.permute(0, 4, 1, 2, 3)]
    # (the weight gradient leaves no word to tell the route by: Ci, Co multiples of 4, dy contiguous with 4 | numel -> f16x3s)
    assert dy.is_contiguous() and dy.numel() % 4 == 0
    return [ops.conv3d_k3_bwd_weight(o["xc"], dy, mode="f16x3s", param_layout=True)[0]]


@functools.lru_cache(maxsize=None)
def _conv3_consumer(which):
    o = _conv3_operands()
    gx, gw = _conv3_refs(o, o["dy0"])
    return _Consumer(o["dy0"], lambda ops, dy: _conv3_run(ops, o, dy, which), [gx if which == "data" else gw], CONV3_GATE)


@functools.lru_cache(maxsize=None)
def _conv2_operands(shape):
    ops = _ops()
    B, H, W, C0, C1, Cout, k, stride = shape
    g = torch.Generator().manual_seed(B * 100 + H + C0 + Cout)
    s0, s1 = torch.randn(B, C0, H, W, generator=g), torch.randn(B, C1, H, W, generator=g)
    w = torch.randn(Cout, C0 + C1, k, k, generator=g) / (k * k * (C0 + C1)) ** 0.5
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(F.leaky_relu(torch.cat((s0, s1), 1), 0.2), w, stride=stride, padding=1)
    dy = torch.randn(ref.shape, generator=g) * torch.exp(torch.randn(B, 1, *ref.shape[2:], generator=g))
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous()      # noqa: E731
    planes = ops.Conv2dPlanes(w.cuda(), stride, want_bwd=True)
    assert not planes.small, "the implicit GEMM was meant"
    return {"s0": s0, "s1": s1, "w": w, "b": b, "g0": cl(s0).cuda(), "g1": cl(s1).cuda(), "bc": b.cuda(), "planes": planes,
            "dy0": cl(dy), "cfg": (Cout, k, stride)}


def _conv2_refs(o, dy_cl):
    """float64 gradients (of the activated, concatenated input, NCHW; of the weight) for a channels-last CPU dy"""
    _, k, stride = o["cfg"]
    xa = F.leaky_relu(torch.cat((o["s0"], o["s1"]), 1).double(), 0.2).requires_grad_(True)
    wd = o["w"].double().requires_grad_(True)
    gxa, gw = torch.autograd.grad(F.conv2d(xa, wd, stride=stride, padding=1), (xa, wd), dy_cl.double().permute(0, 3, 1, 2))
    return gxa, gw


def _conv2_run(ops, o, dy, which):
    Cout, k, stride = o["cfg"]
    if which == "data":
        return [ops.conv2d_bwd_data(o["g0"], o["g1"], k, stride, o["planes"], dy).permute(0, 3, 1, 2)]
    return [ops.conv2d_bwd_weight(o["g0"], o["g1"], k, stride, ops.ACT_LEAKY, dy, Cout)[0]]


@functools.lru_cache(maxsize=None)
def _conv2_consumer(which, shape):
    o = _conv2_operands(shape)
    gxa, gw = _conv2_refs(o, o["dy0"])
    return _Consumer(o["dy0"], lambda ops, dy: _conv2_run(ops, o, dy, which), [gxa if which == "data" else gw], CONV2_GATE)


CONSUMERS = {}
for _s in LINEAR_SHAPES:
    for _kind in ("data", "data_masked", "weight"):
        CONSUMERS[f"linear_bwd_{_kind}_{_s[0]}x{_s[1]}x{_s[2]}"] = functools.partial(_linear_consumer, _kind, *_s)
CONSUMERS["linear_bwd_data_splitk_130x512x64"] = functools.partial(_splitk_consumer, 130, 512, 64)
CONSUMERS["conv3d_k3_bwd_data"] = functools.partial(_conv3_consumer, "data")
CONSUMERS["conv3d_k3_bwd_weight"] = functools.partial(_conv3_consumer, "weight")
CONSUMERS["conv2d_bwd_data"] = functools.partial(_conv2_consumer, "data", CONV2_SHAPE)
CONSUMERS["conv2d_bwd_weight"] = functools.partial(_conv2_consumer, "weight", CONV2_SHAPE)
CONSUMERS["conv2d_bwd_data_54_elements"] = functools.partial(_conv2_consumer, "data", CONV2_ODD_SHAPE)
CONSUMERS["conv2d_bwd_weight_54_elements"] = functools.partial(_conv2_consumer, "weight", CONV2_ODD_SHAPE)

REFILL = {      # how the same tensor object gets f * dy0 as its new contents
    "copy_": lambda dy, dy0, f: dy.copy_((dy0 * f).cuda()),
    "mul_": lambda dy, dy0, f: dy.mul_(f),
    "slice_assignment": lambda dy, dy0, f: dy.__setitem__(slice(None), (dy0 * f).cuda()),
    "foreach_mul_": lambda dy, dy0, f: torch._foreach_mul_([dy], f),
}


# ---- a. refill in place ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", sorted(REFILL))
@pytest.mark.parametrize("factor", [GROW, SHRINK], ids=["grow_2p10", "shrink_2m40"])
@pytest.mark.parametrize("name", sorted(CONSUMERS))
def test_refilled_gradient_tensor(name, factor, how):
    """Consume dy, overwrite the same tensor object with dy0 * factor, consume it again: f32-level results both times, and the
    word amax_of hands out equals the tensor's |max| after the refill."""
    ops = _ops()
    c = CONSUMERS[name]()
    dy = c.dy0.cuda()
    first = _errs(c.run(ops, dy), c.refs)
    REFILL[how](dy, c.dy0, factor)
    assert torch.equal(dy.cpu(), c.dy0 * factor)
    second = _errs(c.run(ops, dy), c.refs, factor)
    word_ok = _amax_is(ops, dy)
    print("amax_lifecycle", name, how, factor, "word == |max| after the refill:", word_ok)
    _assert_errs(first, c.gate, (name, "first call"))
    _assert_errs(second, c.gate, (name, how, factor, "after the refill"))
    assert word_ok, (name, how, factor, "amax_of(dy) != dy.abs().max() after the refill")


# ---- b. two consumers, a hook in between -------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["weight_then_data", "data_then_weight"])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_gradient_scaled_in_place_between_its_two_products(M, N, K, order):
    ops = _ops()
    o = _linear_operands(M, N, K)
    dy = o["dy0"].cuda()
    if order == "weight_then_data":
        dw, _ = ops.linear_bwd_weight(dy, o["xc"], mode="f16x3s")
        dy.mul_(1024)
        dx = ops.linear_bwd_data(dy, o["wc"], mode="f16x3s")
        fw, fx = 1.0, 1024.0
    else:
        dx = ops.linear_bwd_data(dy, o["wc"], mode="f16x3s")
        dy.mul_(1024)
        dw, _ = ops.linear_bwd_weight(dy, o["xc"], mode="f16x3s")
        fw, fx = 1024.0, 1.0
    assert hasattr(dx, "_svr_amax")
    _assert_errs(_errs([dw], [o["dw"]], fw) + _errs([dx], [o["dx"]], fx), LIN_GATE, (M, N, K, order))


# ---- c. views and slices -----------------------------------------------------------------------------------------------------
def test_change_through_a_view_of_the_cached_tensor():
    """Half of t is multiplied by 1024 through t.view(-1): the version counter is shared, the word of t is recomputed."""
    ops = _ops()
    M, N, K = LINEAR_SHAPES[0]
    o = _linear_operands(M, N, K)
    t = o["dy0"].cuda()
    assert _word(ops.amax_of(t)) == float(o["dy0"].abs().max())
    t.view(-1)[: M * N // 2] *= 1024
    now = t.cpu().double()
    dx = ops.linear_bwd_data(t, o["wc"], mode="f16x3s")
    dw, _ = ops.linear_bwd_weight(t, o["xc"], mode="f16x3s")
    _assert_errs(_errs([dx, dw], [now @ o["w"].double(), now.t() @ o["x"].double()]), LIN_GATE, "flat view")
    assert _amax_is(ops, t)


def test_column_slice_of_a_buffer_that_changes_in_place():
    """t[:, :N] of a wider buffer t: the slice object that was consumed before t.mul_ (it remembers a word, and shares t's
    counter) and a slice taken afterwards (a new object: no word) both follow the new contents; so does t itself."""
    ops = _ops()
    M, N, K = LINEAR_SHAPES[0]
    o = _linear_operands(M, N, K)
    t = torch.zeros(M, N + 64, device="cuda")
    t[:, :N] = o["dy0"].cuda()
    t[:, N:] = 1e-3
    assert _word(ops.amax_of(t)) == float(o["dy0"].abs().max())
    old = t[:, :N]
    _assert_errs(_errs([ops.linear_bwd_data(old, o["wc"], mode="f16x3s")], [o["dx"]]), LIN_GATE, "slice, before")
    t.mul_(1024)
    for what, s in (("the slice from before", old), ("a new slice", t[:, :N])):
        dx = ops.linear_bwd_data(s, o["wc"], mode="f16x3s")
        dw, _ = ops.linear_bwd_weight(s, o["xc"], mode="f16x3s")
        assert hasattr(dx, "_svr_amax")
        _assert_errs(_errs([dx, dw], [o["dx"], o["dw"]], 1024.0), LIN_GATE, what)
        assert _word(ops.amax_of(s)) == float(s.abs().max()), what
    assert _amax_is(ops, t)


def test_non_contiguous_gradient_tensors():
    """amax_of's branch that copies (a transposed t): no op hands it a non-contiguous tensor today -- the linear ops send such a dy
    to the exact-f32 kernels, conv3d wants a contiguous dout, conv2d copies first -- so amax_of itself is asked; and the conv2d
    ops on a permuted (NCHW-stored) dy, whose copy is a new tensor on every call."""
    ops = _ops()
    M, N, _ = LINEAR_SHAPES[1]
    g = torch.Generator().manual_seed(3)
    base = torch.randn(N, M, generator=g).cuda()
    t = base.t()
    assert not t.is_contiguous() and _word(ops.amax_of(t)) == float(t.abs().max())
    t.mul_(1024)
    assert _word(ops.amax_of(t)) == float(t.abs().max())
    base.mul_(2.0 ** -40)                                           # (through the tensor t is a view of)
    assert _word(ops.amax_of(t)) == float(t.abs().max())
    o = _conv2_operands(CONV2_SHAPE)
    nchw = o["dy0"].permute(0, 3, 1, 2).contiguous().cuda()
    dy = nchw.permute(0, 2, 3, 1)
    assert not dy.is_contiguous()
    refs = _conv2_refs(o, o["dy0"])
    for f in (1.0, 1024.0):
        outs = _conv2_run(ops, o, dy, "data") + _conv2_run(ops, o, dy, "weight")
        _assert_errs(_errs(outs, refs, f), CONV2_GATE, ("permuted dy", f))
        nchw.mul_(1024)


# ---- d. words left by producing kernels, then accumulated into ---------------------------------------------------------------
def _next_linear_layer(ops, dy, K2, seed):
    """the two backward products of a layer whose output gradient is dy (M, N): -> errors against float64 of dy's contents"""
    M, N = dy.shape
    g = torch.Generator().manual_seed(seed)
    w2 = torch.randn(N, K2, generator=g) / K2 ** 0.5
    x2 = F.relu(torch.randn(M, K2, generator=g))
    assert ops.linear_variant("bwd_data", "f16x3s", M, N, K2)["op"] == "bwd_data_f16x3s"
    assert ops.linear_variant("bwd_weight", "f16x3s", M, N, K2)["op"] == "bwd_weight_f16x3s"
    now = dy.detach().cpu().double()
    dx = ops.linear_bwd_data(dy, w2.cuda(), mode="f16x3s")
    dw, _ = ops.linear_bwd_weight(dy, x2.cuda(), mode="f16x3s")
    return _errs([dx, dw], [now @ w2.double(), now.t() @ x2.double()])


def _accumulate(out, seed):
    """out += a contribution 1000 times larger, in place: what autograd does when a second gradient arrives"""
    g = torch.Generator().manual_seed(seed)
    other = (torch.randn(out.shape, generator=g) * 1000.0 * float(out.abs().max())).cuda()
    out.add_(other)


def _produce_linear_bwd_data(ops):
    o = _linear_operands(*LINEAR_SHAPES[1])
    return ops.linear_bwd_data(o["dy0"].cuda(), o["wc"], mode="f16x3s"), "linear", LIN_GATE       # (130, 64)


def _produce_splitk(ops):
    c = _splitk_consumer(130, 512, 64)
    return c.run(ops, c.dy0.cuda())[0], "linear", LIN_GATE                                             # conv2d_fwd(want_amax=True) inside


def _produce_fc_out_bwd(ops):
    g = torch.Generator().manual_seed(41)
    M, K = 130, 256
    h = F.relu(torch.randn(M, K, generator=g)).cuda()
    w = (torch.randn(K, generator=g) / 16).cuda()
    dh, _, _ = ops.fc_out_bwd(h, w, torch.randn(M, generator=g).cuda())
    return dh, "linear", LIN_GATE                                                                      # (130, 256)


def _produce_conv3_bwd_data(ops):
    o = _conv3_operands()
    return ops.conv3d_k3_bwd_data(o["dy0"].cuda(), o["wc"], mode="f16x3s"), "conv3", CONV3_GATE


def _produce_bn_backward(ops):
    g = torch.Generator().manual_seed(43)
    C = 32
    x = F.relu(torch.randn(1, 8, 8, 8, C, generator=g)).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.rand(C, generator=g) - 0.5).cuda()
    _, _, _, ss, mean = ops.bn_forward(x, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda(), True, want_pool=False)
    dx, _, _ = ops.bn_backward(x, torch.randn(1, 8, 8, 8, C, generator=g).cuda(), None, None, mean, ss, relu_mask=True)
    return dx, "conv3", CONV3_GATE


def _produce_conv2_fwd(ops):
    o = _conv2_operands(CONV2_SHAPE)
    Cout, k, stride = o["cfg"]
    y = ops.conv2d_fwd(o["g0"], o["g1"], k, stride, ops.ACT_LEAKY, o["planes"], o["bc"], want_amax=True)
    return y, "conv2", CONV2_GATE


PRODUCERS = {"linear_bwd_data": _produce_linear_bwd_data, "fc_out_bwd": _produce_fc_out_bwd, "conv3d_k3_bwd_data": _produce_conv3_bwd_data,
             "bn_backward": _produce_bn_backward, "conv2d_fwd_want_amax": _produce_conv2_fwd, "linear_bwd_data_splitk": _produce_splitk}


@pytest.mark.parametrize("name", sorted(PRODUCERS))
def test_producer_word_after_an_in_place_accumulation(name):
    """A gradient that carries its producing kernel's word gets a 1000x larger contribution added in place, then feeds the
    next layer's two backward products."""
    ops = _ops()
    out, nxt, gate = PRODUCERS[name](ops)
    assert hasattr(out, "_svr_amax") and _word(out._svr_amax) == float(out.abs().max()), "no word from the producer"
    _accumulate(out, 47)
    if nxt == "linear":
        errs = _next_linear_layer(ops, out, 36 if out.shape[1] == 256 else 32, 53)
    elif nxt == "conv3":
        o = _conv3_operands()
        refs = _conv3_refs(o, out.cpu())
        errs = _errs(_conv3_run(ops, o, out, "data") + _conv3_run(ops, o, out, "weight"), refs)
    else:
        o = _conv2_operands(CONV2_SHAPE)
        refs = _conv2_refs(o, out.cpu())
        errs = _errs(_conv2_run(ops, o, out, "data") + _conv2_run(ops, o, out, "weight"), refs)
    _assert_errs(errs, gate, (name, "after add_"))
    assert _amax_is(ops, out)


class _BranchFn(torch.autograd.Function):
    """y = h @ w.T; its backward hands autograd the f16x3s dX -- a tensor that carries its kernel's word."""

    @staticmethod
    def forward(ctx, h, w):
        ctx.save_for_backward(w)
        return h @ w.t()

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return _ops().linear_bwd_data(g.contiguous(), w, mode="f16x3s"), None


class _TrunkFn(torch.autograd.Function):
    """h = x @ w0.T; its backward runs both f16x3s products on whatever gradient of h autograd has accumulated."""

    @staticmethod
    def forward(ctx, x, w0, log):
        ctx.save_for_backward(x, w0)
        ctx.log = log
        return x @ w0.t()

    @staticmethod
    def backward(ctx, gh):
        ops = _ops()
        x, w0 = ctx.saved_tensors
        ctx.log["gh"] = gh.detach().clone()
        ctx.log["carried_a_word"] = getattr(gh, "_svr_amax", None) is not None
        dx = ops.linear_bwd_data(gh, w0, mode="f16x3s")
        dw, _ = ops.linear_bwd_weight(gh, x, mode="f16x3s")
        return dx, dw, None


@pytest.mark.parametrize("large", ["first_branch", "second_branch"])
def test_autograd_accumulates_two_branch_gradients_of_one_tensor(large):
    """h feeds two branches whose backward each return a linear_bwd_data result; one branch's gradient is 1000x the other's.
    Autograd sums the two (in place into the first to arrive, where it can) and hands the sum to the trunk's backward."""
    ops = _ops()
    M, N, K = LINEAR_SHAPES[1]
    K0 = 32
    g = torch.Generator().manual_seed(59)
    x = torch.randn(M, K0, generator=g)
    w0 = torch.randn(K, K0, generator=g) / K0 ** 0.5
    w1, w2 = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, K, generator=g) / K ** 0.5
    g1, g2 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    if large == "first_branch":
        g1 = g1 * 1000.0
    else:
        g2 = g2 * 1000.0
    assert ops.linear_variant("bwd_data", "f16x3s", M, K, K0)["op"] == "bwd_data_f16x3s"
    assert ops.linear_variant("bwd_weight", "f16x3s", M, K, K0)["op"] == "bwd_weight_f16x3s"
    xc, w0c = x.cuda().requires_grad_(True), w0.cuda().requires_grad_(True)
    log = {}
    h = _TrunkFn.apply(xc, w0c, log)
    y1, y2 = _BranchFn.apply(h, w1.cuda()), _BranchFn.apply(h, w2.cuda())
    torch.autograd.backward([y1, y2], [g1.cuda(), g2.cuda()])
    gh_ref = g1.double() @ w1.double() + g2.double() @ w2.double()
    gh = log["gh"].cpu().double()
    print("amax_lifecycle autograd", large, "the accumulated gradient carried a word:", log["carried_a_word"])
    errs = _errs([log["gh"]], [gh_ref]) + _errs([xc.grad, w0c.grad], [gh @ w0.double(), gh.t() @ x.double()])
    _assert_errs(errs, LIN_GATE, ("autograd", large))


# ---- e. ops that write into a tensor of the caller through its raw pointer ---------------------------------------------------
def _planted(ops, *shape):
    """a float32 GPU tensor with |max| exactly 1 that carries a remembered word holding 1.0f"""
    t = torch.rand(*shape, device="cuda")
    t.view(-1)[0] = 1.0
    assert _word(ops.amax_of(t)) == 1.0 and _word(t._svr_amax) == 1.0
    return t


def _pyramid(B=2, D=16, N=400):
    chans = [1, 16, 32, 64, 128, 128]
    g = torch.Generator().manual_seed(67)
    vols, d = [], D
    for i, c in enumerate(chans):
        vols.append(torch.randn(B, d, d, d, c, generator=g).cuda())
        if i >= 1:
            d = max(1, d // 2)
    pts = ((torch.rand(B, N, 3, generator=g) - 0.5) * 1.1).cuda()
    return chans, vols, pts, float(np.float32(0.0722))


def _w_linear_fwd(ops, mode):
    g = torch.Generator().manual_seed(71)
    x, w, b = torch.randn(130, 64, generator=g).cuda(), torch.randn(48, 64, generator=g).cuda(), torch.randn(48, generator=g).cuda()
    out = _planted(ops, 130, 48)
    ops.linear_fwd(x, w, b, relu=False, out=out, mode=mode)
    return [out]


def _w_linear_bwd_data(ops, mode):
    o = _linear_operands(*LINEAR_SHAPES[1])
    out = _planted(ops, 130, 64)
    ops.linear_bwd_data(o["dy0"].cuda(), o["wc"], out=out, mode=mode)
    return [out]


def _w_gather_fwd(ops):
    chans, vols, pts, disp = _pyramid()
    layout = ops.FeatureLayout(chans)
    out = _planted(ops, pts.shape[0] * pts.shape[1], layout.row_stride)
    ops.gather_fwd(vols, pts, layout, disp, False, out=out)
    return [out]


def _w_gather_fc0(ops, through):
    chans, vols, pts, disp = _pyramid(N=777)
    B, N, _ = pts.shape
    layout = ops.FeatureLayout(chans)
    g = torch.Generator().manual_seed(73)
    w = (torch.randn(256, layout.row_stride, generator=g) / 30).cuda()
    w[:, layout.width:] = 0
    bias = torch.randn(256, generator=g).cuda()
    assert ops.gather_fc0_supported(vols, pts, layout, disp, False)
    keep = [l for l, c in enumerate(chans) if c < 128]
    klay = layout.subset(keep)
    out = _planted(ops, B * N, klay.row_stride)
    if through == "fwd":
        _, rows = ops.gather_fc0_fwd(vols, pts, layout, disp, False, w, bias, keep_levels=keep, keep_layout=klay, rows_out=out)
    else:
        prep = ops.gather_fc0_prepare(vols, layout, disp, False, w, B, N, keep, klay)
        _, rows = ops.gather_fc0_run(prep, pts, bias, rows_out=out)
    assert rows.data_ptr() == out.data_ptr()
    return [out]


def _w_gather_project_bwd(ops):
    g = torch.Generator().manual_seed(79)
    B, N, dims, disp = 2, 300, (8, 8, 8), float(np.float32(0.0722))
    pts = ((torch.rand(B, N, 3, generator=g) - 0.5) * 1.2).cuda()
    dh = torch.randn(B * N, 256, generator=g).cuda()
    items = ops.item_order(pts, dims, disp, False, with_j=True)
    out = _planted(ops, B, 512, 7, 256)                     # (the scatter adds to what is there)
    assert ops.gather_project_bwd(pts, dh, dims, items, disp, False, out=out).data_ptr() == out.data_ptr()
    return [out]


def _w_gather_bwd(ops):
    chans, vols, pts, disp = _pyramid()
    layout = ops.FeatureLayout(chans)
    g = torch.Generator().manual_seed(83)
    gfeat = torch.randn(pts.shape[0] * pts.shape[1], layout.row_stride, generator=g).cuda()
    gvols = [_planted(ops, *v.shape) for v in vols]          # (accumulated into)
    ops.gather_bwd(vols, gvols, pts, gfeat, layout, disp, False)
    return gvols


def _w_bn_forward(ops):
    g = torch.Generator().manual_seed(89)
    C = 32
    x = (torch.randn(1, 8, 8, 8, C, generator=g) * 3 + 2).cuda()
    rm, rv = _planted(ops, C), _planted(ops, C)
    ops.bn_forward(x, torch.ones(C).cuda(), torch.zeros(C).cuda(), rm, rv, True, want_pool=False)
    return [rm, rv]


def _w_stage1_fwd(ops):
    g = torch.Generator().manual_seed(97)
    x = ((torch.rand(1, 8, 8, 8, 1, generator=g) < 0.3).float() * 4).cuda()
    assert ops.stage1_supported(x, 16)
    w, b = (torch.randn(16, 1, 3, 3, 3, generator=g) * 3).cuda(), torch.randn(16, generator=g).cuda()
    rm, rv = _planted(ops, 16), _planted(ops, 16)
    ops.stage1_fwd(x, w, b, torch.ones(16).cuda(), torch.zeros(16).cuda(), rm, rv, True)
    return [rm, rv]


# Every op of ops.py that writes into a tensor the caller supplies, found by reading the file; (op, argument) -> the call.
# Ops not listed allocate what they return.  The `arena=` arguments (morton_order, pull_plan, item_order, gather_fc0_prepare)
# hand out int32 / uint8 work buffers, which are no f32 operands and never carry a word.
RAW_POINTER_WRITERS = {
    "linear_fwd(out=) f16x3": lambda ops: _w_linear_fwd(ops, "f16x3"),
    "linear_fwd(out=) bf16x6": lambda ops: _w_linear_fwd(ops, "bf16x6"),
    "linear_fwd(out=) f32": lambda ops: _w_linear_fwd(ops, "f32"),
    "linear_bwd_data(out=) f16x3s": lambda ops: _w_linear_bwd_data(ops, "f16x3s"),       # replaces the word
    "linear_bwd_data(out=) bf16x3": lambda ops: _w_linear_bwd_data(ops, "bf16x3"),
    "linear_bwd_data(out=) f32": lambda ops: _w_linear_bwd_data(ops, "f32"),
    "gather_fwd(out=)": _w_gather_fwd,
    "gather_fc0_fwd(rows_out=)": lambda ops: _w_gather_fc0(ops, "fwd"),
    "gather_fc0_run(rows_out=)": lambda ops: _w_gather_fc0(ops, "run"),
    "gather_project_bwd(out=)": _w_gather_project_bwd,
    "gather_bwd(gvols)": _w_gather_bwd,
    "bn_forward(running_mean, running_var)": _w_bn_forward,
    "stage1_fwd(running_mean, running_var)": _w_stage1_fwd,
}


@pytest.mark.parametrize("name", sorted(RAW_POINTER_WRITERS))
def test_raw_pointer_writers_forget_or_replace_the_word(name):
    ops = _ops()
    for i, out in enumerate(RAW_POINTER_WRITERS[name](ops)):
        now = float(out.abs().max())
        assert now != 1.0, (name, i, "the op left the contents as they were: the case shows nothing")
        a = getattr(out, "_svr_amax", None)
        assert a is None or _word(a) == now, (name, i, "the old word is still on the tensor")
        assert _word(ops.amax_of(out)) == now, (name, i)


# ---- g. the split-reduction dX at very few output columns --------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 4, 5])
def test_linear_bwd_data_splitk_at_few_outputs(K):
    """K <= 4 with K * N <= 8192 is the plain-FMA class of the 2-D convolution, which has no 1x1 form: a ValueError that says so
    (not an AttributeError from the missing word); otherwise a result within 2e-6 of float64 that carries its exact |max|."""
    ops = _ops()
    M, N = 77, 1792
    g = torch.Generator().manual_seed(101 + K)
    dy = torch.randn(M, N, generator=g)
    wt = torch.randn(K, N, generator=g) / N ** 0.5
    try:
        got = ops.linear_bwd_data_splitk(dy.cuda(), wt.cuda())
    except ValueError as e:
        assert K <= 4 and "K >= 5" in str(e) and "8192" in str(e), str(e)
        return
    _assert_errs(_errs([got], [dy.double() @ wt.double().t()]), LIN_GATE, ("splitk", K))
    assert _word(got._svr_amax) == float(got.abs().max())


# ---- what the version counter cannot see, and its remedy ---------------------------------------------------------------------
@pytest.mark.parametrize("remedy", ["force", "forget"])
def test_write_through_data_needs_force_or_forget(remedy):
    """t.data.mul_() moves neither t's version counter nor its address (documented in amax_of and INTEGRATION.md): the caller
    says so with amax_of(t, force=True) or amax_forget(t), and the next products are right."""
    ops = _ops()
    M, N, K = LINEAR_SHAPES[0]
    o = _linear_operands(M, N, K)
    dy = o["dy0"].cuda()
    _assert_errs(_errs([ops.linear_bwd_data(dy, o["wc"], mode="f16x3s")], [o["dx"]]), LIN_GATE, "before")
    dy.data.mul_(1024)
    if remedy == "force":
        assert _word(ops.amax_of(dy, force=True)) == float(dy.abs().max())
    else:
        ops.amax_forget(dy)
    dx = ops.linear_bwd_data(dy, o["wc"], mode="f16x3s")
    dw, _ = ops.linear_bwd_weight(dy, o["xc"], mode="f16x3s")
    _assert_errs(_errs([dx, dw], [o["dx"], o["dw"]], 1024.0), LIN_GATE, remedy)
    assert _word(ops.amax_of(dy)) == float(dy.abs().max())
