"""GPU: the fused depth head (csrc/depth_head.hip, ops.depth_head) against the float64 restatement in
tests/depth_head_oracle.py.

WHICH BOUND AND WHY: depth, loss and d raw may be off the float64 result by at most
max(2 x the error of torch's own float32 CPU ops on the same inputs, floor): the kernel rounds source index and weights as
ATen does, so it may be as wrong as ATen and no more than twice that.  Floors (for the shapes on which torch's float32 error
happens to be tiny): 16 ulp of 7.0 = 7.6e-6 for depth, 1e-6 relative for the loss, 4e-6 of max|grad| for the gradient.  An
index or weight bug shows at 1e-2 or more."""
import pytest
import torch

from tests import depth_head_oracle as DO

pytestmark = pytest.mark.gpu

# (B, Hs, Ws, S, r0, r1)
CASES = [(1, 256, 256, 320, 40, 280),       # the real shape
         (2, 16, 16, 20, 2, 18),            # the same 0.8 ratio, small
         (3, 7, 5, 9, 0, 9),                # non-square source, inexact ratio
         (2, 4, 4, 13, 3, 11),              # > 3x up-scaling: many destinations per source pixel
         (1, 20, 20, 8, 1, 7),              # down-scaling: some source pixels receive nothing
         (2, 1, 1, 6, 0, 6),                # 1 x 1 source
         (1, 3, 50, 64, 63, 64),            # one-row crop at the clamped border
         (2, 15, 20, 0, 0, 0)]              # identity mode
IDS = ["x".join(str(v) for v in c) for c in CASES]
DEPTH_FLOOR, LOSS_FLOOR, GRAD_FLOOR = 16 * 2.0 ** -21, 1e-6, 4e-6       # ulp(7.0f) = 2^-21


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _out_shape(case):
    B, Hs, Ws, S, r0, r1 = case
    return (B, 1, r1 - r0, S) if S else (B, 1, Hs, Ws)


_cache = {}


def _case(case):
    """Seeded inputs and both CPU results of a case, computed once and shared (read only)."""
    if case not in _cache:
        B, Hs, Ws, S, r0, r1 = case
        g = torch.Generator().manual_seed(1000 + CASES.index(case))
        raw = 3 * torch.randn(B, 1, Hs, Ws, generator=g)
        target = 5 * torch.rand(_out_shape(case), generator=g) + 0.5
        ref = DO.head_loss_grad(raw, target, S, (r0, r1))
        f32 = DO.head_loss_grad(raw, target, S, (r0, r1), dtype=torch.float32)
        _cache[case] = (raw, target, ref, f32)
    return _cache[case]


def _run(ops, case, raw, target):
    B, Hs, Ws, S, r0, r1 = case
    r = raw.cuda().requires_grad_(True)
    depth, loss = ops.depth_head(r, target.cuda(), size=S, rows=(r0, r1), min_z=DO.MIN_Z, max_z=DO.MAX_Z)
    loss.backward()
    return depth, loss, r.grad


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_depth_loss_and_gradient_against_f64(case):
    ops = _ops()
    raw, target, (rd, rl, rg), (fd, fl, fg) = _case(case)
    depth, loss, grad = _run(ops, case, raw, target)
    assert tuple(depth.shape) == _out_shape(case) and depth.dtype == torch.float32 and not depth.requires_grad
    assert tuple(loss.shape) == () and tuple(grad.shape) == tuple(raw.shape)
    gmax = rg.abs().max().item()
    e_depth, t_depth = (depth.cpu().double() - rd).abs().max().item(), (fd.double() - rd).abs().max().item()
    e_loss, t_loss = abs(loss.item() - rl.item()) / rl.item(), abs(fl.item() - rl.item()) / rl.item()
    e_grad, t_grad = (grad.cpu().double() - rg).abs().max().item() / gmax, (fg.double() - rg).abs().max().item() / gmax
    print(f"{case}: depth {e_depth:.2e} (torch f32 {t_depth:.2e})  loss {e_loss:.2e} ({t_loss:.2e})  grad {e_grad:.2e} ({t_grad:.2e})")
    assert e_depth <= max(2 * t_depth, DEPTH_FLOOR)
    assert e_loss <= max(2 * t_loss, LOSS_FLOOR)
    assert e_grad <= max(2 * t_grad, GRAD_FLOOR)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_untouched_source_rows_get_an_exact_zero(case):
    """Source rows that no cropped destination row reads: 0-30 and 225-255 of the real shape (stated), and whatever the
    float64 autograd leaves at exactly 0 in the down-scaling case (rows and single pixels)."""
    ops = _ops()
    raw, target, (_, _, rg), _ = _case(case)
    _, _, grad = _run(ops, case, raw, target)
    grad = grad.cpu()
    if case == CASES[0]:
        dead = [r for r in range(256) if r <= 30 or r >= 225]
        assert all(not rg[0, 0, r].any() for r in dead) and rg[0, 0, 31].any() and rg[0, 0, 224].any()
        assert not grad[0, 0, dead].any() and grad[0, 0, 31].any() and grad[0, 0, 224].any()
    zero = rg == 0
    assert zero.any() and not grad[zero].any()


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[7]], ids=[IDS[0], IDS[3], IDS[7]])
def test_two_runs_give_the_same_bits_and_inference_mode_the_same_depth(case):
    ops = _ops()
    B, Hs, Ws, S, r0, r1 = case
    raw, target, _, _ = _case(case)
    a, b = _run(ops, case, raw, target), _run(ops, case, raw, target)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    depth, loss = ops.depth_head(raw.cuda(), None, size=S, rows=(r0, r1), min_z=DO.MIN_Z, max_z=DO.MAX_Z)
    assert loss is None and torch.equal(depth.view(torch.int32), a[0].view(torch.int32))


@pytest.mark.parametrize("case", [CASES[1], CASES[7]], ids=[IDS[1], IDS[7]])
def test_saturated_logits_stay_finite_and_in_range(case):
    ops = _ops()
    B, Hs, Ws, S, r0, r1 = case
    _, target, _, _ = _case(case)
    for v in (100.0, -100.0):
        raw = torch.full((B, 1, Hs, Ws), v)
        raw[0, 0, 0, 0] = -v
        depth, loss, grad = _run(ops, case, raw, target)
        assert torch.isfinite(depth).all() and (depth >= DO.MIN_Z).all() and (depth <= DO.MAX_Z).all()
        assert torch.isfinite(loss) and torch.isfinite(grad).all()


@pytest.mark.parametrize("case", [CASES[2], CASES[7]], ids=[IDS[2], IDS[7]])
def test_permuted_view_and_upstream_scaling(case):
    """The HIP UNet returns a permuted view of a (B, Hs, Ws, 1) tensor: the head gives what it gives for the contiguous copy;
    (3 * loss).backward() leaves three times the gradient."""
    ops = _ops()
    B, Hs, Ws, S, r0, r1 = case
    raw, target, _, _ = _case(case)
    depth, loss, grad = _run(ops, case, raw, target)
    cl = raw.permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)          # (B, Hs, Ws, 1)
    d2, l2 = ops.depth_head(cl.permute(0, 3, 1, 2), target.cuda(), size=S, rows=(r0, r1), min_z=DO.MIN_Z, max_z=DO.MAX_Z)
    (3 * l2).backward()
    assert torch.equal(d2, depth) and torch.equal(l2, loss)
    assert torch.equal(cl.grad.permute(0, 3, 1, 2), 3 * grad)
