"""GPU: every kernel of csrc/projection.hip on its own, called through svr_amd.ops, against the numpy float64 references of
tests/projection_f64.py (the clamp: bit for bit against float32 torch on the CPU).  The cases and their seeded inputs are
tests/_projection_cases.py; tests/test_projection_f64_cpu.py ties the references to float64 autograd of the oracle's
restatement (1e-12), measures the gates below on the same inputs and shows that a missing tap flip, a negated tap offset,
exchanged pixel indices, exchanged or missing (D - 1) factors and exclusive clamp bounds all lie >= 100 gates away.

The gates.  e32 is G.rel_err of the stock-torch float32 restatement of the operation (oracle/projection_oracle.py's
formulas, F.conv3d per axis) against the float64 reference, the maximum over the group's cases, measured on one CPU thread
and rounded up to two digits.  The gate of a comparison is 4 * e32 of its group: the kernels add the same float32 terms in
another order than torch does, and the tap gradient adds float32 thread partials in a float64 tree.  No gate is above 1e-5.

    group                    e32        gate = 4 * e32
    unproject forward        2.5e-07    1.0e-06
    unproject backward       1.5e-07    6.0e-07
    splat backward           1.7e-07    6.8e-07
    blur forward             1.6e-07    6.4e-07
    blur adjoint             1.7e-07    6.8e-07
    tap gradient             1.7e-06    6.8e-06
    smooth output            8.5e-08    3.4e-07
    smooth voxel gradient    1.3e-07    5.2e-07
    smooth tap gradient      1.2e-07    4.8e-07

Every comparison is printed next to its gate before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

from oracle import projection_oracle as P
from tests import _golden as G
from tests import _projection_cases as C
from tests import projection_f64 as R

pytestmark = pytest.mark.gpu

E32 = {
    "unproject forward": 2.5e-7,
    "unproject backward": 1.5e-7,
    "splat backward": 1.7e-7,
    "blur forward": 1.6e-7,
    "blur adjoint": 1.7e-7,
    "tap gradient": 1.7e-6,
    "smooth output": 8.5e-8,
    "smooth voxel gradient": 1.3e-7,
    "smooth tap gradient": 1.2e-7,
}
GATE = {group: 4 * e for group, e in E32.items()}


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _check(group, what, got, ref):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    assert got.shape == ref.shape
    err = G.rel_err(got, ref)
    print(f"{group} | {what}: rel_err {err:.2e} (gate {GATE[group]:.1e})")
    assert err <= GATE[group]


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- unproject ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.UNPROJECT_CASES, ids=str)
def test_unproject_forward_and_backward(case):
    ops = _ops()
    shape, intr, scale, norm = case
    consts = C.unproject_consts(intr, scale)
    depth, gpc = C.unproject_inputs(shape)
    pc = ops.unproject(depth.cuda(), consts, norm)
    gd = ops.unproject_bwd(depth.cuda(), gpc.cuda(), consts, norm)
    assert tuple(pc.shape) == (shape[0], shape[1] * shape[2], 3) and tuple(gd.shape) == shape
    _check("unproject forward", case, pc, R.unproject(depth.numpy(), consts, norm))
    _check("unproject backward", case, gd, R.unproject_bwd(gpc.numpy(), shape, consts, norm))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("intr", C.INTRINSICS)
@pytest.mark.parametrize("shape", [s for s in C.UNPROJECT_SHAPES if s[1] > 1], ids=str)
def test_unproject_nonfinite_depth_stays_in_its_pixels(shape, intr, norm):
    """One row of +inf and NaN depth: its points come out non-finite in every coordinate (u * z - cx * z is inf - inf or
    NaN), every other point is the bytes of the clean run, and the backward -- linear in gpc, the depth does not enter --
    stays finite and unchanged."""
    ops = _ops()
    consts = C.unproject_consts(intr, 1)
    depth, gpc = C.unproject_inputs(shape)
    B, Hi, Wi = shape
    bad = depth.clone()
    row = Hi // 2
    bad[B - 1, row, 0::2] = float("inf")
    bad[B - 1, row, 1::2] = float("nan")
    clean = ops.unproject(depth.cuda(), consts, norm).cpu().view(B, Hi, Wi, 3)
    got = ops.unproject(bad.cuda(), consts, norm).cpu().view(B, Hi, Wi, 3)
    hit = torch.zeros(B, Hi, Wi, dtype=torch.bool)
    hit[B - 1, row] = True
    assert not torch.isfinite(got[hit]).any()
    assert torch.isfinite(got[~hit]).all() and torch.equal(got[~hit], clean[~hit])
    gd = ops.unproject_bwd(bad.cuda(), gpc.cuda(), consts, norm)
    assert torch.isfinite(gd).all() and torch.equal(gd, ops.unproject_bwd(depth.cuda(), gpc.cuda(), consts, norm))


# ---- splat backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SPLAT_CASES, ids=str)
def test_splat_backward(case):
    ops = _ops()
    dims, B, N = case
    pts, gacc = C.splat_inputs(case)
    v_ref, b_ref, _ = P.splat_indices(pts, dims)
    valid_np, base_np, _ = R.splat_decisions(pts.numpy(), dims)
    assert np.array_equal(valid_np, v_ref.numpy()) and np.array_equal(base_np[valid_np], b_ref.numpy()[valid_np])
    # before the backward launch: the kernels' integer decisions are the oracle's, bit for bit
    _, base, valid = ops.splat_fwd(pts.cuda(), dims, want_indices=True)
    assert torch.equal(valid.cpu().bool(), v_ref)
    assert torch.equal(base.cpu().long()[v_ref], b_ref[v_ref])
    assert int((~v_ref).sum()) >= 7
    gp = ops.splat_bwd(pts.cuda(), gacc.cuda(), dims).cpu()
    assert tuple(gp.shape) == (B, N, 3)
    _check("splat backward", case, gp, R.splat_bwd(pts.numpy(), gacc.numpy(), dims))
    assert bool((gp[~v_ref] == 0.0).all())                        # invalid points (NaN ones too): exactly 0, never NaN
    for a in range(3):
        if dims[a] == 1:
            assert bool((gp[..., a] == 0.0).all())                # a size-1 axis has no gradient


# ---- clamp(scale * x, 0, 1), bit for bit --------------------------------------------------------------------------------
def _equal_with_nan(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan])


@pytest.mark.parametrize("case", C.CLAMP_CASES, ids=str)
def test_scale_clamp01_is_torch_clamp_bit_for_bit(case):
    """Forward and backward against float32 torch on the CPU.  NaN is loud: the forward returns NaN for NaN (fminf / fmaxf
    alone would return 0 and hide a NaN sigma behind an empty grid), the backward 0, as torch.clamp does.  (torch.equal
    calls NaN unequal to itself, so the NaN positions are compared as a mask and the other elements with torch.equal.)"""
    ops = _ops()
    scale, n = case
    x, gout = C.clamp_inputs(case)
    xr = x.clone().requires_grad_(True)
    want = (xr * scale).clamp(0, 1)
    (gwant,) = torch.autograd.grad(want, xr, gout)
    want = want.detach()
    out = ops.scale_clamp01(x.cuda(), scale).cpu()
    gin = ops.scale_clamp01_bwd(x.cuda(), gout.cuda(), scale).cpu()
    assert int(torch.isnan(want).sum()) == (1 if n > C.CLAMP_NAN_AT else 0) and not torch.isnan(gwant).any()
    bad = (~torch.isnan(want)) & (out != want)
    print(f"clamp {case}: {int(bad.sum())} forward elements differ, NaN out {int(torch.isnan(out).sum())} "
          f"(torch {int(torch.isnan(want).sum())}), {int((gin != gwant).sum())} backward elements differ")
    assert _equal_with_nan(out, want)
    assert torch.equal(gin, gwant)
    assert torch.equal(gin, torch.from_numpy(R.scale_clamp01_bwd(x.numpy(), gout.numpy(), scale)))
    if n > C.CLAMP_NAN_AT:
        assert torch.isnan(out[C.CLAMP_NAN_AT]) and gin[C.CLAMP_NAN_AT] == 0.0


def test_ordered_splat_vox_is_loud_like_the_clamp_kernel():
    """vox of the ordered splat is svr_scale_clamp01_fwd's arithmetic from the same kernel: the same bytes on a crowded
    cloud (values below, inside and above the clamp's interval)."""
    ops = _ops()
    case = C.SPLAT_CASES[-1]
    pts, _ = C.splat_inputs(case)
    acc, _, _, vox = ops.splat_fwd(pts.cuda(), case[0], ordered=True, want_vox=True)
    assert float(acc.max()) * 8.0 > 1.0 > float(acc.min()) * 8.0
    assert _bytes_equal(vox, ops.scale_clamp01(acc, 8.0))


# ---- blur, one axis at a time -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("case", C.BLUR_CASES, ids=str)
def test_blur_axis_forward_adjoint_and_tap_gradient(case, ordered):
    ops = _ops()
    B, dims, K = case
    x, gout, taps = (t.cuda() for t in C.blur_inputs(case))
    for axis in range(3):
        fwd, adj, gt_ref = C.blur_reference(case, axis)
        tag = f"{case} axis {axis} ordered {ordered}"
        _check("blur forward", tag, ops.blur_axis(x, taps, axis), fwd)
        gin, gt = ops.blur_axis_bwd(x, taps, gout, axis, ordered=ordered)
        assert gt.dtype == torch.float64 and tuple(gt.shape) == (K,)
        _check("blur adjoint", tag, gin, adj)
        _check("tap gradient", tag, gt, gt_ref)
        gin_only, none = ops.blur_axis_bwd(x, taps, gout, axis, want_gtaps=False, ordered=ordered)
        assert none is None and _bytes_equal(gin_only, gin)
        none, gt_only = ops.blur_axis_bwd(x, taps, gout, axis, want_gin=False, ordered=ordered)
        assert none is None and gt_only.dtype == torch.float64
        if ordered:
            assert _bytes_equal(gt_only, gt)                      # a fixed order: identical bytes, run to run
        else:
            _check("tap gradient", tag + " want_gin=False", gt_only, gt_ref)


# ---- project.voxels_smooth: which taps on which axis, and the .float() of the tap gradients ------------------------------
def test_voxels_smooth_wiring():
    import svr_amd  # noqa: F401
    from svr_amd.model import project
    x, cot, ks = C.smooth_inputs()
    xr = x.double().requires_grad_(True)
    kr = [k.double().requires_grad_(True) for k in ks]
    ref = P.voxels_smooth(xr, kr)
    before_clamp = R.blur_axis(R.blur_axis(R.blur_axis(x.numpy(), ks[0].numpy(), 2), ks[1].numpy(), 1), ks[2].numpy(), 0)
    assert before_clamp.min() > 0.0 and before_clamp.max() < 1.0   # the final clamp is inert on this input
    gref = torch.autograd.grad(ref, [xr] + kr, cot.double())
    mod = project(C.SMOOTH_SHAPE[1:], C.SMOOTH_KS, [1.0, 1.0, 1.0]).cuda()
    xg = x.cuda().requires_grad_(True)
    kg = [k.cuda().requires_grad_(True) for k in ks]
    out = mod.voxels_smooth(xg, kg)
    got = torch.autograd.grad(out, [xg] + kg, cot.cuda())
    assert all(g.dtype == torch.float32 for g in got)
    _check("smooth output", C.SMOOTH_SHAPE, out, ref.detach().numpy())
    _check("smooth voxel gradient", C.SMOOTH_SHAPE, got[0], gref[0].numpy())
    _check("smooth tap gradient", C.SMOOTH_KS, torch.cat(got[1:]), torch.cat(gref[1:]).numpy())
