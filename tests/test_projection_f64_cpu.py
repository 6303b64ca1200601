"""CPU: ties the numpy float64 references of tests/projection_f64.py to what the project already trusts, measures the gates
of tests/test_gpu_projection_kernels.py and shows that the inputs of tests/_projection_cases.py tell right from wrong.

  1. every reference equals float64 autograd of the stock-torch restatement (the formulas of oracle/projection_oracle.py,
     F.conv3d per axis for the blur) to 1e-12, on every case whose axes are all >= 2 (the restatement cannot index a
     size-1 axis; those cases are compared with the same references on the GPU under the group's gate);
  2. e32 = G.rel_err of the SAME restatement in float32 against the reference; per group its maximum over the cases must stay
     at or below the value recorded in test_gpu_projection_kernels.E32, and no gate (4 * e32) may exceed 1e-5;
  3. every wrong variant of projection_f64 lies at least 100 gates away from the true reference on every case of its group
     on which it CAN differ (the others are listed below and must give the true result exactly).

The float32 restatement runs on one thread, so its summation order does not depend on the machine's core count.
Figures are printed before they are asserted (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import projection_oracle as P
from tests import _golden as G
from tests import _projection_cases as C
from tests import projection_f64 as R
from tests.test_gpu_projection_kernels import E32, GATE

F64_AGREE = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _np(t):
    return t.detach().numpy()


def _leaf(t, dtype):
    """A fresh leaf in `dtype` (never the shared input itself: .to() of the same dtype returns its argument)."""
    return t.detach().clone().to(dtype).requires_grad_(True)


# ---- stock-torch restatements, in `dtype` -------------------------------------------------------------------------------
def t_unproject(depth, consts, normalize, dtype):
    """oracle.depthmap_to_gridspace (+ norm_grid_space) with the kernel's 12 constants: the 4x4 product written out (its
    off-diagonal terms are zeros)."""
    f, cx, cy, s00, t0, s11, t1, s22, t2, d0, d1, d2 = (torch.tensor(float(np.float32(v)), dtype=dtype) for v in consts)
    depth = depth.to(dtype)
    B, Hi, Wi = depth.shape
    v, u = torch.meshgrid(torch.arange(Hi), torch.arange(Wi), indexing="ij")
    X = (torch.multiply(u, depth) - cx * depth) / f
    Y = -((torch.multiply(v, depth) - cy * depth) / f)
    pc = torch.stack([s00 * X + t0, s11 * Y + t1, s22 * depth + t2], dim=-1).reshape(B, -1, 3)
    if normalize:
        d = torch.stack([d0, d1, d2])
        pc = (pc - d / 2) / d
    return pc


def t_unproject_both(depth, gpc, consts, normalize, dtype):
    d = _leaf(depth, dtype)
    out = t_unproject(d, consts, normalize, dtype)
    (gd,) = torch.autograd.grad(out, d, gpc.to(dtype))
    return _np(out), _np(gd)


def t_splat_acc(pts, dims, dtype, p):
    """oracle.pc_voxels up to its accumulated tensor (before the x8 and the clamp), as a function of the leaf `p`.  valid and
    the base voxel come from oracle.splat_indices on the float32 points; in float64, g carries the VALUE of the float32
    product (the integer decisions and the remainders are defined on it) and the derivative of (p + 0.5) * (D - 1)."""
    B, N, _ = pts.shape
    d0, d1, d2 = dims
    valid, base, g32 = P.splat_indices(pts, dims)
    g = (p + 0.5) * (torch.as_tensor(dims) - 1)
    if dtype != torch.float32:
        g = g + (g32.to(dtype) - g).detach()
    r = g - g.floor()
    w01 = (1.0 - r, r)
    acc = p.new_zeros(B * d0 * d1 * d2)
    b = torch.arange(B)[:, None].expand(B, N)
    vflat = valid.reshape(-1)
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                w = w01[k][..., 0] * w01[j][..., 1] * w01[i][..., 2]
                lin = ((b * d0 + base[..., 0] + k) * d1 + base[..., 1] + j) * d2 + base[..., 2] + i
                acc = acc.index_add(0, lin.reshape(-1)[vflat], w.reshape(-1)[vflat])
    return acc.view(B, d0, d1, d2)


def t_splat_bwd(pts, gacc, dims, dtype):
    p = _leaf(pts, dtype)
    acc = t_splat_acc(pts, dims, dtype, p)
    (gp,) = torch.autograd.grad(acc, p, gacc.to(dtype))
    return _np(gp), acc.detach()


def t_blur(x, gout, taps, axis, dtype):
    """One axis of oracle.voxels_smooth: grouped F.conv3d with zero padding K / 2; gin and gtaps by autograd."""
    B, K = x.shape[0], taps.numel()
    xv = _leaf(x.unsqueeze(0), dtype)
    k = _leaf(taps, dtype)
    shp, pad = [1, 1, 1, 1, 1], [0, 0, 0]
    shp[2 + axis], pad[axis] = -1, K // 2
    out = F.conv3d(xv, k.view(shp).repeat(B, 1, 1, 1, 1), stride=1, padding=pad, groups=B)
    gin, gt = torch.autograd.grad(out, (xv, k), gout.to(dtype).unsqueeze(0))
    return _np(out.squeeze(0)), _np(gin.squeeze(0)), _np(gt)


def t_smooth(x, cot, ks, dtype):
    xv = _leaf(x, dtype)
    kk = [_leaf(k, dtype) for k in ks]
    out = P.voxels_smooth(xv, kk)
    grads = torch.autograd.grad(out, [xv] + kk, cot.to(dtype))
    return _np(out), _np(grads[0]), np.concatenate([_np(g) for g in grads[1:]])


# ---- the measurement: {group: [(case, e64, e32, {variant: distance or None})]} ------------------------------------------
def _restatable(dims):
    return min(dims) >= 2


@pytest.fixture(scope="module")
def measured(_one_thread):
    M = {g: [] for g in E32}

    def add(group, case, ref, r64, r32, wrong=None):
        M[group].append((case, G.rel_err(r64, ref), G.rel_err(r32, ref),
                         {n: (None if w is None else G.rel_err(w, ref)) for n, w in (wrong or {}).items()}))

    for case in C.UNPROJECT_CASES:
        shape, intr, scale, norm = case
        consts = C.unproject_consts(intr, scale)
        depth, gpc = C.unproject_inputs(shape)
        o64, g64 = t_unproject_both(depth, gpc, consts, norm, torch.float64)
        o32, g32 = t_unproject_both(depth, gpc, consts, norm, torch.float32)
        add("unproject forward", case, R.unproject(depth.numpy(), consts, norm), o64, o32)
        wrong = R.wrong_unproject_bwd_uv_exchanged(gpc.numpy(), shape, consts, norm)
        add("unproject backward", case, R.unproject_bwd(gpc.numpy(), shape, consts, norm), g64.reshape(shape),
            g32.reshape(shape), {"u and v exchanged": None if shape[1:] == (1, 1) else wrong})
        if shape[1:] == (1, 1):                                   # pixel (0, 0): nothing to exchange
            assert np.array_equal(wrong, R.unproject_bwd(gpc.numpy(), shape, consts, norm))

    for case in C.SPLAT_CASES:
        dims = case[0]
        if not _restatable(dims):
            continue
        pts, gacc = C.splat_inputs(case)
        g64, _ = t_splat_bwd(pts, gacc, dims, torch.float64)
        g32, acc32 = t_splat_bwd(pts, gacc, dims, torch.float32)
        # a NaN point: autograd multiplies its zero cotangent with its NaN weights and returns NaN, there and nowhere else;
        # the kernel (and the reference) route the point to "invalid" first and return exactly 0
        nan_rows = torch.isnan(pts).any(-1).numpy()
        for gr in (g64, g32):
            assert np.array_equal(~np.isfinite(gr).all(-1), nan_rows)
            gr[nan_rows] = 0.0
        assert torch.equal((8.0 * acc32).clamp(0, 1), P.pc_voxels(pts, dims))      # the restatement IS the oracle's splat
        p, ga = pts.numpy(), gacc.numpy()
        same = len(set(dims)) == 1                                                # (2, 2, 2): every factor is 1
        wrong = {"factors exchanged": R.wrong_splat_bwd_factors_exchanged(p, ga, dims),
                 "factor left out": R.wrong_splat_bwd_no_factor(p, ga, dims)}
        ref = R.splat_bwd(p, ga, dims)
        if same and set(dims) == {2}:
            assert all(np.array_equal(w, ref) for w in wrong.values())
            wrong = {n: None for n in wrong}
        add("splat backward", case, ref, g64, g32, wrong)

    for case in C.BLUR_CASES:
        B, dims, K = case
        x, gout, taps = C.blur_inputs(case)
        for axis in range(3):
            if not _restatable(dims):
                continue
            fwd, adj, gt = C.blur_reference(case, axis)
            o64, a64, t64 = t_blur(x, gout, taps, axis, torch.float64)
            o32, a32, t32 = t_blur(x, gout, taps, axis, torch.float32)
            ca = case + (axis,)
            flip = R.wrong_blur_axis_adjoint_no_flip(gout.numpy(), taps.numpy(), axis)
            neg = R.wrong_blur_taps_grad_negated(x.numpy(), gout.numpy(), K, axis)
            if K == 1:                                            # one tap: no flip, no offset
                assert np.array_equal(flip, adj) and np.array_equal(neg, gt)
                flip = neg = None
            add("blur forward", ca, fwd, o64, o32)
            add("blur adjoint", ca, adj, a64, a32, {"no tap flip": flip})
            add("tap gradient", ca, gt, t64, t32, {"offset negated": neg})

    x, cot, ks = C.smooth_inputs()
    ref = t_smooth(x, cot, ks, torch.float64)
    r32 = t_smooth(x, cot, ks, torch.float32)
    rev = t_smooth(x, cot, ks[::-1], torch.float64)               # ks[0] on the FIRST axis instead of the last
    # the float64 autograd of oracle.voxels_smooth is the reference of this group; the numpy functions reproduce it
    k0, k1, k2 = (k.numpy() for k in ks)
    a1 = R.blur_axis(x.numpy(), k0, 2)
    a2 = R.blur_axis(a1, k1, 1)
    a3 = R.blur_axis(a2, k2, 0)
    assert a3.min() > 0.0 and a3.max() < 1.0                      # the final clamp is inert
    g2 = R.blur_axis_adjoint(cot.numpy(), k2, 0)
    g1 = R.blur_axis_adjoint(g2, k1, 1)
    g0 = R.blur_axis_adjoint(g1, k0, 2)
    gt = np.concatenate([R.blur_taps_grad(x.numpy(), g1, len(k0), 2), R.blur_taps_grad(a1, g2, len(k1), 1),
                         R.blur_taps_grad(a2, cot.numpy(), len(k2), 0)])
    add("smooth output", C.SMOOTH_SHAPE, ref[0], a3, r32[0], {"kernels reversed": rev[0]})
    add("smooth voxel gradient", C.SMOOTH_SHAPE, ref[1], g0, r32[1], {"kernels reversed": rev[1]})
    add("smooth tap gradient", C.SMOOTH_SHAPE, ref[2], gt, r32[2])
    return M


def test_every_group_is_measured_on_every_restatable_case(measured):
    n_blur = 3 * sum(1 for c in C.BLUR_CASES if _restatable(c[1]))
    want = {"unproject forward": len(C.UNPROJECT_CASES), "unproject backward": len(C.UNPROJECT_CASES),
            "splat backward": sum(1 for c in C.SPLAT_CASES if _restatable(c[0])), "blur forward": n_blur,
            "blur adjoint": n_blur, "tap gradient": n_blur, "smooth output": 1, "smooth voxel gradient": 1,
            "smooth tap gradient": 1}
    assert {g: len(v) for g, v in measured.items()} == want
    assert [c for c in C.SPLAT_CASES if not _restatable(c[0])] == [((1, 4, 5), 2, 300)]
    assert [c for c in C.BLUR_CASES if not _restatable(c[1])] == [(1, (1, 1, 1), 3)]


@pytest.mark.parametrize("group", sorted(E32))
def test_reference_equals_float64_autograd(measured, group):
    for case, e64, _, _ in measured[group]:
        print(f"{group} {case}: float64 autograd against the numpy reference {e64:.2e}")
    assert max(e64 for _, e64, _, _ in measured[group]) <= F64_AGREE


@pytest.mark.parametrize("group", sorted(E32))
def test_e32_is_reproduced_and_the_gate_is_tight(measured, group):
    for case, _, e32, _ in measured[group]:
        print(f"{group} {case}: e32 {e32:.2e}")
    e32 = max(e for _, _, e, _ in measured[group])
    print(f"{group}: e32 {e32:.3e} (recorded {E32[group]:.1e}), gate {GATE[group]:.1e}")
    assert GATE[group] == 4 * E32[group]
    assert e32 <= E32[group]
    assert GATE[group] <= 1e-5                                     # above: an ill-conditioned input; change the input


@pytest.mark.parametrize("group", sorted(E32))
def test_wrong_variants_are_100_gates_away(measured, group):
    seen = 0
    for case, _, _, wrong in measured[group]:
        for name, dist in wrong.items():
            if dist is None:
                continue
            seen += 1
            print(f"{group} {case}: '{name}' is {dist:.2e} = {dist / GATE[group]:.0f} gates away")
            assert dist >= 100 * GATE[group]
    assert seen > 0 or group in ("unproject forward", "blur forward", "smooth tap gradient")


def test_unproject_restatement_is_the_oracle_at_the_default_intrinsics():
    """t_unproject writes the oracle's 4x4 product out; at the oracle's own intrinsics both give the same float32 points
    (to the rounding of the product's summation order)."""
    for scale in (1, 2):
        consts = C.unproject_consts("default", scale)
        dims = [int(v) for v in consts[9:]]
        assert dims == [int(v) for v in P.camera_to_grid(scale)[0]]
        for shape in C.UNPROJECT_SHAPES:
            depth, _ = C.unproject_inputs(shape)
            want = P.depthmap_to_gridspace(depth, scale)
            assert G.rel_err(_np(t_unproject(depth, consts, False, torch.float32)), _np(want)) < 5e-7
            assert G.rel_err(_np(t_unproject(depth, consts, True, torch.float32)), _np(P.norm_grid_space(want, dims))) < 5e-7


def test_splat_reference_decisions_and_zero_rows():
    """valid / base of the reference are the oracle's; invalid rows and the size-1 axis give exactly 0; the special points
    are where the case says they are."""
    for case in C.SPLAT_CASES:
        dims = case[0]
        pts, gacc = C.splat_inputs(case)
        valid, base, _ = R.splat_decisions(pts.numpy(), dims)
        v_ref, b_ref, _ = P.splat_indices(pts, dims)
        assert np.array_equal(valid, v_ref.numpy()) and np.array_equal(base[valid], b_ref.numpy()[valid])
        assert (~valid).sum() >= 7 and np.isnan(pts.numpy()).any()
        gp = R.splat_bwd(pts.numpy(), gacc.numpy(), dims)
        assert np.all(gp[~valid] == 0.0) and np.isfinite(gp).all()
        for a in range(3):
            if dims[a] == 1:
                assert np.all(gp[..., a] == 0.0)
            else:
                assert np.abs(gp[..., a]).max() > 0.0
        if dims[0] == 5:                                          # k / 4 - 0.5: exactly on a lattice node, r = 0
            _, _, g = R.splat_decisions(pts.numpy(), dims)
            assert ((g[..., 0] == np.floor(g[..., 0])) & valid & (g[..., 0] > 0)).sum() >= 3


def test_large_tap_gradient_sums_are_well_conditioned():
    for case in C.BLUR_SEEDS:
        x, gout, _ = C.blur_inputs(case)
        centre = float((x.double() * gout.double()).sum())
        sigma = (x.numel() / 3.0) ** 0.5
        print(f"{case}: centre tap sum {centre:.1f} = {centre / sigma:.2f} standard deviations")
        assert abs(centre) >= C.BLUR_CENTRE_SIGMAS * sigma
    assert all(case in C.BLUR_SEEDS for case in C.BLUR_CASES if case[0] * np.prod(case[1]) > 1e5)


@pytest.mark.parametrize("case", C.CLAMP_CASES)
def test_clamp_reference_is_torch_bit_for_bit(case):
    scale, n = case
    x, gout = C.clamp_inputs(case)
    xr = x.clone().requires_grad_(True)
    out = (xr * scale).clamp(0, 1)
    (gin,) = torch.autograd.grad(out, xr, gout)
    ref = torch.from_numpy(R.scale_clamp01_bwd(x.numpy(), gout.numpy(), scale))
    assert torch.equal(ref, gin)
    v = x * scale
    at_bound = (v == 0) | (v == 1)
    assert at_bound.sum() >= (1 if n == 1 else 3)
    wrong = torch.from_numpy(R.wrong_scale_clamp01_bwd_exclusive(x.numpy(), gout.numpy(), scale))
    assert torch.equal(wrong != ref, at_bound & (gout != 0))      # wrong at the bounds and nowhere else
    if n > C.CLAMP_NAN_AT:
        assert torch.isnan(x[C.CLAMP_NAN_AT]) and torch.isnan(out[C.CLAMP_NAN_AT]) and gin[C.CLAMP_NAN_AT] == 0
        assert int(torch.isnan(out).sum()) == 1
