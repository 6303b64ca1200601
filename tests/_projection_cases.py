"""Cases and seeded inputs shared by tests/test_projection_f64_cpu.py (which measures the gates on them) and
tests/test_gpu_projection_kernels.py (which runs the kernels on them).  CPU generators only; every input is float32, as the
kernels receive it.  The float64 references of the blur cases are computed once and shared (blur_reference)."""
import functools

import numpy as np
import torch

from tests import projection_f64 as R

# ---- unproject ----------------------------------------------------------------------------------------------------------
UNPROJECT_SHAPES = [(1, 1, 1), (2, 17, 33), (1, 240, 320)]
INTRINSICS = ["default", "f300"]
UNPROJECT_CASES = [(shape, intr, scale, norm) for shape in UNPROJECT_SHAPES for intr in INTRINSICS for scale in (1, 2)
                   for norm in (False, True)]


def intrinsic(name):
    if name == "default":
        return None
    f, cx, cy = 300.5, 150.25, 130.75
    return torch.tensor([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)


def unproject_consts(intr, scale):
    """The 12 constants the kernel receives (project._consts) for the frustum grid of this intrinsic and scale."""
    import svr_amd  # noqa: F401
    from svr_amd.model import project
    from svr_amd.model.projection import _camera_to_grid
    K = intrinsic(intr)
    dims, _, _ = _camera_to_grid(K if K is not None else project.get_intrinsic(), scale)
    mod = project([int(d) for d in dims], (3, 3, 3), [1.0, 1.0, 1.0], intrinsic=K)
    return mod._consts(scale)


def unproject_inputs(shape):
    g = torch.Generator().manual_seed(1100 + shape[1])
    depth = torch.rand(*shape, generator=g) * 5 + 0.5
    gpc = torch.randn(shape[0], shape[1] * shape[2], 3, generator=g)
    return depth, gpc


# ---- splat backward -----------------------------------------------------------------------------------------------------
SPLAT_CASES = [((5, 6, 7), 2, 700), ((2, 2, 2), 2, 257), ((1, 4, 5), 2, 300), ((35, 26, 28), 1, 1000),
               ((5, 4, 6), 2, 300)]          # the last one: _crowded_points() of test_gpu_scene_deterministic.py itself
N_SPECIAL = 40


def _specials(dims):
    """(N_SPECIAL, 3): the special rows of _crowded_points() -- NaN, +-0.5, +-0.4999995 (outside 0.5 - 1e-6), far outside, one
    point 17 times -- and points exactly on lattice nodes (k / (D - 1) - 0.5; exact in float32 where D - 1 is a power of two,
    so r = 0 exactly there)."""
    nan = float("nan")
    rows = [[0.5, 0.0, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, 0.4999995], [-0.4999995, 0.0, 0.0], [0.7, 0.2, -0.9],
            [nan, 0.0, 0.0], [0.0, nan, nan], [-0.5, 0.1, 0.1], [0.1, 0.4999995, 0.1], [1e30, 0.0, 0.0], [0.0, -3.0e9, 0.0]]
    rows += [[0.1234, -0.2345, 0.3456]] * 17
    node = lambda k, D: (k / (D - 1) - 0.5) if D > 1 else 0.0
    for k in (1, 2, 3):
        a = [node(min(k, max(D - 2, 0)), D) for D in dims]
        rows += [a, [a[0], 0.05, -0.05], [0.05, a[1], a[2]]]
    rows += [[0.0, 0.0, 0.0]] * (N_SPECIAL - len(rows))
    assert len(rows) == N_SPECIAL
    return torch.tensor(rows, dtype=torch.float32)


def splat_inputs(case):
    dims, B, N = case
    g = torch.Generator().manual_seed(1200 + SPLAT_CASES.index(case))
    if case == SPLAT_CASES[-1]:
        from tests.test_gpu_scene_deterministic import _crowded_points
        pts = _crowded_points()
        assert tuple(pts.shape) == (B, N, 3)
        pts[1, 20:29] = _specials(dims)[28:37]              # the lattice nodes: D0 = 5 has k / 4 - 0.5
    else:
        pts = (torch.rand(B, N, 3, generator=g) - 0.5) * 1.1
        pts[B - 1, 3:3 + N_SPECIAL] = _specials(dims)
    gacc = torch.randn(B, *dims, generator=g)
    return pts.contiguous(), gacc


# ---- clamp --------------------------------------------------------------------------------------------------------------
CLAMP_CASES = [(scale, n) for scale in (8.0, 1.0) for n in (1, 255, 257, 1000)]
CLAMP_NAN_AT = 12                                         # position of the NaN in clamp_edges (n > 12 has it)


def clamp_edges(scale):
    """0, -0.0, 1 / scale, the float32 neighbours of 0 and of 1 / scale on both sides, +-inf, NaN."""
    f = np.float32
    one = f(1.0) / f(scale)
    e = [f(0.0), f(-0.0), one, np.nextafter(f(0.0), f(1.0)), np.nextafter(f(0.0), f(-1.0)), np.nextafter(one, f(2.0)),
         np.nextafter(one, f(0.0)), f(np.finfo(f).tiny), -f(np.finfo(f).tiny), f(np.inf), f(-np.inf), f(0.5) / f(scale),
         f(np.nan)]
    assert len(e) == CLAMP_NAN_AT + 1
    return torch.from_numpy(np.array(e, dtype=f))


def clamp_inputs(case):
    """x: random values around [0, 1 / scale] with the edge values written over the first elements (n = 1: the value is
    1 / scale, a bound).  gout: randn."""
    scale, n = case
    g = torch.Generator().manual_seed(1300 + n)
    x = (torch.rand(n, generator=g) * 2.0 - 0.5) / scale
    e = clamp_edges(scale)
    if n == 1:
        x[0] = e[2]
    else:
        x[:e.numel()] = e
    return x, torch.randn(n, generator=g)


# ---- blur ---------------------------------------------------------------------------------------------------------------
BLUR_CASES = ([(2, (5, 4, 6), K) for K in (1, 3, 5, 15)] + [(1, (1, 1, 1), 3)] + [(3, (9, 17, 33), K) for K in (3, 11)]
              + [(1, (70, 52, 56), K) for K in (9, 11)] + [(1, (129, 128, 128), 3)])


# The tap gradient is a sum of zero-mean terms gout * x: its size is a matter of luck (standard deviation sqrt(n / 3)) while
# the rounding error of ANY float32 summation grows with n.  The seeds of the small K = 1 case and of the cases above 10^5
# elements are chosen so that the centre tap's sum (the same on every axis) is a large one, above BLUR_CENTRE_SIGMAS
# standard deviations: little cancellation, a well-conditioned sum.  (test_projection_f64_cpu.py asserts it.)
BLUR_SEEDS = {(2, (5, 4, 6), 1): 1523, (1, (70, 52, 56), 9): 2094, (1, (70, 52, 56), 11): 2094, (1, (129, 128, 128), 3): 2058}
BLUR_CENTRE_SIGMAS = 2.6


def blur_inputs(case):
    """x = rand, gout = randn, taps = softmax(randn(K)): asymmetric, so a missing flip or a negated offset shows."""
    B, dims, K = case
    g = torch.Generator().manual_seed(BLUR_SEEDS.get(case, 1400 + BLUR_CASES.index(case)))
    x = torch.rand(B, *dims, generator=g)
    gout = torch.randn(B, *dims, generator=g)
    taps = torch.softmax(torch.randn(K, generator=g), 0)
    return x, gout, taps


@functools.lru_cache(maxsize=2)
def blur_reference(case, axis):
    """(forward, adjoint, tap gradient) in float64; computed once per (case, axis), not to be written to."""
    x, gout, taps = (t.numpy() for t in blur_inputs(case))
    ref = (R.blur_axis(x, taps, axis), R.blur_axis_adjoint(gout, taps, axis), R.blur_taps_grad(x, gout, len(taps), axis))
    for a in ref:
        a.setflags(write=False)
    return ref


# ---- project.voxels_smooth ----------------------------------------------------------------------------------------------
SMOOTH_SHAPE, SMOOTH_KS = (2, 6, 5, 9), (3, 5, 7)


def smooth_inputs():
    """x in (0.05, 0.95): with taps that sum to 1 the blurred grid stays inside (0, 1) and the final clamp is inert."""
    g = torch.Generator().manual_seed(1500)
    x = 0.05 + 0.9 * torch.rand(*SMOOTH_SHAPE, generator=g)
    cot = torch.randn(*SMOOTH_SHAPE, generator=g)
    ks = [torch.softmax(torch.randn(K, generator=g), 0) for K in SMOOTH_KS]
    return x, cot, ks
