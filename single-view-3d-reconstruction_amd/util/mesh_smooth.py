"""Taubin lambda|mu smoothing of a triangle mesh on the device (csrc/mesh_smooth.hip; the rule is in include/svr_hip.h, the
design in DESIGN.md section 24, the numpy restatement in tests/mesh_smooth_oracle.py).

``smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, strict=True) -> SmoothedMesh``: every
iteration moves each vertex by `lam` towards the mean of its face neighbours and then by `mu` (negative: away from it), which
takes the terraces out of a marching-cubes surface without shrinking it the way plain Laplacian smoothing (`mu` = 0) does.
With `fix_boundary` the vertices on an open rim (where the lattice border cut the surface) stay where they are.  The faces
are not touched, so every per-vertex attribute keeps its index.

Every output is the same bits on every run: the iteration is integer arithmetic on 2^-16 fixed point.  There is no CPU
fallback: CPU tensors raise, like every other op."""
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream

MAX_ITERATIONS = 1024
MOVABLE, ISOLATED, FIXED, BAD = 0, 1, 2, 3


@dataclass
class SmoothedMesh:
    """`vertices` (V, 3) float32 and `state` (V,) uint8 on the device (0 moved, 1 in no valid face, 2 held on a boundary, 3 not
    usable: a coordinate that is not finite or not below 2^16 in magnitude; only state 0 changes position), and the number of
    vertices in each state: `moved`, `isolated`, `fixed`, `bad`."""
    vertices: torch.Tensor
    state: torch.Tensor
    moved: int
    isolated: int
    fixed: int
    bad: int


def _device(t, what, dtype):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mesh_smooth HIP path needs GPU tensors (no CPU fallback): {what}")
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"mesh_smooth: {what} must be (N, 3) {str(dtype).replace('torch.', '')}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _weight(value, what, lo, hi):
    """The library's own test (rint of the float32 times 2^16 inside [lo, hi]), so that a bad weight raises before any tensor is looked at."""
    with np.errstate(invalid="ignore", over="ignore"):
        L = np.rint(np.float64(np.float32(value)) * 65536.0)
    if not lo <= L <= hi:
        raise ValueError(f"mesh_smooth: {what}={value} (need {'0 < lam <= 1' if what == 'lam' else '-1 <= mu <= 0'} after rounding to 2^-16)")
    return float(np.float32(value))


def smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, strict=True):
    """`vertices` (V, 3) float32 and `faces` (F, 3) int32 on the device (F <= 2^28); 0 <= `iterations` <= 1024 (0: the identity,
    the states are still computed); 0 < `lam` <= 1; -1 <= `mu` <= 0.  With `strict` an unusable vertex raises ValueError naming
    the count; without, such vertices and their faces take no part and are counted in `bad`.  Reading the four counts is the
    one host synchronisation; the library call itself makes none."""
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"mesh_smooth: iterations={iterations} (need an integer, 0 <= iterations <= {MAX_ITERATIONS})")
    lam, mu = _weight(lam, "lam", 1, 65536), _weight(mu, "mu", -65536, 0)
    v = _device(vertices, "vertices", torch.float32)
    f = _device(faces, "faces", torch.int32)
    V, F = int(v.shape[0]), int(f.shape[0])
    l = _lib.lib()
    dev = v.device
    ws_bytes = int(l.svr_mesh_smooth_workspace_bytes(V, F))
    if ws_bytes < 0:
        check(ws_bytes, "mesh_smooth_workspace_bytes")
    ws = torch.empty(ws_bytes if V and F else 0, device=dev, dtype=torch.uint8)
    out = torch.empty((V, 3), device=dev, dtype=torch.float32)
    state = torch.empty(V, device=dev, dtype=torch.uint8)
    counts = torch.empty(4, device=dev, dtype=torch.int64)
    check(l.svr_mesh_smooth(ptr(v), V, ptr(f), F, int(iterations), lam, mu, int(bool(fix_boundary)), ptr(ws), ws_bytes, ptr(out),
                            ptr(state), ptr(counts), stream()), "mesh_smooth")
    moved, isolated, fixed, bad = counts.tolist()
    if strict and bad:
        raise ValueError(f"mesh_smooth: {bad} of {V} vertices are not usable (a coordinate is not finite or not below 2^16 in "
                         "magnitude); strict=False leaves them and their faces out")
    return SmoothedMesh(out, state, int(moved), int(isolated), int(fixed), int(bad))
