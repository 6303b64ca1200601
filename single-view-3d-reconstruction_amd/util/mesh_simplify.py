"""Mesh simplification by vertex clustering on the device (csrc/mesh_simplify.hip; the rule is in include/svr_hip.h, the design
in DESIGN.md section 23, the numpy restatement in tests/mesh_simplify_oracle.py).

``simplify_mesh(vertices, faces, cell, strict=True, uniform_path=True) -> SimplifiedMesh``: the vertices that share a cube of
edge `cell` (floor(v / cell) per axis) become one vertex at their mean; faces that lose an edge that way, and all but the
first of the faces that end up on the same three vertices with the same orientation, are dropped, and so are the vertices no
face names any more.  `vertex_cluster` says where every input vertex went, so any per-vertex attribute can be pooled over it.
Every member moves by less than `cell` per axis.  A closed mesh can lose manifoldness where it is thinner than a cell.

Every output is the same bits on every run.  There is no CPU fallback: CPU tensors raise, like every other op."""
from dataclasses import dataclass

import torch

from .. import _lib
from .._lib import check, ptr, stream

CELL_MIN, CELL_MAX = 2.0 ** -10, 2.0 ** 16
E_INTERNAL = -7                                          # SVR_E_INTERNAL


@dataclass
class SimplifiedMesh:
    """`vertices` (V', 3) float32, `faces` (F', 3) int32, `vertex_cluster` (V,) int32 (the output vertex of each input vertex;
    -1: not clusterable, or its cluster is in no kept face), `cluster_size` (V',) int32, on the device; `bad`: how many input
    vertices were not clusterable (a coordinate that is not finite or not below 2^16 in magnitude)."""
    vertices: torch.Tensor
    faces: torch.Tensor
    vertex_cluster: torch.Tensor
    cluster_size: torch.Tensor
    bad: int


def _device(t, what, dtype):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mesh_simplify HIP path needs GPU tensors (no CPU fallback): {what}")
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"mesh_simplify: {what} must be (N, 3) {str(dtype).replace('torch.', '')}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def simplify_mesh(vertices, faces, cell, strict=True, uniform_path=True):
    """`vertices` (V, 3) float32 and `faces` (F, 3) int32 on the device; `cell` in the vertices' unit, 2^-10 <= cell <= 2^16
    after rounding to float32.  With `strict` an unclusterable vertex raises ValueError naming the count; without, such vertices
    and their faces are dropped and counted in `bad`.  `uniform_path=False` makes the sums kernel issue its atomics per lane
    (the same bits; tools/bench_mesh_simplify.py times both)."""
    v = _device(vertices, "vertices", torch.float32)
    f = _device(faces, "faces", torch.int32)
    V, F = int(v.shape[0]), int(f.shape[0])
    l = _lib.lib()
    dev = v.device
    ws_bytes = int(l.svr_mesh_simplify_workspace_bytes(V, F))
    if ws_bytes < 0:
        check(ws_bytes, "mesh_simplify_workspace_bytes")
    ws = torch.empty(ws_bytes if V and F else 0, device=dev, dtype=torch.uint8)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    check(l.svr_mesh_simplify_count(ptr(v), V, ptr(f), F, float(cell), ptr(ws), ws_bytes, int(bool(uniform_path)), ptr(totals), stream()),
          "mesh_simplify_count")
    nv, nf, bad = totals.tolist()                        # size the outputs: the one host synchronisation
    if nv == E_INTERNAL:
        raise RuntimeError("libsvr_hip mesh_simplify_count failed (SVR_E_INTERNAL): a hash set found no empty slot")
    if strict and bad:
        raise ValueError(f"mesh_simplify: {bad} of {V} vertices are not clusterable (a coordinate is not finite or not below "
                         "2^16 in magnitude); strict=False drops them and their faces")
    out_v = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    out_f = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    cluster = torch.empty(V, device=dev, dtype=torch.int32)
    size = torch.empty(nv, device=dev, dtype=torch.int32)
    check(l.svr_mesh_simplify_emit(ptr(v), V, ptr(f), F, ptr(ws), ws_bytes, ptr(out_v), ptr(out_f), ptr(cluster), ptr(size), stream()),
          "mesh_simplify_emit")
    return SimplifiedMesh(out_v, out_f, cluster, size, int(bad))
