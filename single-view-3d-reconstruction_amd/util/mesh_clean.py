"""Connected components of a mesh on the device: label them, measure them, drop some (csrc/mesh_components.hip; the rule
is in include/svr_hip.h, the design in DESIGN.md section 22, the numpy restatement in tests/mesh_components_oracle.py).

``mesh_components(vertices, faces, mark=None) -> MeshComponents``: two vertices are in one component iff a chain of valid
faces (all three indices in [0, V)) connects them; components are numbered by their smallest vertex index.  Per vertex and
per face a label, per component its root, vertex / face / marked-vertex counts and bounding box, all on the device; `count`
is a plain int (the one host synchronisation).
``select_components(comps, keep_largest=False, min_faces=0, min_extent=0.0, require_mark=False) -> (C,) bool``: the host's
choice over the C rows, read back once.
``filter_components(vertices, faces, comps, keep) -> (vertices, faces, vertex_index)``: the kept components' faces and the
vertices they use, in their old order, faces renumbered; any per-vertex attribute follows as ``attr[vertex_index]``.
``clean_mesh(vertices, faces, mark=None, **criteria) -> (vertices, faces, vertex_index, comps, keep)``: the three together.

Every output is the same bits on every run.  There is no CPU fallback: CPU tensors raise, like every other op."""
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream


@dataclass
class MeshComponents:
    """`vertex_label` (V,) and `face_label` (F,) int32 (-1: an invalid face); per component `root`, `vertex_count`,
    `face_count`, `marked_count` (C,) int32 and `bbox_min`, `bbox_max` (C, 3) float32; `count` = C."""
    vertex_label: torch.Tensor
    face_label: torch.Tensor
    root: torch.Tensor
    vertex_count: torch.Tensor
    face_count: torch.Tensor
    marked_count: torch.Tensor
    bbox_min: torch.Tensor
    bbox_max: torch.Tensor
    count: int


def _device(t, what, dtype, shape_text, ok):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mesh_components HIP path needs GPU tensors (no CPU fallback): {what}")
    if t.dtype != dtype or not ok(t):
        raise ValueError(f"mesh_components: {what} must be {shape_text} {str(dtype).replace('torch.', '')}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _mesh(vertices, faces):
    v = _device(vertices, "vertices", torch.float32, "(V, 3)", lambda t: t.dim() == 2 and t.shape[1] == 3)
    f = _device(faces, "faces", torch.int32, "(F, 3)", lambda t: t.dim() == 2 and t.shape[1] == 3)
    return v, f


def _workspace(l, V, F, device):
    ws_bytes = int(l.svr_mesh_components_workspace_bytes(V, F))
    if ws_bytes < 0:
        check(ws_bytes, "mesh_components_workspace_bytes")
    return torch.empty(ws_bytes, device=device, dtype=torch.uint8), ws_bytes


def mesh_components(vertices, faces, mark=None, uniform_path=True):
    """`vertices` (V, 3) float32, `faces` (F, 3) int32, `mark` (V,) uint8 or None, on the device.  `uniform_path=False`
    makes the statistics kernels issue their atomics per lane (the same bits; tools/bench_mesh_clean.py times both)."""
    v, f = _mesh(vertices, faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    m = None if mark is None else _device(mark, "mark", torch.uint8, f"({V},)", lambda t: tuple(t.shape) == (V,))
    l = _lib.lib()
    dev = v.device
    ws, ws_bytes = _workspace(l, V, F, dev)
    vertex_label = torch.empty(V, device=dev, dtype=torch.int32)
    face_label = torch.empty(F, device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int64)
    check(l.svr_mesh_components_label(ptr(f), F, V, ptr(ws), ws_bytes, ptr(vertex_label), ptr(face_label), ptr(count), stream()),
          "mesh_components_label")
    n = int(count.item())                                # sizes the statistics
    ints = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(4)]
    boxes = [torch.empty((n, 3), device=dev, dtype=torch.float32) for _ in range(2)]
    check(l.svr_mesh_components_stats(ptr(v), V, ptr(vertex_label), ptr(face_label), F, ptr(m), n, ptr(ws), ws_bytes,
                                      *(ptr(t) for t in ints + boxes), int(bool(uniform_path)), stream()), "mesh_components_stats")
    return MeshComponents(vertex_label, face_label, *ints, *boxes, n)


def select_rows(face_count, marked_count, bbox_min, bbox_max, keep_largest=False, min_faces=0, min_extent=0.0, require_mark=False):
    """The selection rule on host arrays -> (C,) numpy bool.  A component is kept iff face_count >= max(1, min_faces), its
    extent >= min_extent and, with `require_mark`, marked_count >= 1; with `keep_largest` only the one with the most faces
    among those (ties: the lowest label).  The extent is the box diagonal in float64 from the float32 box; an axis without a
    value (+inf / -inf) counts 0."""
    faces = np.asarray(face_count, dtype=np.int64).reshape(-1)
    lo = np.asarray(bbox_min, dtype=np.float64).reshape(-1, 3)
    hi = np.asarray(bbox_max, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        side = np.where(hi > lo, hi - lo, 0.0)           # an axis without a value has min = +inf > max = -inf; min == max = inf is 0 wide
    extent = np.sqrt((side * side).sum(axis=1))
    keep = (faces >= max(1, int(min_faces))) & (extent >= float(min_extent))
    if require_mark:
        keep &= np.asarray(marked_count, dtype=np.int64).reshape(-1) >= 1
    if keep_largest and keep.any():
        best = int(np.argmax(np.where(keep, faces, -1)))  # argmax returns the first of equals: the lowest label
        keep = np.zeros_like(keep)
        keep[best] = True
    return keep


def select_components(comps, keep_largest=False, min_faces=0, min_extent=0.0, require_mark=False):
    """-> (C,) bool tensor on the statistics' device.  The four (C,)-row tensors the rule needs are read back once."""
    host = [t.detach().cpu().numpy() for t in (comps.face_count, comps.marked_count, comps.bbox_min, comps.bbox_max)]
    keep = select_rows(*host, keep_largest=keep_largest, min_faces=min_faces, min_extent=min_extent, require_mark=require_mark)
    return torch.from_numpy(keep).to(comps.face_count.device)


def filter_components(vertices, faces, comps, keep):
    """`keep`: (C,) bool or uint8, a device tensor or a host array.  -> (vertices (V', 3) float32, faces (F', 3) int32,
    vertex_index (V',) int32) on the device; keeping nothing gives three empty tensors."""
    v, f = _mesh(vertices, faces)
    V, F, n = int(v.shape[0]), int(f.shape[0]), int(comps.count)
    k = keep if torch.is_tensor(keep) else torch.from_numpy(np.ascontiguousarray(np.asarray(keep)))
    if k.dtype not in (torch.bool, torch.uint8) or tuple(k.shape) != (n,):
        raise ValueError(f"mesh_components: keep must be ({n},) bool or uint8, got {tuple(k.shape)} {k.dtype}")
    if tuple(comps.vertex_label.shape) != (V,):
        raise ValueError(f"mesh_components: the components label {comps.vertex_label.shape[0]} vertices, the mesh has {V}")
    k = k.to(device=v.device, dtype=torch.uint8).contiguous()
    labels = _device(comps.vertex_label, "vertex_label", torch.int32, f"({V},)", lambda t: True)
    l = _lib.lib()
    dev = v.device
    ws, ws_bytes = _workspace(l, V, F, dev)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    check(l.svr_mesh_filter_count(ptr(f), F, V, ptr(labels), ptr(k), n, ptr(ws), ws_bytes, ptr(totals), stream()), "mesh_filter_count")
    nv, nf = totals.tolist()                             # size the outputs
    out_v = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    out_f = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    index = torch.empty(nv, device=dev, dtype=torch.int32)
    if nv and nf:
        check(l.svr_mesh_filter_emit(ptr(v), V, ptr(f), F, ptr(ws), ws_bytes, ptr(out_v), ptr(out_f), ptr(index), stream()),
              "mesh_filter_emit")
    return out_v, out_f, index


def clean_mesh(vertices, faces, mark=None, **criteria):
    """mesh_components -> select_components(**criteria) -> filter_components."""
    comps = mesh_components(vertices, faces, mark)
    keep = select_components(comps, **criteria)
    return (*filter_components(vertices, faces, comps, keep), comps, keep)
