"""A scene's triangle mesh -> distance_field.df, the file process_sample starts from ("unsigned, untruncated distance
field, voxel size 5 cm, [139, 104, 112]").  The reference never shipped the tool that wrote its .df files; this one is
the project's own, on the device (csrc/mesh_df.hip; the rule is in include/svr_hip.h, the design in DESIGN.md section 18).

The mesh is in grid index space -- what util.visualize.marching_cubes writes: a vertex (x, y, z) has x along axis 0 and
lattice point (i, j, k) sits at (i, j, k).  ``mesh_distance_field`` returns the device tensor(s), ``mesh_to_df`` writes
the file, and

    python -m svr_amd.data_processing.mesh_to_df MESH.obj OUT.df [--dims X Y Z] [--down_scale_factor f] [--truncate T]

prints one line with the extents, the face count and min / max of the field."""
import argparse
import ctypes as C
import sys

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream
from . import sample_io
from .mesh_occupancies import _as_mesh
from .process_sample import EmptyMeshError, sample_dims

DEFAULT_BRICK = 4                      # profiles/mesh_df.json: 18.6 ms of kernels against 21.7 ms with 8
DEFAULT_LIST_BUDGET = 256 << 20
SVR_E_BADSHAPE = -2


def triangle_table(mesh):
    """path / loaded mesh / (V, F) pair -> (F, 9) float64 HOST array a, b, c per face, after the host checks: a face index
    outside [0, V) and a non-finite vertex raise ValueError, a mesh without faces EmptyMeshError."""
    m = _as_mesh(mesh)
    v = np.asarray(m.vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(m.faces)
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"mesh_distance_field: faces must be integers, got {f.dtype}")
    f = f.reshape(-1, 3).astype(np.int64)
    if f.shape[0] == 0:
        raise EmptyMeshError("mesh_distance_field: the mesh has no face")
    if f.shape[0] >= 1 << 31:
        raise ValueError(f"mesh_distance_field: {f.shape[0]} faces (need fewer than 2^31)")
    if f.min() < 0 or f.max() >= v.shape[0]:
        bad = int(np.nonzero(((f < 0) | (f >= v.shape[0])).any(axis=1))[0][0])
        raise ValueError(f"mesh_distance_field: face {bad} = {f[bad].tolist()} indexes outside the {v.shape[0]} vertices")
    if not np.isfinite(v).all():
        bad = int(np.nonzero(~np.isfinite(v).all(axis=1))[0][0])
        raise ValueError(f"mesh_distance_field: vertex {bad} = {v[bad].tolist()} is not finite")
    return np.ascontiguousarray(v[f].reshape(-1, 9))


def cull_slack(tri, dims, truncate=None):
    """What svr_mesh_df_count widens its comparison by: 2^-18 * max(1, S), S the largest coordinate magnitude among the
    vertices, the lattice extents and the truncation (four times a bound on the distance's error)."""
    S = max(1.0, float(np.abs(tri).max()), float(max(dims)), float(truncate or 0.0))
    return S * 2.0 ** -18


def plan_batches(offsets, budget_bytes):
    """Consecutive brick ranges [(b0, b1)] whose candidate lists (int32) fit `budget_bytes`; a brick whose list alone is
    larger is a batch of its own.  `offsets`: the bricks + 1 running totals."""
    cap = max(int(budget_bytes) // 4, 0)
    n = len(offsets) - 1
    ends = np.asarray(offsets[1:], dtype=np.int64)
    batches, b0 = [], 0
    while b0 < n:
        # the last b1 with offsets[b1] - offsets[b0] <= cap, at least one brick
        b1 = int(np.searchsorted(ends, int(offsets[b0]) + cap, side="right"))
        b1 = min(max(b1, b0 + 1), n)
        batches.append((b0, b1))
        b0 = b1
    return batches


def mesh_distance_field(mesh, dims, truncate=None, return_face=False, brick=DEFAULT_BRICK, cull=True,
                        list_budget_bytes=DEFAULT_LIST_BUDGET, stats=None):
    """-> field (X, Y, Z) float32 on the device [, face (X, Y, Z) int32 with `return_face`]: the exact distance from every
    lattice point to the mesh, and the face that realises it (the lowest index among equals; -1 where `truncate` took
    effect).  `mesh`: a path, a loaded mesh or a (V, F) pair, in grid units.  `truncate` = T > 0 caps the field at T (the
    .df format's field is untruncated: the default).  `brick` in {4, 8} is the edge of the bricks the lattice is cut into;
    `cull=False` tests every face against every point (the same arithmetic: the same bits, much slower);
    `list_budget_bytes` bounds the candidate-list buffer, the bricks being walked in batches that fit it.  `stats`: a dict
    that receives the candidate-list figures."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f"mesh_distance_field: lattice {dims} (three extents >= 1, fewer than 2^31 points)")
    if brick not in (4, 8):
        raise ValueError(f"mesh_distance_field: brick={brick} (4 or 8)")
    if int(list_budget_bytes) < 4:
        raise ValueError(f"mesh_distance_field: list_budget_bytes={list_budget_bytes}")
    T = float(truncate) if truncate is not None and float(truncate) > 0 else 0.0
    if T and np.float32(T) <= 0:
        raise ValueError(f"mesh_distance_field: truncate={truncate} rounds to zero in float32")
    host_tri = triangle_table(mesh)
    F = host_tri.shape[0]
    l = _lib.lib()
    X, Y, Z = dims
    tri = torch.from_numpy(host_tri).cuda()
    small = torch.empty(8, device="cuda", dtype=torch.uint8)
    n_valid = C.c_int64(0)
    rc = l.svr_mesh_df_valid_faces(ptr(tri), F, ptr(small), C.byref(n_valid), stream())
    if rc == SVR_E_BADSHAPE:
        raise EmptyMeshError(f"mesh_distance_field: none of the {F} faces has an area")
    check(rc, "mesh_df_valid_faces")
    field = torch.empty(dims, device="cuda", dtype=torch.float32)
    face = torch.empty(dims, device="cuda", dtype=torch.int32) if return_face else None
    nb = int(l.svr_mesh_df_bricks(X, Y, Z, brick))
    if nb < 0:
        check(nb, "mesh_df_bricks")
    if not cull:
        check(l.svr_mesh_df_eval(ptr(tri), F, X, Y, Z, brick, T, None, None, 0, nb, ptr(field), ptr(face), stream()), "mesh_df_eval")
        if stats is not None:
            stats.update(bricks=nb, faces=F, valid_faces=n_valid.value, batches=1, list_entries=nb * F)
        return (field, face) if return_face else field
    ws_bytes = int(l.svr_mesh_df_workspace_bytes(X, Y, Z, brick))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    offsets = torch.empty(nb + 1, device="cuda", dtype=torch.int64)
    check(l.svr_mesh_df_count(ptr(tri), F, X, Y, Z, brick, T, cull_slack(host_tri, dims, T), ptr(ws), ws_bytes, ptr(offsets),
                              stream()), "mesh_df_count")
    host_off = offsets.cpu().numpy()
    batches = plan_batches(host_off, list_budget_bytes)
    for b0, b1 in batches:
        n = int(host_off[b1] - host_off[b0])
        lst = torch.empty(max(n, 1), device="cuda", dtype=torch.int32)
        check(l.svr_mesh_df_emit(ptr(tri), F, X, Y, Z, brick, ptr(ws), ptr(offsets), b0, b1, ptr(lst), n, stream()), "mesh_df_emit")
        check(l.svr_mesh_df_eval(ptr(tri), F, X, Y, Z, brick, T, ptr(offsets), ptr(lst), b0, b1, ptr(field), ptr(face), stream()),
              "mesh_df_eval")
    if stats is not None:
        per = np.diff(host_off)
        stats.update(bricks=nb, faces=F, valid_faces=n_valid.value, batches=len(batches), list_entries=int(host_off[-1]),
                     list_bytes=int(host_off[-1]) * 4, list_mean=float(per.mean()), list_max=int(per.max()),
                     largest_batch_bytes=max(int(host_off[b1] - host_off[b0]) * 4 for b0, b1 in batches))
    return (field, face) if return_face else field


def mesh_to_df(mesh, out_path, dims=None, down_scale_factor=1, truncate=None):
    """Write the mesh's distance field to `out_path` in the .df layout (volume_reader.read_df reads it back bit for bit).
    `dims` defaults to process_sample.sample_dims(down_scale_factor); the mesh is in grid units of that lattice.
    -> the field (device tensor)."""
    if dims is None:
        dims = sample_dims(down_scale_factor)
    field = mesh_distance_field(mesh, dims, truncate=truncate)
    sample_io.df_write(out_path, field)
    return field


def main(argv=None):
    ap = argparse.ArgumentParser(description="triangle mesh (.obj, grid units) -> unsigned distance field (.df)")
    ap.add_argument("mesh")
    ap.add_argument("out")
    ap.add_argument("--dims", type=int, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--down_scale_factor", type=int, default=1)
    ap.add_argument("--truncate", type=float, default=None)
    a = ap.parse_args(argv)
    dims = tuple(a.dims) if a.dims else sample_dims(a.down_scale_factor)
    faces = _as_mesh(a.mesh).faces.shape[0]
    field = mesh_to_df(a.mesh, a.out, dims=dims, truncate=a.truncate)
    print(f"{a.out}: {dims[0]} x {dims[1]} x {dims[2]}, {faces} faces, field min {field.min().item():.6g} max {field.max().item():.6g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
