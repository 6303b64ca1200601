"""Mirror of the reference's util/visualize.py:23-25 (visualize_sdf) and of the two marching_cubes package calls
behind it (marching_cubes.marching_cubes, marching_cubes.export_obj), on the library's marching-cubes kernels.

``marching_cubes(field, level) -> (vertices (V,3) float32, faces (F,3) int32)``: `field` is an (X, Y, Z) array.  A
device tensor gives device tensors; a numpy array is uploaded and gives numpy arrays (the convention of
check_mesh_contains); a CPU tensor is refused like everywhere on the HIP path.  Any other dtype is cast to float32 first
(the reference hands a float64 grid to its marching cubes: values that differ below float32 precision, or lie within a
float32 rounding of `level`, can classify differently).  The comparison with `level` and the vertex interpolation run
in float64.  The mesh is in the field's index space (x along axis 0); the exact rules (inside = v < level, vertex and
face order, outward winding, open surfaces at the lattice border) are in include/svr_hip.h and DESIGN.md section 9.

``export_obj(vertices, faces, path, normals=None)``: `v x y z` lines (%.9g: float32 round trip), then 1-based `f a b c` lines,
written by the library's C++ host code; with `normals` (V, 3) float32 (util.mesh_render.vertex_normals) `vn x y z` lines follow
the `v` lines and the faces read `f a//a b//b c//c`.  ``visualize_sdf(sdf, output_path, level=0.75)``: the two together.
``save_png(rgb, path)``: an (H, W, 3) uint8 image as an 8-bit RGB .png.
``export_ply(vertices, faces, colors, path)``: the same mesh with one uint8 RGB colour per vertex, as a binary PLY.

The other functions of the reference's util/visualize.py (:10-20,28-49), which the scene trainer's validation / test
steps call (kernels in csrc/voxel_mesh.hip, host writers in csrc/io_png.cpp and io_mesh.cpp):

``voxel_mesh(grid, threshold=0.5) -> (vertices (V,3) float32, faces (F,3) int32)``: the boundary surface of the union of
unit cubes centred on the occupied indices of an (X, Y, Z) grid, same input convention as `marching_cubes`.  The
reference builds one 12-triangle box per occupied voxel (trimesh.voxel.ops.multibox) and lets Trimesh merge the
vertices; this is that triangle set MINUS the faces shared by two boxes, which are invisible and, on a filled grid, most
of the file.  Occupied iff v >= threshold (NaN is not); welded corner-lattice vertices in C order, faces by voxel then
direction -x, +x, -y, +y, -z, +z, wound outward (the exact quad corner order: include/svr_hip.h).  trimesh is not
installed here: the semantics are this project's own, pinned by tests/voxel_mesh_oracle.py.
``to_point_list(s)``: the occupied indices (s >= 0.5) in C order as (n, 3) int64; on the device for a device tensor.
``visualize_grid(grid, output_path)``: voxel_mesh + export_obj; writes nothing when no voxel is occupied.
``visualize_depthmap(depthmap, output_path, flip=False)``: `<output_path>.png` and `<output_path>.exr`.
``visualize_point_list(grid, output_path)``: `v x+0.5 y+0.5 z+0.5 1 1 1` lines, formatted like the reference's."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream, to_device

_INT32_LIMIT = 2 ** 31


def _count_emit_mesh(field, level, what, arg, lib_name):
    """The two-launch mesher shared by marching_cubes and voxel_mesh: workspace -> count -> the two totals (the only
    host synchronisation: they size the outputs) -> emit.  `lib_name`: the three entry points are svr_<lib_name>_workspace_bytes
    / _count / _emit; `what` / `arg`: the function's and its array argument's name in messages."""
    l = _lib.lib()
    workspace_bytes, count, emit = (getattr(l, f"svr_{lib_name}_{part}") for part in ("workspace_bytes", "count", "emit"))
    f, as_numpy = to_device(field, what, torch.float32)
    if f.dim() != 3:
        raise ValueError(f"{what}: {arg} must be (X, Y, Z), got {tuple(f.shape)}")
    X, Y, Z = (int(s) for s in f.shape)
    ws_bytes = int(workspace_bytes(X, Y, Z))
    if ws_bytes < 0:
        check(ws_bytes, lib_name + "_workspace_bytes")
    dev = f.device
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    check(count(ptr(f), X, Y, Z, float(level), ptr(ws), ws_bytes, ptr(totals), stream()), lib_name + "_count")
    nv, nf = totals.tolist()
    if nv >= _INT32_LIMIT or nf >= _INT32_LIMIT:
        raise RuntimeError(f"{what}: {nv} vertices / {nf} faces do not fit int32 face indices")
    verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    if nv or nf:
        check(emit(ptr(f), X, Y, Z, float(level), ptr(ws), ptr(verts), ptr(faces), stream()), lib_name + "_emit")
    if as_numpy:
        return verts.cpu().numpy(), faces.cpu().numpy()
    return verts, faces


def marching_cubes(field, level):
    return _count_emit_mesh(field, level, "marching_cubes", "field", "mc")


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def export_obj(vertices, faces, path, normals=None):
    v = _host(vertices, np.float32).reshape(-1, 3)
    f = _host(faces, np.int32).reshape(-1, 3)
    if normals is not None:
        n = _host(normals, np.float32).reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError(f"export_obj: {len(n)} normals for {len(v)} vertices")
        check(_lib.lib().svr_write_obj_normals(os.fsencode(path), v.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), len(v),
                                               f.ctypes.data_as(C.c_void_p), len(f)), "write_obj_normals")
        return
    check(_lib.lib().svr_write_obj(os.fsencode(path), v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p),
                                   len(f)), "write_obj")


def save_png(rgb, path):
    """An (H, W, 3) uint8 image (device tensor or numpy array) as an 8-bit RGB .png: util.mesh_render.save_png."""
    from .mesh_render import save_png as write
    write(rgb, path)


def export_ply(vertices, faces, colors, path):
    """A binary little-endian PLY with per-vertex `uchar red green blue` (the header text is in include/svr_hip.h):
    `colors` is (V, 3) uint8, one row per vertex; host arrays or device tensors, like export_obj."""
    v = _host(vertices, np.float32).reshape(-1, 3)
    f = _host(faces, np.int32).reshape(-1, 3)
    c = _host(colors, np.uint8).reshape(-1, 3)
    if len(c) != len(v):
        raise ValueError(f"export_ply: {len(c)} colours for {len(v)} vertices")
    check(_lib.lib().svr_write_ply(os.fsencode(path), v.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), len(v),
                                   f.ctypes.data_as(C.c_void_p), len(f)), "write_ply")


def visualize_sdf(sdf, output_path, level=0.75):
    vertices, triangles = marching_cubes(sdf, level)
    export_obj(vertices, triangles, output_path)


def voxel_mesh(grid, threshold=0.5):
    return _count_emit_mesh(grid, threshold, "voxel_mesh", "grid", "voxel_mesh")


def to_point_list(s):
    if torch.is_tensor(s):
        if not s.is_cuda:
            raise RuntimeError("to_point_list HIP path needs GPU tensors (no CPU fallback)")
        return torch.nonzero(s >= 0.5)             # C order, (n, ndim) int64 (stock compaction op: plumbing, not arithmetic)
    return np.concatenate([c[:, np.newaxis] for c in np.where(np.asarray(s) >= 0.5)], axis=1)


def visualize_grid(grid, output_path):
    if torch.is_tensor(grid) and grid.dim() != 3:
        grid = grid.reshape(grid.shape[-3:])
    vertices, faces = voxel_mesh(grid, 0.5)
    if len(faces) > 0:
        export_obj(vertices, faces, output_path)


def visualize_depthmap(depthmap, output_path, flip=False):
    """`<output_path>.png`: 8-bit grayscale of ``(255.0 / d.max() * (d - d.min())).astype(np.uint8)`` in float32 (what
    numpy 2 evaluates for a float32 array; the cast truncates toward zero); `<output_path>.exr`: the float32 map as the
    single FLOAT channel ``Z`` (pyexr.write's name for a 2-D array; uncompressed scanlines, the library writer's only
    format, where pyexr's default is ZIP).  With `flip` the columns of both are reversed.  A numpy array or a device
    tensor, squeezed to (H, W); min / max and both planes are computed on the device and only the planes cross to the
    host.  ValueError if max <= 0 or any value is NaN / inf: the reference's expression divides by the maximum and casts
    what comes out, which means nothing there."""
    from ..data_processing.sample_io import exr_write
    if isinstance(depthmap, np.ndarray):
        d = torch.from_numpy(np.ascontiguousarray(depthmap.squeeze(), dtype=np.float32)).cuda()
    elif torch.is_tensor(depthmap):
        if not depthmap.is_cuda:
            raise RuntimeError("visualize_depthmap HIP path needs GPU tensors (no CPU fallback)")
        d = depthmap.detach().squeeze().to(torch.float32).contiguous()
    else:
        raise NotImplementedError
    if d.dim() != 2 or d.numel() == 0:
        raise ValueError(f"visualize_depthmap: the map must squeeze to (H, W), got {tuple(d.shape)}")
    H, W = (int(s) for s in d.shape)
    l = _lib.lib()
    stats = torch.empty(4, device=d.device, dtype=torch.int32)
    plane_f = torch.empty((H, W), device=d.device, dtype=torch.float32)
    plane_u = torch.empty((H, W), device=d.device, dtype=torch.uint8)
    check(l.svr_depth_minmax(ptr(d), H * W, ptr(stats), stream()), "depth_minmax")
    check(l.svr_depth_planes(ptr(d), H, W, int(bool(flip)), ptr(stats), ptr(plane_f), ptr(plane_u), stream()), "depth_planes")
    st = stats.cpu().numpy().view(np.uint32)
    if st[2] != 0:
        raise ValueError("visualize_depthmap: the map holds NaN or inf")
    key = int(st[1])                               # order-preserving key of the maximum (include/svr_hip.h) -> its float
    top = np.array([key & 0x7fffffff if key >> 31 else ~key & 0xffffffff], dtype=np.uint32).view(np.float32)[0]
    if not top > 0:
        raise ValueError(f"visualize_depthmap: the map's maximum is {top}, not positive")
    gray = plane_u.cpu().numpy()
    check(l.svr_write_png_gray8(os.fsencode(str(output_path) + ".png"), gray.ctypes.data_as(C.c_void_p), H, W), "write_png_gray8")
    exr_write(str(output_path) + ".exr", {"Z": plane_f.cpu().numpy()})


def visualize_point_list(grid, output_path):
    pts = _host(grid, np.float32).reshape(-1, 3)
    check(_lib.lib().svr_write_obj_points(os.fsencode(output_path), pts.ctypes.data_as(C.c_void_p), len(pts)), "write_obj_points")
