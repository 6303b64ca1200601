"""Mirror of the reference's util/visualize.py:23-25 (visualize_sdf) and of the two marching_cubes package calls
behind it (marching_cubes.marching_cubes, marching_cubes.export_obj), on the library's marching-cubes kernels.

``marching_cubes(field, level) -> (vertices (V,3) float32, faces (F,3) int32)``: `field` is an (X, Y, Z) array.  A
device tensor gives device tensors; a numpy array is uploaded and gives numpy arrays (the convention of
check_mesh_contains); a CPU tensor is refused like everywhere on the HIP path.  Any other dtype is cast to float32 first
(the reference hands a float64 grid to its marching cubes: values that differ below float32 precision, or lie within a
float32 rounding of `level`, can classify differently).  The comparison with `level` and the vertex interpolation run
in float64.  The mesh is in the field's index space (x along axis 0); the exact rules (inside = v < level, vertex and
face order, outward winding, open surfaces at the lattice border) are in include/svr_hip.h and DESIGN.md section 9.

``export_obj(vertices, faces, path)``: `v x y z` lines (%.9g: float32 round trip), then 1-based `f a b c` lines,
written by the library's C++ host code.  ``visualize_sdf(sdf, output_path, level=0.75)``: the two together."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from .._lib import check

_INT32_LIMIT = 2 ** 31


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def marching_cubes(field, level):
    as_numpy = not torch.is_tensor(field)
    if as_numpy:
        field = torch.from_numpy(np.ascontiguousarray(np.asarray(field), dtype=np.float32)).cuda()
    elif not field.is_cuda:
        raise RuntimeError("marching_cubes HIP path needs GPU tensors (no CPU fallback)")
    if field.dim() != 3:
        raise ValueError(f"marching_cubes: field must be (X, Y, Z), got {tuple(field.shape)}")
    f = field.to(torch.float32).contiguous()
    X, Y, Z = (int(s) for s in f.shape)
    l = _lib.lib()
    ws_bytes = int(l.svr_mc_workspace_bytes(X, Y, Z))
    if ws_bytes < 0:
        check(ws_bytes, "mc_workspace_bytes")
    dev = f.device
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    totals = torch.empty(2, device=dev, dtype=torch.int64)
    fp, wp = C.c_void_p(f.data_ptr()), C.c_void_p(ws.data_ptr())
    check(l.svr_mc_count(fp, X, Y, Z, float(level), wp, ws_bytes, C.c_void_p(totals.data_ptr()), _stream()), "mc_count")
    nv, nf = totals.tolist()                       # the only host synchronisation: sizes the outputs
    if nv >= _INT32_LIMIT or nf >= _INT32_LIMIT:
        raise RuntimeError(f"marching_cubes: {nv} vertices / {nf} faces do not fit int32 face indices")
    verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
    faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
    if nv or nf:
        check(l.svr_mc_emit(fp, X, Y, Z, float(level), wp, C.c_void_p(verts.data_ptr()), C.c_void_p(faces.data_ptr()),
                            _stream()), "mc_emit")
    if as_numpy:
        return verts.cpu().numpy(), faces.cpu().numpy()
    return verts, faces


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def export_obj(vertices, faces, path):
    v = _host(vertices, np.float32).reshape(-1, 3)
    f = _host(faces, np.int32).reshape(-1, 3)
    check(_lib.lib().svr_write_obj(os.fsencode(path), v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p),
                                   len(f)), "write_obj")


def visualize_sdf(sdf, output_path, level=0.75):
    vertices, triangles = marching_cubes(sdf, level)
    export_obj(vertices, triangles, output_path)
