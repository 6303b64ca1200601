"""A scene's triangle mesh -> the view a raw sample needs: distance.exr ("these are distance maps, not depth maps") and a
stand-in rgb.png.  The reference's authors rendered these with a tool they never shipped; this one is the project's own,
a ray caster on the device (csrc/raycast.hip; the rule is in include/svr_hip.h, the design in DESIGN.md section 19).

The mesh is in grid index space, the space of mesh_to_df; the camera is the pinhole camera of the pipeline, given by the
12 constants of svr_unproject_fwd (model.projection._camera_to_grid).  ``render_depth`` returns the device tensors,
``render_view`` writes the two files, and

    python -m svr_amd.data_processing.render_view MESH.obj OUT_DIR [--intrinsic P] [--down_scale_factor f] [--size H W]

prints one line with the size, the face count, the hit share and min / max of the depth over the hits.

rgb.png is NOT a photo-realistic render: it is a grey image of how squarely each ray meets the surface, there so that a
dataset built from meshes alone loads."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream
from . import sample_io
from .distance_to_depth import _grid_consts, get_intrinsic
from .mesh_occupancies import _as_mesh
from .mesh_to_df import DEFAULT_LIST_BUDGET, plan_batches, triangle_table

DEFAULT_TILE = 8                       # profiles/render_view.json
DEFAULT_SIZE = (240, 320)


def transformed(mesh, transform):
    """The mesh with the 4x4 float64 mesh -> grid affine applied on the host, per row x' = ((M00*x + M01*y) + M02*z) + M03
    (the last row of M is not used) -> a (V, F) pair; `transform` None: the mesh as it is."""
    m = _as_mesh(mesh)
    if transform is None:
        return m
    M = np.asarray(transform, dtype=np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"render_depth: transform must be a finite 4x4 matrix, got shape {M.shape}")
    v = np.asarray(m.vertices, dtype=np.float64).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], axis=1), np.asarray(m.faces)


def view_consts(intrinsic=None, scale_factor=1, consts=None):
    """The 12 float32 camera constants: `consts` as given, else those of (intrinsic, scale_factor); `intrinsic` is a path, a
    4x4 tensor or None (the default intrinsic)."""
    if consts is not None:
        k = np.asarray(consts, dtype=np.float32).reshape(-1)
        if k.shape[0] != 12:
            raise ValueError(f"render_depth: consts holds {k.shape[0]} numbers, need 12")
        return k
    K = intrinsic if torch.is_tensor(intrinsic) else get_intrinsic(intrinsic)
    return np.asarray(_grid_consts(K, scale_factor), dtype=np.float32)


def view_triangles(mesh, transform=None):
    """The (F, 9) float64 HOST table of the mesh as the camera sees it (``transformed``, then mesh_to_df.triangle_table and
    its checks): the one table the ray caster and whatever reads its face map afterwards (util.mesh_render) share."""
    host_tri = triangle_table(transformed(mesh, transform))
    if not np.isfinite(host_tri).all():
        raise ValueError("render_depth: the transform sends a vertex to a non-finite position")
    return host_tri


def render_depth(mesh, intrinsic=None, scale_factor=1, size=DEFAULT_SIZE, near=0.0, far=None, miss=0.0, transform=None,
                 return_face=False, return_distance=False, return_normal=False, cull=True, list_budget_bytes=DEFAULT_LIST_BUDGET,
                 stats=None, consts=None, tile=DEFAULT_TILE, return_shade=False, return_tri=False):
    """-> depth (H, W) float32 on the device [, face (H, W) int32][, distance (H, W) float32][, normal (H, W, 3) float32]
    [, shade (H, W) uint8][, tri (F, 9) float64], in this order, for the flags set: the depth in metres of the nearest face
    along every pixel's ray (`miss` where there is none), the face, the ray length (what distance.exr holds), the unit normal
    turned towards the camera, the grey level of rgb.png, and the device copy of ``view_triangles``' table that was cast.

    `mesh`: a path, a loaded mesh or a (V, F) pair in grid units; `transform`: a 4x4 float64 mesh -> grid affine applied
    first (see ``transformed``), so that one world-space mesh can be seen from several poses.  The camera: `intrinsic` (path
    or 4x4, default the pipeline's) and `scale_factor`, or the 12 constants themselves in `consts`.  A hit needs
    near < depth <= far (far None: no limit).  `tile` in {8, 16} is the edge of the screen tiles; `cull=False` tests every
    face against every pixel (the same arithmetic: the same bits, much slower); `list_budget_bytes` bounds the
    candidate-list buffer, the tiles being walked in batches that fit it.  `stats`: a dict that receives the list figures."""
    H, W = (int(v) for v in size)
    if not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"render_depth: size {size} (1 <= H, W <= 32768)")
    if tile not in (8, 16):
        raise ValueError(f"render_depth: tile={tile} (8 or 16)")
    if int(list_budget_bytes) < 4:
        raise ValueError(f"render_depth: list_budget_bytes={list_budget_bytes}")
    near, far = float(near), float("inf") if far is None else float(far)
    if not near < far:
        raise ValueError(f"render_depth: near={near}, far={far}")
    k = view_consts(intrinsic, scale_factor, consts)
    host_tri = view_triangles(mesh, transform)
    F = host_tri.shape[0]
    l = _lib.lib()
    kc = (C.c_float * 12)(*[float(v) for v in k])
    tri = torch.from_numpy(host_tri).cuda()
    depth = torch.empty((H, W), device="cuda", dtype=torch.float32)
    face = torch.empty((H, W), device="cuda", dtype=torch.int32) if return_face else None
    distance = torch.empty((H, W), device="cuda", dtype=torch.float32) if return_distance else None
    normal = torch.empty((H, W, 3), device="cuda", dtype=torch.float32) if return_normal else None
    shade = torch.empty((H, W), device="cuda", dtype=torch.uint8) if return_shade else None
    nt = int(l.svr_raycast_tiles(H, W, tile))
    if nt < 0:
        check(nt, "raycast_tiles")

    def evaluate(offsets, lst, b0, b1):
        check(l.svr_raycast_eval(ptr(tri), F, kc, H, W, tile, near, far, float(miss), ptr(offsets), ptr(lst), b0, b1, ptr(depth),
                                 ptr(face), ptr(distance), ptr(normal), ptr(shade), stream()), "raycast_eval")

    if not cull:
        evaluate(None, None, 0, nt)
        if stats is not None:
            stats.update(tiles=nt, faces=F, batches=1, list_entries=nt * F)
    else:
        rects = torch.empty((F, 4), device="cuda", dtype=torch.int32)
        check(l.svr_raycast_face_bounds(ptr(tri), F, kc, ptr(rects), stream()), "raycast_face_bounds")
        ws_bytes = int(l.svr_raycast_workspace_bytes(H, W, tile))
        ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
        offsets = torch.empty(nt + 1, device="cuda", dtype=torch.int64)
        check(l.svr_raycast_count(ptr(rects), F, H, W, tile, ptr(ws), ws_bytes, ptr(offsets), stream()), "raycast_count")
        host_off = offsets.cpu().numpy()
        batches = plan_batches(host_off, list_budget_bytes)
        for b0, b1 in batches:
            n = int(host_off[b1] - host_off[b0])
            lst = torch.empty(max(n, 1), device="cuda", dtype=torch.int32)
            check(l.svr_raycast_emit(ptr(rects), F, H, W, tile, ptr(offsets), b0, b1, ptr(lst), n, stream()), "raycast_emit")
            evaluate(offsets, lst, b0, b1)
        if stats is not None:
            per = np.diff(host_off)
            stats.update(tiles=nt, faces=F, batches=len(batches), list_entries=int(host_off[-1]), list_bytes=int(host_off[-1]) * 4,
                         list_mean=float(per.mean()), list_max=int(per.max()),
                         every_tile_faces=int((rects[:, 0] == -(1 << 30)).sum().item()),
                         largest_batch_bytes=max(int(host_off[b1] - host_off[b0]) * 4 for b0, b1 in batches))
    out = [depth] + [t for t in (face, distance, normal, shade, tri if return_tri else None) if t is not None]
    return out[0] if len(out) == 1 else tuple(out)


def render_view(mesh, out_dir, intrinsic=None, scale_factor=1, size=DEFAULT_SIZE, near=0.0, far=None, miss=0.0, transform=None,
                consts=None, write_rgb=True, cull=True, list_budget_bytes=DEFAULT_LIST_BUDGET, tile=DEFAULT_TILE):
    """Write <out_dir>/distance.exr (channels B, G, R all equal to the distance map; the loaders read "R") and, with
    `write_rgb`, <out_dir>/rgb.png: 8-bit RGB, grey, round(255 |normal . d| / |d|) per pixel and 0 for a miss -- a stand-in
    so that a mesh-only dataset loads, not a photo-realistic render.  -> (depth, distance, shade) device tensors."""
    depth, distance, shade = render_depth(mesh, intrinsic, scale_factor, size, near, far, miss, transform, return_distance=True,
                                          return_shade=True, consts=consts, cull=cull, list_budget_bytes=list_budget_bytes, tile=tile)
    os.makedirs(out_dir, exist_ok=True)
    d = distance.cpu().numpy()
    sample_io.exr_write(os.path.join(out_dir, "distance.exr"), {"B": d, "G": d, "R": d})
    if write_rgb:
        from PIL import Image
        g = shade.cpu().numpy()
        Image.fromarray(np.stack([g, g, g], axis=-1), "RGB").save(os.path.join(out_dir, "rgb.png"))
    return depth, distance, shade


def main(argv=None):
    ap = argparse.ArgumentParser(description="triangle mesh (.obj, grid units) -> distance.exr and a grey rgb.png of the view")
    ap.add_argument("mesh")
    ap.add_argument("out_dir")
    ap.add_argument("--intrinsic", default=None, help="intrinsic.txt of the view (default: the pipeline's constants)")
    ap.add_argument("--down_scale_factor", type=float, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=list(DEFAULT_SIZE), metavar=("H", "W"))
    a = ap.parse_args(argv)
    faces = _as_mesh(a.mesh).faces.shape[0]
    depth, _, _ = render_view(a.mesh, a.out_dir, intrinsic=a.intrinsic, scale_factor=a.down_scale_factor, size=tuple(a.size))
    hit = depth > 0                      # near = 0: every hit is positive, miss = 0
    n = int(hit.sum().item())
    span = f"depth min {depth[hit].min().item():.6g} max {depth[hit].max().item():.6g}" if n else "no hit"
    print(f"{a.out_dir}: {a.size[0]} x {a.size[1]}, {faces} faces, hit {100.0 * n / depth.numel():.2f} %, {span}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
