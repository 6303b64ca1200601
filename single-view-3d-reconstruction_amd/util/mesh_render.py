"""Shaded previews of a triangle mesh on the device: area-weighted vertex normals (csrc/mesh_normals.hip), a shading pass over
the ray caster's face map and the box filter behind supersampling (csrc/mesh_shade.hip, csrc/shade_pixel.h).  The rules are in
include/svr_hip.h, the design in DESIGN.md section 25, the numpy restatement in tests/mesh_render_oracle.py.

``vertex_normals(vertices, faces) -> (normals, state)``; ``render_mesh(vertices, faces, ...) -> (H, W, 3) uint8``;
``orbit_transform(vertices, faces, yaw, pitch, dolly)``: the 4x4 that turns the mesh in front of the camera;
``save_png(rgb, path)``.

The mesh is in grid index space, the camera is the pipeline's pinhole camera (the 12 constants of svr_unproject_fwd), as for
data_processing.render_view, whose ``render_depth`` makes the face map: culling, batching and the argument checks are the ray
caster's.  Every output is the same bits on every run and equals the oracle's.  There is no CPU fallback: the kernels run on
the device; host arrays are uploaded."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream
from ..data_processing.render_view import DEFAULT_SIZE, DEFAULT_TILE, render_depth, view_consts

HAS_NORMAL, NO_NORMAL, BAD = 0, 1, 3
SHADINGS = ("smooth", "flat")
COORD_LIMIT = 65536.0


def _device(t, what, dtype):
    """(N, 3) `dtype` on the device: a device tensor as it is, a numpy array uploaded; a CPU tensor is refused."""
    if torch.is_tensor(t):
        if not t.is_cuda:
            raise RuntimeError(f"mesh_render HIP path needs GPU tensors (no CPU fallback): {what}")
    else:
        a = np.ascontiguousarray(t)
        t = torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"mesh_render: {what} must be (N, 3) {str(dtype).replace('torch.', '')}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def vertex_normals(vertices, faces, return_counts=False):
    """Area-weighted unit normals per vertex: `vertices` (V, 3) float32 and `faces` (F, 3) int32 (device tensors, or numpy arrays
    that are uploaded) -> `normals` (V, 3) float32 and `state` (V,) uint8 on the device: 0 has a normal, 1 in no valid face or a
    zero sum (the normal is 0), 3 not usable (a coordinate that is not finite or not below 2^16 in magnitude).  The direction
    follows the faces' winding.  With `return_counts` also the vertices per state 0, 1, 3 as a list (the one host
    synchronisation; the library call itself makes none)."""
    v = _device(vertices, "vertices", torch.float32)
    f = _device(faces, "faces", torch.int32)
    V, F = int(v.shape[0]), int(f.shape[0])
    l = _lib.lib()
    ws_bytes = int(l.svr_mesh_vertex_normals_workspace_bytes(V, F))
    if ws_bytes < 0:
        check(ws_bytes, "mesh_vertex_normals_workspace_bytes")
    dev = v.device
    ws = torch.empty(ws_bytes if V and F else 0, device=dev, dtype=torch.uint8)
    normals = torch.empty((V, 3), device=dev, dtype=torch.float32)
    state = torch.empty(V, device=dev, dtype=torch.uint8)
    counts = torch.empty(3, device=dev, dtype=torch.int64)
    check(l.svr_mesh_vertex_normals(ptr(v), V, ptr(f), F, ptr(ws), ws_bytes, ptr(normals), ptr(state), ptr(counts), stream()),
          "mesh_vertex_normals")
    return (normals, state, counts.tolist()) if return_counts else (normals, state)


def ssaa_consts(consts, s):
    """The 12 constants of the fine image, s times as large per axis: f' = s f, cx' = s cx + (s - 1) / 2, cy' likewise, in
    float64 from the float32 constants, rounded to float32; the other nine unchanged.  Sub-pixel i of a pixel then lies at
    offset (i - (s - 1) / 2) / s from its centre."""
    k = np.asarray(consts, dtype=np.float32).copy()
    f, cx, cy = (np.float64(x) for x in k[:3])
    k[0], k[1], k[2] = np.float32(s * f), np.float32(s * cx + (s - 1) / 2), np.float32(s * cy + (s - 1) / 2)
    return k


def _linear_part(transform):
    M = np.asarray(transform, dtype=np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"render_mesh: transform must be a finite 4x4 matrix, got shape {M.shape}")
    L = M[:3, :3]
    det = (L[0, 0] * (L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1]) - L[0, 1] * (L[1, 0] * L[2, 2] - L[1, 2] * L[2, 0])) \
        + L[0, 2] * (L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0])
    if not (np.isfinite(det) and det != 0.0):
        raise ValueError("render_mesh: the transform's linear part is singular: it flattens the mesh and leaves no normal")
    return L


def transform_normals(normals, transform):
    """Unit normals of the mesh as given -> those of the mesh after the 4x4 `transform`, on the host in float64: every normal
    is multiplied by the cofactor matrix C of the linear part L (C = det(L) L^-T: for a rotation L itself, for any other
    invertible L the matrix that keeps normals perpendicular to the transformed surface), per row
    n'_i = ((C_i0 x + C_i1 y) + C_i2 z), then n' / sqrt((n'x n'x + n'y n'y) + n'z n'z) where that length is > 0 (a zero normal
    stays zero), rounded to float32.  A linear part that IS the identity returns the input's bits.  ValueError for a singular
    linear part."""
    L = _linear_part(transform)
    n = np.asarray(normals, dtype=np.float32)
    if np.array_equal(L, np.eye(3)):
        return n
    c = np.array([[L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1], L[1, 2] * L[2, 0] - L[1, 0] * L[2, 2], L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0]],
                  [L[0, 2] * L[2, 1] - L[0, 1] * L[2, 2], L[0, 0] * L[2, 2] - L[0, 2] * L[2, 0], L[0, 1] * L[2, 0] - L[0, 0] * L[2, 1]],
                  [L[0, 1] * L[1, 2] - L[0, 2] * L[1, 1], L[0, 2] * L[1, 0] - L[0, 0] * L[1, 2], L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0]]])
    x, y, z = (n[:, a].astype(np.float64) for a in range(3))
    with np.errstate(all="ignore"):
        m = [(c[i, 0] * x + c[i, 1] * y) + c[i, 2] * z for i in range(3)]
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        ok = length > 0.0
        out = np.stack([np.where(ok, a / np.where(ok, length, 1.0), 0.0) for a in m], axis=1)
    return out.astype(np.float32)


def _bytes3(value, what):
    a = np.asarray(value)
    if a.shape != (3,) or not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
        raise ValueError(f"render_mesh: {what}={value!r} (need three integers in [0, 255])")
    return (C.c_uint8 * 3)(*[int(x) for x in a])


def box_downsample(rgb, s):
    """(s H, s W, 3) uint8 on the device -> (H, W, 3): per channel (sum of the s x s block + s*s // 2) // (s*s)."""
    if s not in (1, 2, 3, 4):
        raise ValueError(f"render_mesh: ssaa={s} (1, 2, 3 or 4)")
    if not torch.is_tensor(rgb) or not rgb.is_cuda:
        raise RuntimeError("mesh_render HIP path needs GPU tensors (no CPU fallback): rgb")
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.shape[0] % s or rgb.shape[1] % s or rgb.numel() == 0:
        raise ValueError(f"render_mesh: the fine image must be (s H, s W, 3) uint8, got {tuple(rgb.shape)} {rgb.dtype}")
    H, W = int(rgb.shape[0]) // s, int(rgb.shape[1]) // s
    out = torch.empty((H, W, 3), device=rgb.device, dtype=torch.uint8)
    check(_lib.lib().svr_box_downsample_rgb8(ptr(rgb.contiguous()), H, W, s, ptr(out), stream()), "box_downsample_rgb8")
    return out


def shade(tri, faces, face_map, consts, n_vertices, normals=None, colors=None, ambient=0.25, albedo=(200, 200, 200),
          background=(255, 255, 255)):
    """The shading pass alone (svr_mesh_shade): `tri` (F, 9) float64, `faces` (F, 3) int32, `face_map` (H, W) int32, optional
    `normals` (V, 3) float32 and `colors` (V, 3) uint8, all on the device; `consts` the 12 constants the map was cast with
    -> (H, W, 3) uint8."""
    for t, what, dtype, rows in ((tri, "tri", torch.float64, None), (faces, "faces", torch.int32, int(tri.shape[0])),
                                 (face_map, "face_map", torch.int32, None), (normals, "normals", torch.float32, int(n_vertices)),
                                 (colors, "colors", torch.uint8, int(n_vertices))):
        if t is None and what in ("normals", "colors"):
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"mesh_render HIP path needs GPU tensors (no CPU fallback): {what}")
        if t.dtype != dtype or t.dim() != 2 or not t.is_contiguous() or (rows is not None and tuple(t.shape) != (rows, 3)):
            raise ValueError(f"mesh_render: {what} is {tuple(t.shape)} {t.dtype}" + (f", need ({rows}, 3) {dtype}" if rows is not None else ""))
    if tri.shape[1] != 9:
        raise ValueError(f"mesh_render: tri must be (F, 9), got {tuple(tri.shape)}")
    H, W = (int(x) for x in face_map.shape)
    k = np.asarray(consts, dtype=np.float32).reshape(-1)
    if k.shape[0] != 12:
        raise ValueError(f"mesh_render: consts holds {k.shape[0]} numbers, need 12")
    kc = (C.c_float * 12)(*[float(x) for x in k])
    rgb = torch.empty((H, W, 3), device=face_map.device, dtype=torch.uint8)
    check(_lib.lib().svr_mesh_shade(ptr(tri), ptr(faces), int(tri.shape[0]), int(n_vertices), ptr(face_map), kc, H, W, ptr(normals),
                                    ptr(colors), _bytes3(albedo, "albedo"), _bytes3(background, "background"), float(ambient), ptr(rgb),
                                    stream()), "mesh_shade")
    return rgb


def render_mesh(vertices, faces, consts=None, intrinsic=None, scale_factor=1, size=DEFAULT_SIZE, colors=None, shading="smooth",
                transform=None, ssaa=1, ambient=0.25, albedo=(200, 200, 200), background=(255, 255, 255), tile=DEFAULT_TILE, **kw):
    """A shaded picture of the mesh -> (H, W, 3) uint8 on the device.

    `vertices` (V, 3) float32 and `faces` (F, 3) int32 in grid units, device tensors or numpy arrays; the camera as for
    ``render_depth``: the 12 constants in `consts`, or `intrinsic` (path or 4x4, default the pipeline's) and `scale_factor`.
    The face map comes from ``render_depth(..., return_face=True)`` (`tile`, and `kw`: near, far, cull, list_budget_bytes, stats),
    so culling, batching and the checks -- a face index outside the vertices and a non-finite vertex raise -- are the ray
    caster's, and the shader reads the very triangle table that was cast.  `shading`: "smooth" interpolates the vertex normals
    of ``vertex_normals`` over each face, "flat" uses the face's own normal.  `colors`: (V, 3) uint8, interpolated likewise;
    None: `albedo`.  The light is at the camera, two-sided: intensity = ambient + (1 - ambient) |N . d| / |d|.  Pixels no face
    covers take `background`; so does every pixel of a mesh without faces.  `ssaa` in 1..4 renders s x s sub-pixels per pixel
    (``ssaa_consts``) and averages them (``box_downsample``).

    `transform`: a 4x4 float64 mesh -> grid affine for the VIEW only (``orbit_transform`` makes one).  The normals are computed
    on the mesh as given and then carried along by the transform's linear part on the host in float64, renormalised and
    rounded to float32 (``transform_normals``); a singular linear part raises ValueError."""
    H, W = (int(x) for x in size)
    if shading not in SHADINGS:
        raise ValueError(f"render_mesh: shading={shading!r} (one of {SHADINGS})")
    if isinstance(ssaa, bool) or ssaa not in (1, 2, 3, 4):
        raise ValueError(f"render_mesh: ssaa={ssaa} (1, 2, 3 or 4)")
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError(f"render_mesh: ambient={ambient} (need 0 <= ambient <= 1)")
    if not (1 <= H and 1 <= W and H * ssaa <= 32768 and W * ssaa <= 32768):
        raise ValueError(f"render_mesh: size {size} at ssaa={ssaa} (1 <= H, W and ssaa H, ssaa W <= 32768)")
    bg, _ = _bytes3(background, "background"), _bytes3(albedo, "albedo")
    if transform is not None:
        _linear_part(transform)
    v = _device(vertices, "vertices", torch.float32)
    f = _device(faces, "faces", torch.int32)
    c = None
    if colors is not None:
        c = _device(colors, "colors", torch.uint8)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"render_mesh: {c.shape[0]} colours for {v.shape[0]} vertices")
    if int(f.shape[0]) == 0:
        return torch.tensor(list(bg), dtype=torch.uint8, device=v.device).repeat(H, W, 1)
    k = ssaa_consts(view_consts(intrinsic, scale_factor, consts), ssaa)
    _, face_map, tri = render_depth((_host(v), _host(f)), size=(H * ssaa, W * ssaa), consts=k, transform=transform, return_face=True,
                                    return_tri=True, tile=tile, **kw)
    normals = None
    if shading == "smooth":
        normals, _ = vertex_normals(v, f)
        if transform is not None:
            normals = torch.from_numpy(transform_normals(_host(normals), transform)).to(v.device)
    rgb = shade(tri, f, face_map, k, int(v.shape[0]), normals, c, ambient, albedo, background)
    return rgb if ssaa == 1 else box_downsample(rgb, ssaa)


def orbit_transform(vertices, faces, yaw, pitch, dolly=0.0, consts=None, intrinsic=None, scale_factor=1):
    """The 4x4 float64 transform that turns the mesh in front of the camera -- the camera stays -- : a rotation about the
    centre of the bounding box of the vertices that valid faces use (indices in range and pairwise distinct, coordinates finite
    and below 2^16 in magnitude; the origin when there is none), `yaw` degrees about the grid's y axis first, then `pitch`
    degrees about its x axis, then a translation by `dolly` grid cells along the optical axis (0, 0, sign(s22)) of the camera
    given as for ``render_mesh``.  yaw = pitch = dolly = 0 gives the identity exactly."""
    v = _host(vertices).astype(np.float64).reshape(-1, 3)
    f = _host(faces).astype(np.int64).reshape(-1, 3)
    s22 = float(view_consts(intrinsic, scale_factor, consts)[7])
    with np.errstate(invalid="ignore"):
        usable = (np.abs(v) < COORD_LIMIT).all(axis=1)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    ok[ok] = usable[f[ok]].all(axis=1)
    used = np.unique(f[ok])
    centre = (v[used].min(axis=0) + v[used].max(axis=0)) / 2 if len(used) else np.zeros(3)
    y, p = np.deg2rad(float(yaw)), np.deg2rad(float(pitch))
    Ry = np.array([[np.cos(y), 0.0, np.sin(y)], [0.0, 1.0, 0.0], [-np.sin(y), 0.0, np.cos(y)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(p), -np.sin(p)], [0.0, np.sin(p), np.cos(p)]])
    R = Rx @ Ry
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = centre - R @ centre
    M[2, 3] += float(dolly) * np.sign(s22)
    return M


def save_png(rgb, path):
    """An (H, W, 3) uint8 image, device tensor or numpy array -> an 8-bit RGB .png (the library's writer)."""
    a = np.ascontiguousarray(_host(rgb))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"save_png: the image must be (H, W, 3) uint8, got {a.shape} {a.dtype}")
    check(_lib.lib().svr_write_png_rgb8(os.fsencode(path), a.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1]), "write_png_rgb8")
