"""Vertex colours for a mesh from the image it was reconstructed from, on the device (csrc/vertex_color.hip; the rule is
in include/svr_hip.h, the design in DESIGN.md section 20, the numpy restatement in tests/vertex_color_oracle.py).

``vertex_colors(vertices, faces, image, depth, consts, ...) -> (colors (V, 3) uint8, state (V,) uint8)``, device tensors.
Every vertex is projected through the pinhole camera of the 12 constants; it is *seen* when the depth map of the same mesh
from the same camera (``render_depth``) holds, in one of the up to four pixels around its projection, a depth no nearer
than the vertex's own minus `bias`; a seen vertex whose image position lies inside the image takes the bilinear sample
(state 1).  With `spread`, the others take the mean colour of their coloured neighbours along mesh edges, pass by pass
(state 2), exactly: integer sums, the same bytes on every run.  What no pass reaches keeps `fill` and state 0.

There is no CPU fallback: CPU tensors raise, like every other op."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream

IDENTITY_MAP = (1.0, 0.0, 1.0, 0.0)
DEFAULT_FILL = (128, 128, 128)
READBACK_INTERVAL = 8                  # passes between two reads of the changed-vertex counter (profiles/vertex_color.json)


def _device(t, what, dtype, shape_text, ok):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"vertex_colors HIP path needs GPU tensors (no CPU fallback): {what}")
    if t.dtype != dtype or not ok(t):
        raise ValueError(f"vertex_colors: {what} must be {shape_text} {str(dtype).replace('torch.', '')}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def vertex_colors(vertices, faces, image, depth, consts, pixel_map=None, bias=None, spread=True, fill=DEFAULT_FILL, max_passes=None,
                  readback_interval=None, stats=None):
    """`vertices` (V, 3) float32 in grid index space (lattice indices divided by inf_res, as ``Reconstruction.render_depth``
    does), `faces` (F, 3) int32, `image` (Hi, Wi, 3) uint8, `depth` (H, W) float32 (0 = no surface), all on the device;
    `consts`: the 12 camera constants (host).  `pixel_map` = (ax, bx, ay, by) sends depth-map pixel (u, v) to image position
    (ax*u + bx, ay*v + by); None is the identity.  `bias` (metres) is how much deeper than the depth map a vertex may lie and
    still count as seen; None is one grid cell, 1 / s22: marching-cubes vertices sit within a cell of the surface the map
    shows.  That default is a choice, not a measurement.  `max_passes` bounds the spread (None: to the fixed point);
    `readback_interval` is how many passes run between two looks at the device's changed-vertex counter and never changes
    the result.  `stats`: a dict that receives `passes`, the spread passes launched."""
    v = _device(vertices, "vertices", torch.float32, "(V, 3)", lambda t: t.dim() == 2 and t.shape[1] == 3)
    f = _device(faces, "faces", torch.int32, "(F, 3)", lambda t: t.dim() == 2 and t.shape[1] == 3)
    img = _device(image, "image", torch.uint8, "(Hi, Wi, 3)", lambda t: t.dim() == 3 and t.shape[2] == 3 and min(t.shape[:2]) >= 1)
    d = _device(depth, "depth", torch.float32, "(H, W)", lambda t: t.dim() == 2 and min(t.shape) >= 1)
    k = np.asarray(consts, dtype=np.float32).reshape(-1)
    if k.shape[0] != 12:
        raise ValueError(f"vertex_colors: consts holds {k.shape[0]} numbers, need 12")
    pm = IDENTITY_MAP if pixel_map is None else tuple(float(x) for x in pixel_map)
    if len(pm) != 4:
        raise ValueError(f"vertex_colors: pixel_map holds {len(pm)} numbers, need 4 (ax, bx, ay, by)")
    fl = tuple(int(x) for x in fill)
    if len(fl) != 3 or not all(0 <= x <= 255 for x in fl):
        raise ValueError(f"vertex_colors: fill must be three values in [0, 255], got {fill!r}")
    bias = 1.0 / float(k[7]) if bias is None else float(bias)
    interval = READBACK_INTERVAL if readback_interval is None else int(readback_interval)
    if interval < 1:
        raise ValueError(f"vertex_colors: readback_interval={readback_interval} (need >= 1)")
    limit = -1 if max_passes is None else int(max_passes)
    if max_passes is not None and limit < 0:
        raise ValueError(f"vertex_colors: max_passes={max_passes} (need >= 0)")
    l = _lib.lib()
    V, F = int(v.shape[0]), int(f.shape[0])
    colors = torch.empty((V, 3), device=v.device, dtype=torch.uint8)
    state = torch.empty((V,), device=v.device, dtype=torch.uint8)
    check(l.svr_vertex_color_sample(ptr(v), V, (C.c_float * 12)(*[float(x) for x in k]), ptr(d), int(d.shape[0]), int(d.shape[1]), bias,
                                    ptr(img), int(img.shape[0]), int(img.shape[1]), (C.c_double * 4)(*pm), (C.c_uint8 * 3)(*fl),
                                    ptr(colors), ptr(state), stream()), "vertex_color_sample")
    passes = C.c_int64(0)
    if spread and V and F:
        ws_bytes = int(l.svr_vertex_color_workspace_bytes(V))
        if ws_bytes < 0:
            check(ws_bytes, "vertex_color_workspace_bytes")
        ws = torch.empty(ws_bytes, device=v.device, dtype=torch.uint8)
        check(l.svr_vertex_color_spread(ptr(f), F, V, ptr(colors), ptr(state), ptr(ws), ws_bytes, limit, interval, C.byref(passes),
                                        stream()), "vertex_color_spread")
    if stats is not None:
        stats["passes"] = int(passes.value)
    return colors, state
