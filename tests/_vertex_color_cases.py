"""Inputs shared by tests/test_vertex_color_cpu.py and tests/test_gpu_vertex_color.py: the committed meshes placed in front
of the camera as tests/test_gpu_raycast.py places them, the oracle's render of each (computed once, read-only), images."""
import os

import numpy as np

from tests import raycast_oracle as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLACES = ("in_view", "partly", "behind", "straddling")
_cache = {}


def gold(name):
    z = np.load(os.path.join(GOLD, "mesh_" + name + ".npz"))
    return z["vertices"].astype(np.float64), z["faces"].astype(np.int32)


def placed(name, where, size, consts, dtype=np.float32):
    """The committed mesh scaled to a largest |coordinate| of 0.6 m, in grid units, as float32 vertices (the kernels' input;
    `dtype` float64 keeps the unrounded placement): at camera-space (0, 0, 2); shifted so that its centre lies on the image's
    right border; behind the camera; across the camera plane."""
    V, F = gold(name)
    V = V * (0.6 / np.abs(V).max())
    H, W = size
    f, cx = float(consts[0]), float(consts[1])
    at = {"in_view": (0.0, 0.0, 2.0), "partly": (2.0 * (W - 1 - cx) / f, 0.0, 2.0), "behind": (0.0, 0.0, -2.0),
          "straddling": (0.0, 0.0, 0.3)}[where]
    return R.camera_to_grid(V + np.array(at), consts).astype(dtype), F


def case(size, mesh, where, dtype=np.float32):
    """-> (vertices, faces, consts, the oracle's depth map of exactly these vertices)."""
    key = (tuple(size), mesh, where, np.dtype(dtype).name)
    if key not in _cache:
        consts = R.make_consts(*size)
        V, F = placed(mesh, where, size, consts, dtype)
        depth = R.render(V, F, consts, size)["depth"]
        for a in (V, F, depth):
            a.setflags(write=False)
        _cache[key] = (V, F, consts, depth)
    return _cache[key]


def random_image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


def ramp_image(Hi, Wi):
    """red = column, green = row, blue = 7 (Hi, Wi <= 256)."""
    img = np.empty((Hi, Wi, 3), dtype=np.uint8)
    img[..., 0] = np.arange(Wi, dtype=np.uint8)[None, :]
    img[..., 1] = np.arange(Hi, dtype=np.uint8)[:, None]
    img[..., 2] = 7
    return img


def one_cell(consts):
    return 1.0 / float(np.asarray(consts, dtype=np.float32)[7])
