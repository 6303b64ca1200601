"""The shared meshes of the mesh-preview tests (tests/test_mesh_render_cpu.py, tests/test_gpu_mesh_render.py): float32 vertices,
int32 faces, seeded, read-only; the oracle's result per case is computed once and shared."""
import numpy as np

from tests import mesh_render_oracle as O
from tests import raycast_oracle as R

_made, _want = {}, {}


def _octahedron():
    v = np.array([[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]], dtype=np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)   # outward
    return v, f


def _cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32) * np.float32(3.5) + np.float32(0.25)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]                            # outward
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    return v, f


def _strip(n=33):
    rng = np.random.default_rng(41)
    x = np.arange(n, dtype=np.float64)
    v = np.concatenate([np.stack([x, np.zeros(n), np.sin(x / 3)], axis=1), np.stack([x, np.ones(n), np.cos(x / 4)], axis=1)])
    v = (v + 0.05 * rng.standard_normal(v.shape)).astype(np.float32)
    f = np.array([t for i in range(n - 1) for t in ((i, i + 1, n + i), (i + 1, n + i + 1, n + i))], dtype=np.int32)
    return v, f


def _fan(k=40):
    rng = np.random.default_rng(42)
    a = 2 * np.pi * np.arange(k) / k
    rim = np.stack([5 * np.cos(a), 5 * np.sin(a), rng.uniform(-0.5, 0.5, k)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], rim]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], dtype=np.int32)
    return v, f


def _coincident():
    v = np.array([[0, 0, 0], [4, 0, 0.5], [0, 3, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int32)


def _lone_vertex():
    v, f = _cube()
    return np.concatenate([v, [[9.0, 9.0, 9.0]]]).astype(np.float32), f


def _bad():
    """Faces with an index out of range (both sides), a repeated index, a NaN, an infinite and a 2^16 vertex, between good ones."""
    rng = np.random.default_rng(43)
    v = rng.uniform(-8, 8, (24, 3)).astype(np.float32)
    v[5, 1] = np.nan
    v[9, 0] = np.float32(65536.0)
    v[13, 2] = -np.inf
    v[17, 0] = np.float32(65535.996)                         # the largest usable magnitude
    f = rng.integers(0, 24, (60, 3)).astype(np.int32)
    f[3] = [1, 24, 2]
    f[7] = [-1, 4, 6]
    f[11] = [2 ** 31 - 1, 0, 1]
    f[15] = [-2 ** 31, 3, 4]
    f[19] = [6, 6, 7]
    f[23] = [8, 10, 8]
    return v, f


def _mc_sphere():
    from tests import mc_oracle as MC
    v, f = MC.marching_cubes(MC.sphere(12, 4.2), 0.0)
    return v.astype(np.float32), f.astype(np.int32)


BUILDERS = {"octahedron": _octahedron, "cube": _cube, "strip": _strip, "fan": _fan, "coincident": _coincident,
            "lone_vertex": _lone_vertex, "bad": _bad,
            "no_vertices": lambda: (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
            "no_faces": lambda: (np.random.default_rng(44).uniform(-3, 3, (70, 3)).astype(np.float32), np.zeros((0, 3), np.int32)),
            "faces_without_vertices": lambda: (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32)),
            "mc_sphere": _mc_sphere}
CASES = tuple(BUILDERS)


def case(name):
    if name not in _made:
        v, f = BUILDERS[name]()
        v.setflags(write=False)
        f.setflags(write=False)
        _made[name] = (v, f)
    return _made[name]


def oracle(name):
    if name not in _want:
        _want[name] = O.vertex_normals(*case(name))
    return _want[name]


def shuffled(name, seed=5):
    """The same mesh with its faces permuted and every face's indices rotated cyclically (the winding stays)."""
    v, f = case(name)
    rng = np.random.default_rng(seed)
    g = f[rng.permutation(len(f))]
    shift = rng.integers(0, 3, len(g))
    return v, np.stack([g[np.arange(len(g)), (k + shift) % 3] for k in range(3)], axis=1).astype(np.int32)


# ---- rendering: the closed meshes placed in front of the camera of raycast_oracle.make_consts(H, W) -------------------------------
RENDER_MESHES = ("mc_sphere", "octahedron")


def placed(name, consts, at=(0.0, 0.0, 2.0), extent=0.6):
    """The case's mesh centred, scaled to a largest |coordinate| of `extent` metres, turned a little so that no face is
    edge-on or axis-aligned, and put at camera-space `at` -> (vertices float32 in grid units, faces)."""
    v, f = case(name)
    p = v.astype(np.float64)
    p = p - (p.min(axis=0) + p.max(axis=0)) / 2
    a, b = 0.4, 0.3
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    p = (p * (extent / np.abs(p).max())) @ (Rx @ Ry).T + np.asarray(at)
    return R.camera_to_grid(p, consts).astype(np.float32), f


def vertex_palette(n, seed=9):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def half_plane(consts, W):
    """Two faces that cover the image's left half and more: a wall at 2 m from far left to the column (W - 1) / 2 - 0.25."""
    k = np.asarray(consts, dtype=np.float64)
    x1 = (((W - 1) / 2 - 0.25) - k[1]) / k[0] * 2.0
    p = np.array([[-50.0, -50.0, 2.0], [x1, -50.0, 2.0], [x1, 50.0, 2.0], [-50.0, 50.0, 2.0]])
    return R.camera_to_grid(p, consts).astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
