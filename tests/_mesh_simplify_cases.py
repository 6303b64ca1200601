"""The seeded meshes that tests/test_mesh_simplify_cpu.py and tests/test_gpu_mesh_simplify.py share: ``CASES`` maps a name to a
function -> (vertices (V, 3) float32, faces (F, 3) int32, cell).  Small on purpose: each shape is the smallest at which the
kernels of csrc/mesh_simplify.hip take another path (a wave of 64, a second block of 256, every thread on one slot, no two
threads on one slot, long probe walks, a wave whose vertices share a cluster or do not)."""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
TORUS_CENTRE, TORUS_R, TORUS_r = (16.3, 16.1, 8.2), 10.0, 4.0
TORUS_GRIDS = {"small": (96, 48), "large": (400, 200)}


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1, 3).astype(np.int32))


def torus(nu, nv, centre=TORUS_CENTRE, R=TORUS_R, r=TORUS_r):
    """A closed torus around the z axis through `centre`: nu x nv quads, each split into two triangles of one orientation."""
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    uu, vv = np.meshgrid(u, v, indexing="ij")
    ring = R + r * np.cos(vv)
    p = np.stack([ring * np.cos(uu), ring * np.sin(uu), r * np.sin(vv)], axis=-1) + np.asarray(centre, dtype=np.float64)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    idx = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)      # noqa: E731
    a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
    faces = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3)
    return _f32(p), _i32(faces)


def _sizes(V, with_faces):
    def case():                                          # around the wave and the block; about four vertices per cell
        rng = _rng(100 + V)
        v = rng.uniform(0, max(1.0, (V / 4) ** (1 / 3)), size=(V, 3))
        f = rng.integers(0, V, size=(min(V, 7), 3)) if with_faces and V else np.zeros((0, 3))
        return _f32(v), _i32(f), 1.0
    return case


def one_cell():                                          # every thread meets on one slot; every face is degenerate: an empty mesh
    rng = _rng(1)
    return _f32(rng.uniform(4.01, 4.99, size=(700, 3))), _i32(rng.integers(0, 700, size=(900, 3))), 1.0


def own_cells():                                         # a 9 x 8 x 7 lattice, one vertex per cell, strips along it: the identity
    g = np.stack(np.meshgrid(np.arange(9), np.arange(8), np.arange(7), indexing="ij"), axis=-1).reshape(-1, 3)
    v = g * 0.75 + _rng(2).uniform(0.05, 0.7, size=g.shape) - 3.0
    i = np.arange(len(g) - 2)
    return _f32(v), _i32(np.stack([i, i + 1, i + 2], axis=1)), 0.75


def _boundaries(cell):
    def case():                                          # k * cell in float32, its float32 neighbours, 0.0, -0.0, negatives
        c = np.float32(cell)
        k = np.arange(-12, 13, dtype=np.float32)
        on = k * c
        x = np.concatenate([on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf)),
                            np.array([0.0, -0.0, -c, c, -c / 2, c / 2], dtype=np.float32)]).astype(np.float32)
        rng = _rng(3)
        v = np.stack([x, rng.permutation(x), rng.permutation(x)], axis=1)
        v = np.concatenate([v, np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0]], dtype=np.float32)])
        f = rng.integers(0, len(v), size=(150, 3))
        return _f32(v), _i32(f), float(cell)
    return case


def bad_indices():                                       # faces holding -1, V, INT32_MIN or INT32_MAX among valid ones
    V = 40
    v = _rng(4).uniform(0, 6, size=(V, 3))
    i = np.arange(20)
    good = np.stack([i, i + 1, i + 2], axis=1)
    bad = [[0, 1, -1], [V, 2, 3], [4, INT32_MIN, 5], [INT32_MAX, 30, 31], [30, 31, V], [-1, -1, -1], [32, 33, INT32_MAX]]
    return _f32(v), _i32(np.concatenate([good[:9], bad[:4], good[9:], bad[4:], [[30, 31, 32], [35, 36, 37]]])), 1.0


def unclusterable():                                     # NaN, +-inf, |v| >= 2^16 and the last float below it, and the faces that use them
    rng = _rng(5)
    v = rng.uniform(0, 5, size=(200, 3)).astype(np.float32)
    below = np.nextafter(np.float32(65536.0), np.float32(0))
    special = [np.nan, np.inf, -np.inf, 65536.0, -65536.0, 1e30, below, -below]
    for n, value in enumerate(special * 3):
        v[7 * n + 3, n % 3] = value
    v[190] = np.nan
    f = rng.integers(0, 200, size=(400, 3))
    return _f32(v), _i32(f), 1.0


def duplicates():                                        # rotated duplicates, an opposite pair, faces repeating an index or a cluster
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [0.6, 0.4, 0.5], [1.4, 0.6, 0.5], [2.5, 2.5, 2.5],
                  [2.5, 3.5, 2.5]])
    # clusters: {0, 4}, {1, 5}, {2}, {3}, {6}, {7}
    f = [[1, 2, 0], [0, 1, 2], [2, 0, 1], [4, 5, 2], [0, 2, 1], [2, 1, 0], [0, 0, 1], [0, 4, 2], [3, 3, 3], [5, 2, 4], [0, 1, 3], [3, 0, 1],
         [6, 7, 6], [1, 3, 2]]
    return _f32(v), _i32(f), 1.0


def _random(extent, seed):
    def case():                                          # 20 000 vertices over extent[0] x extent[1] x extent[2] cells, 40 000 faces
        rng = _rng(seed)
        e = np.asarray(extent, dtype=np.float64)
        v = rng.uniform(0, 1, size=(20000, 3)) * e - e // 2
        return _f32(v), _i32(rng.integers(0, 20000, size=(40000, 3))), 1.0
    return case


def _torus(grid, cell):
    def case():
        return (*torus(*TORUS_GRIDS[grid]), cell)
    return case


def wave_runs():                                         # runs of 64, 64, 1, 63, 200 and 8 vertices per cluster, then alternating ones
    runs = [64, 64, 1, 63, 200, 8] + [1] * 130
    rng = _rng(6)
    v = np.concatenate([rng.uniform(0.05, 0.95, size=(n, 3)) + np.array([c % 2, 3 * c, 0.0]) for c, n in enumerate(runs)])
    return _f32(v), _i32(rng.integers(0, len(v), size=(600, 3))), 1.0


TORUS_CELLS = (1.0, 1.5, 2.0, 3.0, 0.3)
CASES = {
    **{f"v{V}_no_faces": _sizes(V, False) for V in (0, 1, 63, 64, 65, 257)},
    **{f"v{V}_faces": _sizes(V, True) for V in (0, 1, 63, 64, 65, 257)},
    "one_cell": one_cell, "own_cells": own_cells, "boundaries_1.5": _boundaries(1.5), "boundaries_0.3": _boundaries(0.3),
    "bad_indices": bad_indices, "unclusterable": unclusterable, "duplicates": duplicates, "wave_runs": wave_runs,
    "random_50_cells": _random((5, 5, 2), 7), "random_15000_cells": _random((25, 25, 24), 8),   # contention; probing
    **{f"torus_{grid}_{cell}": _torus(grid, cell) for grid in TORUS_GRIDS for cell in TORUS_CELLS},
}
TORI = [name for name in CASES if name.startswith("torus_")]
GPU_CASES = [name for name in CASES if not name.startswith("torus_") or name.rsplit("_", 1)[1] in ("0.3", "1.5", "2.0")]
_cache = {}


def case(name):
    """The arrays of a case, built once; callers must not write to them."""
    if name not in _cache:
        v, f, cell = CASES[name]()
        v.setflags(write=False)
        f.setflags(write=False)
        _cache[name] = (v, f, cell)
    return _cache[name]
