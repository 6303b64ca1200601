"""The seeded meshes that tests/test_mesh_components_cpu.py and tests/test_gpu_mesh_components.py share: ``CASES`` maps a name
to a function -> (vertices (V, 3) float32, faces (F, 3) int32, mark (V,) uint8 or None).  Small on purpose: each shape is
the smallest at which the kernels of csrc/mesh_components.hip take another path (a second block of 256, a second block of
the scan, a wave of 64 with one or two labels, a long find() chain, one contended root)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def golden_mesh(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return z["vertices"].astype(np.float32), z["faces"].astype(np.int32)


def _rng(seed):
    return np.random.default_rng(seed)


def _coords(V, seed):
    return _rng(seed).uniform(-4, 4, size=(V, 3)).astype(np.float32)


def _mesh(V, faces, seed, mark=False):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3).astype(np.int32)
    m = (_rng(seed + 1000).random(V) < 0.3).astype(np.uint8) if mark else None
    return _coords(V, seed), faces, m


def _renamed(faces, order):
    """vertex i becomes order[i]"""
    return np.asarray(order, dtype=np.int64)[np.asarray(faces, dtype=np.int64)]


def _strip(V):
    i = np.arange(V - 2)
    return np.stack([i, i + 1, i + 2], axis=1)


def empty():
    return _mesh(0, np.zeros((0, 3)), 1)


def five_isolated():
    return _mesh(5, np.zeros((0, 3)), 2, mark=True)


def one_triangle():
    return _mesh(3, [[0, 1, 2]], 3, mark=True)


def strip_ascending():
    return _mesh(3000, _strip(3000), 4)


def strip_descending():                                  # vertex i is named 2999 - i: the smallest id is at the far end of every path
    return _mesh(3000, _renamed(_strip(3000), np.arange(3000)[::-1]), 5)


def strip_permuted():
    return _mesh(3000, _renamed(_strip(3000), _rng(6).permutation(3000)), 6, mark=True)


def _fan(hub, rim):
    return np.stack([np.full(len(rim) - 1, hub), rim[:-1], rim[1:]], axis=1)


def fan_hub_first():                                     # 1000 faces, every link ends at root 0
    return _mesh(1002, _fan(0, np.arange(1, 1002)), 7)


def fan_hub_last():                                      # the hub is the largest id: it is hooked once, then every link chases the rim
    return _mesh(1002, _fan(1001, np.arange(0, 1001)), 8)


def disjoint_triangles():                                # C = 5000 roots interleaved over 15000 vertices: past one block of the scan
    order = _rng(9).permutation(15000)
    return _mesh(15000, _renamed(np.arange(15000).reshape(5000, 3), order), 9, mark=True)


def two_combs():                                         # even ids one component, odd ids the other
    i = np.arange(0, 596, 2)
    even = np.stack([i, i + 2, i + 4], axis=1)
    return _mesh(600, np.concatenate([even, even + 1]), 10)


def golden_three():                                      # sphere + torus + open box, ids permuted, faces shuffled
    vs, fs, base = [], [], 0
    for name in ("mesh_sphere", "mesh_torus", "mesh_openbox"):
        v, f = golden_mesh(name)
        vs.append(v)
        fs.append(f.astype(np.int64) + base)
        base += len(v)
    v, f = np.concatenate(vs), np.concatenate(fs)
    rng = _rng(11)
    order = rng.permutation(len(v))
    out = np.empty_like(v)
    out[order] = v
    f = _renamed(f, order)[rng.permutation(len(f))]
    return out, f.astype(np.int32), (rng.random(len(v)) < 0.5).astype(np.uint8)


def scene_mesh():
    v, f = golden_mesh("scene_mesh_00000")
    return v, f, (_rng(12).random(len(v)) < 0.1).astype(np.uint8)


def bad_indices():                                       # faces holding -1, V, INT32_MIN or INT32_MAX among valid ones
    V = 40
    good = _strip(20)
    bad = [[0, 1, -1], [V, 2, 3], [4, INT32_MIN, 5], [INT32_MAX, 30, 31], [30, 31, V], [-1, -1, -1], [32, 33, INT32_MAX]]
    f = np.concatenate([good[:9], bad[:4], good[9:], bad[4:], [[30, 31, 32], [35, 36, 37]]])
    return _mesh(V, f, 13, mark=True)


def repeated_indices():                                  # (a, a, b), (a, a, a) and duplicate faces
    f = [[0, 0, 1], [2, 2, 2], [3, 4, 4], [5, 3, 5], [6, 7, 8], [6, 7, 8], [8, 7, 6], [9, 9, 9], [1, 10, 10]]
    return _mesh(12, f, 14, mark=True)


def _isolated(n):
    def case():                                          # n isolated vertices behind one triangle: around the wave and the block
        return _mesh(n + 3, [[n, n + 1, n + 2]], 20 + n, mark=True)
    return case


def _by_label(labels, seed, special=False):
    """A mesh whose vertex i lies in the component numbered labels[i]: every component is a strip over its vertices in order
    (components of one or two vertices: a face that repeats an index)."""
    labels = np.asarray(labels)
    faces = []
    for c in np.unique(labels):
        ids = np.flatnonzero(labels == c)
        if len(ids) >= 3:
            faces.append(np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1))
        else:
            faces.append(np.array([[ids[0], ids[0], ids[-1]]]))
    v, f, m = _mesh(len(labels), np.concatenate(faces), seed, mark=True)
    if special:
        v = _special(v, seed)
    return v, f, m


def wave_uniform():                                      # 64 vertices per label: every wave of the statistics kernel is uniform
    return _by_label(np.repeat(np.arange(5), 64), 30)


def wave_alternating():
    return _by_label(np.arange(320) % 2, 31)


def wave_one_lane_off():                                 # uniform but for one lane, in the first and in a later wave
    labels = np.zeros(300, dtype=np.int64)
    labels[[17, 170]] = 1
    return _by_label(labels, 32)


def _special(v, seed):
    rng = _rng(seed + 500)
    v = v.copy()
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random(v.shape) < 0.25
    v[hit] = vals[rng.integers(0, 5, size=int(hit.sum()))]
    return v


def special_coordinates():                               # NaN, +-inf, +-0 in uniform waves, in mixed ones, and a component that is all NaN
    v, f, m = _by_label(np.concatenate([np.repeat(np.arange(3), 64), np.arange(128) % 4 + 3, [7, 7, 7]]), 33, special=True)
    v[-3:] = np.nan
    v[:64, 1] = np.nan                                   # a whole uniform wave without a value on one axis
    v[64:128, 0] = np.where(np.arange(64) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    return v, f, m


CASES = {
    "empty": empty, "five_isolated": five_isolated, "one_triangle": one_triangle, "strip_ascending": strip_ascending,
    "strip_descending": strip_descending, "strip_permuted": strip_permuted, "fan_hub_first": fan_hub_first,
    "fan_hub_last": fan_hub_last, "disjoint_triangles": disjoint_triangles, "two_combs": two_combs, "golden_three": golden_three,
    "scene_mesh": scene_mesh, "bad_indices": bad_indices, "repeated_indices": repeated_indices,
    **{f"isolated_{n}": _isolated(n) for n in (63, 64, 65, 255, 256, 257)},
    "wave_uniform": wave_uniform, "wave_alternating": wave_alternating, "wave_one_lane_off": wave_one_lane_off,
    "special_coordinates": special_coordinates,
}
# no invalid face and no isolated vertex: keeping every component is the identity
WHOLE = ("one_triangle", "strip_ascending", "strip_permuted", "fan_hub_last", "disjoint_triangles", "two_combs", "golden_three",
         "scene_mesh", "wave_uniform", "wave_alternating", "wave_one_lane_off")
_cache = {}


def case(name):
    """The arrays of a case, built once; callers must not write to them."""
    if name not in _cache:
        arrays = CASES[name]()
        for a in arrays:
            if a is not None:
                a.setflags(write=False)
        _cache[name] = arrays
    return _cache[name]
