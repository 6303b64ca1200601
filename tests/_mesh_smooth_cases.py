"""The seeded meshes that tests/test_mesh_smooth_cpu.py and tests/test_gpu_mesh_smooth.py share: ``CASES`` maps a name to a
function -> (vertices (V, 3) float32, faces (F, 3) int32, {iterations, lam, mu}); every case runs with `fix_boundary` on and
off.  Small on purpose: each shape is the smallest at which the kernels of csrc/mesh_smooth.hip take another path (a wave of
64, a second block of 256, no face at all, a list of 700 entries in one thread, a list per thread, indices that are no
vertex, vertices that are no position, the clamp)."""
import numpy as np

from tests import _mesh_simplify_cases as SC

DEFAULT = {"iterations": 10, "lam": 0.5, "mu": -0.53}
HUB_RIM = 700
CLAMP_HI, CLAMP_LO = 60000.0, -30000.0
OPEN_N, OPEN_R = 24, 14.0


def _with(v, f, **kw):
    return SC._f32(v), SC._i32(f), {**DEFAULT, **kw}


def _from_simplify(name, **kw):
    def case():
        v, f, _ = SC.CASES[name]()
        return _with(v, f, **kw)
    return case


def _torus(nu, nv, **kw):
    def case():
        return _with(*SC.torus(nu, nv), **kw)
    return case


def binary_sphere(n=24, r=8.0):
    """The occupancy of a sphere on an n^3 lattice as marching cubes sees it from a near-binary network: 1 outside, 0 inside."""
    from tests import mc_oracle
    return (mc_oracle.sphere(n, r) > 0).astype(np.float32)


def _sphere(kind):
    def case():
        from tests import mc_oracle
        if kind == "binary":
            v, f = mc_oracle.marching_cubes(binary_sphere(), 0.5)
        elif kind == "sdf":
            v, f = mc_oracle.marching_cubes(mc_oracle.sphere(24, 8.0), 0.0)
        else:                                            # radius 14 on 24^3: the lattice border cuts six caps off
            v, f = mc_oracle.marching_cubes(mc_oracle.sphere(OPEN_N, OPEN_R), 0.0)
        return _with(v, f)
    return case


def hub_fan():                                           # an apex and a rim of 700: one list of 700 entries, 700 lists of two
    t = 2 * np.pi * np.arange(HUB_RIM) / HUB_RIM
    v = np.concatenate([[[3.0, 2.0, 5.0]], np.stack([3 + 40 * np.cos(t), 2 + 40 * np.sin(t), 1 + 0 * t], axis=1)])
    k = np.arange(HUB_RIM)
    return _with(v, np.stack([0 * k, 1 + k, 1 + (k + 1) % HUB_RIM], axis=1))


def repeated_index():                                    # (a, a, b), (a, b, a), (b, a, a), (a, a, a) among the faces of a tetrahedron
    v = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4], [9, 9, 9]]
    f = [[0, 2, 1], [1, 1, 2], [0, 1, 3], [2, 3, 2], [0, 3, 2], [3, 1, 1], [1, 2, 3], [4, 4, 4], [0, 4, 0]]
    return _with(v, f, iterations=3)


def tetrahedron():                                       # closed, outward; worked out by hand in the CPU test
    v = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 4]]
    return _with(v, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], iterations=1, lam=0.5, mu=0.0)


def _clamp(n):
    def case():                                          # torus(6, 6) with x = 60000 on colour (i + j) % 3 == 0, -30000 elsewhere
        v, f = SC.torus(6, 6)
        i, j = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
        v = v.copy()
        v[:, 0] = np.where((i + j).reshape(-1) % 3 == 0, CLAMP_HI, CLAMP_LO)
        return _with(v, f, iterations=n, lam=1.0, mu=-1.0)
    return case


CASES = {
    **{f"v{V}_no_faces": _from_simplify(f"v{V}_no_faces") for V in (0, 1, 63, 64, 65, 257)},
    **{f"v{V}_faces": _from_simplify(f"v{V}_faces") for V in (0, 1, 63, 64, 65, 257)},
    "torus_n1": _torus(96, 48, iterations=1), "torus_n10": _torus(96, 48), "torus_n0": _torus(96, 48, iterations=0),
    "torus_mu0": _torus(96, 48, mu=0.0, iterations=5),
    "sphere_binary": _sphere("binary"), "sphere_sdf": _sphere("sdf"), "sphere_open": _sphere("open"),
    "hub_fan": hub_fan, "repeated_index": repeated_index, "tetrahedron": tetrahedron,
    **{name: _from_simplify(name, iterations=3) for name in ("bad_indices", "unclusterable", "duplicates", "one_cell", "random_50_cells",
                                                            "random_15000_cells")},
    **{f"clamp_n{n}": _clamp(n) for n in (3, 4, 9)},
}
MODES = (True, False)                                    # fix_boundary
_cache, _want = {}, {}


def case(name):
    """The arrays and arguments of a case, built once; callers must not write to them."""
    if name not in _cache:
        v, f, kw = CASES[name]()
        v.setflags(write=False)
        f.setflags(write=False)
        _cache[name] = (v, f, kw)
    return _cache[name]


def oracle(name, fix_boundary):
    """The oracle's result of a case in one boundary mode, computed once and shared by the tests."""
    from tests import mesh_smooth_oracle as O
    key = (name, bool(fix_boundary))
    if key not in _want:
        v, f, kw = case(name)
        _want[key] = O.smooth(v, f, fix_boundary=fix_boundary, **kw)
    return _want[key]
