"""GPU: the block-sparse lattice kernels (csrc/sparse_lattice.hip) and their driver (util/sparse_grid.py) against the numpy
oracle of tests/sparse_lattice_oracle.py -- state, field, point and round counts, per-round leak counts, all exact -- the
coordinates against make_3d_grid bit for bit, and the IF-Net entry points (evaluate_network_on_grid_sparse,
implicit_to_mesh(block=...)) against the dense path."""
import numpy as np
import pytest
import torch

from oracle import ifnet_oracle as O
from tests import sparse_lattice_oracle as S

pytestmark = pytest.mark.gpu

NORMAL = [float(v) for v in S.NORMAL.astype(np.float32)]


# ---- analytic fields from separate elementwise torch ops: a point's value does not depend on the rows around it ----------
def _sq(p, c=(0.0, 0.0, 0.0)):
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return dx * dx + dy * dy + dz * dz


def _dot_n(p):
    return p[:, 0] * NORMAL[0] + p[:, 1] * NORMAL[1] + p[:, 2] * NORMAL[2]


def f_sphere(p):
    return torch.sqrt(_sq(p)) - 0.3


def f_torus(p):
    q = torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) - 0.28
    return torch.sqrt(q * q + p[:, 2] * p[:, 2]) - 0.11


def f_slab(p):
    return torch.abs(_dot_n(p) - 0.03) - 0.02


def f_plane(p):
    return _dot_n(p) - 0.03


def f_sphere_nan(p):
    v = f_sphere(p)
    return torch.where(p[:, 2] > 0.1, torch.full_like(v, float("nan")), v)


def f_speck(p):
    return torch.sqrt(_sq(p, (0.31, 0.29, 0.33))) - 0.02


FN = {"sphere": f_sphere, "torus": f_torus, "slab": f_slab, "plane": f_plane, "sphere_nan": f_sphere_nan, "speck": f_speck}

# (field, lattice, block, exact: the sparse field has the dense sides everywhere)
CASES = [("sphere", (64, 64, 64), 4, True), ("torus", (64, 64, 64), 4, True), ("slab", (64, 64, 64), 4, True),
         ("plane", (64, 64, 64), 4, True), ("sphere", (37, 30, 23), 8, None), ("slab", (37, 30, 23), 8, True),
         ("torus", (37, 30, 23), 4, None), ("plane", (19, 18, 17), 8, None), ("sphere", (19, 18, 17), 2, None),
         ("sphere", (19, 18, 17), 3, None), ("sphere_nan", (37, 30, 23), 4, None), ("speck", (64, 64, 64), 4, False)]


def _tools():
    import svr_amd  # noqa: F401
    from svr_amd.model import make_3d_grid
    from svr_amd.util.sparse_grid import sparse_lattice_field
    from svr_amd.util.visualize import marching_cubes
    return make_3d_grid, sparse_lattice_field, marching_cubes


_DENSE = {}


def _dense(name, shape):
    """The dense field on the device (fn on make_3d_grid's rows), computed once per case and left unchanged."""
    if (name, shape) not in _DENSE:
        make_3d_grid = _tools()[0]
        grid = make_3d_grid((-0.5,) * 3, (0.5,) * 3, shape).cuda()
        _DENSE[name, shape] = (grid, FN[name](grid).view(*shape))
    return _DENSE[name, shape]


def _same_as_oracle(got, want):
    assert got.state.dtype == torch.uint8 and got.field.dtype == torch.float32 and got.field.is_cuda and got.state.is_cuda
    assert (got.rounds, got.n_points, got.leaks, got.fell_back) == (want.rounds, want.n_points, want.leaks, want.fell_back)
    assert np.array_equal(got.state.cpu().numpy(), want.state)
    assert torch.equal(got.field.cpu().view(torch.int32), torch.from_numpy(want.field).view(torch.int32))    # NaN included


@pytest.mark.parametrize("name,shape,s,exact", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}-s{c[2]}" for c in CASES])
def test_kernels_equal_oracle(name, shape, s, exact):
    _, sparse_lattice_field, marching_cubes = _tools()
    _, dense = _dense(name, shape)
    want = S.sparse_field(dense.cpu().numpy(), 0.0, s)
    got = sparse_lattice_field(FN[name], shape, 0.0, s)
    _same_as_oracle(got, want)
    assert S.leak_free(want.field, want.evaluated, 0.0)
    sides_equal = np.array_equal(S.inside(want.field, 0.0), S.inside(dense.cpu().numpy(), 0.0))
    if exact is not None:
        assert sides_equal == exact
    if name == "speck":
        assert got.rounds == 0 and marching_cubes(got.field, 0.0)[1].shape[0] == 0
    else:
        assert got.rounds >= 1
    if sides_equal:
        (gv, gf), (wv, wf) = marching_cubes(got.field, 0.0), marching_cubes(dense, 0.0)
        assert wf.shape[0] > 100 and torch.equal(gv, wv) and torch.equal(gf, wf)
    # a small chunk size changes nothing
    if shape != (64, 64, 64):
        _same_as_oracle(sparse_lattice_field(FN[name], shape, 0.0, s, points_batch_size=1000), want)


def test_round_cap_falls_back_to_every_block():
    _, sparse_lattice_field, _ = _tools()
    shape = (37, 30, 23)
    _, dense = _dense("slab", shape)
    assert S.sparse_field(dense.cpu().numpy(), 0.0, 8).rounds >= 3
    want = S.sparse_field(dense.cpu().numpy(), 0.0, 8, max_rounds=2)
    got = sparse_lattice_field(f_slab, shape, 0.0, 8, max_rounds=2)
    _same_as_oracle(got, want)
    assert got.fell_back and got.rounds == 3 and torch.equal(got.field, dense) and bool((got.state != 0).all())


@pytest.mark.parametrize("name,shape,s", [("slab", (37, 30, 23), 8), ("sphere", (19, 18, 17), 3)])
def test_point_lists_are_rows_of_make_3d_grid(name, shape, s):
    _, sparse_lattice_field, _ = _tools()
    grid, dense = _dense(name, shape)
    seen = []

    def fn(p):
        seen.append(p.clone())
        return FN[name](p)

    got = sparse_lattice_field(fn, shape, 0.0, s, points_batch_size=1 << 30)      # one call per list
    assert len(seen) == 1 + got.rounds
    rows = grid.view(*shape, 3).cpu()
    coarse = [S.axis_blocks(n, s)[2] for n in shape]
    idx = np.stack(np.meshgrid(*coarse, indexing="ij"), axis=-1).reshape(-1, 3)
    want = S.sparse_field(dense.cpu().numpy(), 0.0, s)
    lists = [idx] + [S.point_list(shape, s, np.nonzero(want.state.reshape(-1) == r)[0]) for r in range(1, want.rounds + 1)]
    for p, idx in zip(seen, lists):
        assert p.dtype == torch.float32 and p.is_cuda and p.shape == (len(idx), 3)
        assert torch.equal(p.cpu().view(torch.int32), rows[idx[:, 0], idx[:, 1], idx[:, 2]].view(torch.int32))


def test_refusals():
    _, sparse_lattice_field, _ = _tools()
    from svr_amd.model import evaluate_network_on_grid_sparse, implicit_to_mesh
    for shape, s in (((16, 16, 16), 1), ((16, 16, 16), 0), ((16, 1, 16), 4), ((1, 16, 16), 4), ((16, 16, 1), 4)):
        with pytest.raises(RuntimeError, match="bad lattice"):
            sparse_lattice_field(f_sphere, shape, 0.0, s)
    with pytest.raises(RuntimeError, match="GPU"):
        sparse_lattice_field(lambda p: f_sphere(p).cpu(), (16, 16, 16), 0.0, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        sparse_lattice_field(f_sphere, (16, 16, 16), 0.0, 4, device="cpu")
    with pytest.raises(ValueError):
        sparse_lattice_field(f_sphere, (16, 16, 16), 0.0, 4, max_rounds=0)
    m = _model()
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate_network_on_grid_sparse(m, torch.zeros(1, 1, 16, 16, 16), (16, 16, 16), 0.5)
    with pytest.raises(ValueError):
        implicit_to_mesh(m, torch.zeros(1, 1, 16, 16, 16).cuda(), (16, 16, 16), 0.5, "unused.obj", block=1)


# ---- the real network ----------------------------------------------------------------------------------------------------
DIMS = (70, 52, 56)


def _model():
    import svr_amd  # noqa: F401
    from svr_amd.model import IFNet
    m = IFNet(net_res=128)
    m.load_state_dict(O.name_seeded_state(128), strict=False)
    return m.cuda().eval()


def _shell():
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in DIMS], indexing="ij"), axis=-1)
    d = np.sqrt(((g - (np.array(DIMS) - 1) / 2.0) ** 2).sum(-1))
    return torch.from_numpy((np.abs(d - 18.0) < 0.8).astype(np.float32)).reshape(1, 1, *DIMS).cuda()


_NET = {}


def _network_case():
    """Model, input, the dense field 1 - p at two chunk sizes (the parent's code path), and a level with a large surface."""
    if not _NET:
        from svr_amd.model import evaluate_network_on_grid_device
        m, x = _model(), _shell()
        dense = 1 - evaluate_network_on_grid_device(m, x, DIMS, 1, points_batch_size=32768)
        dense_small = 1 - evaluate_network_on_grid_device(m, x, DIMS, 1, points_batch_size=4096)
        level = float(dense.view(-1)[::97].median())
        _NET.update(m=m, x=x, dense=dense, d0=float((dense - dense_small).abs().max()), level=level)
    return _NET


def _device_leak_free(field, state, level, s):
    own = [torch.from_numpy(S.axis_blocks(n, s)[1]).to(field.device) for n in field.shape]
    ev = (state != 0)[own[0][:, None, None], own[1][None, :, None], own[2][None, None, :]]
    side = field.double() < level
    for a in range(3):
        lo, hi = side.narrow(a, 0, side.shape[a] - 1), side.narrow(a, 1, side.shape[a] - 1)
        both = ev.narrow(a, 0, side.shape[a] - 1) & ev.narrow(a, 1, side.shape[a] - 1)
        if bool(((lo != hi) & ~both).any()):
            return False, ev
    return True, ev


@pytest.mark.parametrize("which", ["half", "median"])
def test_network_values_equal_the_dense_path(which):
    from svr_amd.model import evaluate_network_on_grid_sparse
    c = _network_case()
    level = 0.5 if which == "half" else c["level"]
    r = evaluate_network_on_grid_sparse(c["m"], c["x"], DIMS, level, block=8)
    ok, ev = _device_leak_free(r.field, r.state, level, 8)
    assert ok
    diff = float((r.field - c["dense"])[ev].abs().max()) if bool(ev.any()) else 0.0
    print(f"d0 = {c['d0']:.3e}  sparse vs dense at evaluated points = {diff:.3e}  level = {level:.6f}  rounds = {r.rounds}  "
          f"evaluated fraction = {r.evaluated_fraction:.3f}  leaks = {r.leaks}")
    assert diff <= 2 * c["d0"]
    if which == "median":
        assert r.rounds >= 1 and bool(ev.any())
    # an unevaluated point holds the value of its block's minimum corner
    own = [torch.from_numpy(np.minimum(np.arange(n) // 8, S.axis_blocks(n, 8)[0] - 1) * 8).cuda() for n in DIMS]
    corner = r.field[own[0][:, None, None], own[1][None, :, None], own[2][None, None, :]]
    assert torch.equal(r.field[~ev], corner[~ev])


def test_implicit_to_mesh_block_writes_the_mesh_of_the_sparse_field(tmp_path):
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.model import evaluate_network_on_grid_sparse, implicit_to_mesh
    from svr_amd.util.visualize import marching_cubes
    c = _network_case()
    level = c["level"]
    v, f = implicit_to_mesh(c["m"], c["x"], DIMS, level, tmp_path / "sparse.obj", block=8)
    assert v.is_cuda and f.is_cuda and f.shape[0] > 1000
    back = load_obj(str(tmp_path / "sparse.obj"))
    assert np.array_equal(back.vertices.astype(np.float32).view(np.uint32), v.cpu().numpy().view(np.uint32))
    assert np.array_equal(back.faces, f.cpu().numpy())
    r = evaluate_network_on_grid_sparse(c["m"], c["x"], DIMS, level, block=8)
    sv, sf = marching_cubes(r.field, level)
    assert torch.equal(v, sv) and torch.equal(f, sf)
    sides_equal = torch.equal(r.field.double() < level, c["dense"].double() < level)
    print("sides equal everywhere:", sides_equal, " d0 =", c["d0"])
    if sides_equal:
        dv, df = marching_cubes(c["dense"], level)
        assert torch.equal(v, dv) and torch.equal(f, df)


def test_default_is_the_dense_path(tmp_path, monkeypatch):
    import svr_amd  # noqa: F401
    from svr_amd.model import ifnet, implicit_to_mesh
    from svr_amd.util import sparse_grid
    from svr_amd.util.visualize import marching_cubes
    c = _network_case()

    def boom(*a, **k):
        raise AssertionError("the dense default entered sparse_grid")

    monkeypatch.setattr(sparse_grid, "sparse_lattice_field", boom)
    monkeypatch.setattr(ifnet, "INFERENCE_BLOCK", 0)
    v, f = implicit_to_mesh(c["m"], c["x"], DIMS, c["level"], tmp_path / "dense.obj")
    wv, wf = marching_cubes(c["dense"], c["level"])                # dense = 1 - evaluate_network_on_grid_device(...): the parent's body
    assert torch.equal(v, wv) and torch.equal(f, wf) and f.shape[0] > 1000
    v0, f0 = implicit_to_mesh(c["m"], c["x"], DIMS, c["level"], tmp_path / "dense0.obj", block=0)
    assert torch.equal(v0, wv) and torch.equal(f0, wf)
    assert (tmp_path / "dense.obj").read_bytes() == (tmp_path / "dense0.obj").read_bytes()
    # the module attribute switches both trainers' call sites over
    monkeypatch.setattr(ifnet, "INFERENCE_BLOCK", 8)
    with pytest.raises(AssertionError, match="entered sparse_grid"):
        implicit_to_mesh(c["m"], c["x"], DIMS, c["level"], tmp_path / "x.obj")
