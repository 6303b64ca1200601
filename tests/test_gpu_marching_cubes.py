"""GPU: the marching-cubes kernels (csrc/marching_cubes.hip) against the numpy oracle of tests/mc_oracle.py -- vertices bit
for bit, faces element for element -- plus mesh topology at the inference lattice sizes, geometry against the independent
check_mesh_contains path, and the public entry points (util.visualize, model.implicit_to_mesh, the trainer's
validation_step)."""
import numpy as np
import pytest
import torch

from oracle import ifnet_oracle as O
from tests import mc_oracle as M

pytestmark = pytest.mark.gpu

DIMS = (139, 104, 112)


def _mc():
    import svr_amd  # noqa: F401
    from svr_amd.util.visualize import marching_cubes
    return marching_cubes


def _same(got, want):
    gv, gf = (t.cpu().numpy() if torch.is_tensor(t) else t for t in got)
    wv, wf = want
    assert gv.dtype == np.float32 and gf.dtype == np.int32
    assert gv.shape == wv.shape and gf.shape == wf.shape, (gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32))
    assert np.array_equal(gf, wf)


def _noise(shape, seed, nan=False):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape).astype(np.float32)
    if nan:
        f[rng.random(shape) < 0.05] = np.nan
    return f


def _border_inside(shape):
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    return (np.sqrt(((g - np.array(shape) * 0.2) ** 2).sum(-1)) - min(shape) * 0.45).astype(np.float32)


FIELDS = {
    "sphere": lambda: (M.sphere(24, 8.0), 0.0),
    "torus": lambda: (M.torus(), 0.0),
    "noise": lambda: (_noise((33, 20, 27), 0), 0.0),
    "noise_nan": lambda: (_noise((17, 19, 23), 1, nan=True), 0.25),
    "integers": lambda: (np.random.default_rng(2).integers(-2, 3, (21, 18, 15)).astype(np.float32), 0.0),
    "integers_level1": lambda: (np.random.default_rng(3).integers(0, 3, (12, 13, 14)).astype(np.float32), 1.0),
    "border_inside": lambda: (_border_inside((30, 26, 22)), 0.0),
    "2x2x2": lambda: (np.array([-1, 1, 1, 1, 1, 1, 1, -1], np.float32).reshape(2, 2, 2), 0.0),
    "1xNxM": lambda: (_noise((1, 9, 11), 4), 0.0),
    "Nx1xM": lambda: (_noise((9, 1, 11), 5), 0.0),
    "3x5x7": lambda: (_noise((3, 5, 7), 6), 0.1),
    "139x104x112": lambda: (_noise(DIMS, 7), 0.3),
    "all_inside": lambda: (np.full((5, 6, 7), -1.0, np.float32), 0.0),
    "all_outside": lambda: (np.full((5, 6, 7), 1.0, np.float32), 0.0),
}


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_cubes_equals_oracle(name):
    mc = _mc()
    field, level = FIELDS[name]()
    want = M.marching_cubes(field, level)
    if name in ("1xNxM", "Nx1xM", "all_inside", "all_outside"):
        assert len(want[0]) == 0 and len(want[1]) == 0
    elif name not in ("2x2x2", "3x5x7"):
        assert len(want[1]) > 50
    got = mc(field, level)                                        # numpy in -> numpy out
    assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
    _same(got, want)
    dev = mc(torch.from_numpy(field).cuda(), level)               # device in -> device out
    assert dev[0].is_cuda and dev[1].is_cuda
    _same(dev, want)
    if name == "139x104x112":                                     # other dtypes are cast to float32 first
        _same(mc(field.astype(np.float64), level), want)


def _model():
    import svr_amd  # noqa: F401
    from svr_amd.model import IFNet
    m = IFNet(net_res=128)
    m.load_state_dict(O.name_seeded_state(128), strict=False)
    return m.cuda().eval()


def _input(dims, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, 1, *dims, generator=g) < 0.03).float().cuda()


def _check_topology(verts, faces, shape):
    """On the device: every directed edge occurs once; it has its reverse, unless both ends lie in one border plane."""
    V = verts.shape[0]
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fw = e[:, 0] * V + e[:, 1]
    bw = e[:, 1] * V + e[:, 0]
    srt, _ = torch.sort(fw)
    assert bool((srt[1:] != srt[:-1]).all()), "a directed edge is used twice"
    pos = torch.searchsorted(srt, bw).clamp(max=len(srt) - 1)
    matched = srt[pos] == bw
    a, b = verts[e[~matched, 0]], verts[e[~matched, 1]]
    hi = torch.tensor([s - 1 for s in shape], device=verts.device, dtype=torch.float32)
    same_plane = ((a == 0) & (b == 0)) | ((a == hi) & (b == hi))
    assert bool(same_plane.any(dim=1).all()), "an open edge off the lattice border"
    return int((~matched).sum())


@pytest.mark.parametrize("res_increase", [1, 2])
def test_topology_of_the_network_lattice(res_increase):
    mc = _mc()
    from svr_amd.model import evaluate_network_on_grid_device
    grid = evaluate_network_on_grid_device(_model(), _input(DIMS, 41), DIMS, res_increase)
    shape = tuple(s * res_increase for s in DIMS)
    assert tuple(grid.shape) == shape
    field = 1 - grid
    level = float(field.view(-1)[::97].median())                  # a level with a large surface
    v, f = mc(field, level)
    assert f.shape[0] > 10000
    _check_topology(v, f, shape)
    assert int(f.min()) >= 0 and int(f.max()) == v.shape[0] - 1 and len(torch.unique(f)) == v.shape[0]


def test_geometry_against_check_mesh_contains():
    from types import SimpleNamespace
    mc = _mc()
    from svr_amd.data_processing.libmesh.inside_mesh import check_mesh_contains
    shape = (40, 36, 30)
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    c = np.array([19.3, 17.6, 14.2])
    d = np.sqrt((((g - c) / np.array([14.0, 11.0, 9.0])) ** 2).sum(-1)) * 9.0 + 0.8 * np.sin(g[..., 0] / 3.0) - 8.0
    d = np.where(np.abs(d) < 0.2, np.where(d < 0, -0.2, 0.2), d).astype(np.float32)   # >= 0.2 from the level
    v, f = mc(torch.from_numpy(d).cuda(), 0.0)
    assert f.shape[0] > 1000
    assert _check_topology(v, f, shape) == 0                       # closed: it does not reach the border
    rng = np.random.default_rng(9)
    pts = g.reshape(-1, 3) + rng.uniform(-0.02, 0.02, (g.size // 3, 3))
    mesh = SimpleNamespace(vertices=v.cpu().numpy().astype(np.float64), faces=f.cpu().numpy())
    contains, holes = check_mesh_contains(mesh, torch.from_numpy(pts).cuda(), 512)
    assert not bool(holes.any())
    assert np.array_equal(contains.cpu().numpy(), (d < 0).reshape(-1))


@pytest.mark.parametrize("res_increase", [1, 2])
def test_implicit_to_mesh_equals_oracle_of_the_host_grid(tmp_path, res_increase):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.model import evaluate_network_on_grid, implicit_to_mesh
    m, x = _model(), _input(DIMS, 43)
    host = evaluate_network_on_grid(m, x, DIMS, res_increase)
    sdf = 1 - host                                                # float32, as the reference's numpy computes it
    q = float(np.median(sdf[::3, ::3, ::3]))
    for threshold in (0.5, q):
        path = tmp_path / f"mesh_{threshold}.obj"
        v, f = implicit_to_mesh(m, x, DIMS, threshold, path, res_increase)
        assert v.is_cuda and f.is_cuda
        want = M.marching_cubes(sdf, threshold)
        _same((v, f), want)
        back = load_obj(str(path))
        _same((back.vertices.astype(np.float32), back.faces), want)
    assert len(want[1]) > 1000


def test_visualize_sdf_numpy_and_device_give_the_same_file(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.util.visualize import visualize_sdf
    sdf = np.abs(M.torus((30, 30, 20), 8.0, 3.0)) + 0.25          # the distance-field shape of a target: level 0.75
    visualize_sdf(sdf, tmp_path / "a.obj")
    visualize_sdf(torch.from_numpy(sdf).cuda(), tmp_path / "b.obj")
    a, b = (tmp_path / "a.obj").read_bytes(), (tmp_path / "b.obj").read_bytes()
    assert len(a) > 1000 and a == b


def test_validation_step_writes_four_files(tmp_path):
    from types import SimpleNamespace
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.trainer import ImplicitRefinementTrainer
    t = ImplicitRefinementTrainer(SimpleNamespace(lr=1e-4, net_res=128, scale_factor=2))
    t.ifnet.load_state_dict(O.name_seeded_state(128), strict=False)
    t = t.cuda().eval()
    dims = (70, 52, 56)                                           # round((139, 104, 112) / 2)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 1, *dims, generator=g) < 0.03).float().cuda()
    target = torch.from_numpy(np.stack([np.abs(M.sphere(70, r)[:, :52, :56]) for r in (12.0, 18.0)])).unsqueeze(1)
    out = t.validation_step({"name": ["s0", "s1"], "input": x, "target": target}, 0, tmp_path / "vis")
    assert out == {"loss": 0}
    files = sorted(p.name for p in (tmp_path / "vis").iterdir())
    assert files == ["s0_gt.obj", "s0_predicted.obj", "s1_gt.obj", "s1_predicted.obj"]
    g0, g1 = load_obj(str(tmp_path / "vis" / "s0_gt.obj")), load_obj(str(tmp_path / "vis" / "s1_gt.obj"))
    assert len(g0.faces) > 100 and len(g1.faces) > len(g0.faces)  # each item meshed from its own target


def test_result_is_the_same_on_a_side_stream():
    mc = _mc()
    field = torch.from_numpy(_noise((60, 50, 40), 11)).cuda()
    want = mc(field, 0.1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = mc(field, 0.1)
    torch.cuda.current_stream().wait_stream(s)
    _same(got, tuple(t.cpu().numpy() for t in want))
