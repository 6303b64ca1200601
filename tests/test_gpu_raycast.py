"""GPU: the ray caster (csrc/raycast.hip, data_processing/render_view.py) against the numpy restatement of the rule
(tests/raycast_oracle.py), bit for bit: depth, face, distance, normal and shade, for both tile sizes, with and without
culling, across batch boundaries, on the reference sample's mesh at the real image size, through the files,
process_sample(render_missing=True), the command line and Reconstruction.render_depth."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import raycast_oracle as O

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def _tile():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.render_view import DEFAULT_TILE
    return DEFAULT_TILE


T = 8                                     # render_view.DEFAULT_TILE (test_sizes_follow_the_default_tile pins the two together)
SIZES = list(dict.fromkeys([(8, 8), (13, 21), (1, 17), (19, 37), (T, T), (T + 1, 2 * T + 1)]))
MESHES = ("sphere", "torus", "openbox")
PLACES = ("in_view", "partly", "behind", "straddling")
SMALL = ("one_triangle", "coincident", "zero_area_mixed", "edge_on")


def _gold(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z["vertices"].astype(np.float64), z["faces"].astype(np.int32)


def _placed(name, where, size, consts):
    """The committed mesh scaled to a largest |coordinate| of 0.6 m, in grid units: at camera-space (0, 0, 2); shifted so
    that its centre lies on the image's right border; behind the camera; across the camera plane."""
    V, F = _gold("mesh_" + name)
    V = V * (0.6 / np.abs(V).max())
    H, W = size
    f, cx = float(consts[0]), float(consts[1])
    at = {"in_view": (0.0, 0.0, 2.0), "partly": (2.0 * (W - 1 - cx) / f, 0.0, 2.0), "behind": (0.0, 0.0, -2.0),
          "straddling": (0.0, 0.0, 0.3)}[where]
    return O.camera_to_grid(V + np.array(at), consts), F


def _small(name, consts):
    cam = np.array([[-0.55, -0.5, 1.75], [0.6, -0.35, 2.25], [-0.1, 0.55, 2.125], [0.3, 0.3, 1.5], [0.7, 0.75, 3.0],
                    [0.0, 0.0, 1.0], [0.1, 0.1, 1.1], [0.2, 0.2, 1.2]])
    g = O.camera_to_grid(cam, consts)
    if name == "one_triangle":
        return g, np.array([[0, 1, 2]], np.int32)
    if name == "coincident":          # faces 0 / 2 and 1 / 3 coincide, vertex order included: the lower index wins
        return g, np.array([[0, 1, 2], [1, 3, 4], [0, 1, 2], [1, 3, 4]], np.int32)
    if name == "zero_area_mixed":     # repeated vertices and three collinear points, in front of and between real faces
        return g, np.array([[5, 5, 6], [5, 6, 7], [0, 1, 2], [3, 3, 3], [1, 3, 4], [6, 7, 7]], np.int32)
    # edge_on: a face that contains the camera centre (vertex a), so every ray's det is 0 up to rounding and exactly 0 on
    # the image row in its plane; a real face behind it
    k = np.asarray(consts, dtype=np.float64)
    e = np.array([[k[4], k[6], k[8]], [k[4], k[6], k[8] + 64.0], [k[4] + 32.0, k[6], k[8] + 64.0]])
    return np.concatenate([e, g[:3]]), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


CASES = [(s, m, w) for s in SIZES for m in MESHES for w in PLACES] + [(s, m, None) for s in SIZES for m in SMALL]
_cache = {}


def _case(size, mesh, where):
    """(V, F, consts, the oracle's maps), computed once per case and left unchanged."""
    key = (size, mesh, where)
    if key not in _cache:
        consts = O.make_consts(*size)
        V, F = _placed(mesh, where, size, consts) if where else _small(mesh, consts)
        want = O.render(V, F, consts, size)
        for a in want.values():
            a.setflags(write=False)
        _cache[key] = (V, F, consts, want)
    return _cache[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _assert_equal(got, want, what):
    names = ("depth", "face", "distance", "normal", "shade")
    assert len(got) == len(names)
    for name, g in zip(names, got):
        g = g.cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(_bits(g), _bits(want[name])), (what, name, int((_bits(g) != _bits(want[name])).sum()))


def test_sizes_follow_the_default_tile():
    assert T == _tile() and (T, T) in SIZES and (T + 1, 2 * T + 1) in SIZES


@pytest.mark.parametrize("size,mesh,where", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_maps_equal_the_oracle_bit_for_bit(size, mesh, where):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.render_view import render_depth
    V, F, consts, want = _case(size, mesh, where)
    hit = want["face"] >= 0
    assert not np.isnan(want["normal"]).any()
    if where == "in_view":
        assert 0.10 <= hit.mean() <= 0.90, hit.mean()               # no case passes by being all miss
    if where == "behind":
        assert not hit.any()
    if mesh == "coincident":
        assert hit.any() and set(np.unique(want["face"])) <= {-1, 0, 1}
    if mesh == "zero_area_mixed":
        assert hit.any() and set(np.unique(want["face"])) <= {-1, 2, 4}
    if mesh == "edge_on":
        assert set(np.unique(want["face"])) <= {-1, 1}
    kw = dict(consts=consts, size=size, return_face=True, return_distance=True, return_normal=True, return_shade=True)
    st = {}
    ref = render_depth((V, F), stats=st, **kw)
    assert ref[0].is_cuda and ref[0].dtype == torch.float32 and tuple(ref[0].shape) == size
    _assert_equal(ref, want, "culled")
    for tile in (8, 16):
        _assert_equal(render_depth((V, F), tile=tile, **kw), want, f"tile {tile}")
    _assert_equal(render_depth((V, F), cull=False, **kw), want, "brute force")
    # a budget of a third of the lists (at least one entry): several batches wherever there are several non-empty tiles
    s2 = {}
    _assert_equal(render_depth((V, F), list_budget_bytes=max(4, st["list_bytes"] // 3), stats=s2, **kw), want, "batched")
    assert s2["list_entries"] == st["list_entries"]
    if st["tiles"] > 2 and st["list_entries"] > st["list_max"] * 2:
        assert s2["batches"] >= 2, (st, s2)
    _assert_equal(render_depth((V, F), list_budget_bytes=4, **kw), want, "one tile per batch")
    # depth alone, and near / far / miss against the oracle on the same case
    assert np.array_equal(_bits(render_depth((V, F), consts=consts, size=size).cpu().numpy()), _bits(want["depth"]))
    if where == "in_view":
        cut = O.render(V, F, consts, size, near=1.9, far=2.3, miss=-1.0)
        got = render_depth((V, F), near=1.9, far=2.3, miss=-1.0, **kw)
        _assert_equal(got, cut, "near / far / miss")
        assert (cut["face"] != want["face"]).any()


def test_culling_culls_and_wrapping_meshes_are_batched():
    """The lists are lists: a mesh in view gives far fewer candidates than tiles x faces, a mesh behind the camera (every
    vertex's depth negative) gives every face to every tile -- and a small budget still bounds the buffer."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.render_view import render_depth
    size = (19, 37)
    V, F, consts, want = _case(size, "torus", "in_view")
    st = {}
    render_depth((V, F), consts=consts, size=size, stats=st)
    assert 0 < st["list_entries"] < st["tiles"] * len(F) // 2 and st["every_tile_faces"] == 0
    Vb, Fb, _, _ = _case(size, "torus", "behind")
    sb = {}
    depth = render_depth((Vb, Fb), consts=consts, size=size, stats=sb, list_budget_bytes=4 * len(Fb))
    assert sb["every_tile_faces"] == len(Fb) and sb["list_entries"] == sb["tiles"] * len(Fb) and sb["batches"] == sb["tiles"]
    assert sb["largest_batch_bytes"] == 4 * len(Fb) and bool((depth == 0).all())


def test_transform_and_bad_input():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.process_sample import EmptyMeshError
    from svr_amd.data_processing.render_view import render_depth
    size = (13, 21)
    V, F, consts, want = _case(size, "sphere", "in_view")
    M = np.array([[0.0, -1.0, 0.0, 3.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
    moved = O.render(O.transform_vertices(V, M), F, consts, size)
    got = render_depth((V, F), consts=consts, size=size, transform=M, return_face=True)
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(moved["depth"])) and np.array_equal(got[1].cpu().numpy(), moved["face"])
    assert (moved["face"] != want["face"]).any()
    with pytest.raises(EmptyMeshError):
        render_depth((V, np.zeros((0, 3), np.int32)), consts=consts, size=size)
    with pytest.raises(ValueError, match="indexes outside"):
        render_depth((V, np.array([[0, 1, len(V)]], np.int32)), consts=consts, size=size)
    bad = V.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        render_depth((bad, F), consts=consts, size=size)
    with pytest.raises(ValueError, match="tile=12"):
        render_depth((V, F), consts=consts, size=size, tile=12)
    with pytest.raises(ValueError, match="size"):
        render_depth((V, F), consts=consts, size=(0, 4))
    # the C ABI itself: a list entry outside [0, F) is never turned into an address
    from svr_amd import _lib
    import ctypes as C
    l = _lib.lib()
    tri = torch.from_numpy(O.triangle_table(V, F)).cuda()
    nt = int(l.svr_raycast_tiles(*size, 8))
    offsets = torch.arange(0, 3 * (nt + 1), 3, device="cuda", dtype=torch.int64)
    lst = torch.tensor([-5, len(F), 2 ** 31 - 1] * nt, device="cuda", dtype=torch.int32)
    depth = torch.full(size, 7.0, device="cuda")
    kc = (C.c_float * 12)(*[float(v) for v in consts])
    rc = l.svr_raycast_eval(_lib.ptr(tri), len(F), kc, size[0], size[1], 8, 0.0, float("inf"), 0.0, _lib.ptr(offsets), _lib.ptr(lst), 0, nt,
                            _lib.ptr(depth), None, None, None, None, _lib.stream())
    assert rc == 0 and bool((depth == 0).all())
    assert l.svr_raycast_tiles(4, 4, 12) == -2 and l.svr_raycast_tiles(0, 4, 8) == -2


@pytest.fixture(scope="module")
def scene():
    z = np.load(os.path.join(GOLD, "scene_mesh_00000.npz"))
    V, F = z["vertices"], z["faces"]
    assert V.dtype == np.float32 and F.shape == (45172, 3)
    return V, F


def test_reference_scene_mesh_at_the_real_size(scene):
    """The reference sample's mesh (45 172 faces) at 240 x 320 on the default intrinsic: culled equals brute force on all
    76 800 pixels, 300 seeded pixels equal the oracle bit for bit, and at least 95 % of them hit."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.render_view import render_depth, view_consts
    V, F = scene
    size = (240, 320)
    kw = dict(size=size, return_face=True, return_distance=True, return_normal=True, return_shade=True)
    st = {}
    culled = render_depth((V, F), stats=st, **kw)
    print("candidate lists:", st)
    brute = render_depth((V, F), cull=False, **kw)
    for a, b in zip(culled, brute):
        assert torch.equal(a, b)
    for tile in (8, 16):
        for a, b in zip(render_depth((V, F), tile=tile, **kw), culled):
            assert torch.equal(a, b)
    assert st["list_mean"] < 0.02 * len(F)
    rng = np.random.default_rng(2025)
    rows, cols = rng.integers(0, size[0], 300), rng.integers(0, size[1], 300)
    want = O.maps_at(O.triangle_table(V, F), view_consts(), size[0], size[1], rows, cols)
    hit = want["face"] >= 0
    print(f"oracle subset: hit share {hit.mean():.3f}, depth {want['depth'][hit].min():.3f} .. {want['depth'][hit].max():.3f}")
    assert hit.mean() >= 0.95
    for name, g in zip(("depth", "face", "distance", "normal", "shade"), culled):
        g = g[rows, cols].cpu().numpy()
        assert np.array_equal(_bits(g), _bits(want[name])), name


def test_through_the_pipeline(scene, tmp_path):
    """A view that holds only scene.obj and intrinsic.txt becomes a sample the loader reads."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    from svr_amd.data_processing.process_sample import process_sample
    from svr_amd.data_processing.render_view import render_depth
    from svr_amd.dataset import scene_net_data
    from svr_amd.util.visualize import export_obj
    from PIL import Image
    V, F = scene
    raw = tmp_path / "data" / "raw" / "tiny" / "v0"
    out = tmp_path / "data" / "processed" / "tiny" / "v0"
    raw.mkdir(parents=True)
    (tmp_path / "splits" / "tiny").mkdir(parents=True)
    (tmp_path / "splits" / "tiny" / "train.txt").write_text("v0\n")
    (raw / "intrinsic.txt").write_text(str(np.load(os.path.join(GOLD, "raw_sample.npz"))["intrinsic_txt"]))
    export_obj(V, F, raw / "scene.obj")
    assert sorted(p.name for p in raw.iterdir()) == ["intrinsic.txt", "scene.obj"]
    g = torch.Generator(device="cuda").manual_seed(3)
    process_sample(tmp_path / "data", "tiny", "v0", sample_num=2048, generator=g, scene_mesh="scene.obj", render_missing=True)
    mesh = load_obj(str(raw / "scene.obj"))
    depth, distance = render_depth(mesh, intrinsic=str(raw / "intrinsic.txt"), return_distance=True)
    back = sample_io.exr_read(raw / "distance.exr", "R")
    assert np.array_equal(_bits(back), _bits(distance.cpu().numpy()))
    assert [c for c, _ in sample_io.exr_info(raw / "distance.exr")["channels"]] == ["B", "G", "R"]
    with Image.open(raw / "rgb.png") as im:
        assert im.mode == "RGB" and im.size == (320, 240)
    grid = np.load(out / "depth_grid.npz")["grid"]
    field = mesh_distance_field(mesh, grid.shape).cpu().numpy()
    marked = grid != 0
    print(f"depth grid: {marked.sum()} voxels set, largest distance to the mesh {field[marked].max():.4f} voxels")
    assert marked.sum() > 0
    assert field[marked].max() <= np.sqrt(3.0) / 2 + 1e-3
    ds = scene_net_data("train", tmp_path / "data", 256, "tiny", SimpleNamespace(W=256, resize_input=True, precision=32),
                        splits_root=tmp_path / "splits")
    item = ds[0]
    assert item["name"] == "v0" and tuple(item["rgb"].shape) == (3, 256, 256) and tuple(item["depthmap_target"].shape) == (240, 320)
    # the loader's depth is the ray caster's up to the round trip of the distance map (tests/test_raycast_cpu.py: 4 * 2^-24)
    rel = ((item["depthmap_target"] - depth).abs() / depth).max().item()
    assert rel <= 4 * 2.0 ** -24, rel
    # a second call touches neither file
    before = [os.stat(raw / n).st_mtime_ns for n in ("distance.exr", "rgb.png")]
    process_sample(tmp_path / "data", "tiny", "v0", sample_num=64, generator=g, scene_mesh="scene.obj", render_missing=True)
    assert before == [os.stat(raw / n).st_mtime_ns for n in ("distance.exr", "rgb.png")]


def test_command_line_and_reconstruction(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    from svr_amd.data_processing.render_view import render_depth, view_consts
    from svr_amd.reconstruct import Reconstruction
    from svr_amd.util.visualize import export_obj
    # 1. the command line, in a fresh child process: a sphere of 0.2 m, 2 m away on the ray of pixel (row 30, column 40) of
    # the default intrinsic -- the middle of the 60 x 80 window, which is the top left corner of the camera's image
    k = view_consts()
    V, F = _gold("mesh_sphere")
    at = np.array([2.0 * (40 - float(k[1])) / float(k[0]), -2.0 * (30 - float(k[2])) / float(k[0]), 2.0])
    Vg = O.camera_to_grid(V * (0.2 / np.abs(V).max()) + at, k).astype(np.float32)
    export_obj(Vg, F, tmp_path / "sphere.obj")
    r = subprocess.run([sys.executable, "-m", "svr_amd.data_processing.render_view", str(tmp_path / "sphere.obj"), str(tmp_path / "view"),
                        "--size", "60", "80"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert "60 x 80" in line and f"{len(F)} faces" in line and "hit" in line and "depth min 1." in line, line
    d = sample_io.exr_read(tmp_path / "view" / "distance.exr", "R")
    assert d.shape == (60, 80) and (d > 0).any() and (d == 0).any() and (tmp_path / "view" / "rgb.png").exists()
    # 2. Reconstruction.render_depth: the lattice vertices / inf_res through the camera the view came from
    inf_res = 2
    verts = torch.from_numpy(Vg * inf_res).cuda()
    faces = torch.from_numpy(F).cuda()
    rec = Reconstruction(torch.zeros(48, 64, device="cuda"), None, None, verts, faces, 1, inf_res, [float(v) for v in k[3:9]])
    got = rec.render_depth()
    want = render_depth(((verts / float(inf_res)).cpu().numpy(), F), size=(48, 64))
    assert tuple(got.shape) == (48, 64) and torch.equal(got, want) and bool((got > 0).any())
    assert torch.equal(rec.render_depth(size=(30, 40)), render_depth(((verts / float(inf_res)).cpu().numpy(), F), size=(30, 40)))
    empty = Reconstruction(None, None, None, verts, faces[:0], 1, inf_res, [float(v) for v in k[3:9]])
    assert empty.render_depth() is None
