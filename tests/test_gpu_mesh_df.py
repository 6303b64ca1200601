"""GPU: the distance field of a mesh on a lattice (csrc/mesh_df.hip, data_processing/mesh_to_df.py) against the numpy
restatement of the rule (tests/df_oracle.py), bit for bit: float32 field and winning face, for both brick sizes, with and
without culling, across batch boundaries, truncated, on the reference sample's mesh at the real lattice, through the .df
writer, process_sample(scene_mesh=...) and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import df_oracle as O

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
LATTICES = [(19, 9, 12), (8, 8, 8), (1, 5, 17)]          # partial bricks on every axis; exactly one brick; an extent of 1


def _gold(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z["vertices"].astype(np.float64), z["faces"].astype(np.int32)


def _placed(name, dims, where):
    """The committed unit-size mesh scaled and shifted into grid units: inside the lattice's box, partly outside, or
    wholly outside (an extent of 1 counts as 3 for the scale, so the mesh keeps a volume)."""
    V, F = _gold(name)
    d = np.array(dims, dtype=np.float64)
    ext = np.abs(V).max(0)
    k = 0.9 * (np.maximum(d - 1, 2) / 2 / ext).min()
    c = (d - 1) / 2
    if where == "inside":
        return c + k * V, F
    if where == "partly":
        return c + 0.3 * d + 2 * k * V, F
    return c + d + 5 + k * V, F                            # wholly outside


def _small_meshes():
    tri = np.array([[1.25, 0.5, 0.75], [6.5, 1.0, 2.25], [2.0, 5.5, 7.125], [3.0, 3.0, -2.5], [7.0, 7.5, 3.0]])
    return {
        "one_triangle": (tri, np.array([[0, 1, 2]], np.int32)),
        # faces 0 / 2 and 1 / 3 coincide, vertex order included (another order rounds differently: no tie): the lower index wins
        "coincident": (tri, np.array([[0, 1, 2], [1, 3, 4], [0, 1, 2], [1, 3, 4]], np.int32)),
        # zero-area faces (a repeated vertex; three collinear points with exact coordinates) in front of and between real ones
        "zero_area_mixed": (np.concatenate([tri, [[0.0, 0, 0], [1, 1, 1], [2, 2, 2]]]),
                            np.array([[0, 0, 1], [5, 6, 7], [0, 1, 2], [3, 3, 3], [1, 3, 4]], np.int32)),
    }


CASES = [(L, "openbox", "inside") for L in LATTICES] + [(L, "torus", w) for L in LATTICES for w in ("inside", "partly", "outside")] \
    + [(L, m, None) for L in LATTICES for m in ("one_triangle", "coincident", "zero_area_mixed")]


def _case_mesh(dims, mesh, where):
    return _placed("mesh_" + mesh, dims, where) if where else _small_meshes()[mesh]


_oracle_cache = {}


def _oracle(dims, mesh, where, truncate=None):
    key = (dims, mesh, where, truncate)
    if key not in _oracle_cache:
        V, F = _case_mesh(dims, mesh, where)
        field, face = O.distance_field(V, F, dims, truncate)
        field.setflags(write=False)
        face.setflags(write=False)
        _oracle_cache[key] = (field, face)
    return _oracle_cache[key]


def _same_bits(got, want):
    return np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("dims,mesh,where", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_field_and_face_equal_the_oracle_bit_for_bit(dims, mesh, where):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    V, F = _case_mesh(dims, mesh, where)
    want, want_face = _oracle(dims, mesh, where)
    assert np.isfinite(want).all() and (want_face >= 0).all()
    if mesh == "coincident":
        assert set(np.unique(want_face)) <= {0, 1}
    if mesh == "zero_area_mixed":
        assert set(np.unique(want_face)) <= {2, 4}
    for brick in (4, 8):
        for cull in (True, False):
            field, face = mesh_distance_field((V, F), dims, return_face=True, brick=brick, cull=cull)
            assert field.is_cuda and field.dtype == torch.float32 and tuple(field.shape) == dims
            assert face.dtype == torch.int32 and tuple(face.shape) == dims
            got, got_face = field.cpu().numpy(), face.cpu().numpy()
            assert _same_bits(got, want), (brick, cull, np.abs(got - want).max())
            assert np.array_equal(got_face, want_face), (brick, cull)


def test_a_mesh_of_zero_area_faces_is_an_empty_mesh():
    import svr_amd
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    from svr_amd.data_processing.process_sample import EmptyMeshError
    V = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 0, 1]])
    for cull in (True, False):
        with pytest.raises(EmptyMeshError, match="has an area"):
            mesh_distance_field((V, np.array([[0, 1, 2], [3, 3, 0]], np.int32)), (8, 8, 8), cull=cull)
    with pytest.raises(EmptyMeshError):
        mesh_distance_field((V, np.zeros((0, 3), np.int32)), (8, 8, 8))
    # the C ABI itself: SVR_E_BADSHAPE for F == 0, before any pointer is looked at
    import ctypes
    n = ctypes.c_int64(7)
    assert svr_amd._lib.lib().svr_mesh_df_valid_faces(None, 0, None, ctypes.byref(n), None) == -2 and n.value == 0


def test_batches_do_not_change_a_bit():
    """Sphere of radius 8 centred in 24^3: the centre bricks keep every face.  A 4-byte budget makes every brick its own
    batch (each with a buffer of exactly its list), a budget of 2/5 of the total puts batch boundaries mid-lattice."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    V, F = _gold("mesh_sphere")
    c0 = 0.5 * (V.min(0) + V.max(0))
    dims = (24, 24, 24)
    V = 11.5 + (V - c0) * (8.0 / np.linalg.norm(V - c0, axis=1).max())
    want, want_face = O.distance_field(V, F, dims)
    for brick in (4, 8):
        st = {}
        ref, ref_face = mesh_distance_field((V, F), dims, return_face=True, brick=brick, stats=st)
        assert st["batches"] == 1 and st["bricks"] == (24 // brick) ** 3
        assert st["list_max"] == len(F) if brick == 8 else 0 < st["list_max"] <= len(F)
        assert _same_bits(ref.cpu().numpy(), want) and np.array_equal(ref_face.cpu().numpy(), want_face)
        for budget, check in ((4, lambda s: s["batches"] == s["bricks"]),
                              (st["list_bytes"] * 2 // 5, lambda s: 2 <= s["batches"] < s["bricks"])):
            s2 = {}
            got, got_face = mesh_distance_field((V, F), dims, return_face=True, brick=brick, list_budget_bytes=budget, stats=s2)
            assert check(s2), s2
            assert s2["list_entries"] == st["list_entries"]
            assert torch.equal(got, ref) and torch.equal(got_face, ref_face)


def test_truncate():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    dims, T = LATTICES[0], 2.5
    V, F = _case_mesh(dims, "torus", "inside")
    full, full_face = _oracle(dims, "torus", "inside")
    over = full > np.float32(T)
    assert over.any() and (~over).any()
    want = np.minimum(full, np.float32(T))
    for brick in (4, 8):
        for cull in (True, False):
            field, face = mesh_distance_field((V, F), dims, truncate=T, return_face=True, brick=brick, cull=cull)
            got, got_face = field.cpu().numpy(), face.cpu().numpy()
            assert _same_bits(got, want), (brick, cull)
            assert np.array_equal(got_face == -1, over) and np.array_equal(got_face[~over], full_face[~over]), (brick, cull)
            # truncate <= 0 is the untruncated field
            assert _same_bits(mesh_distance_field((V, F), dims, truncate=0.0, brick=brick, cull=cull).cpu().numpy(), full)
    # the mesh wholly outside and farther than T from every point: every candidate list is empty, every value is the cap
    Vo, Fo = _case_mesh(dims, "torus", "outside")
    assert _oracle(dims, "torus", "outside")[0].min() > T + 14
    for brick in (4, 8):
        st = {}
        field, face = mesh_distance_field((Vo, Fo), dims, truncate=T, return_face=True, brick=brick, stats=st)
        assert st["list_entries"] == 0
        assert bool((field == T).all()) and bool((face == -1).all())


def test_reference_scene_mesh_on_the_real_lattice():
    """The reference sample's mesh.obj (45 172 faces) on 139 x 104 x 112, default settings: 200 seeded lattice points and
    the 8 corners bit for bit against the oracle; globally finite, below the nearest-vertex distance at those points, and
    1-Lipschitz between axis neighbours up to the float32 rounding of two outputs."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    z = np.load(os.path.join(GOLD, "scene_mesh_00000.npz"))
    V, F = z["vertices"], z["faces"]
    assert V.dtype == np.float32 and F.dtype == np.int32 and V.shape == (22588, 3) and F.shape == (45172, 3)
    dims = (139, 104, 112)
    st = {}
    field, face = mesh_distance_field((V, F), dims, return_face=True, stats=st)
    print("candidate lists:", st)
    rng = np.random.default_rng(2024)
    pts = np.stack([rng.integers(0, d, size=200) for d in dims], axis=1)
    pts = np.concatenate([pts, [[i, j, k] for i in (0, dims[0] - 1) for j in (0, dims[1] - 1) for k in (0, dims[2] - 1)]])
    want, want_face = O.distance_at(pts.astype(np.float64), O.triangle_table(V, F), chunk=16)
    got = field[pts[:, 0], pts[:, 1], pts[:, 2]].cpu().numpy()
    got_face = face[pts[:, 0], pts[:, 1], pts[:, 2]].cpu().numpy()
    assert _same_bits(got, want), np.abs(got - want).max()
    assert np.array_equal(got_face, want_face)
    assert bool(torch.isfinite(field).all()) and float(field.min()) >= 0.0
    nearest_vertex = np.sqrt(((pts[:, None, :].astype(np.float64) - V[None].astype(np.float64)) ** 2).sum(-1).min(1))
    assert (got.astype(np.float64) <= nearest_vertex * (1 + 2.0 ** -23)).all()
    bound = 1.0 + 2.0 * 2.0 ** -24 * float(field.max())
    for axis in range(3):
        step = (field.narrow(axis, 1, dims[axis] - 1) - field.narrow(axis, 0, dims[axis] - 1)).abs().max().item()
        assert step <= bound, (axis, step, bound)


def test_files_pipeline_and_command_line(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field, mesh_to_df
    from svr_amd.data_processing.process_sample import process_sample
    from svr_amd.data_processing.volume_reader import read_df
    from svr_amd.util.visualize import export_obj
    from tests._scene_tree import build_tree
    # 1. mesh_to_df -> read_df round trip
    dims = (19, 9, 12)
    V, F = _case_mesh(dims, "torus", "inside")
    want, _ = _oracle(dims, "torus", "inside")
    field = mesh_to_df((V, F), tmp_path / "torus.df", dims=dims)
    back = read_df(str(tmp_path / "torus.df"))
    assert back.shape == dims and _same_bits(back, field.cpu().numpy()) and _same_bits(back, want)
    # 2. process_sample from a scene mesh: a torus of tube radius ~6.6 voxels around the lattice centre
    full = (139, 104, 112)
    root = build_tree(tmp_path / "tree", {"train": ["v0"]})
    raw, out = root / "data" / "raw" / "tiny" / "v0", root / "data" / "processed" / "tiny" / "v0"
    gold = np.load(os.path.join(GOLD, "raw_sample.npz"))
    (raw / "intrinsic.txt").write_text(str(gold["intrinsic_txt"]))
    Vt, Ft = _gold("mesh_torus")
    Vs = (np.array(full) - 1) / 2 + 60.0 * Vt
    export_obj(Vs.astype(np.float32), Ft, raw / "scene.obj")
    assert not (raw / "distance_field.df").exists()
    g = torch.Generator(device="cuda").manual_seed(3)
    process_sample(root / "data", "tiny", "v0", sample_num=2048, generator=g, scene_mesh="scene.obj")
    df_bytes = (raw / "distance_field.df").read_bytes()
    scene = load_obj(str(raw / "scene.obj"))
    direct = mesh_distance_field(scene, full).cpu().numpy()
    assert _same_bits(read_df(str(raw / "distance_field.df")), direct)
    assert (out / "target.df").read_bytes() == df_bytes
    z = np.load(out / "depth_grid.npz")
    assert z.files == ["grid"] and z["grid"].dtype == np.float64 and z["grid"].shape == full
    mesh = load_obj(str(raw / "mesh.obj"))
    assert len(mesh.faces) > 1000 and len(mesh.faces) != len(scene.faces)        # the level-1.0 surface, not the input mesh
    M = 2048 + int(0.1 * 2048)
    for sigma in ("0.01", "0.10"):
        o = np.load(out / f"occupancy_{sigma}.npz")
        assert sorted(o.files) == ["grid_coords", "occupancies", "points"]
        assert o["points"].shape == (M, 3) and o["occupancies"].shape == (M,) and o["grid_coords"].shape == (M, 3)
        assert o["points"].dtype == np.float64 and o["occupancies"].dtype == np.bool_ and o["grid_coords"].dtype == np.float64
        assert o["occupancies"].any() and not o["occupancies"].all()
    # a second call leaves the existing field alone (even with another mesh under that name)
    export_obj((Vs + 3.0).astype(np.float32), Ft, raw / "scene.obj")
    before = os.stat(raw / "distance_field.df").st_mtime_ns
    process_sample(root / "data", "tiny", "v0", sample_num=256, generator=g, scene_mesh="scene.obj")
    assert (raw / "distance_field.df").read_bytes() == df_bytes and os.stat(raw / "distance_field.df").st_mtime_ns == before
    # 3. the command line, in a fresh child process
    small = tmp_path / "small.obj"
    export_obj(V.astype(np.float32), F, small)
    r = subprocess.run([sys.executable, "-m", "svr_amd.data_processing.mesh_to_df", str(small), str(tmp_path / "cli.df"),
                        "--dims", "19", "9", "12", "--truncate", "2.5"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert "19 x 9 x 12" in line and f"{len(F)} faces" in line and "max 2.5" in line, line
    cli = read_df(str(tmp_path / "cli.df"))
    assert cli.shape == dims and cli.max() == np.float32(2.5)


def test_pipeline_quarantines_a_view_whose_scene_mesh_is_empty(tmp_path):
    """The field comes first, so the view is moved before anything else of it is read or written."""
    import shutil

    import svr_amd  # noqa: F401
    from svr_amd.data_processing.process_sample import process_sample_pipeline
    view = tmp_path / "train" / "scene0" / "0"
    view.mkdir(parents=True)
    shutil.copyfile(os.path.join(GOLD, "raw_distance.exr"), view / "distance.exr")
    (view / "scene.obj").write_text("v 0 0 0\nv 1 1 1\nv 2 2 2\nf 1 2 3\n")          # three collinear points: no area
    (tmp_path / "intrinsics.txt").write_text(str(np.load(os.path.join(GOLD, "raw_sample.npz"))["intrinsic_txt"]))
    moved = process_sample_pipeline(tmp_path, "train", sample_num=64, scene_mesh="scene.obj")
    assert moved == [tmp_path / "quarantine" / "train" / "scene0" / "0"] and not view.exists()
    assert sorted(p.name for p in moved[0].iterdir()) == ["distance.exr", "scene.obj"]


def test_bad_input_raises_before_any_launch():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.mesh_to_df import mesh_distance_field
    V = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0]])
    F = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError, match="indexes outside the 3 vertices"):
        mesh_distance_field((V, np.array([[0, 1, 3]], np.int32)), (8, 8, 8))
    bad = V.copy()
    bad[2, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        mesh_distance_field((bad, F), (8, 8, 8))
    with pytest.raises(ValueError, match="brick=5"):
        mesh_distance_field((V, F), (8, 8, 8), brick=5)
    with pytest.raises(ValueError, match="lattice"):
        mesh_distance_field((V, F), (8, 0, 8))
