"""CPU: the numpy oracle of the smoothing rule (tests/mesh_smooth_oracle.py) against what the rule promises, on every shared
case in both boundary modes, against results worked out by hand, and against the quality figures of DESIGN.md section 24; the
workspace size function, the wrapper's argument checks, the command line's flags and the method, which need no GPU."""
import numpy as np
import pytest

from tests import mesh_smooth_oracle as O
from tests._mesh_smooth_cases import CASES, CLAMP_HI, CLAMP_LO, HUB_RIM, MODES, OPEN_N, binary_sphere, case, oracle


@pytest.mark.parametrize("fix_boundary", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_keeps_the_rules_promises(name, fix_boundary):
    v, f, kw = case(name)
    got = oracle(name, fix_boundary)
    assert got.vertices.dtype == np.float32 and got.vertices.shape == v.shape
    assert got.state.dtype == np.uint8 and got.state.shape == (len(v),) and got.counts.dtype == np.int64
    assert np.array_equal(got.counts, np.bincount(got.state, minlength=4)) and got.counts.sum() == len(v)
    ok = O.usable(v)
    assert np.array_equal(got.state == O.BAD, ~ok)
    if not fix_boundary:
        assert got.counts[O.FIXED] == 0
    if len(f) == 0:
        assert np.isin(got.state, (O.ISOLATED, O.BAD)).all()
    moved = (got.state == O.MOVABLE) & (kw["iterations"] > 0)
    words, want = got.vertices.view(np.uint32), v.view(np.uint32)
    assert np.array_equal(words[~moved], want[~moved])                              # NaN payloads included
    out = got.vertices[moved].astype(np.float64)
    assert (np.abs(out) <= 131072.0).all() and np.array_equal(out * 65536.0, np.rint(out * 65536.0))
    # a movable vertex is named by a valid face, whose corners are usable
    owner, nxt, prv, m = O.entries(v, f)
    assert ((got.state == O.MOVABLE) <= (m > 0)).all() and ok[nxt].all() and ok[prv].all() and m.sum() == len(owner)


def test_zero_iterations_is_the_identity_on_the_words():
    for fix_boundary in MODES:
        v, f, kw = case("torus_n0")
        got = oracle("torus_n0", fix_boundary)
        assert kw["iterations"] == 0 and np.array_equal(got.vertices.view(np.uint32), v.view(np.uint32))
        assert got.counts.tolist() == [len(v), 0, 0, 0]                              # the states are still computed
    v, f, _ = case("unclusterable")
    got = O.smooth(v, f, iterations=0)
    assert np.array_equal(got.vertices.view(np.uint32), v.view(np.uint32)) and got.counts[O.BAD] == 19


def test_one_tetrahedron_pass_by_hand():
    got = oracle("tetrahedron", True)
    assert got.counts.tolist() == [4, 0, 0, 0]
    # vertex 0 at the origin: three entries whose next and prev name 1, 2, 3 twice each: S = 8 * 65536 per axis, m = 3,
    # mean = floor((524288 + 3) / 6) = 87381, step = (32768 * 87381 + 32768) >> 16 = 43691
    # vertex 1 at (4, 0, 0): x: S = 0, mean = floor(3 / 6) = 0, step = (32768 * -262144 + 32768) >> 16 = floor(-131071.5) = -131072
    assert got.q.tolist() == [[43691] * 3, [131072, 43691, 43691], [43691, 131072, 43691], [43691, 43691, 131072]]
    assert np.array_equal(got.vertices, (got.q / 65536.0).astype(np.float32)) and got.vertices[1, 0] == 2.0


def test_clamp_torus_by_hand():
    """A colour-0 vertex (60000) has six neighbours at -30000; the others have three at 60000 and three at -30000.  lam = 1:
    0 -> -30000, others -> mean 15000.  mu = -1 from there: 0: -30000 - (15000 + 30000) = -75000; others: mean of three at
    -30000 and three at 15000 = -7500, 15000 + 22500 = 37500.  Every iteration multiplies x by -1.25: the fourth would give
    146484.375 and is clamped to 2^33 / 2^16."""
    colour0 = np.isclose(case("clamp_n3")[0][:, 0], CLAMP_HI)
    assert colour0.sum() == 12 and np.isclose(case("clamp_n3")[0][~colour0, 0], CLAMP_LO).all()
    v, f, _ = case("clamp_n3")
    for fix_boundary in MODES:
        one = O.smooth(v, f, iterations=1, lam=1.0, mu=-1.0, fix_boundary=fix_boundary)
        assert (one.vertices[colour0, 0] == -75000.0).all() and (one.vertices[~colour0, 0] == 37500.0).all()
        three, four, nine = (oracle(f"clamp_n{n}", fix_boundary).vertices[:, 0] for n in (3, 4, 9))
        assert (three[colour0] == CLAMP_HI * -1.25 ** 3).all() and np.abs(three).max() < 131072.0
        assert (four[colour0] == 131072.0).all() and (np.abs(four[~colour0]) < 131072.0).all()
        assert np.abs(nine).max() == 131072.0 and np.isfinite(oracle("clamp_n9", fix_boundary).vertices).all()


def test_hub_states_and_the_open_spheres_border():
    on, off = oracle("hub_fan", True), oracle("hub_fan", False)
    assert on.counts.tolist() == [1, 0, HUB_RIM, 0] and on.state[0] == O.MOVABLE and (on.state[1:] == O.FIXED).all()
    assert off.counts.tolist() == [HUB_RIM + 1, 0, 0, 0]
    v, f, _ = case("sphere_open")
    border = ((v == 0.0) | (v == OPEN_N - 1.0)).any(axis=1)
    got = oracle("sphere_open", True)
    assert np.array_equal(got.state == O.FIXED, border) and (len(v), int(border.sum())) == (1968, 384)
    assert got.counts.tolist() == [1968 - 384, 0, 384, 0]
    assert np.array_equal(got.vertices[border].view(np.uint32), v[border].view(np.uint32))      # the rims stay on the border
    for name in ("sphere_binary", "sphere_sdf", "torus_n10"):                                  # closed: nothing is fixed
        assert oracle(name, True).counts.tolist() == [len(case(name)[0]), 0, 0, 0]
        assert np.array_equal(oracle(name, True).vertices.view(np.uint32), oracle(name, False).vertices.view(np.uint32))


def test_invalid_faces_and_unusable_vertices_take_no_part():
    v, f, kw = case("repeated_index")
    got = oracle("repeated_index", True)
    clean = O.smooth(v, f[[0, 2, 4, 6]], fix_boundary=True, **kw)                  # the tetrahedron alone
    assert np.array_equal(got.vertices.view(np.uint32), clean.vertices.view(np.uint32)) and got.state.tolist() == [0, 0, 0, 0, 1]
    v, f, kw = case("bad_indices")
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    assert not ok.all() and np.array_equal(oracle("bad_indices", False).vertices, O.smooth(v, f[ok], fix_boundary=False, **kw).vertices)
    assert oracle("unclusterable", False).counts[O.BAD] == 19 and oracle("unclusterable", False).counts[O.MOVABLE] > 100
    for name in ("random_50_cells", "random_15000_cells"):                        # nearly all boundary: only the other mode moves them
        assert oracle(name, True).counts[O.MOVABLE] < 100 and oracle(name, False).counts[O.MOVABLE] > 19000


def test_arguments_outside_their_range_are_refused():
    v, f, _ = case("tetrahedron")
    below = -1.0 - 2.0 ** -16                                                    # the range is tested after the rounding to 2^-16
    for kw in ({"iterations": -1}, {"iterations": 1025}, {"iterations": 1.5}, {"lam": 0.0}, {"lam": 2.0 ** -18}, {"lam": 1.0001},
               {"lam": np.nan}, {"lam": -0.5}, {"mu": 0.1}, {"mu": below}, {"mu": np.nan}, {"mu": -np.inf}):
        with pytest.raises(ValueError):
            O.smooth(v, f, **kw)
    assert O.weights(1.0, -1.0) == (65536, -65536) and O.weights(1.0, -0.0) == (65536, 0)
    assert O.weights(0.5, -0.53) == (32768, int(np.rint(np.float64(np.float32(-0.53)) * 65536)))
    assert O.weights(2.0 ** -16, -2.0 ** -18) == (1, 0)                           # mu rounds to 0: plain Laplacian
    O.smooth(v, f, iterations=1024, lam=1.0, mu=-1.0)


def test_taubin_smooths_the_binary_sphere_and_keeps_its_volume():
    """DESIGN.md section 24's figures: the terraced marching-cubes surface of a binary sphere (radius 8 on 24^3, level 0.5)."""
    v, f, kw = case("sphere_binary")
    assert kw == {"iterations": 10, "lam": 0.5, "mu": -0.53}
    c, r = (11.5, 11.5, 11.5), 8.0
    before = O.sphere_quality(v, f, c, r)
    after = O.sphere_quality(oracle("sphere_binary", True).vertices, f, c, r)
    laplace = O.sphere_quality(O.smooth(v, f, iterations=10, lam=0.5, mu=0.0).vertices, f, c, r)
    print(f"rms {before.rms:.4f} -> {after.rms:.4f}; normal consistency {before.normal_consistency:.4f} -> {after.normal_consistency:.4f}; "
          f"volume {before.volume:.1f} -> {after.volume:.1f} (Taubin), {laplace.volume:.1f} (mu = 0)")
    assert after.rms < before.rms and after.normal_consistency > before.normal_consistency
    assert abs(after.volume - before.volume) < 0.01 * before.volume
    assert laplace.volume < 0.95 * before.volume
    assert binary_sphere().dtype == np.float32 and set(np.unique(binary_sphere())) == {0.0, 1.0}


# ---- what needs the library or the package, but no GPU -------------------------------------------------------------------
def test_workspace_size_is_positive_monotonic_and_refuses_too_many_faces():
    import svr_amd
    size = svr_amd._lib.lib().svr_mesh_smooth_workspace_bytes
    shapes_v = [0, 1, 63, 64, 65, 257, 100000, 2 ** 31 - 1]
    shapes_f = [0, 1, 63, 64, 65, 257, 200000, 2 ** 28]
    table = np.array([[int(size(V, F)) for F in shapes_f] for V in shapes_v], dtype=np.int64)
    assert (table > 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert table[6, 6] >= 100000 * (2 * 32 + 3 * 4) + 200000 * 3 * 8              # two rows of q, three words, the entries
    for V, F in ((2 ** 31, 0), (0, 2 ** 28 + 1), (-1, 0), (0, -1), (2 ** 40, 2 ** 40)):
        assert size(V, F) == -2                                                     # SVR_E_BADSHAPE


def test_wrapper_checks_its_arguments_before_it_needs_a_device():
    import torch
    import svr_amd  # noqa: F401
    from svr_amd.util.mesh_smooth import SmoothedMesh, smooth_mesh
    v, f, _ = case("tetrahedron")
    tv, tf = torch.from_numpy(v.copy()), torch.from_numpy(f.copy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smooth_mesh(tv, tf)
    for kw, what in (({"iterations": -1}, "iterations"), ({"iterations": 1025}, "iterations"), ({"iterations": 2.5}, "iterations"),
                     ({"lam": 0.0}, "lam"), ({"lam": 1.5}, "lam"), ({"lam": float("nan")}, "lam"), ({"mu": 0.25}, "mu"),
                     ({"mu": -1.5}, "mu"), ({"mu": float("nan")}, "mu")):
        with pytest.raises(ValueError, match=f"mesh_smooth: {what}"):
            smooth_mesh(tv, tf, **kw)
    assert [x for x in SmoothedMesh.__dataclass_fields__] == ["vertices", "state", "moved", "isolated", "fixed", "bad"]


def test_command_line_accepts_smooth_and_the_method_exists(tmp_path, capsys):
    from svr_amd.reconstruct import Reconstruction, main
    assert callable(getattr(Reconstruction, "smooth"))
    # the parser is run before the checkpoint is opened: a known later refusal shows that the flags themselves were accepted
    common = ["--checkpoint", str(tmp_path / "no_such.ckpt"), "--rgb", str(tmp_path / "a.png"), "--out", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as e:
        main(common + ["--smooth", "10", "--smooth_lambda", "0.4", "--smooth_mu", "-0.42", "--simplify", "2", "--drop_unseen"])
    assert e.value.code == 2 and "--drop_unseen needs --color" in capsys.readouterr().err
    for bad in ("0", "-1"):
        with pytest.raises(SystemExit) as e:
            main(common + ["--smooth", bad])
        assert e.value.code == 2 and "--smooth needs a positive number of iterations" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(common + ["--smooth", "1.5"])
    assert e.value.code == 2 and "--smooth" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
