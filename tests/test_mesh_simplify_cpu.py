"""CPU: the numpy oracle of the vertex-clustering rule (tests/mesh_simplify_oracle.py) against the properties the rule promises,
on every shared case and on the closed torus; the workspace size function, the command line's flag and the method, which
need no GPU."""
import numpy as np
import pytest

from tests import mesh_simplify_oracle as O
from tests._mesh_simplify_cases import CASES, TORI, case

_memo = {}


def oracle(name):
    """The oracle's result of a case, computed once."""
    if name not in _memo:
        _memo[name] = O.simplify(*case(name))
    return _memo[name]


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_keeps_its_own_invariants(name):
    v, f, cell = case(name)
    V = len(v)
    got = oracle(name)
    nv, nf = got.vertices, got.faces
    assert nv.dtype == np.float32 and nf.dtype == np.int32 and got.vertex_cluster.dtype == np.int32 and got.cluster_size.dtype == np.int32
    assert nv.shape == (len(got.cluster_size), 3) and nf.shape[1:] == (3,) and got.vertex_cluster.shape == (V,)
    # no kept face is degenerate, no two share a canonical triple, every output vertex is named by a face
    assert not ((nf[:, 0] == nf[:, 1]) | (nf[:, 1] == nf[:, 2]) | (nf[:, 2] == nf[:, 0])).any()
    assert len(np.unique(O.canonical(nf), axis=0)) == len(nf)
    assert np.array_equal(np.unique(nf), np.arange(len(nv)))
    # vertex_cluster against cluster_size, against the cells, and the kept faces against the input faces they were
    ok = O.clusterable(v)
    assert got.bad == int((~ok).sum()) and (got.vertex_cluster[~ok] == -1).all()
    named = got.vertex_cluster >= 0
    assert got.vertex_cluster.max(initial=-1) == len(nv) - 1
    assert np.array_equal(np.bincount(got.vertex_cluster[named], minlength=len(nv)), got.cluster_size)
    q = O.cells(v, cell)
    for j in np.unique(got.vertex_cluster[named])[:50]:
        members = np.flatnonzero(got.vertex_cluster == j)
        assert (q[members] == q[members[0]]).all()
        others = ok & (got.vertex_cluster != j)
        assert not (q[others] == q[members[0]]).all(axis=1).any()                    # the whole cell, nothing but the cell
    assert (np.diff(got.face_index) > 0).all()
    assert np.array_equal(got.vertex_cluster[f[got.face_index]], nf)               # their own rotation, the new numbers
    firsts = np.array([np.flatnonzero(got.vertex_cluster == j)[0] for j in range(min(len(nv), 50))], dtype=np.int64)
    assert (np.diff(firsts) > 0).all()                                             # numbered by ascending root
    # every member within cell + 2^-16 per axis of its vertex (the cases' coordinates are below 256)
    if named.any() and np.abs(v[named]).max() < 256:
        moved = np.abs(v[named].astype(np.float64) - nv[got.vertex_cluster[named]].astype(np.float64))
        assert moved.max() < float(np.float32(cell)) + 2.0 ** -16
    single = got.cluster_size == 1
    roots = np.array([np.flatnonzero(got.vertex_cluster == j)[0] for j in np.flatnonzero(single)[:50]], dtype=np.int64)
    assert np.array_equal(nv[np.flatnonzero(single)[:50]].view(np.uint32), v[roots].view(np.uint32))


def _identity_check(v, f, cell):
    """A cell below the vertex spacing: positions bit-identical to the input, the faces minus degenerate ones and duplicates."""
    got = O.simplify(v, f, cell)
    assert (got.cluster_size == 1).all()
    kept = np.flatnonzero(got.vertex_cluster >= 0)
    assert np.array_equal(got.vertices.view(np.uint32), v[kept].view(np.uint32))
    live = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    _, first = np.unique(O.canonical(f[live]), axis=0, return_index=True)
    want = f[live][np.sort(first)]
    assert np.array_equal(kept[got.faces], want)
    return got


def test_a_cell_below_the_vertex_spacing_is_the_identity():
    v, f, cell = case("own_cells")
    got = _identity_check(v, f, cell)
    assert len(got.vertices) == len(v) and np.array_equal(got.faces, f)
    v, f = (a.copy() for a in case("torus_small_0.3")[:2])
    f = np.concatenate([f, f[5:9][:, [1, 2, 0]], f[:3][:, [0, 2, 1]], [[7, 7, 9]]]).astype(np.int32)   # rotated copies go, flipped ones stay
    got = _identity_check(v, f, 0.03)
    assert len(got.faces) == len(f) - 4 - 1


def test_duplicates_orientation_and_repeated_indices_by_hand():
    got = oracle("duplicates")
    # clusters {0, 4} {1, 5} {2} {3}; {6} and {7} are only in a degenerate face.  Faces 0 (1, 2, 0), 4 (0, 2, 1: the other
    # side), 10 (0, 1, 3) and 13 (1, 3, 2) stay; 1, 2, 3, 9 repeat face 0; 5 repeats 4; 11 repeats 10; 6, 7, 8, 12 are degenerate
    assert got.face_index.tolist() == [0, 4, 10, 13]
    assert got.faces.tolist() == [[1, 2, 0], [0, 2, 1], [0, 1, 3], [1, 3, 2]]
    assert got.vertex_cluster.tolist() == [0, 1, 2, 3, 0, 1, -1, -1] and got.cluster_size.tolist() == [2, 2, 1, 1] and got.bad == 0
    # vertex 0 of the output: 0.5 -> 32768, float32(0.6) 2^16 = 39321.6.. -> 39322, float32(0.4) 2^16 = 26214.4.. -> 26214
    assert np.array_equal(got.vertices[0], (np.array([32768 + 39322, 32768 + 26214, 2 * 32768]) / 2 / 65536).astype(np.float32))
    assert oracle("one_cell").faces.shape == (0, 3) and oracle("one_cell").vertices.shape == (0, 3)
    assert (oracle("one_cell").vertex_cluster == -1).all()


def test_unclusterable_vertices_are_counted_and_their_faces_dropped():
    v, f, cell = case("unclusterable")
    got = oracle("unclusterable")
    ok = O.clusterable(v)
    assert got.bad == 19 and not ok[190] and ok.sum() == 181      # 6 of the 8 values, three times, and the NaN row
    below = np.nextafter(np.float32(65536.0), np.float32(0))
    assert ok[(np.abs(v) == below).any(axis=1)].all() and not ok[(np.abs(v) == 65536.0).any(axis=1)].any()
    assert ok[f[got.face_index]].all()
    for bad in (np.nan, np.inf, 0.0, 2.0 ** -11, 2.0 ** 17, -1.0):
        with pytest.raises(ValueError):
            O.simplify(v, f, bad)


@pytest.mark.parametrize("name", TORI)
def test_torus_stays_closed_shrinks_and_moves_less_than_a_cell(name):
    v, f, cell = case(name)
    got = oracle(name)
    assert O.is_closed(f) and not O.is_closed(f[1:]) and O.is_closed(got.faces)
    assert got.bad == 0 and (got.vertex_cluster >= 0).all()                        # no vertex is dropped
    if cell >= 1:
        assert len(got.vertices) < len(v) and len(got.faces) < len(f)
    moved = np.abs(v.astype(np.float64) - got.vertices[got.vertex_cluster].astype(np.float64))
    assert moved.max() < float(np.float32(cell)) + 2.0 ** -16                       # per axis: the rule's bound
    assert np.sqrt((moved ** 2).sum(axis=1)).max() < np.sqrt(3.0) * (float(np.float32(cell)) + 2.0 ** -16)


# ---- what needs the library or the package, but no GPU -------------------------------------------------------------------
def test_workspace_size_is_positive_monotonic_and_refuses_2_to_the_31():
    import svr_amd
    size = svr_amd._lib.lib().svr_mesh_simplify_workspace_bytes
    shapes = [0, 1, 63, 64, 65, 257, 100000, 200000, 2 ** 31 - 1]
    table = np.array([[int(size(V, F)) for F in shapes] for V in shapes], dtype=np.int64)
    assert (table > 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert table[6, 7] >= 100000 * 48 + 200000 * 12 + 4 * (2 ** 18 + 2 ** 19)           # the per-item pieces and the two tables
    for V, F in ((2 ** 31, 0), (0, 2 ** 31), (-1, 0), (0, -1), (2 ** 40, 2 ** 40)):
        assert size(V, F) == -2                                                     # SVR_E_BADSHAPE


def test_command_line_accepts_simplify_and_the_method_exists(tmp_path, capsys):
    from svr_amd.reconstruct import Reconstruction, main
    assert callable(getattr(Reconstruction, "simplify"))
    # the parser is run before the checkpoint is opened: a known later refusal shows that --simplify itself was accepted
    common = ["--checkpoint", str(tmp_path / "no_such.ckpt"), "--rgb", str(tmp_path / "a.png"), "--out", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as e:
        main(common + ["--simplify", "2", "--drop_unseen"])
    assert e.value.code == 2 and "--drop_unseen needs --color" in capsys.readouterr().err
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit) as e:
            main(common + ["--simplify", bad])
        assert e.value.code == 2 and "--simplify needs a positive number" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_cpu_tensors_are_refused():
    import torch
    import svr_amd  # noqa: F401
    from svr_amd.util.mesh_simplify import simplify_mesh
    v, f, cell = case("duplicates")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify_mesh(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), cell)
