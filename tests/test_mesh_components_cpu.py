"""CPU: the numpy oracle of the connected-components rule (tests/mesh_components_oracle.py) against scipy and against counts made
by hand, the filter oracle's own properties, the host's selection rule (svr_amd.util.mesh_clean.select_rows /
select_components), and the command line's argument check."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_components_oracle as O
from tests._mesh_component_cases import CASES, WHOLE, case, golden_mesh

import svr_amd  # noqa: F401
from svr_amd.util import mesh_clean as M


@pytest.fixture(scope="module")
def oracle():
    """The oracle's components of every case, computed once."""
    memo = {}

    def get(name):
        if name not in memo:
            v, f, mark = case(name)
            memo[name] = O.components(v, f, mark)
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_scipy_and_numbers_by_smallest_vertex(name, oracle):
    v, f, mark = case(name)
    V = len(v)
    got = oracle(name)
    # the canonical numbering, on its own: label c's smallest vertex is root[c], roots ascend, every label is used
    assert got.vertex_label.dtype == np.int32 and got.vertex_label.shape == (V,) and got.face_label.shape == (len(f),)
    assert got.count == len(got.root) and (np.diff(got.root) > 0).all()
    for c in range(got.count):
        assert np.flatnonzero(got.vertex_label == c)[0] == got.root[c]
    ok = O.valid_faces(f, V)
    assert (got.face_label[~ok] == -1).all()
    for k in range(3):
        assert np.array_equal(got.face_label[ok], got.vertex_label[f[ok, k]])
    assert got.vertex_count.sum() == V and got.face_count.sum() == ok.sum()
    assert got.marked_count.sum() == (0 if mark is None else int((mark != 0).sum()))
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return
    g = f[ok].astype(np.int64)
    rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    n, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False) if V else (0, np.zeros(0, int))
    assert n == got.count
    # the same partition: the pairs (scipy label, oracle label) are a bijection
    pairs = np.unique(np.stack([lab, got.vertex_label], axis=1), axis=0)
    assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n


def test_counts_of_the_golden_meshes(oracle):
    scene = oracle("scene_mesh")
    assert scene.count == 7 and sorted(scene.face_count.tolist(), reverse=True) == [44172, 348, 320, 308, 8, 8, 8]
    assert scene.vertex_count.sum() == 22588 and (scene.vertex_count > 0).all() and (scene.face_count > 0).all()
    for name in ("mesh_sphere", "mesh_torus"):
        assert O.components(*golden_mesh(name)).count == 1
    three = oracle("golden_three")
    assert three.count == 3 and sorted(three.face_count.tolist()) == [10, 320, 1280]


def test_box_follows_fmin_fmax(oracle):
    v, f, _ = case("special_coordinates")
    got = oracle("special_coordinates")
    assert np.isnan(v).any() and np.isinf(v).any()
    for c in range(got.count):
        mine = v[got.vertex_label == c]
        for k in range(3):
            x = mine[:, k][~np.isnan(mine[:, k])]
            assert got.bbox_min[c, k] == (x.min() if len(x) else np.inf) and got.bbox_max[c, k] == (x.max() if len(x) else -np.inf)
    assert np.isinf(got.bbox_min[-1]).all() and np.isinf(got.bbox_min[0, 1])        # the all-NaN component, the NaN axis


@pytest.mark.parametrize("name", WHOLE)
def test_filter_keeping_everything_is_the_identity(name, oracle):
    v, f, _ = case(name)
    comps = oracle(name)
    nv, nf, index = O.filter_mesh(v, f, comps, np.ones(comps.count, dtype=bool))
    assert np.array_equal(nv.view(np.uint32), v.view(np.uint32)) and np.array_equal(nf, f)
    assert np.array_equal(index, np.arange(len(v), dtype=np.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_filter_keeping_nothing_is_empty_and_kept_vertices_are_copies(name, oracle):
    v, f, _ = case(name)
    comps = oracle(name)
    nv, nf, index = O.filter_mesh(v, f, comps, np.zeros(comps.count, dtype=bool))
    assert nv.shape == (0, 3) and nf.shape == (0, 3) and index.shape == (0,)
    keep = np.arange(comps.count) % 2 == 0
    nv, nf, index = O.filter_mesh(v, f, comps, keep)
    assert nv.dtype == np.float32 and nf.dtype == np.int32 and index.dtype == np.int32
    assert np.array_equal(nv.view(np.uint32), v[index].view(np.uint32)) and (np.diff(index) > 0).all()
    assert keep[comps.vertex_label[index]].all()
    face_kept = O.valid_faces(f, len(v))
    face_kept[face_kept] = keep[comps.face_label[face_kept]]
    assert np.array_equal(index[nf], f[face_kept])                                  # the same faces, renumbered, in order
    assert len(np.unique(nf)) == len(nv) if len(nf) else len(nv) == 0               # no kept vertex without a face


def test_every_kept_component_of_the_scene_mesh_keeps_its_edges(oracle):
    v, f, _ = case("scene_mesh")
    comps = oracle("scene_mesh")
    for c in range(comps.count):
        keep = np.arange(comps.count) == c
        nv, nf, index = O.filter_mesh(v, f, comps, keep)
        assert len(nf) == comps.face_count[c] and len(nv) == comps.vertex_count[c]
        pairs, n = O.edge_counts(nf)
        want_pairs, want_n = O.edge_counts(f[comps.face_label == c])
        assert np.array_equal(index[pairs], want_pairs) and np.array_equal(n, want_n)


def _rows(face_count, marked=None, lo=None, hi=None):
    C = len(face_count)
    lo = np.zeros((C, 3), np.float32) if lo is None else np.asarray(lo, np.float32)
    hi = np.ones((C, 3), np.float32) if hi is None else np.asarray(hi, np.float32)
    return SimpleNamespace(face_count=np.asarray(face_count, np.int32), marked_count=np.asarray(marked if marked is not None else [0] * C, np.int32),
                           bbox_min=lo, bbox_max=hi, count=C)


def _both(rows, want, **kw):
    """The oracle's rule, the module's on host arrays, and the module's on a MeshComponents: all three give `want`."""
    want = np.asarray(want, dtype=bool)
    assert np.array_equal(O.select(rows, **kw), want), kw
    assert np.array_equal(M.select_rows(rows.face_count, rows.marked_count, rows.bbox_min, rows.bbox_max, **kw), want), kw
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                         # noqa: E731
    comps = M.MeshComponents(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(rows.count, dtype=torch.int32),
                             torch.zeros(rows.count, dtype=torch.int32), t(rows.face_count), t(rows.marked_count), t(rows.bbox_min),
                             t(rows.bbox_max), rows.count)
    got = M.select_components(comps, **kw)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want), kw


def test_selection_rule_on_hand_made_statistics():
    rows = _rows([5, 0, 9, 9, 2], marked=[0, 3, 0, 1, 1])
    _both(rows, [1, 0, 1, 1, 1])                                                    # min_faces = 0 still drops the 0-face component
    _both(rows, [1, 0, 1, 1, 1], min_faces=1)
    _both(rows, [1, 0, 1, 1, 0], min_faces=3)
    _both(rows, [0, 0, 1, 0, 0], keep_largest=True)                                 # a tie goes to the lowest label
    _both(rows, [0, 0, 0, 1, 0], keep_largest=True, require_mark=True)              # the largest among those that pass
    _both(rows, [0, 0, 0, 1, 1], require_mark=True)
    _both(rows, [0, 0, 0, 0, 0], min_faces=10)
    _both(rows, [0, 0, 0, 0, 0], min_faces=10, keep_largest=True)                   # nothing passes: nothing is kept
    _both(_rows([]), [], keep_largest=True)
    # extent: the diagonal in float64 from the float32 box; an axis without a value counts 0
    inf = np.inf
    lo = [[0, 0, 0], [0, inf, 0], [inf, inf, inf], [0, 0, 0], [1, 1, 1]]
    hi = [[3, 4, 12], [3, -inf, 4], [-inf, -inf, -inf], [inf, 0, 0], [1, 1, 1]]
    rows = _rows([1] * 5, lo=lo, hi=hi)
    _both(rows, [1, 1, 1, 1, 1])
    _both(rows, [1, 1, 0, 1, 0], min_extent=5.0)                                    # 13, 5, 0, inf, 0
    _both(rows, [1, 0, 0, 1, 0], min_extent=13.0)
    _both(rows, [0, 0, 0, 1, 0], min_extent=13.000001)
    third = np.float32(1) / np.float32(3)
    rows = _rows([1], lo=[[0, 0, 0]], hi=[[third, 0, 0]])
    _both(rows, [1], min_extent=float(third))                                       # the float32 value widened: compared in float64
    _both(rows, [0], min_extent=float(np.nextafter(np.float64(third), 1.0)))


def test_drop_unseen_without_color_is_refused_before_the_checkpoint_is_opened(tmp_path, capsys):
    from svr_amd.reconstruct import main
    missing = tmp_path / "no_such.ckpt"
    with pytest.raises(SystemExit) as e:
        main(["--checkpoint", str(missing), "--rgb", str(tmp_path / "a.png"), "--out", str(tmp_path / "out"), "--drop_unseen"])
    assert e.value.code == 2 and "--drop_unseen needs --color" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
