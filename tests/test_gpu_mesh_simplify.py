"""GPU: csrc/mesh_simplify.hip through svr_amd.util.mesh_simplify, Reconstruction.simplify() and the command line, against the
numpy oracle (tests/mesh_simplify_oracle.py), every output bit for bit: the vertices as uint32 words, the faces,
`vertex_cluster`, `cluster_size` and the three totals.

The cases with face indices outside [0, V) test the kernels' guards, they read nothing outside the buffers: face_roots()
compares all three indices with [0, V) (in_range) before any of them addresses `root_of`, and it is the only way
ms_face_insert_kernel, ms_face_keep_kernel and ms_emit_kernel reach a face's vertices; FaceKeys is only applied to faces that
passed it.  Unclusterable vertices never become a table key: ms_vertex_insert_kernel tests clusterable() first and marks them
root_of = -1, which face_roots() and ms_sums_kernel (`live`) refuse."""
import numpy as np
import pytest
import torch

from tests import mesh_components_oracle as CO
from tests import mesh_simplify_oracle as O
from tests._mesh_simplify_cases import GPU_CASES, case

pytestmark = pytest.mark.gpu
_want = {}


def _api():
    import svr_amd  # noqa: F401
    from svr_amd.util import mesh_simplify
    return mesh_simplify


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                                # a copy: the cases' arrays are read-only


def _oracle(name):
    if name not in _want:
        _want[name] = O.simplify(*case(name))
    return _want[name]


def _same(got, want, what):
    gv, gf, gc, gs = (t.cpu().numpy() for t in (got.vertices, got.faces, got.vertex_cluster, got.cluster_size))
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gc.dtype == np.int32 and gs.dtype == np.int32, what
    assert (gv.shape, gf.shape, got.bad) == (want.vertices.shape, want.faces.shape, want.bad), (what, gv.shape, gf.shape, got.bad)
    assert np.array_equal(gv.view(np.uint32), want.vertices.view(np.uint32)), what
    assert np.array_equal(gf, want.faces) and np.array_equal(gc, want.vertex_cluster) and np.array_equal(gs, want.cluster_size), what


def _same_bits(a, b, what):
    assert a.bad == b.bad, what
    for k in ("vertices", "faces", "vertex_cluster", "cluster_size"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, k)


@pytest.mark.parametrize("name", GPU_CASES)
def test_simplify_equals_the_oracle_on_both_paths_and_twice(name):
    S = _api()
    v, f, cell = case(name)
    want = _oracle(name)
    dv, df = _dev(v), _dev(f)
    got = S.simplify_mesh(dv, df, cell, strict=False)
    _same(got, want, name)
    per_lane = S.simplify_mesh(dv, df, cell, strict=False, uniform_path=False)
    _same(per_lane, want, name + " per lane")
    _same_bits(got, per_lane, name + " folded against per lane")
    _same_bits(got, S.simplify_mesh(dv, df, cell, strict=False), name + " twice")
    if want.bad:
        with pytest.raises(ValueError, match=f"{want.bad} of {len(v)} vertices"):
            S.simplify_mesh(dv, df, cell)
    else:
        _same(S.simplify_mesh(dv, df, cell), want, name + " strict")


def test_the_cases_cover_what_they_are_for():
    assert _oracle("unclusterable").bad == 19 and _oracle("bad_indices").bad == 0
    assert _oracle("one_cell").faces.shape == (0, 3) and (_oracle("one_cell").vertex_cluster == -1).all()
    own = _oracle("own_cells")
    assert np.array_equal(own.vertices.view(np.uint32), case("own_cells")[0].view(np.uint32)) and np.array_equal(own.faces, case("own_cells")[1])
    assert 45 <= len(_oracle("random_50_cells").vertices) <= 50 and 10000 <= len(_oracle("random_15000_cells").vertices) <= 15000
    assert _oracle("duplicates").face_index.tolist() == [0, 4, 10, 13]
    sizes = _oracle("wave_runs").cluster_size
    assert sizes.max() == 200 and (sizes == 64).sum() >= 2 and (sizes == 1).sum() >= 50


@pytest.mark.parametrize("cell", [2.0, 3.0])
def test_marching_cubes_sphere(cell):
    S = _api()
    from svr_amd.util.visualize import marching_cubes
    from tests import mc_oracle
    v, f = marching_cubes(torch.from_numpy(mc_oracle.sphere(24, 8.0)).cuda(), 0.0)
    want = O.simplify(v.cpu().numpy(), f.cpu().numpy(), cell)
    got = S.simplify_mesh(v, f, cell)
    _same(got, want, cell)
    _same_bits(got, S.simplify_mesh(v, f, cell, uniform_path=False), cell)
    assert 0 < len(want.faces) < f.shape[0] // 4 and O.is_closed(want.faces) and (want.vertex_cluster >= 0).all()


def test_a_cell_outside_its_range_is_refused_and_nothing_is_launched():
    S = _api()
    import svr_amd
    from svr_amd._lib import ptr, stream
    l = svr_amd._lib.lib()
    v, f, _ = case("duplicates")
    dv, df = _dev(v), _dev(f)
    ws_bytes = int(l.svr_mesh_simplify_workspace_bytes(len(v), len(f)))
    ws = torch.full((ws_bytes,), 0x5a, dtype=torch.uint8, device="cuda")
    totals = torch.full((3,), 12345, dtype=torch.int64, device="cuda")
    for cell in (float("nan"), float("inf"), -1.0, 0.0, 2.0 ** -11, float(np.nextafter(np.float32(2.0 ** -10), np.float32(0))),
                 float(np.nextafter(np.float32(2.0 ** 16), np.float32(np.inf))), 1e30):
        rc = l.svr_mesh_simplify_count(ptr(dv), len(v), ptr(df), len(f), cell, ptr(ws), ws_bytes, 1, ptr(totals), stream())
        assert rc == -1 and b"cell=" in l.svr_last_error(), cell                   # SVR_E_BADARG
        with pytest.raises(RuntimeError, match="need 2\\^-10 <= cell <= 2\\^16"):
            S.simplify_mesh(dv, df, cell)
    torch.cuda.synchronize()
    assert totals.tolist() == [12345] * 3 and bool((ws == 0x5a).all())             # not even the totals were cleared
    for cell in (2.0 ** -10, 2.0 ** 16):                                            # the two ends are inside
        _same(S.simplify_mesh(dv, df, cell), O.simplify(v, f, cell), cell)


def test_arguments_are_checked():
    S = _api()
    v, f, cell = case("duplicates")
    dv, df = _dev(v), _dev(f)
    for bad in ((dv.cpu(), df), (dv, df.cpu()), (v, df)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.simplify_mesh(*bad, cell)
    for bad in ((dv.double(), df), (dv[:, :2], df), (dv.reshape(-1), df), (dv, df.long()), (dv, df[:, :2])):
        with pytest.raises(ValueError, match="mesh_simplify: "):
            S.simplify_mesh(*bad, cell)


# ---- Reconstruction.simplify() and the command line ---------------------------------------------------------------------------
# the hand-made Reconstruction (two spheres and a triangle, with an image) and the tiny trained checkpoint of the components tests
from tests.test_gpu_mesh_components import _reconstruction, checkpoint  # noqa: E402, F401


@pytest.mark.parametrize("inf_res", [1, 2])
def test_reconstruction_simplify_resets_colours_and_save_recolours(inf_res, tmp_path):
    from tests import vertex_color_oracle as VO
    rec, m = _reconstruction(inf_res)
    assert rec.vertex_cluster is None
    rec.colorize()
    assert rec.colors is not None
    cells = 4.0                                                               # the spheres' edges are about 3 grid cells long
    want = O.simplify(m.V * np.float32(inf_res), m.F, cells * inf_res)        # in lattice units: `cell` is multiplied by inf_res
    assert 0 < len(want.faces) < len(m.F) and 0 < len(want.vertices) < len(m.V)
    assert rec.simplify(cells) is rec
    assert rec.colors is None and rec.color_state is None and rec.components is None
    got = (rec.vertices.cpu().numpy(), rec.faces.cpu().numpy(), rec.vertex_cluster.cpu().numpy())
    assert np.array_equal(got[0].view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(got[1], want.faces)
    assert np.array_equal(got[2], want.vertex_cluster) and got[2].shape == (len(m.V),)
    paths = rec.save(tmp_path / "v", color=True)                              # colours the simplified mesh
    assert rec.colors.shape == (len(want.vertices), 3) and rec.color_state.shape == (len(want.vertices),)
    pv, pc, pf, _ = VO.read_ply(paths["predicted_ply"])
    assert len(pv) == len(want.vertices) and len(pf) == len(want.faces) and np.array_equal(pc, rec.colors.cpu().numpy())


def test_clean_then_simplify_chains_and_an_empty_mesh_passes_through():
    rec, m = _reconstruction()
    want_clean = CO.clean(m.V, m.F, keep_largest=True)
    want = O.simplify(want_clean[0], want_clean[1], 4.0)
    assert 0 < len(want.faces) < len(want_clean[1])
    assert rec.clean(keep_largest=True).simplify(4.0) is rec
    assert np.array_equal(rec.vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(rec.faces.cpu().numpy(), want.faces) and rec.vertex_cluster.shape == (len(want_clean[0]),)
    assert rec.components.count == 3 and int(rec.kept.sum()) == 1             # clean()'s results stay
    rec.clean(min_faces=10 ** 6)
    assert rec.faces.shape == (0, 3)
    before = (rec.vertices, rec.faces, rec.vertex_cluster)
    assert rec.simplify() is rec and all(a is b for a, b in zip(before, (rec.vertices, rec.faces, rec.vertex_cluster)))


def _obj_counts(path):
    lines = open(path).read().splitlines()
    return sum(l.startswith("v ") for l in lines), sum(l.startswith("f ") for l in lines)


def test_command_line_simplify_writes_fewer_faces(checkpoint, tmp_path, capsys):  # noqa: F811
    from svr_amd.reconstruct import main
    base = ["--checkpoint", str(checkpoint.ckpt), "--rgb", str(checkpoint.image), "--inf_res", "1"]
    assert main(base + ["--out", str(tmp_path / "plain")]) == 0
    capsys.readouterr()
    assert main(base + ["--out", str(tmp_path / "simple"), "--simplify", "2"]) == 0
    (line,) = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    api = checkpoint.rec.reconstruct(checkpoint.image)
    raw = (api.vertices.shape[0], api.faces.shape[0])
    api.simplify(2.0)
    nv, nf = _obj_counts(tmp_path / "simple" / "rgb_predicted.obj")
    assert _obj_counts(tmp_path / "plain" / "rgb_predicted.obj") == raw
    assert (nv, nf) == (api.vertices.shape[0], api.faces.shape[0]) and 0 < nf < raw[1] and 0 < nv < raw[0]
    assert line.endswith(f"vertices={nv} faces={nf}")
