"""GPU: csrc/mesh_smooth.hip through svr_amd.util.mesh_smooth, Reconstruction.smooth() and the command line, against the numpy
oracle (tests/mesh_smooth_oracle.py), every output bit for bit: the vertices as uint32 words, `state` and the four counts.

The cases with face indices outside [0, V) test the kernels' guards, they read nothing outside the buffers: face_corners()
compares all three indices with [0, V) before any of them addresses `state`, and it is the only way sm_count_kernel and
sm_fill_kernel reach a face's vertices; a list entry is written from a face that passed it, so what sm_classify_kernel and
sm_step_kernel read through the lists names vertices.  Unusable vertices are state 3 from sm_prepare_kernel on, which
face_corners() refuses."""
import numpy as np
import pytest
import torch

from tests import mesh_components_oracle as CO
from tests import mesh_simplify_oracle as SO
from tests import mesh_smooth_oracle as O
from tests._mesh_smooth_cases import CASES, MODES, case, oracle

pytestmark = pytest.mark.gpu


def _api():
    import svr_amd  # noqa: F401
    from svr_amd.util import mesh_smooth
    return mesh_smooth


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                                # a copy: the cases' arrays are read-only


def _same(got, want, what):
    gv, gs = got.vertices.cpu().numpy(), got.state.cpu().numpy()
    assert gv.dtype == np.float32 and gs.dtype == np.uint8 and gv.shape == want.vertices.shape and gs.shape == want.state.shape, what
    assert [got.moved, got.isolated, got.fixed, got.bad] == want.counts.tolist(), (what, got.moved, got.isolated, got.fixed, got.bad)
    assert np.array_equal(gs, want.state), what
    differ = np.flatnonzero((gv.view(np.uint32) != want.vertices.view(np.uint32)).any(axis=1))
    assert len(differ) == 0, (what, len(differ), differ[:5], gv[differ[:5]], want.vertices[differ[:5]])


def _same_bits(a, b, what):
    assert (a.moved, a.isolated, a.fixed, a.bad) == (b.moved, b.isolated, b.fixed, b.bad), what
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.state, b.state), what


@pytest.mark.parametrize("fix_boundary", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_smooth_equals_the_oracle_twice_strict_and_not(name, fix_boundary):
    S = _api()
    v, f, kw = case(name)
    want = oracle(name, fix_boundary)
    dv, df = _dev(v), _dev(f)
    got = S.smooth_mesh(dv, df, fix_boundary=fix_boundary, strict=False, **kw)
    _same(got, want, name)
    _same_bits(got, S.smooth_mesh(dv, df, fix_boundary=fix_boundary, strict=False, **kw), name + " twice")
    assert np.array_equal(dv.cpu().numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(df.cpu().numpy(), f)   # inputs untouched
    bad = int(want.counts[O.BAD])
    if bad:
        with pytest.raises(ValueError, match=f"{bad} of {len(v)} vertices"):
            S.smooth_mesh(dv, df, fix_boundary=fix_boundary, **kw)
    else:
        _same(S.smooth_mesh(dv, df, fix_boundary=fix_boundary, **kw), want, name + " strict")


def test_many_iterations_and_the_largest_count():
    S = _api()
    v, f, _ = case("sphere_open")
    dv, df = _dev(v), _dev(f)
    for n, lam, mu in ((30, 0.5, -0.53), (1024, 1.0, -1.0), (7, 2.0 ** -16, 0.0), (2, 1.0, -2.0 ** -16)):
        want = O.smooth(v, f, iterations=n, lam=lam, mu=mu)
        _same(S.smooth_mesh(dv, df, iterations=n, lam=lam, mu=mu), want, (n, lam, mu))


def _raw_call(l, dv, df, n, lam, mu, ws, ws_bytes, out, state, counts, fix=1):
    from svr_amd._lib import ptr, stream
    return l.svr_mesh_smooth(ptr(dv), dv.shape[0], ptr(df), df.shape[0], n, lam, mu, fix, ptr(ws), ws_bytes, ptr(out), ptr(state), ptr(counts),
                             stream())


def test_refusals_come_before_anything_is_enqueued():
    S = _api()
    import svr_amd
    l = svr_amd._lib.lib()
    v, f, kw = case("tetrahedron")
    dv, df = _dev(v), _dev(f)
    ws_bytes = int(l.svr_mesh_smooth_workspace_bytes(len(v), len(f)))
    ws = torch.full((ws_bytes,), 0x5a, dtype=torch.uint8, device="cuda")
    out = torch.full((len(v), 3), 7.0, device="cuda")
    state = torch.full((len(v),), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), 12345, dtype=torch.int64, device="cuda")
    nan, inf = float("nan"), float("inf")
    for n, lam, mu, what in ((-1, 0.5, -0.53, b"iterations="), (1025, 0.5, -0.53, b"iterations="), (1, 0.0, -0.53, b"lam="),
                             (1, 2.0 ** -18, -0.53, b"lam="), (1, 1.0 + 2.0 ** -16, -0.53, b"lam="), (1, nan, -0.53, b"lam="),
                             (1, inf, -0.53, b"lam="), (1, -0.5, -0.53, b"lam="), (1, 0.5, 2.0 ** -16, b"mu="),
                             (1, 0.5, -1.0 - 2.0 ** -16, b"mu="), (1, 0.5, nan, b"mu="), (1, 0.5, -inf, b"mu=")):
        assert _raw_call(l, dv, df, n, lam, mu, ws, ws_bytes, out, state, counts) == -1 and what in l.svr_last_error(), (n, lam, mu)
    assert _raw_call(l, dv, df, 1, 0.5, -0.53, ws, ws_bytes, dv, state, counts) == -1 and b"overlaps" in l.svr_last_error()
    assert _raw_call(l, dv, df, 1, 0.5, -0.53, ws, ws_bytes - 1, out, state, counts) == -1 and b"workspace of" in l.svr_last_error()
    assert _raw_call(l, dv, df, 1, 0.5, -0.53, ws[:0], 0, out, state, counts) == -1
    from svr_amd._lib import ptr, stream
    for V, F in ((len(v), 2 ** 28 + 1), (2 ** 31, len(f)), (-1, len(f)), (len(v), -1)):            # refused by size: nothing is read
        assert l.svr_mesh_smooth(ptr(dv), V, ptr(df), F, 1, 0.5, -0.53, 1, ptr(ws), ws_bytes, ptr(out), ptr(state), ptr(counts), stream()) == -2
    for bad in ({"iterations": -1}, {"iterations": 1025}, {"lam": 0.0}, {"lam": nan}, {"mu": 0.5}, {"mu": -1.5}):
        with pytest.raises(ValueError, match="mesh_smooth: "):
            S.smooth_mesh(dv, df, **bad)
    torch.cuda.synchronize()
    assert counts.tolist() == [12345] * 4 and bool((ws == 0x5a).all()) and bool((out == 7.0).all()) and bool((state == 9).all())
    assert np.array_equal(dv.cpu().numpy(), v)
    assert _raw_call(l, dv, df, kw["iterations"], kw["lam"], kw["mu"], ws, ws_bytes, out, state, counts) == 0      # and the same buffers serve
    want = oracle("tetrahedron", True)
    assert counts.tolist() == want.counts.tolist() and np.array_equal(out.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32))
    assert np.array_equal(state.cpu().numpy(), want.state)


def test_empty_meshes_write_what_the_header_says():
    import svr_amd
    l = svr_amd._lib.lib()
    none = torch.empty(0, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), 12345, dtype=torch.int64, device="cuda")
    v0, f0 = torch.empty((0, 3), device="cuda"), torch.empty((0, 3), dtype=torch.int32, device="cuda")
    assert _raw_call(l, v0, f0, 3, 0.5, -0.53, none, 0, v0, none, counts) == 0 and counts.tolist() == [0, 0, 0, 0]      # V = 0: only counts
    v, _, _ = case("unclusterable")
    dv = _dev(v)
    out, state = torch.full((len(v), 3), 7.0, device="cuda"), torch.full((len(v),), 9, dtype=torch.uint8, device="cuda")
    assert _raw_call(l, dv, f0, 3, 0.5, -0.53, none, 0, out, state, counts) == 0                                     # F = 0: ws may be null
    assert counts.tolist() == [0, len(v) - 19, 0, 19] and np.array_equal(out.cpu().numpy().view(np.uint32), v.view(np.uint32))
    assert np.array_equal(state.cpu().numpy(), np.where(O.usable(v), 1, 3))


def test_arguments_are_checked():
    S = _api()
    v, f, _ = case("tetrahedron")
    dv, df = _dev(v), _dev(f)
    for bad in ((dv.cpu(), df), (dv, df.cpu()), (v, df)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.smooth_mesh(*bad)
    for bad in ((dv.double(), df), (dv[:, :2], df), (dv.reshape(-1), df), (dv, df.long()), (dv, df[:, :2])):
        with pytest.raises(ValueError, match="mesh_smooth: "):
            S.smooth_mesh(*bad)


def test_marching_cubes_sphere_on_the_device():
    S = _api()
    from svr_amd.util.visualize import marching_cubes
    from tests._mesh_smooth_cases import binary_sphere
    v, f = marching_cubes(torch.from_numpy(binary_sphere()).cuda(), 0.5)
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    want = O.smooth(hv, hf)
    got = S.smooth_mesh(v, f)
    _same(got, want, "binary sphere")
    assert got.moved == len(hv) and got.fixed == got.isolated == got.bad == 0
    before, after = (O.sphere_quality(x, hf, (11.5, 11.5, 11.5), 8.0) for x in (hv, got.vertices.cpu().numpy()))
    assert after.rms < before.rms and after.normal_consistency > before.normal_consistency
    assert abs(after.volume - before.volume) < 0.01 * before.volume


# ---- Reconstruction.smooth() and the command line -----------------------------------------------------------------------------
# the hand-made Reconstruction (two spheres and a triangle, with an image) and the tiny trained checkpoint of the components tests
from tests.test_gpu_mesh_components import _reconstruction, checkpoint  # noqa: E402, F401


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("inf_res", [1, 2])
def test_reconstruction_smooth_keeps_faces_and_colours_and_save_writes_them(inf_res, tmp_path):
    from tests import vertex_color_oracle as VO
    rec, m = _reconstruction(inf_res)
    assert rec.smooth_state is None
    colors, state = (t.clone() for t in rec.colorize())
    faces = rec.faces
    want = O.smooth(m.V * np.float32(inf_res), m.F, iterations=4, lam=0.5, mu=-0.53)     # in lattice units, as the vertices are stored
    assert want.counts.tolist() == [len(m.V) - 3, 0, 3, 0]                               # the lone triangle is all boundary
    assert rec.smooth(4) is rec
    assert np.array_equal(_words(rec.vertices), want.vertices.view(np.uint32)) and np.array_equal(rec.smooth_state.cpu().numpy(), want.state)
    assert rec.faces is faces and torch.equal(rec.colors, colors) and torch.equal(rec.color_state, state)
    assert rec.components is None and rec.vertex_cluster is None
    paths = rec.save(tmp_path / "v", color=True)                              # the kept colours at the smoothed positions
    pv, pc, pf, _ = VO.read_ply(paths["predicted_ply"])
    assert len(pv) == len(m.V) and len(pf) == len(m.F) and np.array_equal(pc, colors.cpu().numpy())
    assert np.array_equal(pv.view(np.uint32), want.vertices.view(np.uint32))
    free = O.smooth(m.V * np.float32(inf_res), m.F, iterations=4, lam=0.5, mu=-0.53, fix_boundary=False)
    rec2, _ = _reconstruction(inf_res)
    rec2.smooth(4, fix_boundary=False)
    assert np.array_equal(_words(rec2.vertices), free.vertices.view(np.uint32)) and int((rec2.smooth_state == 0).sum()) == len(m.V)
    rec2.colorize()                                                            # a second colorize() resamples at the new positions
    assert rec2.colors.shape == (len(m.V), 3)


def test_clean_then_smooth_then_simplify_chains_and_an_empty_mesh_passes_through():
    rec, m = _reconstruction()
    cleaned = CO.clean(m.V, m.F, keep_largest=True)
    smoothed = O.smooth(cleaned[0], cleaned[1], iterations=3)
    want = SO.simplify(smoothed.vertices, cleaned[1], 4.0)
    assert 0 < len(want.faces) < len(cleaned[1])
    assert rec.clean(keep_largest=True).smooth(3) is rec
    assert np.array_equal(_words(rec.vertices), smoothed.vertices.view(np.uint32)) and np.array_equal(rec.faces.cpu().numpy(), cleaned[1])
    assert rec.components.count == 3 and int(rec.kept.sum()) == 1             # clean()'s results stay
    assert rec.simplify(4.0) is rec
    assert np.array_equal(_words(rec.vertices), want.vertices.view(np.uint32)) and np.array_equal(rec.faces.cpu().numpy(), want.faces)
    assert rec.smooth_state.shape == (len(cleaned[0]),)                       # of the mesh smooth() saw
    rec.clean(min_faces=10 ** 6)
    assert rec.faces.shape == (0, 3)
    before = (rec.vertices, rec.faces, rec.smooth_state)
    assert rec.smooth() is rec and all(a is b for a, b in zip(before, (rec.vertices, rec.faces, rec.smooth_state)))


def _obj(path):
    lines = open(path).read().splitlines()
    v = np.array([[float(x) for x in l.split()[1:4]] for l in lines if l.startswith("v ")], dtype=np.float64).reshape(-1, 3)
    return v, sum(l.startswith("f ") for l in lines)


def test_command_line_smooth_moves_vertices_and_keeps_the_counts(checkpoint, tmp_path, capsys):  # noqa: F811
    from svr_amd.reconstruct import main
    base = ["--checkpoint", str(checkpoint.ckpt), "--rgb", str(checkpoint.image), "--inf_res", "1"]
    assert main(base + ["--out", str(tmp_path / "plain")]) == 0
    capsys.readouterr()
    assert main(base + ["--out", str(tmp_path / "smooth"), "--smooth", "5", "--smooth_lambda", "0.4", "--smooth_mu", "-0.42"]) == 0
    (line,) = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    api = checkpoint.rec.reconstruct(checkpoint.image)
    raw = api.vertices.clone()
    want = O.smooth(raw.cpu().numpy(), api.faces.cpu().numpy(), iterations=5, lam=0.4, mu=-0.42)
    api.smooth(5, lam=0.4, mu=-0.42)
    assert np.array_equal(_words(api.vertices), want.vertices.view(np.uint32)) and want.counts[O.MOVABLE] > 0
    pv, pf = _obj(tmp_path / "plain" / "rgb_predicted.obj")
    sv, sf = _obj(tmp_path / "smooth" / "rgb_predicted.obj")
    assert (len(pv), pf) == (raw.shape[0], api.faces.shape[0]) == (len(sv), sf)
    assert line.endswith(f"vertices={len(sv)} faces={sf}")
    written = api.vertices.cpu().numpy().astype(np.float64)
    assert np.allclose(sv, written, rtol=1e-6, atol=1e-6) and not np.allclose(sv, pv, rtol=1e-6, atol=1e-6)
    fixed = want.state == O.FIXED                                              # the rims on the lattice border did not move
    assert np.allclose(sv[fixed], pv[fixed], rtol=0, atol=0)
