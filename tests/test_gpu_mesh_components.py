"""GPU: csrc/mesh_components.hip through svr_amd.util.mesh_clean, Reconstruction.clean() and the command line, against the
numpy oracle (tests/mesh_components_oracle.py): every integer output and every kept vertex bit for bit, the box by value.

The case with face indices outside [0, V) tests the kernels' guard: mcc_hook_kernel, mcc_relabel_kernel and mcc_keep_kernel
compare all three indices with [0, V) (valid_face) before any of them addresses memory."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_components_oracle as O
from tests._mesh_component_cases import CASES, case

pytestmark = pytest.mark.gpu
INT_FIELDS = ("vertex_label", "face_label", "root", "vertex_count", "face_count", "marked_count")
_want = {}


def _api():
    import svr_amd  # noqa: F401
    from svr_amd.util import mesh_clean
    return mesh_clean


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle(name):
    if name not in _want:
        _want[name] = O.components(*case(name))
    return _want[name]


def _same_components(got, want, what):
    assert got.count == want.count, what
    for k in INT_FIELDS:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, getattr(want, k)), (what, k)
    for k in ("bbox_min", "bbox_max"):                                    # by value: -0.0 == +0.0; no NaN can be in a box
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.float32 and g.shape == (want.count, 3) and np.array_equal(g, getattr(want, k)), (what, k)


def _same_mesh(got, want, what):
    gv, gf, gi = (t.cpu().numpy() for t in got)
    wv, wf, wi = want
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gi.dtype == np.int32, what
    assert gv.shape == wv.shape and gf.shape == wf.shape and gi.shape == wi.shape, (what, gv.shape, wv.shape, gf.shape, wf.shape)
    assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(gf, wf) and np.array_equal(gi, wi), what


@pytest.mark.parametrize("name", list(CASES))
def test_components_equal_the_oracle(name):
    M = _api()
    v, f, mark = case(name)
    want = _oracle(name)
    got = M.mesh_components(_dev(v), _dev(f), _dev(mark))
    _same_components(got, want, name)
    again = M.mesh_components(_dev(v), _dev(f), _dev(mark), uniform_path=False)      # the per-lane statistics path: the same bits
    _same_components(again, want, name + " per lane")
    for k in ("bbox_min", "bbox_max"):
        assert torch.equal(getattr(got, k).view(torch.int32), getattr(again, k).view(torch.int32)), k
    if mark is not None:
        assert not M.mesh_components(_dev(v), _dev(f)).marked_count.any()


@pytest.mark.parametrize("name", ["strip_permuted", "fan_hub_last", "golden_three", "scene_mesh"])
def test_same_bits_twice_and_in_any_face_order(name):
    M = _api()
    v, f, mark = case(name)
    a = M.mesh_components(_dev(v), _dev(f), _dev(mark))
    b = M.mesh_components(_dev(v), _dev(f), _dev(mark))
    for k in INT_FIELDS + ("bbox_min", "bbox_max"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
    order = np.random.default_rng(5).permutation(len(f))
    c = M.mesh_components(_dev(v), _dev(f[order]), _dev(mark))
    assert torch.equal(c.vertex_label, a.vertex_label) and torch.equal(c.face_label.cpu(), a.face_label.cpu()[torch.from_numpy(order)])
    for k in INT_FIELDS[2:] + ("bbox_min", "bbox_max"):
        assert torch.equal(getattr(c, k).view(torch.int32), getattr(a, k).view(torch.int32)), k


def _keeps(name, want):
    C = want.count
    keeps = {"all": np.ones(C, dtype=bool), "none": np.zeros(C, dtype=bool), "every_other": np.arange(C) % 2 == 1}
    if C:
        keeps["without_vertex_0"] = np.arange(C) != want.vertex_label[0]
    return keeps


@pytest.mark.parametrize("name", list(CASES))
def test_filter_equals_the_oracle(name):
    M = _api()
    v, f, mark = case(name)
    want = _oracle(name)
    dv, df = _dev(v), _dev(f)
    comps = M.mesh_components(dv, df)
    for what, keep in _keeps(name, want).items():
        expect = O.filter_mesh(v, f, want, keep)
        _same_mesh(M.filter_components(dv, df, comps, torch.from_numpy(keep).cuda()), expect, (name, what))
    _same_mesh(M.filter_components(dv, df, comps, keep.astype(np.uint8)), expect, (name, "a host uint8 mask"))


def test_clean_mesh_and_selection_on_the_scene_mesh():
    M = _api()
    v, f, mark = case("scene_mesh")
    for kw in (dict(keep_largest=True), dict(min_faces=300), dict(min_faces=9, min_extent=12.0), dict(require_mark=True),
               dict(min_faces=10 ** 6)):
        want = O.clean(v, f, mark, **kw)
        got = M.clean_mesh(_dev(v), _dev(f), _dev(mark), **kw)
        _same_mesh(got[:3], want[:3], kw)
        _same_components(got[3], want[3], kw)
        assert got[4].dtype == torch.bool and got[4].is_cuda and np.array_equal(got[4].cpu().numpy(), want[4]), kw
    assert want[0].shape == (0, 3) and want[1].shape == (0, 3)               # keeping nothing: an empty mesh, no error
    largest = O.clean(v, f, keep_largest=True)
    assert len(largest[1]) == 44172 and largest[4].sum() == 1


def _two_spheres_and_blobs():
    """The field tests/test_gpu_marching_cubes.py builds its sphere from, twice, plus three lattice points below the level on
    their own (each becomes an octahedron of 8 faces): five closed pieces, all away from the border."""
    shape = (40, 36, 32)
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    dist = lambda c, r: np.sqrt(((g - np.array(c, dtype=np.float64)) ** 2).sum(-1)) - r      # noqa: E731
    field = np.minimum(dist((12.3, 12.1, 12.4), 7.3), dist((28.2, 24.4, 18.1), 5.2)).astype(np.float32)
    for p in ((35, 5, 5), (5, 30, 27), (20, 5, 28)):
        assert field[p] > 2
        field[p] = -0.5
    return field


def test_marching_cubes_into_clean_mesh_keeps_one_closed_sphere():
    M = _api()
    from svr_amd.util.visualize import marching_cubes
    v, f = marching_cubes(torch.from_numpy(_two_spheres_and_blobs()).cuda(), 0.0)
    want = O.clean(v.cpu().numpy(), f.cpu().numpy(), keep_largest=True)
    nv, nf, index, comps, keep = M.clean_mesh(v, f, keep_largest=True)
    assert comps.count == want[3].count == 5 and sorted(comps.face_count.tolist())[:3] == [8, 8, 8]
    _same_mesh((nv, nf, index), want[:3], "two spheres")
    assert torch.equal(v[index.long()], nv) and int(keep.sum()) == 1
    pairs, n = O.edge_counts(nf.cpu().numpy())
    assert (n == 2).all()                                                    # closed: every edge lies in exactly two faces
    assert len(nv) - len(pairs) + len(nf) == 2                               # Euler characteristic of a sphere
    assert 0 < len(nf) == int(comps.face_count.max()) < len(f)


def test_arguments_are_checked():
    M = _api()
    v, f, mark = (_dev(a) for a in case("golden_three"))
    comps = M.mesh_components(v, f, mark)
    for bad in ((v.cpu(), f), (v, f.cpu()), (v.cpu().numpy(), f)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.mesh_components(*bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.mesh_components(v, f, mark.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.filter_components(v.cpu(), f, comps, np.ones(comps.count, dtype=bool))
    for bad in ((v.double(), f), (v[:, :2], f), (v.reshape(-1), f), (v, f.long()), (v, f[:, :2]), (v, f.float())):
        with pytest.raises(ValueError, match="mesh_components: "):
            M.mesh_components(*bad)
        with pytest.raises(ValueError, match="mesh_components: "):
            M.filter_components(*bad, comps, np.ones(comps.count, dtype=bool))
    for bad in (mark[:-1], mark.int(), mark[:, None]):
        with pytest.raises(ValueError, match="mesh_components: mark"):
            M.mesh_components(v, f, bad)
    for bad in (np.ones(comps.count + 1, dtype=bool), torch.ones(comps.count - 1, dtype=torch.bool).cuda(), np.ones(comps.count, dtype=np.int32)):
        with pytest.raises(ValueError, match="mesh_components: keep"):
            M.filter_components(v, f, comps, bad)
    with pytest.raises(ValueError, match="mesh_components: "):
        M.filter_components(v[:-1], f, comps, np.ones(comps.count, dtype=bool))
    with pytest.raises(TypeError):
        M.clean_mesh(v, f, min_area=1.0)                                     # face area is no criterion


# ---- Reconstruction.clean() ---------------------------------------------------------------------------------------------------
def _reconstruction(inf_res=1, image=True):
    """The Reconstruction tests/test_gpu_vertex_color.py builds by hand around the placed sphere (the camera of
    make_consts(240, 320) as its intrinsic), with two more pieces that lie behind the camera and add nothing to the render:
    the same sphere, and one small triangle."""
    import svr_amd  # noqa: F401
    from svr_amd.reconstruct import Reconstruction
    from tests import _vertex_color_cases as K
    size = (240, 320)
    V, F, consts, depth = K.case(size, "sphere", "in_view")
    Vb, _ = K.placed("sphere", "behind", size, consts)
    tri = (Vb[:3] - Vb[:3].mean(axis=0)) * np.float32(0.125) + Vb.mean(axis=0)          # inside the hidden sphere, touching nothing
    V3 = np.concatenate([V, Vb, tri]).astype(np.float32)
    F3 = np.concatenate([F, F + len(V), [[2 * len(V), 2 * len(V) + 1, 2 * len(V) + 2]]]).astype(np.int32)
    Kmat = np.eye(4)
    Kmat[0, 0] = Kmat[1, 1] = float(consts[0])
    Kmat[0, 2], Kmat[1, 2] = float(consts[1]), float(consts[2])
    img = K.random_image(size, 20)
    rec = Reconstruction(torch.ones(size, device="cuda"), None, torch.zeros((1, 4, 4, 4), device="cuda"), _dev(V3 * np.float32(inf_res)),
                         _dev(F3), 1, inf_res, [float(x) for x in consts[3:9]], torch.from_numpy(Kmat), _dev(img) if image else None)
    return rec, SimpleNamespace(V=V3, F=F3, consts=consts, depth=depth, img=img, n=len(V))


def test_clean_carries_colours_by_index():
    from tests import vertex_color_oracle as VO
    rec, m = _reconstruction()
    assert rec.components is None and rec.kept is None
    colors, state = (t.clone() for t in rec.colorize())
    want_colors, want_state = VO.vertex_colors(m.V, m.F, m.img, m.depth, m.consts)
    assert np.array_equal(colors.cpu().numpy(), want_colors) and np.array_equal(state.cpu().numpy(), want_state)
    want = O.clean(m.V, m.F, keep_largest=True)                               # two spheres of 320 faces: the tie goes to vertex 0's
    assert rec.clean(keep_largest=True) is rec
    _same_mesh((rec.vertices, rec.faces, torch.from_numpy(want[2]).cuda()), want[:3], "keep_largest")
    assert want[3].count == 3 and np.array_equal(want[2], np.arange(m.n))
    _same_components(rec.components, want[3], "components before the filter")
    assert np.array_equal(rec.kept.cpu().numpy(), [True, False, False])
    assert torch.equal(rec.colors, colors[: m.n]) and torch.equal(rec.color_state, state[: m.n])
    assert np.array_equal(rec.colors.cpu().numpy(), want_colors[want[2]])
    rec.clean(min_faces=10 ** 6)                                              # nothing left: an empty mesh, colours included
    assert rec.vertices.shape == (0, 3) and rec.faces.shape == (0, 3) and rec.colors.shape == (0, 3) and rec.color_state.shape == (0,)


@pytest.mark.parametrize("inf_res", [1, 2])
def test_drop_unseen_equals_the_oracle_on_the_oracles_states(inf_res):
    from tests import vertex_color_oracle as VO
    rec, m = _reconstruction(inf_res)
    _, state = VO.vertex_colors(m.V, m.F, m.img, m.depth, m.consts)
    assert (state[: m.n] == 1).any() and not (state[m.n:] == 1).any()
    lattice = m.V * np.float32(inf_res)
    want = O.clean(lattice, m.F, (state == 1).astype(np.uint8), require_mark=True)
    rec.clean(drop_unseen=True)                                               # no state stored: colorize() runs first
    _same_mesh((rec.vertices, rec.faces, torch.from_numpy(want[2]).cuda()), want[:3], "drop_unseen")
    _same_components(rec.components, want[3], "drop_unseen")
    assert np.array_equal(rec.kept.cpu().numpy(), want[4]) and want[4].tolist() == [True, False, False]
    assert np.array_equal(rec.color_state.cpu().numpy(), state[want[2]])


@pytest.mark.parametrize("inf_res", [1, 2])
def test_min_extent_is_in_grid_cells(inf_res):
    rec, m = _reconstruction(inf_res)
    comps = O.components(m.V, m.F)                                            # of the grid-space mesh, whatever inf_res is
    extent = np.sqrt(((comps.bbox_max.astype(np.float64) - comps.bbox_min.astype(np.float64)) ** 2).sum(axis=1))
    assert extent[2] * 4 < extent[0] and extent[2] * 4 < extent[1]
    cells = 2.0 * extent[2]                                                   # between the triangle's and the spheres'
    want = O.select(comps, min_extent=cells)
    assert want.tolist() == [True, True, False]
    rec.clean(min_extent=cells)
    assert np.array_equal(rec.kept.cpu().numpy(), want) and rec.faces.shape[0] == 640
    # doubling float32 coordinates is exact: the lattice mesh's box is inf_res times the grid mesh's, bit for bit
    assert np.array_equal(rec.components.bbox_max.cpu().numpy(), comps.bbox_max * np.float32(inf_res))


def test_drop_unseen_on_a_depth_only_result_raises():
    rec, _ = _reconstruction(image=False)
    with pytest.raises(RuntimeError, match="holds no image"):
        rec.clean(drop_unseen=True)
    assert rec.components is None and rec.faces.shape[0] == 641               # nothing was replaced
    rec.clean(min_faces=2)                                                    # the size criteria need no image
    assert rec.faces.shape[0] == 640 and rec.colors is None


# ---- the command line ---------------------------------------------------------------------------------------------------------
DIMS = (70, 52, 56)
SPLITS = {"train": ["00000", "00001"], "val": ["00004"], "test": ["00001", "00004"]}
SEED = 11                                                                     # of the tiny tree; see the C > 1 assertion below


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """The tiny checkpoint of tests/test_gpu_reconstruct.py: one deterministic training step on the tiny tree, then fc_out's
    bias moved by the median logit of one view's lattice, so that the mesh at p = 0.5 is not empty."""
    import svr_amd  # noqa: F401
    from svr_amd.model import ifnet as ifn
    from svr_amd.model.ifnet import evaluate_network_on_grid_device
    from svr_amd.reconstruct import Reconstructor
    from svr_amd.trainer import load_checkpoint, save_checkpoint, train_scene_net
    from svr_amd.util.arguments import parse_arguments
    from tests._scene_tree import build_tree
    tree = build_tree(tmp_path_factory.mktemp("clean_tree"), SPLITS, dims=DIMS, seed=SEED)
    root = tmp_path_factory.mktemp("clean_runs")
    a = parse_arguments(["--num_points", "256", "--batch_size", "2", "--scale_factor", "2", "--splitsdir", "tiny", "--datasetdir",
                         str(tree / "data"), "--sanity_steps", "0", "--val_check_percent", "1.0", "--seed", "3"], timestamp=False)
    a.splits_root = str(tree / "splits")
    a.experiment, a.val_check_interval, a.max_epoch, a.inf_res = "clean", 1.0, 1, 1
    image = tree / "data" / "raw" / "tiny" / "00004" / "rgb.png"
    saved = ifn.DETERMINISTIC
    try:
        ifn.DETERMINISTIC = True
        train_scene_net(a, steps=1, output_root=str(root))
        rec = Reconstructor.from_checkpoint(root / "clean" / "last.ckpt")
        vox = rec.reconstruct(image).voxel_occupancy
        p = evaluate_network_on_grid_device(rec.model.ifnet, vox.reshape(1, 1, *DIMS), DIMS, 1)
        with torch.no_grad():
            rec.model.ifnet.fc_out.bias -= torch.logit(p.double()).median().float()
        ckpt = root / "clean" / "shifted.ckpt"
        save_checkpoint(rec.model, ckpt, global_step=int(load_checkpoint(root / "clean" / "last.ckpt")["global_step"]))
        yield SimpleNamespace(ckpt=ckpt, image=image, rec=Reconstructor.from_checkpoint(ckpt, inf_res=1))
    finally:
        ifn.DETERMINISTIC = saved
        ifn._pull_hint.clear()


def _files(directory):
    return {name: open(os.path.join(directory, name), "rb").read() for name in sorted(os.listdir(directory))}


def test_command_line_cleans_only_when_asked(checkpoint, tmp_path, capsys):
    from svr_amd.reconstruct import main
    api = checkpoint.rec.reconstruct(checkpoint.image)
    api.save(tmp_path / "api" / "rgb")
    base = ["--checkpoint", str(checkpoint.ckpt), "--rgb", str(checkpoint.image), "--inf_res", "1"]
    capsys.readouterr()
    assert main(base + ["--out", str(tmp_path / "plain")]) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    assert len(line) == 1 and line[0].endswith(f"vertices={api.vertices.shape[0]} faces={api.faces.shape[0]}")
    assert _files(tmp_path / "plain") == _files(tmp_path / "api")             # without the new flags: save()'s bytes
    C = O.components(api.vertices.cpu().numpy(), api.faces.cpu().numpy()).count
    assert C > 1                                                              # a one-step network's mesh: many pieces (else: another SEED)
    assert main(base + ["--out", str(tmp_path / "largest"), "--keep_largest"]) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    api.clean(keep_largest=True).save(tmp_path / "cleaned" / "rgb")
    assert api.components.count == C and int(api.kept.sum()) == 1
    assert len(line) == 1 and line[0].endswith(f"vertices={api.vertices.shape[0]} faces={api.faces.shape[0]} components={C} kept=1")
    assert _files(tmp_path / "largest") == _files(tmp_path / "cleaned")
    assert _files(tmp_path / "largest")["rgb_predicted.obj"] != _files(tmp_path / "plain")["rgb_predicted.obj"]
