"""GPU: csrc/mesh_normals.hip and csrc/mesh_shade.hip through svr_amd.util.mesh_render, Reconstruction.normals() / render() /
save() and the command line, against the numpy oracle (tests/mesh_render_oracle.py), every output bit for bit.

The cases with face indices outside [0, V) test the kernels' guards, they read nothing outside the buffers: mn_face_kernel
compares a face's three indices with [0, V) before any of them addresses a vertex or an accumulator (face_corners), and
shade_pixel compares the face-map entry with [0, F) and the three vertex indices with [0, V) before it reads a triangle, a
normal or a colour."""
import os

import numpy as np
import pytest
import torch

from tests import _mesh_render_cases as K
from tests import mesh_render_oracle as O
from tests import raycast_oracle as R

pytestmark = pytest.mark.gpu
SIZES = ((13, 19), (24, 32))
CONFIGS = {"smooth": ("smooth", False), "smooth_colors": ("smooth", True), "flat": ("flat", False), "flat_colors": ("flat", True)}
_scene, _image = {}, {}


def _api():
    import svr_amd  # noqa: F401
    from svr_amd.util import mesh_render
    return mesh_render


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                                # a copy: the cases' arrays are read-only


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", K.CASES)
def test_vertex_normals_equal_the_oracle_and_themselves_under_a_face_permutation(name):
    M = _api()
    v, f = K.case(name)
    want = K.oracle(name)
    dv, df = _dev(v), _dev(f)
    normals, state, counts = M.vertex_normals(dv, df, return_counts=True)
    assert normals.dtype == torch.float32 and tuple(normals.shape) == v.shape and state.dtype == torch.uint8
    assert counts == want.counts and np.array_equal(state.cpu().numpy(), want.state)
    differ = np.flatnonzero((_words(normals) != want.normals.view(np.uint32)).any(axis=1))
    assert len(differ) == 0, (name, len(differ), differ[:5], normals.cpu().numpy()[differ[:5]], want.normals[differ[:5]])
    assert np.array_equal(_words(dv), v.view(np.uint32)) and np.array_equal(df.cpu().numpy(), f)          # inputs untouched
    for seed in (5, 6):
        _, g = K.shuffled(name, seed)
        n2, s2, c2 = M.vertex_normals(dv, _dev(g), return_counts=True)
        assert torch.equal(n2.view(torch.int32), normals.view(torch.int32)) and torch.equal(s2, state) and c2 == counts
    n3, s3 = M.vertex_normals(v, f)                                                                      # host arrays are uploaded
    assert torch.equal(n3.view(torch.int32), normals.view(torch.int32)) and torch.equal(s3, state)


def test_vertex_normals_wrap_like_the_oracle():
    M = _api()
    big = np.float32(65535.0)
    v = np.array([[-big, -big, 0], [big, -big, 0], [big, big, 0]], dtype=np.float32)
    f = np.tile(np.array([[0, 1, 2]], dtype=np.int32), (600, 1))
    want = O.vertex_normals(v, f)
    normals, state = M.vertex_normals(_dev(v), _dev(f))
    assert np.array_equal(_words(normals), want.normals.view(np.uint32)) and state.tolist() == [0, 0, 0]
    assert normals[0, 2].item() == -1.0                                        # 600 faces towards +z: the wrapped sum points down


def test_vertex_normals_refusals_come_before_any_work():
    M = _api()
    from svr_amd import _lib
    from svr_amd._lib import ptr, stream
    l = _lib.lib()
    v, f = (_dev(a) for a in K.case("cube"))
    V, F = len(v), len(f)
    nbytes = int(l.svr_mesh_vertex_normals_workspace_bytes(V, F))
    assert nbytes >= 24 * V and l.svr_mesh_vertex_normals_workspace_bytes(-1, 0) == -2 and l.svr_mesh_vertex_normals_workspace_bytes(0, 2 ** 28 + 1) == -2
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    out = torch.full((V, 3), 7.0, device="cuda")
    state = torch.full((V,), 9, device="cuda", dtype=torch.uint8)
    counts = torch.full((3,), -1, device="cuda", dtype=torch.int64)
    call = lambda verts, o, w, wb, c=counts: l.svr_mesh_vertex_normals(ptr(verts), V, ptr(f), F, ptr(w), wb, ptr(o), ptr(state), ptr(c), stream())   # noqa: E731
    both = torch.empty((2 * V, 3), device="cuda")
    both[:V] = v
    assert call(both[:V], both[V - 1:2 * V - 1], ws, nbytes) == -1 and b"overlaps" in l.svr_last_error()
    assert call(v, v, ws, nbytes) == -1
    assert call(v, out, ws, nbytes - 1) == -1 and b"workspace" in l.svr_last_error()
    assert call(v, out, None, nbytes) == -1 and call(v, out, ws, nbytes, None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (state == 9).all() and (counts == -1).all()
    assert call(v, out, ws, nbytes) == 0
    assert np.array_equal(_words(out), K.oracle("cube").normals.view(np.uint32)) and counts.tolist() == [8, 0, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.vertex_normals(v.cpu(), f)
    with pytest.raises(ValueError, match="mesh_render: "):
        M.vertex_normals(v.double(), f)


# ---- the shader ----------------------------------------------------------------------------------------------------------------
def _placed(size):
    """The 12^3 marching-cubes sphere in front of the camera of make_consts(size), with its oracle normals and a palette."""
    if size not in _scene:
        consts = R.make_consts(*size)
        v, f = K.placed("mc_sphere", consts)
        _scene[size] = dict(consts=consts, v=v, f=np.array(f), normals=O.vertex_normals(v, f).normals, colors=K.vertex_palette(len(v)))
    return _scene[size]


def _oracle_image(size, config, ssaa=1):
    key = (size, config, ssaa)
    if key not in _image:
        s = _placed(size)
        shading, coloured = CONFIGS[config]
        _image[key] = O.render_ssaa(s["v"], s["f"], s["consts"], size, ssaa, normals=s["normals"] if shading == "smooth" else None,
                                    colors=s["colors"] if coloured else None)
        _image[key].setflags(write=False)
    return _image[key]


def _same_image(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == np.uint8 and g.shape == want.shape, (what, g.shape, g.dtype)
    differ = np.argwhere((g != want).any(axis=2))
    assert len(differ) == 0, (what, len(differ), differ[:5], [g[r, c].tolist() for r, c in differ[:5]], [want[r, c].tolist() for r, c in differ[:5]])


@pytest.mark.parametrize("tile", [8, 16])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("size", SIZES)
def test_render_mesh_equals_the_oracle(size, config, tile):
    M = _api()
    s = _placed(size)
    shading, coloured = CONFIGS[config]
    want = _oracle_image(size, config)
    assert 0.1 < (want != 255).any(axis=2).mean() < 0.9                         # the sphere and the background both show
    got = M.render_mesh(_dev(s["v"]), _dev(s["f"]), consts=s["consts"], size=size, colors=_dev(s["colors"]) if coloured else None,
                        shading=shading, tile=tile)
    _same_image(got, want, (size, config, tile))


def test_other_light_albedo_background_and_host_arrays():
    M = _api()
    size = (13, 19)
    s = _placed(size)
    kw = dict(ambient=0.6, albedo=(250, 120, 7), background=(3, 40, 200))
    want = O.render(s["v"], s["f"], s["consts"], size, normals=s["normals"], **kw)
    _same_image(M.render_mesh(s["v"], s["f"], consts=s["consts"], size=size, **kw), want, "host arrays")
    for bad in (dict(shading="phong"), dict(ssaa=5), dict(ssaa=0), dict(ambient=1.5), dict(albedo=(1, 2)), dict(background=(0, 0, 256)),
                dict(colors=s["colors"][:-1]), dict(transform=np.diag([1.0, 0.0, 1.0, 1.0])), dict(tile=4)):
        with pytest.raises(ValueError):
            M.render_mesh(s["v"], s["f"], consts=s["consts"], size=size, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.render_mesh(torch.from_numpy(s["v"]), s["f"], consts=s["consts"], size=size)


def test_bad_vertex_indices_and_normals_fall_back_to_the_face():
    """The shading pass alone on a doctored mesh: a face whose index list names no vertex and NaN / zero normals take the face's own
    normal and the albedo, a face-map entry outside [0, F) takes the background -- as the oracle says, bit for bit."""
    M = _api()
    size = (24, 32)
    s = _placed(size)
    rows, cols = (a.reshape(-1) for a in np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij"))
    tri = R.triangle_table(s["v"], s["f"])
    _, face = R.cast(tri, s["consts"], cols, rows)
    hit = np.unique(face[face >= 0])
    f = s["f"].copy()
    f[hit[0]] = [0, len(s["v"]), 1]
    f[hit[1]] = [-5, 2, 3]
    normals = s["normals"].copy()
    normals[f[hit[2]]] = 0
    normals[f[hit[3], 1]] = np.nan
    face = face.copy()
    face[:4] = [len(f), 2 ** 31 - 1, -7, -2 ** 31]
    want = O.shade_pixels(tri, f, len(s["v"]), face, cols, rows, s["consts"], normals, s["colors"]).reshape(*size, 3)
    got = M.shade(_dev(tri), _dev(f), _dev(face.astype(np.int32).reshape(size)), s["consts"], len(s["v"]), _dev(normals), _dev(s["colors"]))
    _same_image(got, want, "doctored")
    assert (want.reshape(-1, 3)[:4] == 255).all()


def test_a_mesh_over_half_the_image_leaves_the_background_on_the_rest():
    M = _api()
    for size in SIZES:
        H, W = size
        consts = R.make_consts(H, W)
        v, f = K.half_plane(consts, W)
        got = M.render_mesh(v, f, consts=consts, size=size, background=(1, 2, 3))
        _same_image(got, O.render(v, f, consts, size, normals=O.vertex_normals(v, f).normals, background=(1, 2, 3)), size)
        g = got.cpu().numpy()
        edge = int(np.floor((W - 1) / 2 - 0.25)) + 1                           # the first column right of the wall
        assert (g[:, edge:] == np.array([1, 2, 3], dtype=np.uint8)).all() and not (g[:, :edge] == np.array([1, 2, 3], dtype=np.uint8)).all(axis=2).any()


@pytest.mark.parametrize("ssaa", [2, 3])
def test_supersampling_equals_the_oracles_downsample_of_its_fine_image(ssaa):
    M = _api()
    for size, config in (((13, 19), "smooth_colors"), ((24, 32), "smooth")):
        s = _placed(size)
        want = _oracle_image(size, config, ssaa)
        got = M.render_mesh(_dev(s["v"]), _dev(s["f"]), consts=s["consts"], size=size, ssaa=ssaa,
                            colors=_dev(s["colors"]) if CONFIGS[config][1] else None)
        _same_image(got, want, (size, config, ssaa))
        assert not np.array_equal(want, _oracle_image(size, config))            # the rim is anti-aliased
    rng = np.random.default_rng(3)
    for s_ in (1, 2, 3, 4):
        fine = rng.integers(0, 256, (5 * s_, 7 * s_, 3)).astype(np.uint8)
        assert np.array_equal(M.box_downsample(_dev(fine), s_).cpu().numpy(), O.box_downsample(fine, s_))


def test_orbit_transform():
    M = _api()
    size = (24, 32)
    s = _placed(size)
    dv, df = _dev(s["v"]), _dev(s["f"])
    plain = M.render_mesh(dv, df, consts=s["consts"], size=size, colors=_dev(s["colors"]))
    still = M.orbit_transform(dv, df, 0, 0, 0, consts=s["consts"])
    assert np.array_equal(still, np.eye(4))
    assert torch.equal(M.render_mesh(dv, df, consts=s["consts"], size=size, colors=_dev(s["colors"]), transform=still), plain)
    turn = M.orbit_transform(dv, df, 30.0, 10.0, -2.0, consts=s["consts"])
    want = O.render(R.transform_vertices(s["v"], turn), s["f"], s["consts"], size, normals=O.transform_normals(s["normals"], turn),
                    colors=s["colors"])
    got = M.render_mesh(dv, df, consts=s["consts"], size=size, colors=_dev(s["colors"]), transform=turn)
    _same_image(got, want, "turned")
    assert not torch.equal(got, plain)


# ---- Reconstruction and the command line -----------------------------------------------------------------------------------------
def _reconstruction(inf_res=1, faces=True):
    import svr_amd  # noqa: F401
    from svr_amd.reconstruct import Reconstruction
    size = (240, 320)
    consts = R.make_consts(*size)
    v, f = K.placed("mc_sphere", consts)
    Kmat = np.eye(4)
    Kmat[0, 0] = Kmat[1, 1] = float(consts[0])
    Kmat[0, 2], Kmat[1, 2] = float(consts[1]), float(consts[2])
    f = f if faces else f[:0]
    rec = Reconstruction(torch.ones(size, device="cuda"), None, torch.zeros((1, 4, 4, 4), device="cuda"), _dev(v * np.float32(inf_res)),
                         _dev(f), 1, inf_res, [float(x) for x in consts[3:9]], torch.from_numpy(Kmat))
    return rec, v, np.array(f), consts


def _obj_counts(path):
    tags = [l.split()[0] for l in open(path)]
    return tags.count("v"), tags.count("vn"), tags.count("f")


def test_reconstruction_normals_render_and_save(tmp_path):
    from PIL import Image
    M = _api()
    rec, v, f, consts = _reconstruction()
    assert rec.vertex_normals is None and rec.normal_state is None
    n, state = rec.normals()
    assert n is rec.vertex_normals and np.array_equal(_words(n), O.vertex_normals(v, f).normals.view(np.uint32)) and not state.any()
    img = rec.render()
    assert img.dtype == torch.uint8 and tuple(img.shape) == (240, 320, 3) and img.is_cuda
    assert torch.equal(img, M.render_mesh(v, f, consts=consts, size=(240, 320), ssaa=2))
    assert 0.02 < (img != 255).any(dim=2).float().mean().item() < 0.9
    side = rec.render(yaw=30.0, pitch=10.0, ssaa=1, size=(120, 160))           # the camera's top left quarter: part of the sphere
    assert tuple(side.shape) == (120, 160, 3) and (side != 255).any() and not torch.equal(side, rec.render(ssaa=1, size=(120, 160)))
    plain = rec.save(tmp_path / "plain" / "a")
    assert set(plain) == {"predicted", "depthmap_png", "depthmap_exr"} and sorted(os.listdir(tmp_path / "plain")) == \
        ["a_depthmap.exr", "a_depthmap.png", "a_predicted.obj"]
    paths = rec.save(tmp_path / "full" / "a", preview=3, normals=True)
    assert set(paths) == set(plain) | {"preview", "preview_1", "preview_2"}
    assert [os.path.basename(paths[k]) for k in ("preview", "preview_1", "preview_2")] == ["a_preview.png", "a_preview_1.png", "a_preview_2.png"]
    assert _obj_counts(paths["predicted"]) == (len(v), len(v), len(f)) and _obj_counts(plain["predicted"]) == (len(v), 0, len(f))
    with Image.open(paths["preview"]) as im:
        assert im.mode == "RGB" and np.array_equal(np.array(im), img.cpu().numpy())
    with Image.open(paths["preview_1"]) as a, Image.open(paths["preview_2"]) as b:
        assert a.size == (320, 240) and not np.array_equal(np.array(a), np.array(b))
        assert np.array_equal(np.array(a), rec.render(yaw=-30.0, pitch=10.0).cpu().numpy())
    for k in plain:                                                             # everything but the OBJ with vn lines is byte for byte
        if k != "predicted":
            assert open(plain[k], "rb").read() == open(paths[k], "rb").read()
    head = open(paths["predicted"]).read().split("vn ")[0]
    assert open(plain["predicted"]).read().startswith(head)
    for forget in (lambda r: r.smooth(1), lambda r: r.simplify(2.0), lambda r: r.clean(keep_largest=True)):
        rec.normals()
        forget(rec)
        assert rec.vertex_normals is None and rec.normal_state is None


def test_reconstruction_inf_res_and_an_empty_mesh(tmp_path):
    rec1, v, f, consts = _reconstruction()
    rec2 = _reconstruction(inf_res=2)[0]
    one = rec1.render(ssaa=1)
    assert torch.equal(rec2.render(ssaa=1), one) and (one != 255).any()         # the lattice indices are divided by inf_res first
    empty = _reconstruction(faces=False)[0]
    img = empty.render(size=(13, 19), background=(9, 8, 7), yaw=20.0)
    assert tuple(img.shape) == (13, 19, 3) and (img.cpu().numpy() == np.array([9, 8, 7], dtype=np.uint8)).all()
    paths = empty.save(tmp_path / "e", preview=1, normals=True)
    assert _obj_counts(paths["predicted"]) == (len(v), len(v), 0) and os.path.exists(paths["preview"])


# the tiny trained checkpoint of the components tests (tests/test_gpu_reconstruct.py's approach: one deterministic step, bias shifted)
from tests.test_gpu_mesh_components import checkpoint  # noqa: E402, F401


def test_command_line_previews_and_normals(checkpoint, tmp_path, capsys):  # noqa: F811
    from svr_amd.reconstruct import main
    base = ["--checkpoint", str(checkpoint.ckpt), "--rgb", str(checkpoint.image), "--inf_res", "1"]
    assert main(base + ["--out", str(tmp_path / "plain")]) == 0
    (plain,) = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    assert "previews=" not in plain and sorted(os.listdir(tmp_path / "plain")) == sorted(
        n for n in ("rgb_depthmap.exr", "rgb_depthmap.png", "rgb_predicted.obj", "rgb_voxelized.obj") if os.path.exists(tmp_path / "plain" / n))
    assert "_preview.png" not in plain and not any("preview" in n for n in os.listdir(tmp_path / "plain"))
    assert main(base + ["--out", str(tmp_path / "shown"), "--preview", "2", "--normals", "--preview_size", "60", "80"]) == 0
    (line,) = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    assert line.endswith(" previews=2") and line.replace(str(tmp_path / "shown"), str(tmp_path / "plain")).startswith(plain.split(" vertices=")[0])
    made = sorted(os.listdir(tmp_path / "shown"))
    assert made == sorted(os.listdir(tmp_path / "plain") + ["rgb_preview.png", "rgb_preview_1.png"])
    from PIL import Image
    with Image.open(tmp_path / "shown" / "rgb_preview.png") as a, Image.open(tmp_path / "shown" / "rgb_preview_1.png") as b:
        assert a.mode == b.mode == "RGB" and a.size == b.size == (80, 60) and not np.array_equal(np.array(a), np.array(b))
        assert (np.array(a) != 255).any()
    nv, nvn, nf = _obj_counts(tmp_path / "shown" / "rgb_predicted.obj")
    assert nv == nvn > 0 and (nv, 0, nf) == _obj_counts(tmp_path / "plain" / "rgb_predicted.obj")
    for n in os.listdir(tmp_path / "plain"):                                    # without the flags: today's files, byte for byte
        if n != "rgb_predicted.obj":
            assert open(tmp_path / "plain" / n, "rb").read() == open(tmp_path / "shown" / n, "rb").read(), n
    assert main(base + ["--out", str(tmp_path / "one"), "--preview"]) == 0
    (line,) = [l for l in capsys.readouterr().out.splitlines() if "_predicted.obj" in l]
    assert line.endswith(" previews=1") and os.path.exists(tmp_path / "one" / "rgb_preview.png") and not os.path.exists(tmp_path / "one" / "rgb_preview_1.png")
