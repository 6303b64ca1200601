"""GPU: svr_amd.reconstruct (image -> mesh without a dataset tree) and DeviceSceneLoader(device_rgb=True), on the tiny tree and
the arguments of tests/test_gpu_fit.py (half-scale lattice, 256 points per sigma, batch 2, no input resize).

The comparisons with the trainer are bit for bit, so the module runs under ifnet.DETERMINISTIC: the default voxel splat adds
with float atomics, whose order -- and with it the last bits of the voxel grid and of everything behind it -- may differ
between two runs of the SAME code; the ordered splat has one result.  Depth map and point cloud come from atomic-free
kernels and are compared in the default mode as well."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from tests._scene_tree import build_tree

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (70, 52, 56)
SPLITS = {"train": ["00000", "00001"], "val": ["00004"], "test": ["00001", "00004"]}
FILES = ("predicted.obj", "voxelized.obj", "depthmap.png", "depthmap.exr")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return build_tree(tmp_path_factory.mktemp("reconstruct"), SPLITS, dims=DIMS, seed=11)


def _args(tree, **kw):
    import svr_amd  # noqa: F401
    from svr_amd.util.arguments import parse_arguments
    a = parse_arguments(["--num_points", "256", "--batch_size", "2", "--scale_factor", "2", "--splitsdir", "tiny",
                         "--datasetdir", str(tree / "data"), "--sanity_steps", "0", "--val_check_percent", "1.0", "--seed", "3"],
                        timestamp=False)
    a.splits_root = str(tree / "splits")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rgb_paths(tree):
    return [tree / "data" / "raw" / "tiny" / name / "rgb.png" for name in SPLITS["test"]]


def _with_a_surface(ckpt, image, out):
    """After one step the network's logits sit on one side of 0 and the mesh at p = 0.5 is empty: move fc_out's bias by the
    median logit over one view's lattice and save that as the checkpoint every comparison below starts from."""
    from svr_amd.model.ifnet import evaluate_network_on_grid_device
    from svr_amd.reconstruct import Reconstructor
    from svr_amd.trainer import load_checkpoint, save_checkpoint
    rec = Reconstructor.from_checkpoint(ckpt)
    vox = rec.reconstruct(image).voxel_occupancy
    p = evaluate_network_on_grid_device(rec.model.ifnet, vox.reshape(1, 1, *DIMS), DIMS, 1)
    with torch.no_grad():
        rec.model.ifnet.fc_out.bias -= torch.logit(p.double()).median().float()
    save_checkpoint(rec.model, out, global_step=int(load_checkpoint(ckpt)["global_step"]))
    return out


@pytest.fixture(scope="module")
def run(tree, tmp_path_factory):
    """One training step -> last.ckpt -> shifted.ckpt; under DETERMINISTIC: the --test files of that checkpoint, the Reconstructor built from
    it and its reconstruction of the test split's two images as one batch."""
    from svr_amd.model import ifnet as ifn
    from svr_amd.reconstruct import Reconstructor
    from svr_amd.trainer import train_scene_net
    root = tmp_path_factory.mktemp("reconstruct_runs")
    saved = ifn.DETERMINISTIC
    try:
        ifn.DETERMINISTIC = True
        train_scene_net(_args(tree, experiment="rec", val_check_interval=1.0, max_epoch=1, inf_res=1), steps=1, output_root=str(root))
        ckpt = _with_a_surface(root / "rec" / "last.ckpt", _rgb_paths(tree)[0], root / "rec" / "shifted.ckpt")
        tested = train_scene_net(_args(tree, experiment="tested", test=str(ckpt), inf_res=1), output_root=str(root))
        rec = Reconstructor.from_checkpoint(ckpt, inf_res=1, scale_factor=2, skip_unet=False)
        views = rec.reconstruct(_rgb_paths(tree))
        yield SimpleNamespace(root=root, ckpt=ckpt, test_dir=tested["output_dir"], rec=rec, views=views)
    finally:
        ifn.DETERMINISTIC = saved
        ifn._pull_hint.clear()


@pytest.mark.parametrize("resize_input", [False, True])
def test_device_rgb_loader_serves_the_default_loaders_batches(tree, resize_input):
    import svr_amd  # noqa: F401
    from svr_amd.dataset import DeviceSceneLoader, scene_net_data
    kw = SimpleNamespace(W=256, resize_input=resize_input, precision=32)
    ds = scene_net_data("train", tree / "data", 256, "tiny", kw, splits_root=tree / "splits")
    old, new = DeviceSceneLoader(ds), DeviceSceneLoader(ds, device_rgb=True)
    assert old.device_rgb is False and new.device_rgb is True
    for seed, order in ((4, [1, 0]), (5, [0, 0])):                   # first touch, then cached views
        np.random.seed(seed)
        want = old.batch(order)
        np.random.seed(seed)
        got = new.batch(order)
        torch.cuda.synchronize()
        assert list(got) == list(want) and got["name"] == want["name"] and got["mesh"] == want["mesh"]
        for k in ("rgb", "points", "occupancies", "depthmap_target"):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert tuple(got["rgb"].shape) == ((2, 3, 256, 256) if resize_input else (2, 3, 240, 320))


def _forward(model, tree):
    """model.forward on the test split's two views from the default device loader -> depth, point cloud, voxel grid."""
    np.random.seed(2)
    batch = model.device_loader("test").batch([0, 1])
    assert batch["name"] == SPLITS["test"]
    with torch.no_grad():
        _, depth, point_cloud = model(batch)
        return depth, point_cloud, model.project(point_cloud)


def test_reconstruct_equals_the_trainers_forward(tree, run):
    model = run.rec.model
    assert not model.training and len(run.views) == 2
    depth, point_cloud, vox = _forward(model, tree)
    for i, view in enumerate(run.views):
        assert tuple(view.depth.shape) == (240, 320) and tuple(view.point_cloud.shape) == (76800, 3)
        assert tuple(view.voxel_occupancy.shape) == (1,) + DIMS
        assert torch.equal(view.depth, depth[i]) and torch.equal(view.point_cloud, point_cloud[i])
        assert torch.equal(view.voxel_occupancy, vox[i])
        assert view.vertices.is_cuda and view.vertices.dtype == torch.float32 and view.vertices.shape[1:] == (3,)
        assert view.faces.is_cuda and view.faces.dtype == torch.int32 and view.faces.shape[1:] == (3,)


def test_depth_and_point_cloud_also_agree_without_the_switch(tree, run):
    from svr_amd.model import ifnet as ifn
    try:
        ifn.DETERMINISTIC = False
        depth, point_cloud, _ = _forward(run.rec.model, tree)
        views = run.rec.reconstruct(_rgb_paths(tree))
    finally:
        ifn.DETERMINISTIC = True
    for i, view in enumerate(views):
        assert torch.equal(view.depth, depth[i]) and torch.equal(view.point_cloud, point_cloud[i])


def test_saved_files_equal_the_test_modes(run, tmp_path):
    for name, view in zip(SPLITS["test"], run.views):
        paths = view.save(tmp_path / name)
        assert sorted(os.path.basename(p) for p in paths.values()) == sorted(f"{name}_{f}" for f in FILES)
        for f in FILES:
            want = os.path.join(run.test_dir, f"{name}_{f}")
            assert open(tmp_path / f"{name}_{f}", "rb").read() == open(want, "rb").read(), (name, f)


def test_reconstruct_never_queries_training_points(tree, run):
    ifnet = run.rec.model.ifnet

    def refuse(*a, **k):
        raise AssertionError("IFNet.forward was called during reconstruct")

    ifnet.forward = refuse
    try:
        with pytest.raises(AssertionError):
            ifnet(torch.zeros(1, 1, *DIMS, device="cuda"), torch.zeros(1, 4, 3, device="cuda"))      # the trap is armed
        # the other input forms on the way: a device tensor and a PIL image, the same batch of two as the fixture's
        first, second = (Image.open(p) for p in _rgb_paths(tree))
        views = run.rec.reconstruct([torch.from_numpy(np.array(first)).cuda(), second])
    finally:
        del ifnet.forward
    for view, want in zip(views, run.views):
        assert torch.equal(view.depth, want.depth) and torch.equal(view.voxel_occupancy, want.voxel_occupancy)
        assert torch.equal(view.vertices, want.vertices) and torch.equal(view.faces, want.faces)


def test_reconstruct_depth_for_a_skip_unet_model(tree, run):
    from svr_amd.reconstruct import Reconstructor
    rec = Reconstructor.from_checkpoint(run.ckpt, scale_factor=2, skip_unet=True)
    assert rec.model.unet is None and not rec.model.training
    with pytest.raises(RuntimeError, match="skip_unet"):
        rec.reconstruct(_rgb_paths(tree)[0])
    depth, point_cloud, vox = _forward(rec.model, tree)
    exr = tree / "data" / "raw" / "tiny" / SPLITS["test"][0] / "distance.exr"
    view = rec.reconstruct_depth(exr)
    assert torch.equal(view.depth, depth[0]) and torch.equal(view.point_cloud, point_cloud[0])
    assert torch.equal(view.voxel_occupancy, vox[0])
    both = rec.reconstruct_depth(depth)                                # the tensor form, batched
    assert len(both) == 2 and torch.equal(both[1].voxel_occupancy, vox[1]) and torch.equal(both[0].vertices, view.vertices)
    with pytest.raises(ValueError):
        rec.reconstruct_depth(depth[:, :100])
    with pytest.raises(RuntimeError):
        rec.reconstruct_depth(depth.cpu())


def test_output_spaces(run, tmp_path):
    from svr_amd.data_processing.convert_to_scaled_obj import normalize_meshes
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.model.projection import _camera_to_grid, project
    view = run.views[0]
    assert view.vertices.shape[0] > 0 and view.faces.shape[0] > 0
    grid = view.save(tmp_path / "g" / "v")["predicted"]
    (normed,) = normalize_meshes(tmp_path / "g", scale_factor=2)
    assert open(view.save(tmp_path / "n" / "v", space="normalized")["predicted"], "rb").read() == open(normed, "rb").read()
    cam = load_obj(view.save(tmp_path / "c" / "v", space="camera")["predicted"])
    g = torch.from_numpy(np.asarray(load_obj(grid).vertices, dtype=np.float32).reshape(-1, 3))
    assert torch.equal(g, view.vertices.cpu()) and np.array_equal(cam.faces, view.faces.cpu().numpy())
    _, inv, t = _camera_to_grid(project.get_intrinsic(), 2)
    back = torch.from_numpy(np.asarray(cam.vertices, dtype=np.float32).reshape(-1, 3)) * inv + t
    # c = fl(fl(g - t) / s) was written (%.9g round-trips float32), back = fl(fl(c * s) + t): three roundings on g - t and
    # one on the sum, each at most u = 2^-24 relative -> |back - g| <= 3u |g - t| + u |g| to first order; 4u of both covers it
    bound = 4 * 2.0 ** -24 * ((g - t).abs() + g.abs())
    assert ((back - g).abs() <= bound).all()
    with pytest.raises(ValueError):
        view.save(tmp_path / "x" / "v", space="world")


def test_grid_to_camera_inverts_the_unprojections_affine():
    """The kernel on its own (a one-step network's mesh may be empty): 1000 points, 4 blocks, the last partly filled."""
    import svr_amd  # noqa: F401
    from svr_amd import ops
    from svr_amd.model.projection import _camera_to_grid, project
    _, inv, t = _camera_to_grid(project.get_intrinsic(), 2)
    k = [float(inv), float(t[0]), float(inv), float(t[1]), float(inv), float(t[2])]
    g = torch.rand(1000, 3, generator=torch.Generator().manual_seed(3)) * 70 - 2
    c = ops.grid_to_camera(g.cuda(), k).cpu()
    s32, t32 = torch.tensor(k[0::2]), torch.tensor(k[1::2])
    want = (g.double() - t32.double()) / s32.double()
    # two float32 roundings (difference, quotient) against float64: 2u relative on the quotient, to first order; 3u covers it
    assert ((c.double() - want).abs() <= 3 * 2.0 ** -24 * want.abs()).all()
    assert torch.equal(c, (g - t32) / s32)
    assert ops.grid_to_camera(g[:0].cuda(), k).shape == (0, 3)
    with pytest.raises(RuntimeError):
        ops.grid_to_camera(g, k)


def test_command_line_writes_the_apis_files(tree, run, tmp_path):
    image = _rgb_paths(tree)[1]
    api = run.rec.reconstruct(image)
    want = api.save(tmp_path / "api" / "00004")
    env = dict(os.environ, SVR_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-m", "svr_amd.reconstruct", "--checkpoint", str(run.ckpt), "--rgb", str(image), "--out",
                        str(tmp_path / "cli"), "--inf_res", "1"], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if "_predicted.obj" in l]
    assert len(lines) == 1 and f"vertices={api.vertices.shape[0]} faces={api.faces.shape[0]}" in lines[0]
    got = tmp_path / "cli" / "rgb_predicted.obj"
    assert str(got) in lines[0] and open(got, "rb").read() == open(want["predicted"], "rb").read()
