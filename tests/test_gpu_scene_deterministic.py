"""GPU: the bit-reproducible scene step (ifnet.DETERMINISTIC / SVR_DETERMINISTIC=1 on config 5).

Every order-dependent reduction of the step has an ordered form; each is pinned on its own -- the ordered splat bit for bit
against the numpy restatement of its summation order (tests/splat_oracle.py), the others for identical bytes run to run and
against the atomic form within the rounding of the two orders -- and then the whole step and the resumed fit loop.
Figures are printed before they are asserted (pytest -s)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests import splat_oracle as SO
from tests._scene_tree import build_tree

pytestmark = pytest.mark.gpu


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. ordered splat ---------------------------------------------------------------------------------------------------
def _crowded_points():
    """(2, 300, 3) for dims (5, 4, 6): uniform points (60 base cells per sample, ~4.5 points each), one point repeated 17
    times, points at +-0.5, just outside the valid interval, and NaN."""
    g = torch.Generator().manual_seed(41)
    pts = torch.rand(2, 300, 3, generator=g) - 0.5
    pts[0, 100:117] = torch.tensor([0.1234, -0.2345, 0.3456])
    pts[1, 7] = torch.tensor([0.5, 0.0, 0.0])
    pts[1, 8] = torch.tensor([0.0, -0.5, 0.0])
    pts[0, 9] = torch.tensor([0.0, 0.0, 0.4999995])          # above 0.5 - 1e-6
    pts[0, 10] = torch.tensor([-0.4999995, 0.0, 0.0])
    pts[1, 11] = torch.tensor([0.7, 0.2, -0.9])
    pts[0, 12] = torch.tensor([float("nan"), 0.0, 0.0])
    pts[1, 13] = torch.tensor([0.0, float("nan"), float("nan")])
    return pts


def _scene_points():
    """The scene_cfg5small fixture's depth map unprojected: (2, 76 800, 3) normalised points for the 35 x 26 x 28 grid."""
    from svr_amd.model import project
    z = G.load("scene_cfg5small")
    batch, dims, scale = G.scene_inputs(z)
    mod = project(dims, (3, 3, 3), [1.5, 1.5, 1.5])
    with torch.no_grad():
        pts = mod.depthmap_to_gridspace(batch["depthmap_target"].cuda(), scale, normalize=True)
    return pts.contiguous(), dims


def _check_ordered_splat(ops, pts, dims):
    want, v_ref, _ = SO.splat_ordered(pts.cpu().numpy(), dims)
    acc, base, valid, vox = ops.splat_fwd(pts, dims, want_indices=True, ordered=True, want_vox=True)
    acc2, _, _ = ops.splat_fwd(pts, dims, ordered=True)
    ref, rbase, rvalid = ops.splat_fwd(pts, dims, want_indices=True)
    torch.cuda.synchronize()
    assert _bytes_equal(acc, acc2)                                                  # two launches, identical bytes
    assert torch.equal(acc.cpu(), torch.from_numpy(want))                           # the stated order, bit for bit
    assert torch.equal(vox.cpu(), torch.from_numpy(SO.clamp8(want)))
    assert torch.equal(vox, ops.scale_clamp01(acc, 8.0))
    assert torch.equal(valid, rvalid) and torch.equal(base, rbase)
    assert np.array_equal(valid.cpu().numpy().astype(bool), v_ref)
    err = G.rel_err(acc.cpu().numpy(), ref.cpu().numpy())
    print(f"ordered splat {tuple(pts.shape)} -> {dims}: rel_err against the atomic kernel {err:.2e}")
    assert err < 1e-5
    return want


def test_ordered_splat_crowded_cells_equal_the_numpy_oracle_bit_for_bit():
    ops = _ops()
    dims = (5, 4, 6)
    pts = _crowded_points()
    valid, base, _ = SO.splat_terms(pts.numpy(), dims)                              # the premise, on the host, before the launch
    assert valid.sum() == 2 * 300 - 7 and not valid[0, 12] and not valid[1, 7] and not valid[0, 9]
    cells = {}
    for b in range(2):
        for i0, i1, i2 in base[b][valid[b]]:
            cells[(b, i0, i1, i2)] = cells.get((b, i0, i1, i2), 0) + 1
    assert sum(1 for c in cells.values() if c >= 2) >= len(cells) / 2 and max(cells.values()) >= 17
    want = _check_ordered_splat(ops, pts.cuda(), dims)
    assert want.max() > 1.0                                                         # many points per voxel: the sums are real sums


@pytest.mark.parametrize("N", [1, 257])
def test_ordered_splat_strip_tails_and_partial_blocks(N):
    ops = _ops()
    g = torch.Generator().manual_seed(43 + N)
    pts = (torch.rand(2, N, 3, generator=g) - 0.5) * 1.02                           # a few points outside
    _check_ordered_splat(ops, pts.cuda(), (6, 5, 9))                                # W = 9: strips of 4, 4 and 1 voxels


def test_ordered_splat_at_the_scene_density():
    ops = _ops()
    pts, dims = _scene_points()
    assert tuple(pts.shape) == (2, 76800, 3) and dims == (35, 26, 28)
    _check_ordered_splat(ops, pts, dims)


def test_ordered_splat_empty_cloud_and_limits():
    ops = _ops()
    from svr_amd import _lib
    acc, _, _, vox = ops.splat_fwd(torch.zeros(2, 0, 3).cuda(), (4, 4, 4), ordered=True, want_vox=True)
    assert float(acc.abs().sum()) == 0.0 and float(vox.abs().sum()) == 0.0          # written, not left uninitialised
    with pytest.raises(RuntimeError, match="32-bit limits"):                        # 2048 * 1024 * 1024 cells = 2^31
        ops.splat_fwd(torch.zeros(1, 1, 3).cuda(), (2047, 1023, 1023), ordered=True)
    # the C entry point refuses B * N = 2^31 points (and the cell limit) before it touches a buffer
    l = _lib.lib()
    buf = torch.zeros(64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    for B, N, dims in ((32768, 65536, (1, 1, 1)), (1, 1, (2047, 1023, 1023))):
        assert l.svr_voxelize_splat_ordered_workspace(B, N, *dims) < 0
        rc = l.svr_voxelize_splat_fwd_ordered(p, p, None, None, None, B, N, *dims, p, _lib.stream())
        assert rc == -4 and b"32-bit" in l.svr_last_error()                         # SVR_E_UNSUPPORTED


# ---- 2. ordered blur-tap gradient ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(5, 4, 6), (35, 26, 28)])
@pytest.mark.parametrize("K", [3, 5])
def test_ordered_blur_tap_gradient(dims, K):
    """Both kernels combine the SAME float32 thread partials in float64; only the order of the float64 additions differs
    (relative 1e-16 per addition), so after .float() the two results are the same float32 or neighbours: <= 2 ulp = 2.4e-7."""
    ops = _ops()
    g = torch.Generator().manual_seed(47)
    x = torch.rand(2, *dims, generator=g).cuda()
    gout = torch.randn(2, *dims, generator=g).cuda()
    taps = torch.softmax(torch.randn(K, generator=g), 0).cuda()
    for axis in range(3):
        gin_a, gt_a = ops.blur_axis_bwd(x, taps, gout, axis)
        gin_1, gt_1 = ops.blur_axis_bwd(x, taps, gout, axis, ordered=True)
        gin_2, gt_2 = ops.blur_axis_bwd(x, taps, gout, axis, ordered=True)
        torch.cuda.synchronize()
        assert gt_1.dtype == torch.float64 and _bytes_equal(gt_1, gt_2) and _bytes_equal(gin_1, gin_2)
        assert torch.equal(gin_1, gin_a)
        a, o = gt_a.float(), gt_1.float()
        rel = float(((a - o).abs() / a.abs().clamp_min(1e-30)).max())
        print(f"blur taps dims {dims} K {K} axis {axis}: ordered vs atomic {rel:.2e}")
        assert rel <= 2.4e-7
        _, none = ops.blur_axis_bwd(x, taps, gout, axis, want_gtaps=False, ordered=True)
        assert none is None


# ---- 3. level-0 (C = 1) pull scatter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(12, 10, 14), (5, 3, 2)])
@pytest.mark.parametrize("N", [1, 257])
def test_level0_pull_scatter(dims, N):
    ops = _ops()
    from svr_amd import _lib
    g = torch.Generator().manual_seed(53 + N)
    B = 2
    layout = ops.FeatureLayout([1, 16])
    disp = float(np.float32(0.0722))
    pts = ((torch.rand(B, N, 3, generator=g) - 0.5) * 1.3).cuda()                   # partly outside the volume
    vol0 = torch.rand(B, *dims, 1, generator=g).cuda()
    vol1 = torch.rand(B, *dims, 16, generator=g).cuda()
    gfeat = torch.randn(B * N, layout.row_stride, generator=g).cuda()
    assert not ops.pull_plan_supported(B, N, dims, 1, layout.row_stride)            # the "auto" form's answer is unchanged
    plan0 = ops.pull_plan(pts, dims, 1, layout.col[0], layout.row_stride, disp)

    def pull():                                                                     # (level 1 only gives the row its layout)
        g0 = torch.full_like(vol0, float("nan"))                                    # every voxel must be WRITTEN
        ops.gather_bwd([vol0, vol1], [g0, None], pts, gfeat, layout, disp, False, level_plans=[plan0, None], skip_levels=(1,))
        return g0

    a, b = pull(), pull()
    ref0 = torch.zeros_like(vol0)
    ops.gather_bwd([vol0, vol1], [ref0, None], pts, gfeat, layout, disp, False, flags=_lib.GATHER_DETERMINISTIC, skip_levels=(1,))
    torch.cuda.synchronize()
    assert _bytes_equal(a, b) and not torch.isnan(a).any()
    err = G.rel_err(a.cpu().numpy(), ref0.cpu().numpy())
    print(f"level-0 pull dims {dims} N {N}: rel_err against the serial scatter {err:.2e}")
    assert err < 1e-5
    empty = ref0 == 0                                                               # zeros where nothing lands
    assert float(a[empty].abs().sum()) == 0.0 and (N > 1 or int(empty.sum()) > 0)


# ---- 4. differentiable depth head ---------------------------------------------------------------------------------------
MIN_Z, MAX_Z = 0.1953997164964676, 7.0


@pytest.mark.parametrize("shape,size", [((2, 1, 64, 64), 320), ((2, 1, 240, 320), 0)], ids=["64x64_to_320_crop", "identity_240x320"])
def test_depth_head_scene(shape, size):
    """depth = ops.depth_head's, bit for bit; d raw for a random upstream gradient against float64 autograd of the stock
    expression under the gate of tests/test_gpu_depth_head.py: max(2 x torch's own float32 CPU error, 4e-6) of max|grad|."""
    import torch.nn.functional as F
    ops = _ops()
    g = torch.Generator().manual_seed(59)
    raw = 3 * torch.randn(shape, generator=g)
    out_shape = (shape[0], 1, 240, 320)
    up = torch.randn(out_shape, generator=g)

    def stock(dtype):
        r = raw.detach().clone().to(dtype).requires_grad_(True)
        zz = F.interpolate(r, size=320, mode="bilinear")[:, :, 40:280, :] if size else r
        d = torch.sigmoid(zz) * (MAX_Z - MIN_Z) + MIN_Z
        (d * up.to(dtype)).sum().backward()
        return r.grad

    rg, fg = stock(torch.float64), stock(torch.float32)
    r = raw.cuda().requires_grad_(True)
    depth = ops.depth_head_scene(r, size, (40, 280), MIN_Z, MAX_Z)
    assert tuple(depth.shape) == out_shape and depth.requires_grad
    assert torch.equal(depth.detach(), ops.depth_head(raw.cuda(), None, size=size, rows=(40, 280), min_z=MIN_Z, max_z=MAX_Z)[0])
    (depth * up.cuda()).sum().backward()
    gmax = rg.abs().max().item()
    e, t = (r.grad.cpu().double() - rg).abs().max().item() / gmax, (fg.double() - rg).abs().max().item() / gmax
    print(f"depth_head_scene {shape} size {size}: d raw {e:.2e} (torch f32 {t:.2e})")
    assert e <= max(2 * t, 4e-6)
    again = raw.cuda().requires_grad_(True)
    (ops.depth_head_scene(again, size, (40, 280), MIN_Z, MAX_Z) * up.cuda()).sum().backward()
    assert _bytes_equal(again.grad, r.grad)


# ---- 5. ordered BCE -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(2, 300), (3, 50000)])
def test_ordered_bce(B, N):
    ops = _ops()
    g = torch.Generator().manual_seed(61)
    z = (4 * torch.randn(B, N, generator=g)).cuda()
    y = (torch.rand(B, N, generator=g) < 0.5).float().cuda()
    l1, d1 = ops.bce_logits_sum_mean(z, y, gscale=1.0 / N, ordered=True)
    l2, d2 = ops.bce_logits_sum_mean(z, y, gscale=1.0 / N, ordered=True)
    la, da = ops.bce_logits_sum_mean(z, y, gscale=1.0 / N)
    torch.cuda.synchronize()
    assert _bytes_equal(l1, l2) and _bytes_equal(d1, d2) and torch.equal(d1, da)
    ulp = float(torch.nextafter(la.abs(), la.abs() + 1) - la.abs())
    print(f"ordered BCE ({B}, {N}): {float(l1)!r} against atomic {float(la)!r} (ulp {ulp:.2e})")
    assert abs(float(l1) - float(la)) <= ulp


# ---- 6. the whole scene step --------------------------------------------------------------------------------------------
def _scene_step(state, batch, scale):
    from svr_amd.trainer import SceneNetTrainer, default_hparams
    tr = SceneNetTrainer(default_hparams(scale_factor=scale))
    tr.load_state_dict(state)
    tr = tr.cuda().train()
    opt = tr.configure_optimizers()[0][0]
    loss = tr.training_step(batch, 0)["loss"]
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in tr.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    return loss.detach().clone(), grads, {n: p.detach().clone() for n, p in tr.named_parameters()}


# THE GRADIENT GATE AGAINST THE DEFAULT STEP.  The IF-Net deterministic test gates at 1e-4 relative L2.  At this fixture the
# DEFAULT scene step does not repeat itself to 1e-4: its float atomics (splat, scatters) sit in front of a clamp, five
# BatchNorm stages and the UNet's backward, and ten default steps from one state dict differ from each other, pair by pair,
# by a median of 6e-5 .. 1.0e-4 in most tensors (max 2.8e-4; conv_3_1.bias, the deepest and smallest: median 1.8e-4, max
# 4.9e-4).  The deterministic step, which is ONE fixed result, was between 2e-6 and 2.8e-4 from those ten; 66 of the 95
# tensors passed 1e-4 in at least one of them.  So every tensor's gate is max(1e-4, 3 x the median difference of two DEFAULT
# steps for that tensor), measured with default steps only and recorded in tests/golden/scene_default_step_noise.json
# (which also keeps the deterministic-against-default figures, for the record, not for the gate).
# A UNet convolution bias directly in front of a BatchNorm has a true gradient of 0: what the step leaves there is rounding
# noise (norm 1e-7 .. 4e-6 beside 1.5e+1 .. 8e+1 for the same layers' weights), its relative difference between any two runs
# is of order 1 (two default steps: median 1.2 .. 1.4, the same rule gives 3.6 .. 4.2), and it must BE noise: below 1e-5 of
# the largest gradient norm.
NOISE_ONLY = {f"unet.{c}.bias" for c in ("conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "dconv1", "dconv2", "dconv3",
                                         "dconv4", "dconv5", "dconv6", "dconv7")}


def _gradient_gates():
    import json
    import os
    with open(os.path.join(G.GOLD, "scene_default_step_noise.json")) as f:
        rows = json.load(f)["tensors"]
    return {n: max(1e-4, 3 * r["median_default_vs_default"]) for n, r in rows.items()}


def test_scene_step_is_bit_reproducible_under_the_switch():
    """Loss, every gradient (UNet, project.sigma, IF-Net) and every parameter after one Adam step: torch.equal between two
    runs under the switch; against the default step the gates of the IF-Net deterministic test (loss 1e-6 relative,
    gradients 1e-4 relative L2, or 3 x the default step's own run-to-run difference where that is larger: see above)."""
    from oracle import scene_oracle as S
    from svr_amd.model import ifnet as ifn
    from svr_amd.trainer import SceneNetTrainer, default_hparams
    z = G.load("scene_cfg5small")
    batch, dims, scale = G.scene_inputs(z)
    seed_tr = SceneNetTrainer(default_hparams(scale_factor=scale))
    seed_tr.unet.load_state_dict(S.name_seeded_like(seed_tr.unet.state_dict(), 1.0, "unet."), strict=False)
    seed_tr.ifnet.load_state_dict(G.state(128, z=z), strict=False)
    state = copy.deepcopy(seed_tr.state_dict())
    b = {k: v.cuda() for k, v in batch.items()}
    saved = ifn.DETERMINISTIC
    try:
        ifn.DETERMINISTIC = True
        l1, g1, p1 = _scene_step(state, b, scale)
        l2, g2, p2 = _scene_step(state, b, scale)
        assert any(n.startswith("unet.") for n in g1) and "project.sigma" in g1 and any(n.startswith("ifnet.") for n in g1)
        assert torch.equal(l1, l2)
        for n in g1:
            assert torch.equal(g1[n], g2[n]), n
            assert torch.equal(p1[n], p2[n]), n
        ifn.DETERMINISTIC = False
        l3, g3, _ = _scene_step(state, b, scale)
        dl = abs(float(l3) - float(l1)) / abs(float(l1))
        worst = max(((float((g3[n] - g1[n]).norm() / g1[n].norm().clamp_min(1e-30)), n) for n in g1))
        print(f"scene step, deterministic vs default: loss {dl:.2e}, worst gradient {worst[0]:.2e} ({worst[1]})")
        assert dl <= 1e-6
        top = max(float(v.norm()) for v in g1.values())
        gates = _gradient_gates()
        assert set(gates) == set(g1)
        for n in g1:
            d = float((g3[n] - g1[n]).norm() / g1[n].norm().clamp_min(1e-30))
            assert d < gates[n], (n, d, gates[n])
            assert (float(g1[n].norm()) < 1e-5 * top) == (n in NOISE_ONLY), n
    finally:
        ifn.DETERMINISTIC = saved
        ifn._pull_hint.clear()


# ---- 7. resume on the scene loop ----------------------------------------------------------------------------------------
DIMS = (70, 52, 56)
SPLITS = {"train": ["00000", "00001", "00002", "00003"], "val": ["00004"], "test": ["00001", "00004"]}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return build_tree(tmp_path_factory.mktemp("scene_det"), SPLITS, dims=DIMS, seed=11)


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


def test_scene_resume_follows_the_uninterrupted_run_bit_for_bit(tree, tmp_path):
    """test_gpu_fit.py's resume test on train_scene_net: the restored model, optimizer and counters equal the checkpoint, and
    one further step of the resumed model equals the uninterrupted one's in every parameter and buffer."""
    from svr_amd.model import ifnet as ifn
    from svr_amd.trainer import load_checkpoint, train_scene_net
    saved = ifn.DETERMINISTIC
    try:
        ifn.DETERMINISTIC = True
        args = _args(tree, experiment="resumed", val_check_interval=1.0, max_epoch=5)
        first = train_scene_net(args, steps=2, output_root=str(tmp_path / "runs"))
        last = tmp_path / "runs" / "resumed" / "last.ckpt"
        assert first["last_checkpoint"] == str(last)
        ck = load_checkpoint(last)
        again = copy.copy(args)
        again.resume = str(last)
        second = train_scene_net(again, steps=2, output_root=str(tmp_path / "runs"))          # restores, steps no further
        assert second["global_step"] == 2 and second["model"] is not first["model"]
        for k, v in second["model"].state_dict().items():
            assert torch.equal(v.cpu(), ck["state_dict"][k]), k
        restored, written = second["optimizer"].state_dict(), ck["optimizer_states"][0]
        assert restored["param_groups"] == written["param_groups"] and len(restored["state"]) == len(written["state"]) > 0
        for i, s in written["state"].items():
            for name in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(restored["state"][i][name].cpu(), s[name]), (i, name)
        np.random.seed(8)
        batch = first["model"].device_loader("train").batch([0, 3])
        for run in (first, second):
            run["model"].train()
            run["driver"].step(batch, 0)
        torch.cuda.synchronize()
        for (k, a), b in zip(first["model"].state_dict().items(), second["model"].state_dict().values()):
            assert torch.equal(a, b), k
        assert not torch.equal(first["model"].ifnet.fc_out.weight.detach().cpu(), ck["state_dict"]["ifnet.fc_out.weight"])
        assert not torch.equal(first["model"].project.sigma.detach().cpu(), ck["state_dict"]["project.sigma"])
    finally:
        ifn.DETERMINISTIC = saved
        ifn._pull_hint.clear()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_the_switch_refuses_what_it_cannot_order():
    from svr_amd.model import ifnet as ifn
    from svr_amd.trainer import SceneNetTrainer, default_hparams
    z = G.load("scene_cfg5small")
    batch, _, scale = G.scene_inputs(z)
    b = {k: v.cuda() for k, v in batch.items()}
    tr = SceneNetTrainer(default_hparams(scale_factor=scale, subsample_points=5, skip_unet=True)).cuda().train()
    saved = ifn.DETERMINISTIC
    try:
        ifn.DETERMINISTIC = True
        with pytest.raises(RuntimeError, match="subsample_points"):
            tr(b)
        ifn.DETERMINISTIC = False
        with torch.no_grad():
            logits, _, _ = tr(b)                                                    # the default mode takes the same arguments
        assert tuple(logits.shape) == (2, 240 * 320 + 300) and bool(torch.isfinite(logits).all())
    finally:
        ifn.DETERMINISTIC = saved
        ifn._pull_hint.clear()
