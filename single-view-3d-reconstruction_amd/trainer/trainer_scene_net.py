"""Mirror of the reference's SceneNetTrainer forward / training_step / losses contract
(trainer/trainer_scene_net.py:22-55,69-119,145-168) -- BASELINE config 5 -- without Lightning:

    rgb -> Unet -> resize 320 / crop rows 40:280 -> sigmoid*(max_z-min_z)+min_z          (:71-80)
        -> project.depthmap_to_gridspace -> norm_grid_space -> project() voxel occupancy (:85-88)
        -> IFNet(voxel_occupancy, points)                                                 (:101)
    loss = BCE(mean) + MSE(depth, depthmap_target)   (or BCE only with no_depth_sup)      (:147-168)
    Adam groups: unet lr, project 10*lr, ifnet lr                                        (:45-55)

The UNet is stock PyTorch-ROCm ops; unprojection, splat, blur, encoder, gather,
MLP and the BCE run in the HIP kernels.  `subsample_points != 0` (:91-99,108-114): the projected point cloud is
queried too and labelled against the sample's mesh ON THE DEVICE (..data_processing.mesh_occupancies.determine_occupancy,
SURVEY §8 f3) -- the reference copies it to the host and runs trimesh + Cython + numpy per step.

``validation_step`` / ``test_step`` / ``visualize_intermediates`` (:121-143,170-188) write every stage of a view -- the
predicted depth map (.png + .exr), its voxelisation (.obj of boxes) and the predicted mesh (.obj) -- into an `output_dir`
the caller names (the reference's runs/<experiment>/vis/<global_step // 100>: there is no Lightning here).  Grid, lattice
and depth map stay on the device; meshes and image planes are what crosses to the host.

``train_dataloader`` / ``val_dataloader`` / ``test_dataloader`` (:57-67): main-process DataLoaders over ``scene_net_data``
(its items are device tensors).  ``train_scene_net(args, steps=None, output_root='runs')`` stands in for the reference's
``Trainer(...).fit`` / ``.test`` (:215-242) on the loop of trainer/fit.py with ``DeviceSceneLoader`` batches: the best two
checkpoints by mean val_ce_loss plus last.ckpt, ``resume``, ``pretrain_unet`` and the ``test`` mode.
``python -m svr_amd.trainer.trainer_scene_net`` runs it on util/arguments.py's flags.
"""
import argparse
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..dataset.scene_net_data import DeviceSceneLoader, scene_net_data
from ..model import ifnet as _ifnet
from ..model.ifnet import IFNet, implicit_to_mesh
from ..model.projection import project
from ..model.unet import UNetMini, Unet
from ..data_processing.mesh_occupancies import determine_occupancy
from ..util.visualize import visualize_depthmap, visualize_grid


class _BCELogitsMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        B, N = logits.shape
        loss, dz = ops.bce_logits_sum_mean(logits.contiguous(), targets.contiguous().float(), want_grad=True,
                                           gscale=1.0 / N, ordered=_ifnet.DETERMINISTIC)
        ctx.save_for_backward(dz)
        return loss.squeeze(0) / N

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None


def default_hparams(**kw):
    h = dict(lr=1e-4, kernel_size=[3, 3, 3], sigma=[1.5, 1.5, 1.5], scale_factor=1, resize_input=True, skip_unet=False,
             subsample_points=0, no_depth_sup=False, min_z=0.1953997164964676, max_z=7.0, net_res=128,
             reference_occupancy_quirk=True, miopen_benchmark=True, visualize=False, inf_res=1)
    h.update(kw)
    return SimpleNamespace(**h)


class SceneNetTrainer(nn.Module):
    def __init__(self, kwargs=None, dims=None):
        super().__init__()
        self.hparams = kwargs if kwargs is not None else default_hparams()
        h = self.hparams
        self.ifnet = IFNet(net_res=getattr(h, "net_res", 128))
        self.kernel_size = h.kernel_size
        if dims is None:
            dims = (torch.tensor([139, 104, 112]) / h.scale_factor).round().long()
        self.dims = torch.as_tensor(dims).long()
        self.project = project(self.dims, self.kernel_size, torch.tensor(h.sigma, dtype=torch.float32))
        if not h.skip_unet and getattr(h, "miopen_benchmark", True):
            # The UNet's stock MIOpen convolutions fall back to `naive_conv_*` solvers on gfx950 unless MIOpen is allowed
            # to time its solvers once per shape: config-5 step 79 -> 27 ms (tools/bench_scene.py).  Process-wide switch.
            torch.backends.cudnn.benchmark = True
        if h.skip_unet:
            self.unet = None
        elif h.resize_input:
            self.unet = Unet(channels_in=3, channels_out=1)
        else:
            self.unet = UNetMini(channels_in=3, channels_out=1)

    def configure_optimizers(self):
        h = self.hparams
        groups = []
        if self.unet is not None:
            groups.append({"params": self.unet.parameters(), "lr": h.lr})
        groups += [{"params": self.project.parameters(), "lr": 10 * h.lr}, {"params": self.ifnet.parameters()}]
        return [torch.optim.Adam(groups, lr=h.lr)], []

    def dataset(self, split):
        h = self.hparams
        return scene_net_data(split, h.datasetdir, h.num_points, h.splitsdir, h, splits_root=getattr(h, "splits_root", "data/splits"),
                              intrinsics_path=getattr(h, "intrinsics_path", None))

    def device_loader(self, split):
        return DeviceSceneLoader(self.dataset(split))

    def train_dataloader(self):
        return torch.utils.data.DataLoader(self.dataset("train"), batch_size=self.hparams.batch_size, shuffle=True, num_workers=0,
                                           drop_last=True)

    def val_dataloader(self):
        return torch.utils.data.DataLoader(self.dataset("val"), batch_size=self.hparams.batch_size, shuffle=False, num_workers=0,
                                           drop_last=False)

    def test_dataloader(self):
        return torch.utils.data.DataLoader(self.dataset("test"), batch_size=self.hparams.batch_size, shuffle=False, num_workers=0,
                                           drop_last=False)

    def _depth_and_voxels(self, batch):
        """The stages in front of the IF-Net query, shared with reconstruct.Reconstructor: batch['rgb'] (or, without a UNet,
        batch['depthmap_target']) -> (depth (B, 240, 320), point_cloud (B, 76800, 3) normalised grid space,
        voxel_occupancy (B, 1, *dims)).  Reads no other key."""
        depth = self._predict_depth(batch["rgb"]) if self.unet is not None else batch["depthmap_target"]
        return (depth,) + self._voxels_from_depth(depth)

    def _predict_depth(self, rgb):
        """rgb (B, 3, H, W) -> depth (B, 240, 320): the UNet and its depth head."""
        h = self.hparams
        raw = self.unet(rgb)
        if _ifnet.DETERMINISTIC:                      # read at call time, like the IF-Net's own use of it
            # ATen's backward of F.interpolate(mode="bilinear") accumulates with float atomics: the depth head's gather-form
            # transposed interpolation instead (resize_input False: identity mode, the sigmoid map alone)
            return ops.depth_head_scene(raw, 320 if h.resize_input else 0, (40, 280), h.min_z, h.max_z).squeeze(1)
        if h.resize_input:
            logits = F.interpolate(raw, size=320, mode="bilinear")[:, :, 40:280, :].squeeze(1)
        else:
            # UNetMini's (B, 1, 240, 320): one map per item, like the resized branch.  (The reference keeps the channel
            # axis here, :77, and its mse_loss then broadcasts (B, 1, H, W) against the (B, H, W) target to B x B pairs.)
            logits = raw.squeeze(1)
        return torch.sigmoid(logits) * (h.max_z - h.min_z) + h.min_z

    def _voxels_from_depth(self, depth):
        """depth (B, 240, 320) -> (point_cloud, voxel_occupancy): unproject + normalise fused in one kernel, then project()."""
        point_cloud = self.project.depthmap_to_gridspace(depth.contiguous(), self.hparams.scale_factor, normalize=True)
        return point_cloud, self.project(point_cloud)

    def forward(self, batch):
        h = self.hparams
        if _ifnet.DETERMINISTIC:
            self._check_deterministic(batch)
        depth, point_cloud, voxel_occupancy = self._depth_and_voxels(batch)
        # trainer_scene_net.py:91-99.  The reference's first condition reads `n < (240*320) & n > 0`: `&` binds tighter
        # than the comparisons, so it is the chain  n < (76800 & n) > 0 , which no n satisfies (76800 & n <= n) -- the
        # random-subset branch is dead code there and the whole point cloud is used whenever n != 0.  Mirrored as is.
        n = h.subsample_points
        masked = (240 * 320) & n if n > 0 else 0
        if n < masked and masked > 0:
            indices = torch.randperm(point_cloud.shape[1], device=point_cloud.device)[:n]
            point_cloud = point_cloud[:, indices, :].contiguous()
            points = torch.cat((point_cloud, batch["points"]), dim=1)
        elif n == 0:
            points = batch["points"]
        else:
            points = torch.cat((point_cloud, batch["points"]), dim=1)
        logits_depth = self.ifnet(voxel_occupancy, points)
        return logits_depth, depth, point_cloud

    def _check_deterministic(self, batch):
        """What ifnet.DETERMINISTIC (SVR_DETERMINISTIC=1) cannot make bit-reproducible raises instead of running with atomics."""
        h = self.hparams
        if h.subsample_points != 0:
            raise RuntimeError("SceneNetTrainer, DETERMINISTIC: subsample_points != 0 queries the projected point cloud, and "
                               "d(loss)/d(points) of the gather is accumulated with float atomics (no atomic-free form)")
        if getattr(h, "net_res", 128) == 32:
            raise RuntimeError("SceneNetTrainer, DETERMINISTIC: net_res=32 has 128-channel levels without an atomic-free scatter")
        B = int(batch["points"].shape[0])
        dims = tuple(int(v) for v in self.dims)
        if not ops.splat_ordered_supported(B, 240 * 320, dims):
            raise RuntimeError(f"SceneNetTrainer, DETERMINISTIC: batch {B} x grid {dims} exceeds the ordered splat's 32-bit limits "
                               "(B*(D0+1)(D1+1)(D2+1) < 2^31 - 1, B*N < 2^31)")

    def _occupancies(self, batch, point_cloud):
        """trainer_scene_net.py:108-114: ground truth of the extra query points = on-the-fly labelling against the mesh."""
        if self.hparams.subsample_points == 0:
            return batch["occupancies"]
        # (the reference calls it with the default dims (139, 104, 112) whatever scale_factor is, :112)
        _, occ_pc = determine_occupancy(batch["mesh"], point_cloud.detach(),
                                        reference_quirk=getattr(self.hparams, "reference_occupancy_quirk", True),
                                        points_normalized=True)
        return torch.cat((occ_pc.to(batch["occupancies"].dtype), batch["occupancies"]), dim=1)

    def losses_and_logging(self, batch, depthmap, logits, occupancies, mode="train"):
        ce_loss = _BCELogitsMeanFn.apply(logits, occupancies)
        mse_loss = F.mse_loss(depthmap, batch["depthmap_target"], reduction="mean")
        mesh_ce_loss = ce_loss
        if self.hparams.subsample_points > 0:          # :151-154 (logged only)
            k = self.hparams.subsample_points
            mesh_ce_loss = _BCELogitsMeanFn.apply(logits[:, k:].contiguous(), occupancies[:, k:].contiguous())
        self.last_log = {f"{mode}_ce_loss": ce_loss.detach(), f"{mode}_mse_depth_loss": mse_loss.detach(),
                         f"{mode}_mesh_ce_loss": mesh_ce_loss.detach(),
                         "sigma_x": self.project.sigma[2].detach(), "sigma_y": self.project.sigma[1].detach(),
                         "sigma_z": self.project.sigma[0].detach()}
        if self.hparams.no_depth_sup:
            return ce_loss
        return ce_loss + mse_loss

    def training_step(self, batch, batch_idx):
        logits, depthmap, point_cloud = self.forward(batch)
        occupancies = self._occupancies(batch, point_cloud)
        loss = self.losses_and_logging(batch, depthmap, logits, occupancies, "train")
        return {"loss": loss}

    def validation_step(self, batch, batch_idx, output_dir=None):
        """trainer_scene_net.py:121-137: the training step's forward and loss without gradients, logged as val_*; with
        ``hparams.visualize`` the intermediates go to `output_dir`.  The module's train / eval mode is the caller's (as
        under Lightning, which switches to eval around validation)."""
        with torch.no_grad():
            logits, depthmap, point_cloud = self.forward(batch)
            occupancies = self._occupancies(batch, point_cloud)
            if getattr(self.hparams, "visualize", False):
                if output_dir is None:
                    raise ValueError("validation_step: hparams.visualize needs an output_dir")
                self.visualize_intermediates(batch, depthmap, point_cloud, output_dir)
            loss = self.losses_and_logging(batch, depthmap, logits, occupancies, "val")
        return {"val_loss": loss}

    def test_step(self, batch, batch_idx, output_dir):
        """trainer_scene_net.py:139-143 (the reference's --test mode): forward, then every intermediate of every item."""
        with torch.no_grad():
            _, depthmap, point_cloud = self.forward(batch)
            self.visualize_intermediates(batch, depthmap, point_cloud, output_dir)
        return {"loss": 0}

    def visualize_intermediates(self, batch, depthmap, point_cloud, output_dir):
        """trainer_scene_net.py:170-188.  Per item, with base = "_".join(name.split("/")[-3:]):
        ``<base>_voxelized.obj`` (visualize_grid of the re-projected point cloud's occupancy), ``<base>_predicted.obj``
        (implicit_to_mesh at threshold_p = 0.5 on self.dims, res_increase = hparams.inf_res) and ``<base>_depthmap.png`` /
        ``.exr`` (columns flipped, as the reference)."""
        out = Path(output_dir)
        out.mkdir(exist_ok=True, parents=True)
        dims = self.dims.cpu().numpy().astype(np.int32)
        inf_res = int(getattr(self.hparams, "inf_res", 1))
        with torch.no_grad():
            voxel_occupancy = self.project(point_cloud)
            for i in range(len(batch["name"])):
                base = "_".join(batch["name"][i].split("/")[-3:])
                vox = voxel_occupancy[i]
                visualize_grid(vox.reshape(vox.shape[-3:]), out / f"{base}_voxelized.obj")
                implicit_to_mesh(self.ifnet, vox.reshape(1, 1, *vox.shape[-3:]), dims, 0.5, out / f"{base}_predicted.obj",
                                 res_increase=inf_res)
                visualize_depthmap(depthmap[i], out / f"{base}_depthmap", flip=True)


def use_pretrained_unet(args, path=None):
    """trainer_scene_net.py:204-212 (``--pretrain_unet``): a SceneNetTrainer(args) whose `unet.*` entries come from the
    checkpoint at `path` (default ``args.pretrain_unet``; written by trainer_unet.train_unet or by the reference).  Only the
    entries whose key contains 'unet' are taken; ``load_state_dict(strict=False)`` leaves everything else as constructed."""
    from .checkpoint import load_checkpoint
    model = SceneNetTrainer(args)
    pretrained_dict = load_checkpoint(path if path is not None else args.pretrain_unet)["state_dict"]
    pretrained_dict = {k: v for k, v in pretrained_dict.items() if "unet" in k}
    model.load_state_dict(pretrained_dict, strict=False)
    return model


def run_scene_net_test(args, output_root="runs"):
    """The reference's ``--test`` (:233-240): the trainer is built from the hyper-parameters of the checkpoint ``args.test``,
    with inf_res, scale_factor and skip_unet taken from `args`; ``test_step`` runs over the test split in eval mode and
    writes every view's intermediates to <output_root>/<args.experiment>/vis/<checkpoint's global_step // 100>.  Nothing is
    trained."""
    from . import fit as F
    from .checkpoint import load_checkpoint
    ck = load_checkpoint(args.test)
    hparams = argparse.Namespace(**ck["hyper_parameters"])
    hparams.inf_res, hparams.scale_factor, hparams.skip_unet = args.inf_res, args.scale_factor, args.skip_unet
    model = SceneNetTrainer(hparams)
    state = {k: v for k, v in ck["state_dict"].items() if model.unet is not None or not k.startswith("unet.")}
    model.load_state_dict(state)
    model = model.cuda().eval()
    global_step = int(ck.get("global_step", 0))
    out = Path(output_root) / getattr(args, "experiment", hparams.experiment) / "vis" / f"{global_step // 100:05d}"
    loader = model.device_loader("test")
    for i, indices in enumerate(F.epoch_batches(len(loader), int(hparams.batch_size), shuffle=False, drop_last=False)):
        model.test_step(loader.batch(indices), i, out)
    return {"model": model, "checkpoint": str(args.test), "best_val_loss": None, "global_step": global_step, "history": {},
            "output_dir": str(out)}


def train_scene_net(args, steps=None, output_root="runs"):
    """Fit loop (trainer_scene_net.py:215-242).  Reads from `args`, beside the trainer's hyper-parameters and the dataset's
    (datasetdir, splitsdir, num_points, W, resize_input, precision, optional splits_root / intrinsics_path): seed (< 0:
    none), experiment, batch_size, sanity_steps, max_epoch, val_check_interval (capped at half an epoch, :228),
    val_check_percent, save_epoch, resume, pretrain_unet, test, optional log_every (50).  `steps` caps the number of
    optimizer steps.  Validation output (``visualize``) goes to <output_root>/<experiment>/vis/<global_step // 100>;
    <output_root>/<experiment>/ holds the best two by mean val_ce_loss (epoch=<n>-step=<s>.ckpt) and last.ckpt.  ``args.test`` set: ``run_scene_net_test`` instead.
    Returns {'model', 'checkpoint' (the best one), 'best_val_loss' (its mean val_ce_loss), 'global_step', 'history',
    'optimizer', 'driver', 'last_checkpoint'}."""
    from . import fit as F
    F.init_distributed(getattr(args, "gpu", None))
    F.seed_everything(getattr(args, "seed", -1))
    if int(getattr(args, "precision", 32)) != 32:
        raise ValueError("train_scene_net supports precision == 32 only")
    if getattr(args, "test", None) is not None:
        return run_scene_net_test(args, output_root)
    if getattr(args, "resume", None) is None and getattr(args, "pretrain_unet", None) is not None:
        model = use_pretrained_unet(args)
    else:
        model = SceneNetTrainer(args)
    model = model.cuda()
    loop = F.FitLoop(model, args, model.device_loader("train"), model.device_loader("val"),
                     F.TopK(2, "val_ce_loss", getattr(args, "save_epoch", 1)), vis_div=100, interval_cap=0.5, output_root=output_root)
    if getattr(args, "resume", None) is not None:
        loop.resume(args.resume)
    return loop.fit(steps)


if __name__ == "__main__":
    from ..util import arguments
    train_scene_net(arguments.parse_arguments())
