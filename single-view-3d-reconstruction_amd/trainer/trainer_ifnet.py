"""Mirror of the reference's trainer/trainer_ifnet.py training-step contract, without
PyTorch-Lightning (a third-party loop, out of scope): ``ImplicitRefinementTrainer`` keeps
``forward(batch)``, ``training_step(batch, batch_idx) -> {'loss': ...}`` and
``configure_optimizers()`` with the same semantics (trainer/trainer_ifnet.py:28-30,40-47):

    logits = ifnet(batch['input'], batch['points'])
    loss   = BCEWithLogits(logits, batch['occupancies'], reduction='none').sum(-1).mean()
    Adam(ifnet.parameters(), lr=hparams.lr)

so a Lightning ``Trainer`` (or the data-parallel loop in ..dp) can drive it unchanged.  ``validation_step(batch,
batch_idx, output_dir)`` writes the predicted and target meshes as .obj (:49-56).

``train_dataloader`` / ``val_dataloader``: torch DataLoaders with the reference's shuffle / drop_last over the samples of a
``BatchedSampleLoader`` (a ``DeviceSampleLoader``: device tensors, so main-process loaders: num_workers=0, nothing to pin).  ``train_implicit_refinement
(args, steps=None, output_root='runs')`` stands in for ``Trainer.fit`` (:59-66) on the loop of trainer/fit.py: every
``save_epoch``-th epoch's checkpoint is kept; ``python -m svr_amd.trainer.trainer_ifnet`` runs it on util/arguments.py's flags.
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..dataset.implicit_dataset import BatchedSampleLoader, ImplicitDataset
from ..model import ifnet as _ifnet      # _ifnet.DETERMINISTIC is read at call time
from ..model.ifnet import IFNet, implicit_to_mesh
from ..util.visualize import visualize_sdf


class _BCELogitsSumMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        loss, dz = ops.bce_logits_sum_mean(logits.contiguous(), targets.contiguous().float(), want_grad=True,
                                           ordered=_ifnet.DETERMINISTIC)
        ctx.save_for_backward(dz)
        return loss.squeeze(0)

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None


def bce_with_logits_sum_mean(logits, targets):
    """F.binary_cross_entropy_with_logits(reduction='none').sum(-1).mean() on the HIP path."""
    return _BCELogitsSumMeanFn.apply(logits, targets)


class ImplicitRefinementTrainer(nn.Module):
    def __init__(self, kwargs=None, net_res=None):
        super().__init__()
        if kwargs is None:
            kwargs = SimpleNamespace(lr=1e-4, net_res=128)
        self.hparams = kwargs
        self.ifnet = IFNet(net_res=net_res or getattr(kwargs, "net_res", 128))

    def dataset(self, split):
        h = self.hparams
        return ImplicitDataset(split, h.datasetdir, h.num_points, h.splitsdir, splits_root=getattr(h, "splits_root", "data/splits"))

    def device_loader(self, split):
        return BatchedSampleLoader(self.dataset(split))

    def configure_optimizers(self):
        opt_g = torch.optim.Adam(self.ifnet.parameters(), lr=self.hparams.lr)
        return [opt_g], []

    def train_dataloader(self):
        from .fit import DeviceItems
        return torch.utils.data.DataLoader(DeviceItems(self.device_loader("train")), batch_size=self.hparams.batch_size,
                                           shuffle=True, num_workers=0, drop_last=True)

    def val_dataloader(self):
        from .fit import DeviceItems
        return torch.utils.data.DataLoader(DeviceItems(self.device_loader("val")), batch_size=self.hparams.batch_size,
                                           shuffle=False, num_workers=0, drop_last=False)

    def test_dataloader(self):
        from .fit import DeviceItems
        return torch.utils.data.DataLoader(DeviceItems(self.device_loader("test")), batch_size=self.hparams.batch_size,
                                           shuffle=False, num_workers=0, drop_last=False)

    def forward(self, batch):
        return self.ifnet(batch["input"], batch["points"])

    def training_step(self, batch, batch_idx):
        logits = self.forward(batch)
        ce_loss = bce_with_logits_sum_mean(logits, batch["occupancies"])
        return {"loss": ce_loss}

    def validation_step(self, batch, batch_idx, output_dir):
        """trainer_ifnet.py:49-56: for every item, ``<name>_predicted.obj`` (implicit_to_mesh of the network at
        threshold_p = 0.5 on the round((139, 104, 112) / scale_factor) lattice) and ``<name>_gt.obj`` (visualize_sdf of
        the target distance field at level 1) in `output_dir` (the reference's runs/<experiment>/vis/<step // 1000>).
        Unlike the reference, item i is meshed from its own input ``batch['input'][i:i+1]`` and named after its own
        name: the reference passes the whole batch and names every file after item 0, which is only right at batch
        size 1."""
        out = Path(output_dir)
        out.mkdir(exist_ok=True, parents=True)
        dims = np.round(np.array((139, 104, 112), dtype=np.float32) / getattr(self.hparams, "scale_factor", 1)).astype(np.int32)
        x = batch["input"]
        for i in range(len(batch["name"])):
            name = batch["name"][i]
            implicit_to_mesh(self.ifnet, x[i:i + 1], dims, 0.5, out / f"{name}_predicted.obj")
            target = batch["target"][i]
            visualize_sdf(target.reshape(target.shape[-3:]).to(x.device), out / f"{name}_gt.obj", level=1)
        return {"loss": 0}


def train_implicit_refinement(args, steps=None, output_root="runs"):
    """Fit loop (trainer_ifnet.py:59-66).  Reads from `args`, beside the trainer's hyper-parameters and the dataset's
    (datasetdir, splitsdir, num_points, optional splits_root): seed (< 0: none), experiment, batch_size, sanity_steps,
    max_epoch, val_check_interval, val_check_percent, save_epoch, resume, optional log_every (50).  `steps` caps the number
    of optimizer steps.  Validation output goes to <output_root>/<experiment>/vis/<global_step // 1000>, checkpoints to
    <output_root>/<experiment>/epoch=<n>.ckpt and last.ckpt.  Returns {'model', 'checkpoint' (the last one
    written), 'best_val_loss' (None: nothing is monitored), 'global_step', 'history', 'optimizer', 'driver',
    'last_checkpoint'}."""
    from . import fit as F
    F.init_distributed(getattr(args, "gpu", None))
    F.seed_everything(getattr(args, "seed", -1))
    model = ImplicitRefinementTrainer(args).cuda()
    loop = F.FitLoop(model, args, model.device_loader("train"), model.device_loader("val"),
                     F.EveryEpoch(getattr(args, "save_epoch", 1)), vis_div=1000, interval_cap=1.0, output_root=output_root)
    if getattr(args, "resume", None) is not None:
        loop.resume(args.resume)
    return loop.fit(steps)


if __name__ == "__main__":
    from ..util import arguments
    train_implicit_refinement(arguments.parse_arguments())
