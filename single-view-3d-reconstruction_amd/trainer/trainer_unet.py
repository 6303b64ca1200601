"""Mirror of the reference's trainer/trainer_unet.py:19-89 -- stage one of its recipe, the depth regressor trained alone on
rgb.png / distance.exr -- without Lightning, in the style of trainer_ifnet.py:

    raw   = unet(batch['input'])                                   Unet (resize_input) or UNetMini
    depth = sigmoid(interpolate(raw, 320, bilinear)[:, :, 40:280, :]) * (max_z - min_z) + min_z      (no resize: raw itself)
    loss  = mse_loss(depth, batch['target'])
    Adam(unet.parameters(), lr)

The head behind the UNet is ops.depth_head (depth_head.hip): at most three launches for forward and backward together.
State-dict keys are `unet.*`, as in the reference's checkpoints, so trainer_scene_net.use_pretrained_unet (and the
reference's) load what ``train_unet`` saves.

``train_dataloader`` / ``val_dataloader``: torch DataLoaders over ..dataset.ScenesDataset with the reference's shuffle /
drop_last.  The items are DEVICE tensors (the dataset converts distance to depth on the GPU), so the loaders run in the
main process -- num_workers=0 -- and there is no pin_memory: there is nothing left on the host to pin.

``train_unet(args, steps=None, output_root='runs')`` stands in for ``Trainer.fit``: epochs over the train loader, a validation
pass every ``val_check_interval`` of an epoch over ``val_check_percent`` of the val loader (module in eval mode, as Lightning
switches it), and the checkpoint with the best val_loss under <output_root>/<experiment>/checkpoints/best.ckpt (Lightning's
ModelCheckpoint(save_top_k=1, monitor='val_loss')).  No tensorboard."""
from pathlib import Path
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import ops
from ..data_processing import sample_io
from ..dataset.scenes_dataset import ScenesDataset
from ..model.unet import UNetMini, Unet
from .checkpoint import save_checkpoint


def default_hparams(**kw):
    """The defaults of the reference's util/arguments.py that this trainer reads."""
    h = dict(lr=1e-4, resize_input=True, min_z=0.1953997164964676, max_z=7.0, W=256, batch_size=16, num_workers=0,
             datasetdir="data", splitsdir="overfit")
    h.update(kw)
    return SimpleNamespace(**h)


class DepthRegressorTrainer(nn.Module):
    def __init__(self, kwargs=None):
        super().__init__()
        self.hparams = kwargs if kwargs is not None else default_hparams()
        if self.hparams.resize_input:
            self.unet = Unet(channels_in=3, channels_out=1)
        else:
            self.unet = UNetMini(channels_in=3, channels_out=1)
        self.last_log = {}

    def dataset(self, split):
        h = self.hparams
        return ScenesDataset(split, h.datasetdir, h.splitsdir, h, splits_root=getattr(h, "splits_root", "data/splits"),
                             intrinsics_path=getattr(h, "intrinsics_path", None))

    def configure_optimizers(self):
        opt_g = torch.optim.Adam(self.unet.parameters(), lr=self.hparams.lr)
        return [opt_g], []

    def train_dataloader(self):
        return torch.utils.data.DataLoader(self.dataset("train"), batch_size=self.hparams.batch_size, shuffle=True, num_workers=0,
                                           drop_last=True)

    def val_dataloader(self):
        return torch.utils.data.DataLoader(self.dataset("val"), batch_size=self.hparams.batch_size, shuffle=False, num_workers=0,
                                           drop_last=False)

    def _head(self, raw, target):
        h = self.hparams
        # resize back to 320 and drop the rows of the square padding if the input was resized (:47-51)
        size, rows = (320, (40, 280)) if h.resize_input else (0, (0, 0))
        return ops.depth_head(raw, target, size=size, rows=rows, min_z=h.min_z, max_z=h.max_z)

    def forward(self, batch):
        """The renormalised depth map (B, 1, 240, 320).  It is an output of ops.depth_head, which is not differentiable
        through `depth`; the training step differentiates the loss."""
        depth, _ = self._head(self.unet(batch["input"]), None)
        return depth

    def training_step(self, batch, batch_idx):
        _, mse_loss = self._head(self.unet(batch["input"]), batch["target"])
        self.last_log = {"train_loss": mse_loss.detach()}
        return {"loss": mse_loss}

    def validation_step(self, batch, batch_idx, output_dir):
        """trainer_unet.py:65-78: every item's prediction as <output_dir>/<name>/depth_map.exr (one FLOAT channel 'Z': what
        pyexr.write makes of a 2-D array; the reference's directory is runs/<experiment>/vis/<global_step // 1000>), and the
        loss as val_loss.  The module's train / eval mode is the caller's."""
        with torch.no_grad():
            prediction, mse_loss = self._head(self.unet(batch["input"]), batch["target"])
            maps = prediction.cpu().numpy()
            for i in range(len(batch["name"])):
                out = Path(output_dir) / batch["name"][i]
                out.mkdir(exist_ok=True, parents=True)
                sample_io.exr_write(out / "depth_map.exr", {"Z": maps[i].reshape(maps.shape[-2:])})
        self.last_log = {"val_loss": mse_loss.detach()}
        return {"loss": mse_loss}


def _validate(model, loader, n_batches, output_dir):
    was_training = model.training
    model.eval()
    total, count = 0.0, 0
    for i, batch in enumerate(loader):
        if i >= n_batches:
            break
        total += float(model.validation_step(batch, i, output_dir)["loss"])
        count += 1
    model.train(was_training)
    return total / max(count, 1)


def train_unet(args, steps=None, output_root="runs"):
    """Fit loop (trainer_unet.py:81-89).  Reads from `args`, beside the trainer's hyper-parameters: seed (-1: none),
    experiment ('scenes_net'), max_epoch (100), val_check_interval (0.25 of an epoch), val_check_percent (0.5 of the val
    batches, at least one).  `steps` caps the number of optimizer steps; a capped run validates once more at its end if
    its last step was not followed by a validation.  Returns {'model', 'checkpoint' (path of the best one or None),
    'best_val_loss', 'global_step'}."""
    if getattr(args, "seed", -1) is not None and getattr(args, "seed", -1) >= 0:
        torch.manual_seed(args.seed)
    model = DepthRegressorTrainer(args).cuda().train()
    opt = model.configure_optimizers()[0][0]
    train_loader, val_loader = model.train_dataloader(), model.val_dataloader()
    run = Path(output_root) / getattr(args, "experiment", "scenes_net")
    every = max(1, int(len(train_loader) * min(float(getattr(args, "val_check_interval", 0.25)), 1.0)))
    n_val = max(1, int(len(val_loader) * float(getattr(args, "val_check_percent", 0.5))))
    state = {"model": model, "checkpoint": None, "best_val_loss": float("inf"), "global_step": 0}

    def validate(epoch):
        step = state["global_step"]
        val_loss = _validate(model, val_loader, n_val, run / "vis" / f"{step // 1000:05d}")
        if val_loss < state["best_val_loss"]:
            state["best_val_loss"] = val_loss
            state["checkpoint"] = save_checkpoint(model, run / "checkpoints" / "best.ckpt", epoch=epoch, global_step=step,
                                                  val_loss=val_loss)

    validated = True
    for epoch in range(int(getattr(args, "max_epoch", 100))):
        for batch_idx, batch in enumerate(train_loader):
            opt.zero_grad(set_to_none=True)
            model.training_step(batch, batch_idx)["loss"].backward()
            opt.step()
            state["global_step"] += 1
            validated = (batch_idx + 1) % every == 0
            if validated:
                validate(epoch)
            if steps is not None and state["global_step"] >= steps:
                break
        if steps is not None and state["global_step"] >= steps:
            break
    if not validated:
        validate(epoch)
    return state
