"""The fit loop behind ``train_implicit_refinement`` and ``train_scene_net``: what the reference hands to Lightning's
``Trainer(...).fit`` / ``.test`` (trainer_ifnet.py:59-66, trainer_scene_net.py:215-242), written for this package's step.

  * The step is driven through ``dp.DataParallelTrainer``: at most two steps in flight, and under ``torch.distributed.run``
    one gradient all-reduce per step.  Rank r takes batches r, r + world, ... of the epoch's order (``shard_batches``);
    only rank 0 validates and writes files.
  * Batches come from a device loader (``BatchedSampleLoader`` / ``DeviceSceneLoader``): ``loader.batch(indices)``.
  * No value is read on the host per step.  The step's logged scalars are summed on the device (``DeviceMeans``: one stack
    and one add per step) and read once per validation pass or every ``log_every`` steps into the returned history
    ``{name: [(global_step, mean), ...]}``, which is printed as it grows.  No tensorboard.
  * ``gc.collect(); gc.freeze()`` once after the first steps (the collector's full passes over the
    framework's long-lived objects are 75-200 ms pauses); unfrozen again when the loop returns.
  * Checkpoints keep trainer/checkpoint.py's Lightning-compatible layout and add ``optimizer_states`` (a list holding
    ``opt.state_dict()``), ``epoch``, ``global_step`` and ``checkpoint_callback`` (the policy's bookkeeping).  ``resume``
    restores all of them; training restarts at the beginning of the epoch the checkpoint was written in.

The two policies are the reference's ModelCheckpoint settings: ``EveryEpoch`` (save_top_k=-1, period=save_epoch) and ``TopK``
(save_top_k=2, save_last, monitor='val_ce_loss').  Both also write ``last.ckpt``, the file ``--resume`` is usually given."""
import gc
import os
import shutil
import tempfile
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from .. import dp
from .checkpoint import TopKCheckpoints, load_checkpoint, save_checkpoint

FREEZE_AFTER_STEPS = 3


def seed_everything(seed):
    """torch and numpy (the loaders draw their point subsets from numpy's global state) when seed >= 0."""
    if seed is not None and int(seed) >= 0:
        torch.manual_seed(int(seed))
        np.random.seed(int(seed))


def epoch_batches(n_items, batch_size, shuffle, drop_last):
    """The index lists of one epoch: what a DataLoader's sampler + batch sampler produce."""
    order = torch.randperm(n_items).tolist() if shuffle else list(range(n_items))
    batches = [order[i:i + batch_size] for i in range(0, n_items, batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    return batches


def shard_batches(n_batches, rank=0, world=1, pad=False):
    """The batches of an epoch that rank `rank` of `world` takes: rank, rank + world, ...  Together the ranks cover every
    batch exactly once.  ``pad=True`` (the training loop: every rank must join every all-reduce) extends a shard that came
    out one short by wrapping around to its own first batch, so that all ranks take ceil(n_batches / world) steps."""
    own = list(range(rank, n_batches, world))
    if pad and n_batches > 0:
        per_rank = -(-n_batches // world)
        fill = own if own else [rank % n_batches]
        own = own + [fill[i % len(fill)] for i in range(per_rank - len(own))]
    return own


class DeviceMeans:
    """Running sums of named device scalars; ``read()`` is the one host read: {name: mean} and a reset."""

    def __init__(self):
        self.keys, self.sums, self.count = None, None, 0

    def add(self, logs):
        if not logs:
            return
        if self.keys is None:
            self.keys = list(logs)
        values = torch.stack([logs[k].detach().reshape(()).float() for k in self.keys])
        self.sums = values if self.sums is None else self.sums.add_(values)
        self.count += 1

    def read(self):
        if self.count == 0:
            return {}
        means = dict(zip(self.keys, (self.sums / self.count).tolist()))
        self.keys, self.sums, self.count = None, None, 0
        return means


class EveryEpoch:
    """ModelCheckpoint(save_top_k=-1, period=save_epoch): every save_epoch-th epoch's checkpoint is kept."""
    monitor = None

    def __init__(self, save_epoch=1):
        self.save_epoch = max(1, int(save_epoch))

    def validated(self, loop, epoch, means):
        pass

    def epoch_end(self, loop, epoch):
        if (epoch + 1) % self.save_epoch == 0:
            loop.save(f"epoch={epoch}.ckpt", epoch)

    def finish(self, loop, epoch):
        """A run that stops inside an epoch (`steps`) leaves that epoch's checkpoint as well."""
        if loop.saved_at != loop.global_step:
            loop.save(f"epoch={epoch}.ckpt", epoch)

    def state(self):
        return {}

    def load_state(self, state):
        pass


class TopK:
    """ModelCheckpoint(save_top_k=k, save_last=True, monitor=..., period=save_epoch): after a validation pass of every
    save_epoch-th epoch the checkpoint is kept if its monitored mean is among the best k (the one it pushes out is deleted),
    and ``last.ckpt`` is rewritten either way."""

    def __init__(self, k=2, monitor="val_ce_loss", save_epoch=1):
        self.keeper = TopKCheckpoints(k, monitor)
        self.monitor = monitor
        self.save_epoch = max(1, int(save_epoch))

    def validated(self, loop, epoch, means):
        if (epoch + 1) % self.save_epoch != 0 or self.monitor not in means:
            return
        name = f"epoch={epoch}-step={loop.global_step}.ckpt"
        kept = self.keeper.offer(means[self.monitor], loop.run / name)
        loop.save(name if kept else None, epoch, **{self.monitor: means[self.monitor]})

    def epoch_end(self, loop, epoch):
        pass

    def finish(self, loop, epoch):
        pass

    def state(self):
        return self.keeper.state()

    def load_state(self, state):
        self.keeper.load_state(state)


class FitLoop:
    def __init__(self, model, args, train_loader, val_loader, policy, vis_div, interval_cap=1.0, output_root="runs"):
        self.model, self.args, self.policy = model, args, policy
        self.train_loader, self.val_loader = train_loader, val_loader
        self.vis_div, self.interval_cap = int(vis_div), float(interval_cap)
        self.run = Path(output_root) / getattr(args, "experiment", "scenes_net")
        self.rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.driver = dp.DataParallelTrainer(model)
        self.optimizer = self.driver.optimizer
        self.global_step, self.start_epoch = 0, 0
        self.history, self.checkpoint, self.saved_at = {}, None, -1
        self.train_means = DeviceMeans()

    # -- checkpoints -------------------------------------------------------------------------------------------------
    def save(self, name, epoch, **extra):
        """<run>/<name> (None: only last.ckpt) and <run>/last.ckpt, with everything ``resume`` restores.  The files sit in
        the experiment's folder itself, where the reference's ModelCheckpoint(filepath=runs/<experiment>/checkpoints) puts
        them: ``--resume`` names the experiment after the checkpoint's parent folder (util/arguments.py)."""
        if self.rank != 0:
            return
        folder = self.run
        last = save_checkpoint(self.model, folder / "last.ckpt", epoch=epoch, global_step=self.global_step,
                               optimizer_states=[self.optimizer.state_dict()], checkpoint_callback=self.policy.state(), **extra)
        self.checkpoint = last
        if name is not None:
            shutil.copyfile(last, folder / name)
            self.checkpoint = str(folder / name)
        self.saved_at = self.global_step

    def resume(self, path):
        ck = load_checkpoint(path)
        self.model.load_state_dict(ck["state_dict"])
        self.optimizer.load_state_dict(ck["optimizer_states"][0])
        self.start_epoch, self.global_step = int(ck["epoch"]), int(ck["global_step"])
        self.policy.load_state(ck.get("checkpoint_callback", {}))
        self.saved_at = self.global_step
        return ck

    # -- validation --------------------------------------------------------------------------------------------------
    def _record(self, means):
        for k, v in means.items():
            self.history.setdefault(k, []).append((self.global_step, v))
        if means and self.rank == 0:
            print(f"step {self.global_step}: " + " ".join(f"{k}={v:.6g}" for k, v in means.items()), flush=True)

    def _val_batches(self):
        batches = epoch_batches(len(self.val_loader.ds), int(self.args.batch_size), shuffle=False, drop_last=False)
        return batches, max(1, int(len(batches) * float(getattr(self.args, "val_check_percent", 0.5))))

    def validate(self, n_batches, output_dir):
        """`n_batches` validation batches with the module in eval mode; the val_* scalars' means, read once."""
        model = self.model
        was_training = model.training
        model.eval()
        means = DeviceMeans()
        batches, _ = self._val_batches()
        for i, indices in enumerate(batches[:n_batches]):
            model.last_log = {}
            model.validation_step(self.val_loader.batch(indices), i, output_dir)
            means.add({k: v for k, v in model.last_log.items() if k.startswith("val_")})
        model.train(was_training)
        return means.read()

    def sanity(self):
        """Lightning's num_sanity_val_steps: the validation path is exercised before the first step.  Nothing is kept --
        what the steps write goes to a directory that is removed, no checkpoint, no history."""
        n = int(getattr(self.args, "sanity_steps", 2))
        if n > 0 and self.rank == 0:
            with tempfile.TemporaryDirectory() as scratch:
                self.validate(n, scratch)

    def _validate_and_record(self, epoch):
        self._record(self.train_means.read())
        if self.rank != 0:
            return
        _, n_val = self._val_batches()
        means = self.validate(n_val, self.run / "vis" / f"{self.global_step // self.vis_div:05d}")
        self._record(means)
        self.policy.validated(self, epoch, means)

    # -- training ----------------------------------------------------------------------------------------------------
    def _epoch_order(self):
        a = self.args
        batches = epoch_batches(len(self.train_loader.ds), int(a.batch_size), shuffle=True, drop_last=True)
        if self.world > 1:                               # one order for all ranks: rank 0's
            flat = torch.tensor(batches, dtype=torch.int64, device="cuda")
            dist.broadcast(flat, src=0)
            batches = flat.cpu().tolist()
        return [batches[i] for i in shard_batches(len(batches), self.rank, self.world, pad=True)]

    def fit(self, steps=None):
        a, model = self.args, self.model
        interval = getattr(a, "val_check_interval", 0.25)
        every_n_epochs = max(1, int(interval))           # check_val_every_n_epoch=max(1, val_check_interval)
        log_every = int(getattr(a, "log_every", 50))

        def done():
            return steps is not None and self.global_step >= steps

        taken, frozen, epoch, validated = 0, False, self.start_epoch, True
        model.train()
        try:
            if not done():
                self.sanity()
            for epoch in range(self.start_epoch, int(getattr(a, "max_epoch", 100))):
                if done():
                    break
                batches = self._epoch_order()
                every = max(1, int(len(batches) * min(float(interval), self.interval_cap)))
                for batch_idx, indices in enumerate(batches):
                    out = self.driver.step(self.train_loader.batch(indices), batch_idx)
                    logs = getattr(model, "last_log", None) or {"train_loss": out["loss"]}
                    self.train_means.add({k: v for k, v in logs.items() if not k.startswith("val_")})
                    self.global_step += 1
                    taken += 1
                    if taken == FREEZE_AFTER_STEPS and not frozen:
                        gc.collect()
                        gc.freeze()
                        frozen = True
                    validated = (batch_idx + 1) % every == 0 and (epoch + 1) % every_n_epochs == 0
                    if validated:
                        self._validate_and_record(epoch)
                    elif self.global_step % log_every == 0:
                        self._record(self.train_means.read())
                    if done():
                        break
                if done():
                    break
                self.policy.epoch_end(self, epoch)
            if taken and not validated:                  # a capped run validates once more at its end, as train_unet
                self._validate_and_record(epoch)
            if taken:
                self.policy.finish(self, epoch)
            self._record(self.train_means.read())
        finally:
            if frozen:
                gc.unfreeze()
        return self.result()

    def result(self):
        best = self.policy.keeper.best_value if isinstance(self.policy, TopK) else None
        if isinstance(self.policy, TopK) and self.policy.keeper.best_path is not None:
            self.checkpoint = self.policy.keeper.best_path
        return {"model": self.model, "checkpoint": self.checkpoint, "best_val_loss": best, "global_step": self.global_step,
                "history": self.history, "optimizer": self.optimizer, "driver": self.driver,
                "last_checkpoint": str(self.run / "last.ckpt") if self.saved_at >= 0 and self.rank == 0 else None}


class DeviceItems(torch.utils.data.Dataset):
    """A DeviceSampleLoader's samples as a map-style dataset, for a main-process DataLoader: item i is ``loader.get(i)``."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader.ds)

    def __getitem__(self, idx):
        return self.loader.get(idx)


def init_distributed(gpu=None):
    """Under ``torch.distributed.run`` (WORLD_SIZE > 1 in the environment): join the process group on this rank's GPU.
    Otherwise ``--gpu`` (an index, or a list whose first entry counts) selects the device, as the reference's
    ``Trainer(gpus=[args.gpu])``."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and dist.is_available():
        if not dist.is_initialized():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group("nccl")
    elif gpu is not None:
        torch.cuda.set_device(int(gpu[0] if isinstance(gpu, (list, tuple)) else gpu))
