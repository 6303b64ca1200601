"""Checkpoints in the layout PyTorch-Lightning writes and the reference reads (``torch.load(path)['state_dict']``,
trainer/trainer_scene_net.py:204-212): ``{'state_dict': ..., 'hyper_parameters': ..., **extra}``, tensors on the CPU."""
import argparse
import os
import types

import torch


def _to_cpu(v):
    if torch.is_tensor(v):
        return v.detach().cpu()
    if isinstance(v, dict):
        return type(v)((k, _to_cpu(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)):
        return type(v)(_to_cpu(x) for x in v)
    return v


def save_checkpoint(module, path, **extra):
    """`module`: an nn.Module with `hparams` (a Namespace; absent = no hyper-parameters).  `extra`: further top-level entries
    (epoch, global_step, val_loss, ...)."""
    hparams = getattr(module, "hparams", None)
    ckpt = {"state_dict": _to_cpu(module.state_dict()),
            "hyper_parameters": _to_cpu(dict(vars(hparams))) if hparams is not None else {}}
    ckpt.update(_to_cpu(extra))
    path = os.fspath(path)
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(ckpt, path)
    return path


def load_checkpoint(path):
    """The checkpoint dict, on the CPU, through the restricted unpickler (weights_only); namespaces among the entries pass."""
    with torch.serialization.safe_globals([argparse.Namespace, types.SimpleNamespace]):
        return torch.load(os.fspath(path), map_location="cpu", weights_only=True)


class TopKCheckpoints:
    """The bookkeeping of Lightning's ModelCheckpoint(save_top_k=k, monitor=..., mode='min'): which checkpoint files are the
    best `k` so far.  ``offer(value, path)`` answers whether a checkpoint with this monitor value belongs among them; if so
    it is entered under `path` (the caller writes the file afterwards) and the entry it pushes out is returned to the caller
    as deleted: its file is removed here.  A value that is not finite never enters.  ``state()`` / ``load_state()`` carry the
    list through a checkpoint (plain lists, floats and strings: the restricted unpickler reads them)."""

    def __init__(self, k=2, monitor="val_ce_loss"):
        self.k, self.monitor = int(k), monitor
        self.best = []                                    # [(value, path)], best first

    def offer(self, value, path):
        value, path = float(value), os.fspath(path)
        if self.k == 0 or value != value or value in (float("inf"), float("-inf")):
            return False
        if len(self.best) >= self.k and value >= self.best[-1][0]:
            return False
        self.best = sorted([e for e in self.best if e[1] != path] + [(value, path)], key=lambda e: e[0])
        for _, evicted in self.best[self.k:]:
            if os.path.exists(evicted):
                os.remove(evicted)
        self.best = self.best[:self.k]
        return True

    @property
    def best_path(self):
        return self.best[0][1] if self.best else None

    @property
    def best_value(self):
        return self.best[0][0] if self.best else float("inf")

    def state(self):
        return {"monitor": self.monitor, "k": self.k, "best_k": [[v, p] for v, p in self.best]}

    def load_state(self, state):
        self.best = [(float(v), str(p)) for v, p in state.get("best_k", [])]
