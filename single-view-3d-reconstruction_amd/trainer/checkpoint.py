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
