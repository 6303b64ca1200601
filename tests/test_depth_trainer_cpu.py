"""CPU: the host side of UNet depth pre-training -- imports, state-dict names, checkpoints, --pretrain_unet, the dataset's
listing and mirroring.  No kernel runs here."""
import argparse
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image


def test_modules_import_and_state_dict_names_are_the_references():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    from svr_amd.dataset import ScenesDataset  # noqa: F401
    from svr_amd.model import UNetMini, Unet
    from svr_amd.trainer import DepthRegressorTrainer, load_checkpoint, save_checkpoint, train_unet, use_pretrained_unet  # noqa: F401
    from svr_amd.trainer import trainer_unet as TU
    assert callable(ops.depth_head)
    h = TU.default_hparams()
    assert (h.lr, h.resize_input, h.min_z, h.max_z, h.W, h.batch_size, h.num_workers, h.datasetdir, h.splitsdir) == \
           (1e-4, True, 0.1953997164964676, 7.0, 256, 16, 0, "data", "overfit")
    t = DepthRegressorTrainer()
    assert list(t.state_dict()) == ["unet." + k for k in Unet(channels_in=3, channels_out=1).state_dict()]
    mini = DepthRegressorTrainer(TU.default_hparams(resize_input=False))
    assert list(mini.state_dict()) == ["unet." + k for k in UNetMini(channels_in=3, channels_out=1).state_dict()]
    (opt,), _ = t.configure_optimizers()
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == 1e-4
    assert sum(p.numel() for g in opt.param_groups for p in g["params"]) == sum(p.numel() for p in t.unet.parameters())


def test_depth_head_refuses_cpu_tensors():
    import pytest
    import svr_amd  # noqa: F401
    from svr_amd import ops
    with pytest.raises(RuntimeError):
        ops.depth_head(torch.zeros(1, 1, 4, 4), None, size=0)


def test_checkpoint_round_trip(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.trainer import DepthRegressorTrainer, load_checkpoint, save_checkpoint
    from svr_amd.trainer import trainer_unet as TU
    for hp in (TU.default_hparams(resize_input=False, lr=3e-4), argparse.Namespace(resize_input=False, lr=3e-4, sigma=[1.5])):
        t = DepthRegressorTrainer(hp)
        path = save_checkpoint(t, tmp_path / "runs" / "x" / "checkpoints" / "best.ckpt", epoch=2, global_step=40, val_loss=0.5,
                               args=hp)
        ck = load_checkpoint(path)
        assert set(ck) == {"state_dict", "hyper_parameters", "epoch", "global_step", "val_loss", "args"}
        assert ck["hyper_parameters"] == vars(hp) and (ck["epoch"], ck["global_step"], ck["val_loss"]) == (2, 40, 0.5)
        assert type(ck["args"]) is type(hp) and vars(ck["args"]) == vars(hp)
        st = t.state_dict()
        assert list(ck["state_dict"]) == list(st)
        for k, v in ck["state_dict"].items():
            assert v.device.type == "cpu" and v.dtype == st[k].dtype and torch.equal(v, st[k]), k
    assert torch.load(path, weights_only=False)["state_dict"].keys() == st.keys()       # the reference's plain torch.load


def test_use_pretrained_unet_changes_only_the_unet(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.trainer import SceneNetTrainer, default_hparams, use_pretrained_unet
    args = default_hparams(resize_input=False, net_res=32, miopen_benchmark=False)
    torch.manual_seed(5)
    donor = SceneNetTrainer(args)
    ck = {"state_dict": {k: (v + 1 if v.is_floating_point() else v + 7) for k, v in donor.state_dict().items()}}
    assert any(k.startswith("ifnet.") for k in ck["state_dict"]) and any(k.startswith("project.") for k in ck["state_dict"])
    torch.save(ck, tmp_path / "pre.ckpt")
    torch.manual_seed(9)
    fresh = SceneNetTrainer(args).state_dict()
    torch.manual_seed(9)
    args.pretrain_unet = str(tmp_path / "pre.ckpt")
    got = use_pretrained_unet(args)
    assert isinstance(got, SceneNetTrainer)
    torch.manual_seed(9)
    st = use_pretrained_unet(args, path=tmp_path / "pre.ckpt").state_dict()
    n_unet = 0
    for k, v in got.state_dict().items():
        assert torch.equal(v, st[k]), k
        if "unet" in k:
            n_unet += 1
            assert torch.equal(v, ck["state_dict"][k]), k
        else:
            assert torch.equal(v, fresh[k]) and not torch.equal(v, ck["state_dict"][k]), k
    assert n_unet == sum(1 for k in fresh if k.startswith("unet.")) > 0


def test_dataset_listing_and_mirroring(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.dataset import scenes_dataset as SD
    from svr_amd.dataset.scene_net_data import rgb_transform
    for sd in ("overfit", "my_overfit"):
        (tmp_path / "splits" / sd).mkdir(parents=True)
        for split in ("train", "val"):
            (tmp_path / "splits" / sd / f"{split}.txt").write_text("a/b\n\n  c \n")
    assert SD.list_items("train", "overfit", tmp_path / "splits") == ["a/b", "c"] * 500
    assert SD.list_items("val", "overfit", tmp_path / "splits") == ["a/b", "c"]
    assert SD.list_items("train", "my_overfit", tmp_path / "splits") == ["a/b", "c"]
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    mirrored = Image.fromarray(np.ascontiguousarray(rgb[:, ::-1]))
    for resize, shape in ((True, (3, 128, 128)), (False, (3, 240, 320))):
        x = SD.load_input(tmp_path / "rgb.png", 128, resize)
        assert tuple(x.shape) == shape and torch.equal(x, rgb_transform(mirrored, 128, resize))
    x = SD.load_input(tmp_path / "rgb.png", 128, False)
    assert torch.equal(x, torch.flip(rgb_transform(Image.fromarray(rgb), 128, False), dims=(2,)))
