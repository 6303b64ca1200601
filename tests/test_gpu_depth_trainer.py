"""GPU: DepthRegressorTrainer (UNet depth pre-training) -- one training step against the CPU oracle (oracle/scene_oracle.py's
UNet + tests/depth_head_oracle.py's head, stock torch ops), the validation step's files, and the two-stage recipe:
train_unet -> checkpoint -> use_pretrained_unet."""
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import scene_oracle as S
from tests import depth_head_oracle as DO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _trainer(resize, **kw):
    import svr_amd  # noqa: F401
    from svr_amd.trainer import DepthRegressorTrainer
    from svr_amd.trainer import trainer_unet as TU
    tr = DepthRegressorTrainer(TU.default_hparams(resize_input=resize, **kw))
    st = S.name_seeded_like(tr.unet.state_dict(), 1.0, "unet.")
    tr.unet.load_state_dict(st, strict=False)
    return tr.cuda().train(), st


def _batch(B, H, W, seed=41):
    g = torch.Generator().manual_seed(seed)
    return {"name": [f"scene{i}/view" for i in range(B)], "input": torch.rand(B, 3, H, W, generator=g) * 2 - 1,
            "target": 5 * torch.rand(B, 1, 240, 320, generator=g) + 0.5 if (H, W) == (256, 256)
            else 5 * torch.rand(B, 1, H, W, generator=g) + 0.5}


def _cuda(batch):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


@pytest.mark.parametrize("variant,B,H,W", [("full", 2, 256, 256), ("mini", 2, 48, 64)])
def test_training_step_matches_the_oracle(variant, B, H, W):
    """Loss within 2e-5 (the gate tests/test_gpu_unet.py holds the UNet output to), every parameter gradient by that file's
    criteria, every parameter after one Adam step of lr 1e-4 within 2.1e-4 of the oracle's (at most one sign flip)."""
    resize = variant == "full"
    tr, st = _trainer(resize)
    batch = _batch(B, H, W)
    (opt,), _ = tr.configure_optimizers()
    opt.zero_grad(set_to_none=True)
    loss = tr.training_step(_cuda(batch), 0)["loss"]
    loss.backward()
    assert torch.equal(tr.last_log["train_loss"], loss.detach())

    ref_st = {k: v.clone().requires_grad_(not k.endswith(("running_mean", "running_var"))) for k, v in st.items()}
    raw = S.unet_forward(ref_st, batch["input"], variant, True)
    depth = DO.head(raw, 320 if resize else 0, (40, 280))
    ref_loss = F.mse_loss(depth, batch["target"], reduction="mean")
    ref_loss.backward()
    e = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    print(variant, "loss", loss.item(), "oracle", ref_loss.item(), "rel", e)
    assert e < 2e-5
    with torch.no_grad():
        fwd = tr(_cuda(batch))
    assert tuple(fwd.shape) == ((B, 1, 240, 320) if resize else (B, 1, H, W))

    top = max(v.grad.norm().item() for v in ref_st.values() if v.grad is not None)
    for name, p in tr.unet.named_parameters():
        r = ref_st[name].grad.double()
        q = p.grad.detach().cpu().double()
        if r.norm().item() < 1e-3 * top:          # conv bias directly in front of BatchNorm: true gradient 0
            assert q.norm().item() < 2e-3 * top, name
            continue
        n = abs(q.norm().item() - r.norm().item()) / r.norm().item()
        med = float((q - r).abs().median() / r.abs().max())
        assert n < 5e-3 and med < 2e-3, (name, n, med)

    ref_params = [v for v in ref_st.values() if v.requires_grad]
    torch.optim.Adam(ref_params, lr=1e-4).step()
    opt.step()
    for name, p in tr.unet.named_parameters():
        assert float((p.detach().cpu() - ref_st[name].detach()).abs().max()) <= 2.1e-4, name


def test_validation_step_writes_the_prediction_and_leaves_no_gradient(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    tr, _ = _trainer(False)
    tr.eval()                                                  # the caller's choice; the step must not change it
    batch = _cuda(_batch(2, 48, 64))
    out = tr.validation_step(batch, 0, tmp_path / "vis")
    assert set(out) == {"loss"} and torch.equal(tr.last_log["val_loss"], out["loss"]) and not out["loss"].requires_grad
    with torch.no_grad():
        pred = tr(batch)
    assert not tr.training
    assert abs(out["loss"].item() - F.mse_loss(pred, batch["target"]).item()) < 1e-5 * out["loss"].item()
    for i, name in enumerate(batch["name"]):
        assert "/" in name
        path = tmp_path / "vis" / name / "depth_map.exr"
        assert path.exists()
        info = sample_io.exr_info(path)
        assert info["channels"] == [("Z", "FLOAT")] and (info["height"], info["width"]) == (48, 64)
        z = sample_io.exr_read(path, "Z")
        assert np.array_equal(z.view(np.int32), pred[i, 0].cpu().numpy().view(np.int32))
    assert all(p.grad is None for p in tr.parameters())


def test_train_unet_then_use_pretrained_unet(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.trainer import SceneNetTrainer, load_checkpoint, train_unet, use_pretrained_unet
    from svr_amd.trainer import default_hparams as scene_hparams
    from svr_amd.trainer import trainer_unet as TU
    names = ["00000", "00001"]
    rng = np.random.default_rng(2)
    for name in names:
        d = tmp_path / "data" / "raw" / "tiny" / name
        d.mkdir(parents=True)
        Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(d / "rgb.png")
        shutil.copyfile(os.path.join(GOLD, "raw_distance.exr"), d / "distance.exr")
    (tmp_path / "splits" / "tiny").mkdir(parents=True)
    for split in ("train", "val"):
        (tmp_path / "splits" / "tiny" / f"{split}.txt").write_text("\n".join(names) + "\n")
    args = TU.default_hparams(resize_input=False, batch_size=2, datasetdir=str(tmp_path / "data"), splitsdir="tiny",
                              splits_root=str(tmp_path / "splits"), experiment="pre", seed=3, max_epoch=10,
                              val_check_interval=1.0, val_check_percent=1.0)
    res = train_unet(args, steps=3, output_root=tmp_path / "runs")
    assert res["global_step"] == 3 and np.isfinite(res["best_val_loss"])
    ckpt = tmp_path / "runs" / "pre" / "checkpoints" / "best.ckpt"
    assert ckpt.exists() and str(ckpt) == str(res["checkpoint"])
    assert (tmp_path / "runs" / "pre" / "vis" / "00000" / "00001" / "depth_map.exr").exists()
    ck = load_checkpoint(ckpt)
    assert ck["hyper_parameters"]["splitsdir"] == "tiny" and ck["val_loss"] == res["best_val_loss"]
    assert all(k.startswith("unet.") for k in ck["state_dict"])

    sargs = scene_hparams(resize_input=False, net_res=32, pretrain_unet=str(ckpt))
    torch.manual_seed(17)
    fresh = {k: v.clone() for k, v in SceneNetTrainer(sargs).state_dict().items()}
    torch.manual_seed(17)
    scene = use_pretrained_unet(sargs)
    changed = 0
    for k, v in scene.state_dict().items():
        if k.startswith("unet."):
            assert torch.equal(v, ck["state_dict"][k]), k
            changed += not torch.equal(v, fresh[k])
        else:
            assert k.startswith(("ifnet.", "project.")) and torch.equal(v, fresh[k]), k
    assert changed > 0
