"""GPU: dataset/scenes_dataset.py (the items of UNet depth pre-training) on a tree under tmp_path: a seeded, left-right
asymmetric rgb.png, the golden distance.exr, a splits file."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
FOCAL = F32(277.1281435)
NAMES = ["00000", "scene7/view3"]


def np_depth(d, f):
    """depth = sqrt(d*d / ((r*r + c*c) / (f*f) + 1)), r = row - H//2, c = col - W//2: float32, every operation rounded on its
    own, in the order include/svr_hip.h states."""
    H, W = d.shape
    rc = ((np.arange(H)[:, None] - H // 2) ** 2 + (np.arange(W)[None, :] - W // 2) ** 2).astype(F32)
    return np.sqrt(d * d / (rc / (F32(f) * F32(f)) + F32(1)))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("scenes")
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    rgb[:, :160, 0] //= 4                                         # left half darker in red: mirroring it is visible
    for name in NAMES:
        d = root / "data" / "raw" / "overfit" / name
        d.mkdir(parents=True)
        Image.fromarray(rgb).save(d / "rgb.png")
        shutil.copyfile(os.path.join(GOLD, "raw_distance.exr"), d / "distance.exr")
    for sd in ("overfit", "overfit_small"):
        s = root / "splits" / sd
        s.mkdir(parents=True)
        (s / "train.txt").write_text("\n".join(NAMES) + "\n\n")
        (s / "val.txt").write_text(NAMES[0] + "\n")
    return root, rgb


def _dataset(root, split="val", splitsdir="overfit", **kw):
    import svr_amd  # noqa: F401
    from svr_amd.dataset import ScenesDataset
    return ScenesDataset(split, root / "data", splitsdir, SimpleNamespace(**kw) if kw else None, splits_root=root / "splits")


def test_input_is_the_transform_of_the_mirrored_image(tree):
    root, rgb = tree
    import svr_amd  # noqa: F401
    from svr_amd.dataset.scene_net_data import rgb_transform
    flipped = Image.fromarray(np.ascontiguousarray(rgb[:, ::-1]))
    assert not np.array_equal(rgb[:, ::-1], rgb)
    for resize, shape in ((True, (3, 256, 256)), (False, (3, 240, 320))):
        item = _dataset(root, W=256, resize_input=resize)[0]
        assert item["name"] == NAMES[0] and item["input"].is_cuda and tuple(item["input"].shape) == shape
        assert item["input"].dtype == torch.float32
        assert torch.equal(item["input"].cpu(), rgb_transform(flipped, 256, resize))
        assert not torch.equal(item["input"].cpu(), rgb_transform(Image.fromarray(rgb), 256, resize))
    assert tuple(_dataset(root)[0]["input"].shape) == (3, 256, 256)            # kwargs=None: W = 256, resize


def test_target_is_the_depth_map_flipped_after_the_conversion(tree):
    root, _ = tree
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    from svr_amd.data_processing.distance_to_depth import FromDistanceToDepth
    target = _dataset(root)[0]["target"]
    assert target.is_cuda and tuple(target.shape) == (1, 240, 320) and target.dtype == torch.float32
    dist = sample_io.exr_read(os.path.join(GOLD, "raw_distance.exr"), "R")
    after = torch.flip(FromDistanceToDepth(FOCAL)(dist), dims=(1,)).cpu().numpy()
    got = target.cpu().numpy()[0]
    assert np.array_equal(got.view(np.int32), after.view(np.int32))
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(np_depth(dist, FOCAL)[:, ::-1]).view(np.int32))
    # the other order -- mirror the distance map, then convert -- is a different map: col - 160 is not symmetric in 0..319
    before = np_depth(np.ascontiguousarray(dist[:, ::-1]), FOCAL)
    assert not np.array_equal(before, got) and np.abs(before - got).max() > 1e-4


def test_overfit_train_split_is_repeated_500_times(tree):
    root, _ = tree
    assert len(_dataset(root, "train", "overfit")) == 500 * len(NAMES)
    assert len(_dataset(root, "val", "overfit")) == 1
    ds = _dataset(root, "train", "overfit_small")                 # equality with 'overfit', not containment
    assert len(ds) == len(NAMES) and ds.data == NAMES


def test_dataloader_collates_device_tensors(tree):
    root, _ = tree
    ds = _dataset(root, "train", "overfit")
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0)))
    assert batch["name"] == NAMES
    assert batch["input"].is_cuda and tuple(batch["input"].shape) == (2, 3, 256, 256)
    assert batch["target"].is_cuda and tuple(batch["target"].shape) == (2, 1, 240, 320)
    assert torch.equal(batch["target"][1], ds[1]["target"])
