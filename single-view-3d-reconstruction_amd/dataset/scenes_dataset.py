"""Mirror of the reference's dataset/scenes_dataset.py:21-75: the items DepthRegressorTrainer eats (UNet depth pre-training).

``ScenesDataset(split, dataset_path, splitsdir, kwargs, device="cuda")`` keeps the reference's constructor (kwargs: W,
resize_input -- defaults 256 / True where the namespace lacks them), ``__len__`` and the item dict:

  name   : the line of the splits file.
  input  : rgb.png, mirrored left-right (``transpose(Image.FLIP_LEFT_RIGHT)``), through scene_net_data's transform chain
           (SquarePad, bilinear resize to (W, W), [0, 1], (x - 0.5) / 0.5): (3, W, W), or (3, 240, 320) without resize.
  target : (1, 240, 320) float32 on the device: channel R of distance.exr (native reader) -> z-depth (svr_distance_to_depth,
           focal length of data/intrinsics.txt) -> columns reversed.  The conversion centres on ``col - W // 2``, which is
           not symmetric in the columns, so the flip comes AFTER the conversion, as in the reference (:65-66).

The item list is repeated x500 when ``splitsdir == 'overfit'`` and ``split == 'train'`` (equality, unlike scene_net_data's
``in``).  The reference reads data/splits and data/intrinsics.txt relative to the working directory; `splits_root` and
`intrinsics_path` say where they are (None = the same intrinsic constants, built in).  No torchvision, no pyexr."""
from pathlib import Path
from types import SimpleNamespace

import torch
from PIL import Image

from ..data_processing import sample_io
from ..data_processing.distance_to_depth import FromDistanceToDepth, get_intrinsic
from .implicit_dataset import _split_items
from .scene_net_data import rgb_transform


def list_items(split, splitsdir, splits_root="data/splits"):
    """The dataset's item list (host only): the splits file's lines, x500 for the overfit training split."""
    items = _split_items(splitsdir, split, splits_root)
    return items * (500 if splitsdir == "overfit" and split == "train" else 1)


def load_input(path, W=256, resize_input=True):
    """rgb.png -> the mirrored, transformed (3, H, W) float32 host tensor."""
    with Image.open(path) as image:
        return rgb_transform(image.transpose(Image.FLIP_LEFT_RIGHT), W, resize_input)


class ScenesDataset(torch.utils.data.Dataset):
    def __init__(self, split, dataset_path, splitsdir, kwargs=None, device="cuda", splits_root="data/splits",
                 intrinsics_path=None):
        self.kwargs = kwargs if kwargs is not None else SimpleNamespace()
        self.dataset_path = Path(dataset_path)
        self.split = split
        self.splitsdir = splitsdir
        self.split_shapes = _split_items(splitsdir, split, splits_root)
        self.data = list_items(split, splitsdir, splits_root)
        self.device = torch.device(device)
        self.W = int(getattr(self.kwargs, "W", 256))
        self.resize_input = bool(getattr(self.kwargs, "resize_input", True))
        self.to_depth = FromDistanceToDepth(get_intrinsic(intrinsics_path)[0][0])

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        item = self.data[idx]
        sample_folder = self.dataset_path / "raw" / self.splitsdir / item
        sample_input = load_input(sample_folder / "rgb.png", self.W, self.resize_input)
        distance_map = sample_io.exr_read(sample_folder / "distance.exr", "R")
        depth_map = self.to_depth(distance_map)                       # (H, W) on the device
        target = torch.flip(depth_map, dims=(1,)).unsqueeze(0).to(self.device)
        return {"name": item, "input": sample_input.to(self.device), "target": target}
