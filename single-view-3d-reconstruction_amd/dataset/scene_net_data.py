"""Mirror of the reference's dataset/scene_net_data.py:24-103: the items SceneNetTrainer.training_step eats.

``scene_net_data(split, dataset_path, num_points, splitsdir, kwargs, device="cuda")`` keeps the reference's constructor
(kwargs: W, resize_input, precision -- defaults 256 / True / 32 where the namespace lacks them), ``__len__`` and the item
dict: 'name', 'mesh' (path of raw/.../mesh.obj), 'rgb', 'points', 'occupancies', 'depthmap_target'.  The tensors live on
`device`.

  points / occupancies : the two occupancy files in the order '0.10', '0.01', one ``np.random.randint`` draw each, through
      the native .npz reader as in ImplicitDataset: with the same numpy random state, the reference's rows.
  depthmap_target      : channel R of distance.exr (native reader) -> svr_distance_to_depth with the focal length of
      data/intrinsics.txt (`intrinsics_path`; None = the same constants, built in), (H, W).
  rgb                  : host work, as in the reference.  torchvision is not a dependency, so its transform chain is written
      out: PIL open; SquarePad = constant-0 pad of hp = int((max - w) / 2) columns and vp = int((max - h) / 2) rows on both
      sides; ``Image.resize((W, W), Image.BILINEAR)`` when resize_input; scale to [0, 1], channel first; (x - 0.5) / 0.5.
      Parity of the resize with torchvision.transforms.Resize is NOT pinned: torchvision is absent where this was
      written (PIL's bilinear filter is what Resize applies to a PIL image, antialiasing included, but no test proves it).

The reference reads data/splits and data/intrinsics.txt relative to the working directory; `splits_root` and
`intrinsics_path` say where they are."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from ..data_processing import sample_io
from ..data_processing.distance_to_depth import FromDistanceToDepth, get_intrinsic
from .implicit_dataset import SIGMAS, _split_items


def square_pad(image):
    """SquarePad of scene_net_data.py:13-20 on a PIL image."""
    w, h = image.size
    max_wh = max(w, h)
    hp = int((max_wh - w) / 2)
    vp = int((max_wh - h) / 2)
    out = Image.new(image.mode, (w + 2 * hp, h + 2 * vp), 0)
    out.paste(image, (hp, vp))
    return out


def rgb_transform(image, W, resize_input):
    """PIL image -> (C, H, W) float32 in [-1, 1]: [SquarePad, Resize((W, W))] when resize_input, ToTensor, Normalize(0.5, 0.5)."""
    if resize_input:
        image = square_pad(image).resize((W, W), Image.BILINEAR)
    a = np.asarray(image, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    x = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).float().div(255)
    return (x - 0.5) / 0.5


class scene_net_data(torch.utils.data.Dataset):
    def __init__(self, split, dataset_path, num_points, splitsdir, kwargs=None, device="cuda", splits_root="data/splits",
                 intrinsics_path=None):
        self.kwargs = kwargs if kwargs is not None else SimpleNamespace()
        self.dataset_path = Path(dataset_path)
        self.split = split
        self.splitsdir = splitsdir
        self.split_shapes = _split_items(splitsdir, split, splits_root)
        self.data = [x for x in self.split_shapes]
        self.data = self.data * (50 if ("overfit" in splitsdir) and split == "train" else 1)
        self.num_points = num_points
        self.device = torch.device(device)
        self.W = int(getattr(self.kwargs, "W", 256))
        self.resize_input = bool(getattr(self.kwargs, "resize_input", True))
        self.dtype = {16: torch.float16, 32: torch.float32, 64: torch.float64}[int(getattr(self.kwargs, "precision", 32))]
        self.to_depth = FromDistanceToDepth(get_intrinsic(intrinsics_path)[0][0])

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        item = self.data[idx]
        sample_folder = self.dataset_path / "raw" / self.splitsdir / item
        df_folder = self.dataset_path / "processed" / self.splitsdir / item

        with Image.open(sample_folder / "rgb.png") as image:
            rgb_img = rgb_transform(image, self.W, self.resize_input)

        points, occupancies = [], []
        for sigma in SIGMAS:                                   # '0.10' then '0.01' (:61)
            f = df_folder / f"occupancy_{sigma}.npz"
            p = sample_io.npz_load(f, "points")
            o = sample_io.npz_load(f, "occupancies")
            idxs = np.random.randint(0, p.shape[0], self.num_points)
            points.append(p[idxs])
            occupancies.append(o[idxs])
        np_dtype = torch.empty(0, dtype=self.dtype).numpy().dtype
        sample_points = torch.from_numpy(np.concatenate(points).astype(np_dtype))
        sample_occupancies = torch.from_numpy(np.concatenate(occupancies).astype(np_dtype))

        distance_map = sample_io.exr_read(sample_folder / "distance.exr", "R")
        depthmap_target = self.to_depth(distance_map).to(self.dtype)

        return {
            "name": item,
            "mesh": str(sample_folder / "mesh.obj"),
            "rgb": rgb_img.to(self.dtype).to(self.device),
            "points": sample_points.to(self.device),
            "occupancies": sample_occupancies.to(self.device),
            "depthmap_target": depthmap_target.to(self.device),
        }
