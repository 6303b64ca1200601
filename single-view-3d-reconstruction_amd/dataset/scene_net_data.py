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
      The resize's arithmetic IS pinned against Pillow: ops.rgb_preprocess (csrc/rgb_preprocess.hip) restates Pillow's 8-bit
      bilinear resampler and the tests compare it, and the tables behind it, with ``Image.resize`` byte for byte (DESIGN.md
      section 17).  Parity with torchvision.transforms.Resize is still NOT pinned: torchvision is absent where this was
      written (PIL's bilinear filter is what Resize applies to a PIL image, antialiasing included, but no test proves it).

The reference reads data/splits and data/intrinsics.txt relative to the working directory; `splits_root` and
`intrinsics_path` say where they are.

``DeviceSceneLoader(dataset)`` serves the same items as collated device batches without the per-item host work: see the
class."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

from .. import ops
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


class DeviceSceneLoader:
    """GPU-resident views for SceneNetTrainer: the scene counterpart of implicit_dataset.DeviceSampleLoader, around a
    ``scene_net_data`` dataset (precision 32 only).

    A view is decoded on first touch -- PNG + transform, the EXR's channel R, both occupancy files' `points` / `occupancies`
    in their stored dtype -- into pinned staging and copied on a side stream; with ``cache=True`` the transformed `rgb`, the
    `depthmap_target` and the four occupancy arrays stay on the device (about 6 MB per view at 110 k points), so a later visit
    reads no file.  ``batch(indices)`` draws like a DataLoader over the dataset would -- item by item, '0.10' then '0.01',
    one ``np.random.randint(0, n_rows, num_points)`` each -- straight into one pinned int64 buffer that also carries the
    segment table, and issues one H2D copy, one svr_subsample_rows_batched launch that writes `points` (B, 2n, 3) and
    `occupancies` (B, 2n) in place, and one stack each for `rgb` and `depthmap_target`.  The result is the dictionary
    ``default_collate`` makes of the dataset's items, bit for bit under the same numpy random state.

    ``device_rgb=True``: the PNG's raw uint8 pixels (mode L or RGB) are what is staged and copied, and ops.rgb_preprocess runs
    the transform on the copy stream -- the same `rgb` bit for bit, under a third of the bytes across the bus and no
    Pillow resize on the host.  Off by default (DESIGN.md section 17 has the measurement).

    ``bad_rows()`` reads (synchronising) whether any launch saw a row outside its source: with indices drawn here it cannot."""

    ARRAYS = ("points", "occupancies")

    def __init__(self, dataset, device=None, cache=True, device_rgb=False):
        if dataset.dtype != torch.float32:
            raise ValueError("DeviceSceneLoader supports precision == 32 only")
        self.ds = dataset
        self.device_rgb = bool(device_rgb)
        self.device = torch.device(device) if device is not None else dataset.device
        self.cache = {} if cache else None
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.bad = torch.zeros(1, device=self.device, dtype=torch.int32)

    def __len__(self):
        return len(self.ds)

    def _folders(self, item):
        ds = self.ds
        return ds.dataset_path / "raw" / ds.splitsdir / item, ds.dataset_path / "processed" / ds.splitsdir / item

    def _decode_rgb(self, path):
        """rgb.png -> (the transformed image on the device, its pinned staging buffer); the copy (and with device_rgb the
        transform) is queued on the copy stream."""
        with Image.open(path) as image:
            if self.device_rgb:
                if image.mode not in ("L", "RGB"):
                    raise ValueError(f"{path}: mode {image.mode}; device_rgb takes 8-bit L or RGB images")
                pixels = np.asarray(image, dtype=np.uint8)
                pixels = pixels.reshape(pixels.shape[0], pixels.shape[1], -1)
            else:
                rgb = rgb_transform(image, self.ds.W, self.ds.resize_input)
        with torch.cuda.stream(self.copy_stream):
            if self.device_rgb:                              # the raw bytes cross, the transform runs behind the copy
                stage = torch.empty(pixels.shape, dtype=torch.uint8, pin_memory=True)
                stage.numpy()[...] = pixels
                return ops.rgb_preprocess(stage.to(self.device, non_blocking=True).unsqueeze(0), self.ds.W,
                                          self.ds.resize_input)[0], stage
            stage = torch.empty(rgb.shape, dtype=torch.float32, pin_memory=True).copy_(rgb)
            return stage.to(self.device, non_blocking=True), stage

    def _decode(self, item):
        raw, processed = self._folders(item)
        s, keep = {"mesh": str(raw / "mesh.obj")}, []
        s["rgb"], stage = self._decode_rgb(raw / "rgb.png")
        keep.append(stage)
        with torch.cuda.stream(self.copy_stream):
            info = sample_io.exr_info(raw / "distance.exr")
            stage = torch.empty(info["height"] * info["width"], dtype=torch.float32, pin_memory=True)
            sample_io.exr_read(raw / "distance.exr", "R", out=stage.numpy())
            distance = stage.to(self.device, non_blocking=True).view(info["height"], info["width"])
            s["depthmap_target"] = self.ds.to_depth(distance)
            keep.append(stage)
            for sigma in SIGMAS:
                f = processed / f"occupancy_{sigma}.npz"
                for key in self.ARRAYS:
                    dtype, shape, fortran = sample_io.npz_member_info(f, key)
                    if fortran:                             # the kernel indexes the flat payload as C order
                        raise ValueError(f"{f}[{key}]: fortran_order arrays are not supported by DeviceSceneLoader")
                    stage = torch.empty(int(np.prod(shape)), dtype=torch.from_numpy(np.empty(0, dtype)).dtype, pin_memory=True)
                    sample_io.npz_load(f, key, out=stage.numpy())
                    s[(sigma, key)] = stage.to(self.device, non_blocking=True).view(shape)
                    keep.append(stage)
                if s[(sigma, "points")].shape[0] != s[(sigma, "occupancies")].shape[0]:
                    raise ValueError(f"{f}: points and occupancies differ in length")
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        s["_ready"], s["_staging"] = done, keep              # the pinned buffers live until the copies have finished
        return s

    def _sample(self, idx):
        item = self.ds.data[idx]
        s = self.cache.get(item) if self.cache is not None else None
        if s is None:
            s = self._decode(item)
            if self.cache is not None:
                self.cache[item] = s
        cur = torch.cuda.current_stream()
        cur.wait_event(s["_ready"])
        # allocated under copy_stream, read by the caller's stream: see DeviceSampleLoader.get
        for t in s.values():
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        if s.get("_staging") is not None and s["_ready"].query():
            s["_staging"] = None
        return item, s

    def batch(self, indices):
        indices = [int(i) for i in indices]
        B, n = len(indices), int(self.ds.num_points)
        samples = [self._sample(i) for i in indices]
        # one float32 block behind both outputs: points (B, 2n, 3) then occupancies (B, 2n)
        out = torch.empty(B * 2 * n * 4, device=self.device, dtype=torch.float32)
        occ_base = B * 2 * n * 3
        segments = []
        for b, (_, s) in enumerate(samples):
            for k, sigma in enumerate(SIGMAS):
                at = (b * 2 + k) * n
                segments.append((s[(sigma, "points")], at, n, at * 3))
                segments.append((s[(sigma, "occupancies")], at, n, occ_base + at))
        packed, draws, total = sample_io.pack_row_segments(segments, B * 2 * n, out.numel())
        for b, (_, s) in enumerate(samples):                 # the dataset's draws, in the dataset's order
            for k, sigma in enumerate(SIGMAS):
                at = (b * 2 + k) * n
                draws[at:at + n] = np.random.randint(0, s[(sigma, "points")].shape[0], n)
        sample_io.subsample_rows_batched(packed.to(self.device, non_blocking=True), len(segments), total, out, self.bad)
        return {"name": [item for item, _ in samples], "mesh": [s["mesh"] for _, s in samples],
                "rgb": torch.stack([s["rgb"] for _, s in samples]),
                "points": out[:occ_base].view(B, 2 * n, 3), "occupancies": out[occ_base:].view(B, 2 * n),
                "depthmap_target": torch.stack([s["depthmap_target"] for _, s in samples])}

    def bad_rows(self):
        return bool(self.bad.item())
