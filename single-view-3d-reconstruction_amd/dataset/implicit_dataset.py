"""Sample loading for the IF-Net trainer: mirror of the reference's dataset/implicit_dataset.py:10-56 on the native
readers.

``ImplicitDataset(split, dataset_path, num_points, splitsdir)`` keeps the reference's constructor, ``__len__`` and the
``__getitem__`` dict (CPU tensors 'name', 'grid', 'points', 'input', 'occupancies', 'target': a torch DataLoader can
wrap it unchanged) and draws its random subset with the same two ``np.random.randint`` calls, so with the same numpy
random state the tensors equal the reference's bit for bit.  What changes is how the bytes arrive: one fread for the .df
payload instead of a struct.unpack per float, native .npz member reads, one fancy-index per array instead of Python
lists of rows.

``DeviceSampleLoader`` goes further for a 22 ms step: a sample's arrays are decoded ONCE into pinned staging buffers,
copied to the GPU asynchronously and (optionally) kept there; every later visit of the sample -- the overfit split
repeats each sample 50x per epoch, :18 -- costs three tiny kernels (row subset with cast).  The float64 -> float32
casts, the .df transpose and the subset all run on the device."""
from pathlib import Path

import numpy as np
import torch

from ..data_processing import sample_io
from ..data_processing.volume_reader import read_df

SIGMAS = ("0.10", "0.01")


def _split_items(splitsdir, split, splits_root="data/splits"):
    return [x.strip() for x in (Path(splits_root) / splitsdir / f"{split}.txt").read_text().split("\n") if x.strip() != ""]


class ImplicitDataset(torch.utils.data.Dataset):
    def __init__(self, split, dataset_path, num_points, splitsdir, splits_root="data/splits"):
        self.dataset_path = Path(dataset_path)
        self.split = split
        self.splitsdir = splitsdir
        self.split_shapes = _split_items(splitsdir, split, splits_root)
        self.data = [x for x in self.split_shapes]
        self.data = self.data * (50 if ("overfit" in splitsdir) and split == "train" else 1)
        self.num_points = num_points

    def __len__(self):
        return len(self.data)

    def sample_folder(self, idx):
        return Path(self.dataset_path) / "processed" / self.splitsdir / self.data[idx]

    def __getitem__(self, idx):
        item = self.data[idx]
        folder = self.sample_folder(idx)
        sample_input = torch.from_numpy(sample_io.npz_load(folder / "depth_grid.npz", "grid")).float()
        sample_target = torch.from_numpy(read_df(str(folder / "target.df"))).float()
        points, occupancies, grids = [], [], []
        for sigma in SIGMAS:
            f = folder / f"occupancy_{sigma}.npz"
            p = sample_io.npz_load(f, "points")
            g = sample_io.npz_load(f, "grid_coords")
            o = sample_io.npz_load(f, "occupancies")
            idxs = np.random.randint(0, p.shape[0], self.num_points)       # same call, same order as the reference (:40)
            points.append(p[idxs])
            grids.append(g[idxs])
            occupancies.append(o[idxs])
        return {
            "name": item,
            "grid": torch.from_numpy(np.concatenate(grids).astype(np.float32)),
            "points": torch.from_numpy(np.concatenate(points).astype(np.float32)),
            "input": sample_input.unsqueeze(0),
            "occupancies": torch.from_numpy(np.concatenate(occupancies).astype(np.float32)),
            "target": sample_target.unsqueeze(0),
        }


class DeviceSampleLoader:
    """GPU-resident samples: `get(idx)` returns the reference's sample dict with CUDA tensors.  Decoding (zip inflate,
    fread) happens on first touch into pinned memory; copies run on a side stream; with `cache=True` the decoded arrays
    stay on the device (a sample is ~23 MB: the 139x104x112 float32 grid and target + two 100k-point occupancy sets), so
    repeated visits only run the subset kernels.  Indices come from `np.random.randint` like the reference (pass
    `generator=` for a torch device generator instead)."""

    def __init__(self, dataset, device="cuda", cache=True):
        self.ds = dataset
        self.device = torch.device(device)
        self.cache = {} if cache else None
        self.copy_stream = torch.cuda.Stream(device=self.device)

    def _pinned(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, pin_memory=True)

    @staticmethod
    def _c_order(fortran, path, key):
        # the device path reinterprets the flat payload as C order (process_sample.py writes C-order arrays); a
        # Fortran-order member would be silently transposed: refuse it (ImplicitDataset / npz_load honour the flag)
        if fortran:
            raise ValueError(f"{path}[{key}]: fortran_order arrays are not supported by DeviceSampleLoader")

    def _decode(self, folder):
        s = {}
        with torch.cuda.stream(self.copy_stream):
            dtype, shape, fortran = sample_io.npz_member_info(folder / "depth_grid.npz", "grid")
            self._c_order(fortran, folder / "depth_grid.npz", "grid")
            stage = self._pinned(int(np.prod(shape)), torch.from_numpy(np.empty(0, dtype)).dtype)
            sample_io.npz_load(folder / "depth_grid.npz", "grid", out=stage.numpy())
            s["input"] = sample_io.cast_to_f32(stage.to(self.device, non_blocking=True).view(shape))
            dims = sample_io.df_dims(folder / "target.df")
            stage_t = self._pinned(dims[0] * dims[1] * dims[2], torch.float32)
            sample_io.df_read_payload(folder / "target.df", out=stage_t.numpy())
            s["target"] = sample_io.df_to_grid(stage_t.to(self.device, non_blocking=True), dims)
            keep = [stage, stage_t]
            for sigma in SIGMAS:
                f = folder / f"occupancy_{sigma}.npz"
                for key in ("points", "grid_coords", "occupancies"):
                    dtype, shape, fortran = sample_io.npz_member_info(f, key)
                    self._c_order(fortran, f, key)
                    st = self._pinned(int(np.prod(shape)), torch.from_numpy(np.empty(0, dtype)).dtype)
                    sample_io.npz_load(f, key, out=st.numpy())
                    s[(sigma, key)] = st.to(self.device, non_blocking=True).view(shape)
                    keep.append(st)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        s["_ready"], s["_staging"] = done, keep          # the pinned buffers live until the copies have finished
        return s

    def get(self, idx, generator=None):
        item = self.ds.data[idx]
        folder = self.ds.sample_folder(idx)
        s = self.cache.get(item) if self.cache is not None else None
        if s is None:
            s = self._decode(folder)
            if self.cache is not None:
                self.cache[item] = s
        cur = torch.cuda.current_stream()
        cur.wait_event(s["_ready"])
        # The decoded tensors were allocated under copy_stream but are read by kernels on the CALLER's stream (the subset
        # kernels below; `input` / `target` by whatever consumes the sample).  Without record_stream a cache=False sample
        # dropped at return hands its blocks back to copy_stream's pool while those kernels are still queued, and the next
        # _decode overwrites them with H2D copies that never wait for the consumer.
        for t in s.values():
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        if s.get("_staging") is not None and s["_ready"].query():
            s["_staging"] = None                       # the copies have landed: give the pinned staging buffers back
        pts, occ, grid = [], [], []
        for sigma in SIGMAS:
            n = s[(sigma, "points")].shape[0]
            if generator is None:
                idxs = torch.from_numpy(np.random.randint(0, n, self.ds.num_points)).to(self.device)
            else:
                idxs = torch.randint(0, n, (self.ds.num_points,), device=self.device, generator=generator)
            pts.append(sample_io.subsample_rows(s[(sigma, "points")], idxs)[0])
            grid.append(sample_io.subsample_rows(s[(sigma, "grid_coords")], idxs)[0])
            occ.append(sample_io.subsample_rows(s[(sigma, "occupancies")], idxs)[0])
        return {"name": item, "grid": torch.cat(grid), "points": torch.cat(pts), "input": s["input"].unsqueeze(0),
                "occupancies": torch.cat(occ), "target": s["target"].unsqueeze(0)}

    def batch(self, indices, generator=None):
        """Collated batch (what a DataLoader's default collate would produce), on the device."""
        samples = [self.get(i, generator) for i in indices]
        out = {"name": [s["name"] for s in samples]}
        for k in ("grid", "points", "input", "occupancies", "target"):
            out[k] = torch.stack([s[k] for s in samples])
        return out


class BatchedSampleLoader(DeviceSampleLoader):
    """DeviceSampleLoader for a loop that must not stall: ``batch(indices)`` returns the same dictionary from the same numpy
    draws (item by item, '0.10' then '0.01'), but the draws go into one pinned int64 buffer next to the segment table, cross
    in one asynchronous copy, and one svr_subsample_rows_batched launch writes `points`, `grid` (B, 2n, 3) and `occupancies`
    (B, 2n) in place.  ``get`` uploads each draw from pageable memory: that copy blocks the host until the stream has
    drained, once per item and sigma, which cost the fit loop 4.7 ms on a 15.2 ms step."""

    ARRAYS = ("points", "grid_coords", "occupancies")

    def _resident(self, idx):
        """The decoded sample, handed over to the caller's stream (the first half of ``get``)."""
        item = self.ds.data[idx]
        s = self.cache.get(item) if self.cache is not None else None
        if s is None:
            s = self._decode(self.ds.sample_folder(idx))
            if self.cache is not None:
                self.cache[item] = s
        cur = torch.cuda.current_stream()
        cur.wait_event(s["_ready"])
        for t in s.values():
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        if s.get("_staging") is not None and s["_ready"].query():
            s["_staging"] = None
        return item, s

    def batch(self, indices, generator=None):
        if generator is not None:                       # device-side draws: the per-item path
            return super().batch(indices, generator)
        B, n = len(indices), int(self.ds.num_points)
        samples = [self._resident(int(i)) for i in indices]
        out = torch.empty(B * 2 * n * 7, device=self.device, dtype=torch.float32)
        base = {"points": 0, "grid_coords": B * 2 * n * 3, "occupancies": B * 2 * n * 6}
        segments = []
        for b, (_, s) in enumerate(samples):
            for k, sigma in enumerate(SIGMAS):
                at = (b * 2 + k) * n
                for key in self.ARRAYS:
                    segments.append((s[(sigma, key)], at, n, base[key] + at * (1 if key == "occupancies" else 3)))
        packed, draws, total = sample_io.pack_row_segments(segments, B * 2 * n, out.numel())
        for b, (_, s) in enumerate(samples):
            for k, sigma in enumerate(SIGMAS):
                at = (b * 2 + k) * n
                draws[at:at + n] = np.random.randint(0, s[(sigma, "points")].shape[0], n)
        sample_io.subsample_rows_batched(packed.to(self.device, non_blocking=True), len(segments), total, out)
        return {"name": [item for item, _ in samples], "grid": out[base["grid_coords"]:base["occupancies"]].view(B, 2 * n, 3),
                "points": out[:base["grid_coords"]].view(B, 2 * n, 3),
                "input": torch.stack([s["input"].unsqueeze(0) for _, s in samples]),
                "occupancies": out[base["occupancies"]:].view(B, 2 * n),
                "target": torch.stack([s["target"].unsqueeze(0) for _, s in samples])}
