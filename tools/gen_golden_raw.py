"""Generate tests/golden/raw_sample.npz and raw_sample_coords.npz (and copy tests/golden/raw_distance.exr) by running the REFERENCE's
data_processing/distance_to_depth.py on the CPU.  Needs a checkout of the reference (--reference DIR or $SVR_REFERENCE);
no test does.

STAND-INS.  `pyexr`, `trimesh` and `marching_cubes` are not installed where this is run.  The last two are stubbed as
empty modules (distance_to_depth.py imports util.visualize, which imports them, and uses neither); `pyexr.open(path)
.get(name)` is served by the small numpy + zlib OpenEXR decoder below -- a second, independent decoder next to the
library's C++ one, so the golden channel pins the library against it, not against itself.

Stored (raw_sample.npz; `coords` alone in raw_sample_coords.npz, which keeps each file under the 1 MiB limit for committed files):
  distance          (240, 320) float32  channel R of data/raw/overfit/00000/distance.exr
  depth             (240, 320) float32  FromDistanceToDepth(focal of data/intrinsics.txt)(distance), the reference's torch ops
  depth_sample      only if the sample's intrinsic.txt gives another focal length: the same with that one
  coords            (76800, 3) float32  depth_to_gridspace(distance.exr, intrinsic.txt, 1) FLATTENED to (H*W, 3)
  intrinsics_txt / intrinsic_txt        the two files' text
  n_ones            5466: voxels set by np.round(coords) -- checked here to reproduce the reference's own
                    data/processed/overfit/00000/depth_grid.npz (tests/golden/ref_depth_grid.npz) with no voxel different
Nothing of the reference's text is stored; only these arrays, and its data file distance.exr byte for byte."""
import argparse
import os
import shutil
import struct
import sys
import types
import zlib
from pathlib import Path

import numpy as np

SAMPLE = ("data", "raw", "overfit", "00000")


def read_exr(path):
    """{channel: (H, W) float32} of a single-part scanline file, compression NONE / ZIPS / ZIP, FLOAT channels."""
    b = open(path, "rb").read()
    assert struct.unpack("<I", b[:4])[0] == 20000630 and struct.unpack("<I", b[4:8])[0] == 2
    p, attrs = 8, {}
    while b[p] != 0:
        e = b.index(0, p)
        name = b[p:e].decode()
        p = b.index(0, e + 1) + 1
        size = struct.unpack("<i", b[p:p + 4])[0]
        attrs[name] = b[p + 4:p + 4 + size]
        p += 4 + size
    p += 1
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"])
    W, H = x1 - x0 + 1, y1 - y0 + 1
    names, c, q = [], attrs["channels"], 0
    while c[q] != 0:
        e = c.index(0, q)
        assert struct.unpack("<i", c[e + 1:e + 5])[0] == 2, "FLOAT channels only"
        names.append(c[q:e].decode())
        q = e + 17
    comp = attrs["compression"][0]
    lines = {0: 1, 2: 1, 3: 16}[comp]
    nblk = (H + lines - 1) // lines
    out = {n: np.zeros((H, W), np.float32) for n in names}
    for off in struct.unpack(f"<{nblk}Q", b[p:p + 8 * nblk]):
        y, size = struct.unpack("<ii", b[off:off + 8])
        data = b[off + 8:off + 8 + size]
        nl = min(lines, H - (y - y0))
        raw = nl * W * 4 * len(names)
        if comp and size < raw:
            d = np.frombuffer(zlib.decompress(data), np.uint8).astype(np.int64)
            assert d.size == raw
            t = (np.cumsum(np.concatenate([d[:1], d[1:] - 128])) % 256).astype(np.uint8)   # t[i] = t[i-1] + d[i] - 128
            half = (raw + 1) // 2
            u = np.empty(raw, np.uint8)
            u[0::2], u[1::2] = t[:half], t[half:]
            data = u.tobytes()
        rows = np.frombuffer(data, "<f4").reshape(nl, len(names), W)       # scanline by scanline, channel by channel
        for k, n in enumerate(names):
            out[n][y - y0:y - y0 + nl] = rows[:, k]
    return out


def load_reference(ref):
    class _File:
        def __init__(self, path):
            self.channels = read_exr(path)

        def get(self, name):
            return self.channels[name][:, :, None]

    pyexr = types.ModuleType("pyexr")
    pyexr.open = lambda path: _File(path)
    sys.modules.update({"pyexr": pyexr, "trimesh": types.ModuleType("trimesh"), "marching_cubes": types.ModuleType("marching_cubes")})
    sys.path.insert(0, ref)
    import data_processing.distance_to_depth as D
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVR_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    assert a.reference, "pass --reference DIR (a checkout of the reference) or set SVR_REFERENCE"
    ref, out = Path(a.reference), Path(a.out)
    D = load_reference(str(ref))
    sample = ref.joinpath(*SAMPLE)
    exr = read_exr(sample / "distance.exr")
    assert sorted(exr) == ["B", "G", "R"] and (exr["R"] == exr["G"]).all() and (exr["R"] == exr["B"]).all()
    distance = exr["R"]

    intrinsics_txt = (ref / "data" / "intrinsics.txt").read_text()
    intrinsic_txt = (sample / "intrinsic.txt").read_text()
    f_data = D.get_intrinsic(ref / "data" / "intrinsics.txt")[0][0]
    f_sample = D.get_intrinsic(sample / "intrinsic.txt")[0][0]
    depth = np.asarray(D.FromDistanceToDepth(f_data)(distance), dtype=np.float32)
    arrays = {"distance": distance, "depth": depth, "intrinsics_txt": np.array(intrinsics_txt), "intrinsic_txt": np.array(intrinsic_txt)}
    if float(f_sample) != float(f_data):
        arrays["depth_sample"] = np.asarray(D.FromDistanceToDepth(f_sample)(distance), dtype=np.float32)

    coords = D.depth_to_gridspace(str(sample / "distance.exr"), sample / "intrinsic.txt", 1).reshape(-1, 3).numpy()
    assert coords.shape == (240 * 320, 3) and coords.dtype == np.float32
    dims = (139, 104, 112)
    idx = np.round(coords).astype(np.int32)
    assert ((idx >= 0) & (idx < np.array(dims))).all(), "an index of the real sample leaves the grid"
    grid = np.zeros(dims)
    grid[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
    shipped = np.load(ref / "data" / "processed" / "overfit" / "00000" / "depth_grid.npz")["grid"]
    committed = np.load(out / "ref_depth_grid.npz")["grid"]
    assert (grid == shipped).all() and (grid == committed).all(), "the flattened chain does not reproduce the reference's depth_grid.npz"
    arrays["n_ones"] = np.array(int(grid.sum()))
    tie = np.abs(np.abs(coords - np.floor(coords)) - 0.5)

    # a float32 restatement with separately rounded operations: reported, not stored (what the device kernel computes)
    H, W = distance.shape
    f = np.float32(f_data)
    rc = ((np.arange(H)[:, None] - H // 2) ** 2 + (np.arange(W)[None, :] - W // 2) ** 2).astype(np.float32)
    restated = np.sqrt(distance * distance / (rc / (f * f) + np.float32(1)))
    ulp = np.abs(restated.view(np.int32).astype(np.int64) - depth.view(np.int32).astype(np.int64))
    print(f"depth: float32 restatement vs the reference's torch ops: {int((ulp != 0).sum())} of {ulp.size} differ, max {int(ulp.max())} ulp")
    print(f"coords: closest rounding tie {tie.min():.3g}; {int((tie < 1e-4).sum())} within 1e-4; ones {int(grid.sum())}")

    np.savez_compressed(out / "raw_sample.npz", **arrays)
    np.savez_compressed(out / "raw_sample_coords.npz", coords=coords)
    shutil.copyfile(sample / "distance.exr", out / "raw_distance.exr")
    for name in ("raw_sample.npz", "raw_sample_coords.npz", "raw_distance.exr"):
        print("wrote", out / name, os.path.getsize(out / name), "bytes")


if __name__ == "__main__":
    main()
