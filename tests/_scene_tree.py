"""Shared by the scene-loader and fit-loop GPU tests: a small dataset tree in the reference's layout.

    <root>/data/raw/<splitsdir>/<name>/rgb.png         PIL-written, random pixels
                                      /distance.exr    tests/golden/raw_distance.exr
    <root>/data/processed/<splitsdir>/<name>/...       occupancy_0.10.npz / occupancy_0.01.npz (numpy-written); with `dims`
                                                       also depth_grid.npz and target.df (oracle.dataset_oracle.make_sample)
    <root>/splits/<splitsdir>/{train,val,test}.txt
"""
import os
import shutil

import numpy as np
from PIL import Image

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def build_tree(root, splits, splitsdir="tiny", rows=None, dims=None, seed=0):
    """`splits`: {split: [names]}.  `rows`: {name: (rows of occupancy_0.10, rows of occupancy_0.01)} for numpy-written
    occupancy files of those lengths; otherwise (`dims` given) make_sample writes the whole processed sample."""
    from oracle.dataset_oracle import make_sample
    rng = np.random.default_rng(seed)
    names = sorted({n for items in splits.values() for n in items})
    for k, name in enumerate(names):
        raw = root / "data" / "raw" / splitsdir / name
        processed = root / "data" / "processed" / splitsdir / name
        raw.mkdir(parents=True)
        processed.mkdir(parents=True)
        Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(raw / "rgb.png")
        shutil.copyfile(os.path.join(GOLD, "raw_distance.exr"), raw / "distance.exr")
        if dims is not None:
            make_sample(processed, dims=dims, n_pts=1500 + 211 * k, seed=seed + k)
        if rows is not None:
            for sigma, n in zip(("0.10", "0.01"), rows[name]):
                np.savez(processed / f"occupancy_{sigma}", points=rng.uniform(-0.5, 0.5, size=(n, 3)), occupancies=rng.random(n) < 0.4)
    (root / "splits" / splitsdir).mkdir(parents=True)
    for split, items in splits.items():
        (root / "splits" / splitsdir / f"{split}.txt").write_text("\n".join(items) + "\n")
    return root
