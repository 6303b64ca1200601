"""Stage times of process_sample on one raw view: the real distance map (tests/golden/raw_distance.exr, 320 x 240) plus a
synthetic 139 x 104 x 112 distance field (unsigned distance to a sphere of radius 30 voxels), down_scale_factor 1,
100 000 surface samples -- EXR read, depth grid, df -> mesh, each sample_points, the file writes, and process_sample end to
end.  Medians of --reps wall-clock runs with a device synchronisation behind every stage; one JSON object on stdout and in
--out (default profiles/raw_sample_bench.json).

Numbers only, no threshold and no speed-up claim: the reference's CPU path (pyexr, trimesh, the marching_cubes package)
is not available to run next to it."""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import svr_amd  # noqa: E402,F401
from svr_amd.data_processing import sample_io  # noqa: E402
from svr_amd.data_processing.distance_to_depth import depth_grid  # noqa: E402
from svr_amd.data_processing.mesh_occupancies import sample_points  # noqa: E402
from svr_amd.data_processing.process_sample import process_sample  # noqa: E402
from svr_amd.data_processing.volume_reader import read_df  # noqa: E402
from svr_amd.util.visualize import export_obj, marching_cubes  # noqa: E402

DIMS = (139, 104, 112)
INTRINSIC = ("[[277.1281435,   0.       , 159.5,  0.],\n[  0.       , 277.1281435, 119.5,  0.],\n"
             "[  0.       ,   0.       ,   1. ,  0.],\n[  0.       ,   0.       ,   0. ,  1.]]")


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample-num", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "raw_sample_bench.json"))
    a = ap.parse_args()
    root = tempfile.mkdtemp()
    raw = os.path.join(root, "raw", "bench", "00000")
    os.makedirs(raw)
    exr = os.path.join(raw, "distance.exr")
    shutil.copyfile(os.path.join(REPO, "tests", "golden", "raw_distance.exr"), exr)
    intrinsic = os.path.join(raw, "intrinsic.txt")
    with open(intrinsic, "w") as f:
        f.write(INTRINSIC)
    g = np.indices(DIMS).astype(np.float32)
    r = np.sqrt(sum((g[k] - np.float32(DIMS[k] / 2)) ** 2 for k in range(3)))
    dfp = os.path.join(raw, "distance_field.df")
    with open(dfp, "wb") as f:
        f.write(struct.pack("<3Q", *DIMS))
        f.write(np.abs(r - np.float32(30)).astype(np.float32).tobytes(order="F"))

    dist = sample_io.exr_read(exr, "R")
    grid, count = depth_grid(dist, DIMS, intrinsic)
    df = read_df(dfp, 1)
    field = torch.from_numpy(np.ascontiguousarray(df, dtype=np.float32)).cuda()
    v, fc = marching_cubes(field, 1.0)
    mesh = (v.cpu().numpy(), fc.cpu().numpy())
    pts = {s: sample_points(mesh, DIMS, a.sample_num, s) for s in (0.01, 0.1)}
    host = {s: [t.cpu().numpy() for t in p] for s, p in pts.items()}
    grid64 = grid.cpu().numpy().astype(np.float64)
    out = {
        "device": torch.cuda.get_device_name(0), "reps": a.reps, "map": list(dist.shape), "dims": list(DIMS), "sample_num": a.sample_num,
        "ones": int(grid.sum()), "out_of_range": int(count), "V": int(v.shape[0]), "F": int(fc.shape[0]),
        "exr_read_ms": wall(lambda: sample_io.exr_read(exr, "R"), a.reps),
        "depth_grid_ms": wall(lambda: depth_grid(dist, DIMS, intrinsic)[1].item(), a.reps),
        "depth_grid_to_host_f64_ms": wall(lambda: grid.cpu().numpy().astype(np.float64), a.reps),
        "write_depth_grid_npz_ms": wall(lambda: np.savez_compressed(os.path.join(root, "depth_grid"), grid=grid64), a.reps),
        "read_df_ms": wall(lambda: read_df(dfp, 1), a.reps),
        "df_to_mesh_ms": wall(lambda: [t.cpu() for t in marching_cubes(torch.from_numpy(df).cuda(), 1.0)], a.reps),
        "write_obj_ms": wall(lambda: export_obj(mesh[0], mesh[1], os.path.join(root, "mesh.obj")), a.reps),
        "sample_points_0.01_ms": wall(lambda: sample_points(mesh, DIMS, a.sample_num, 0.01), a.reps),
        "sample_points_0.10_ms": wall(lambda: sample_points(mesh, DIMS, a.sample_num, 0.1), a.reps),
        "write_occupancy_npz_ms": wall(lambda: np.savez(os.path.join(root, "occupancy"), points=host[0.1][0], occupancies=host[0.1][1],
                                                        grid_coords=host[0.1][2]), a.reps),
        "process_sample_ms": wall(lambda: process_sample(root, "bench", "00000", sample_num=a.sample_num), max(1, a.reps // 2)),
    }
    shutil.rmtree(root)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
