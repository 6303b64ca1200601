"""Mesh output timings at the inference lattices (139 x 104 x 112 and res_increase 2: 278 x 208 x 224): the dense-grid
evaluation, marching cubes on the device, implicit_to_mesh end to end and the .obj write, with V and F.  One JSON
object per lattice on stdout (--out FILE: also written there).  Random-weight IFNet, 3 % occupied input.

The kernel / scan split comes from a run under `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py`."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import svr_amd  # noqa: E402,F401
from oracle import ifnet_oracle as O  # noqa: E402
from svr_amd.model import IFNet, evaluate_network_on_grid, evaluate_network_on_grid_device, implicit_to_mesh  # noqa: E402
from svr_amd.util.visualize import export_obj, marching_cubes  # noqa: E402

DIMS = (139, 104, 112)


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = IFNet(net_res=128)
    m.load_state_dict(O.name_seeded_state(128), strict=False)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(1, 1, *DIMS, generator=g) < 0.03).float().cuda()
    rows = []
    tmp = tempfile.mkdtemp()
    for ri in (1, 2):
        field = 1 - evaluate_network_on_grid_device(m, x, DIMS, ri)
        v, f = marching_cubes(field, 0.5)
        level = 0.5
        if f.shape[0] == 0:            # random weights: use a level that gives a surface as large as a trained net's
            level = float(field.view(-1)[::97].median())
            v, f = marching_cubes(field, level)
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        path = os.path.join(tmp, f"m{ri}.obj")
        r = {
            "lattice": list(field.shape), "points": field.numel(), "level": level, "V": int(v.shape[0]), "F": int(f.shape[0]),
            "evaluate_network_on_grid_ms": wall(lambda: evaluate_network_on_grid(m, x, DIMS, ri), a.reps),
            "evaluate_network_on_grid_device_ms": wall(lambda: evaluate_network_on_grid_device(m, x, DIMS, ri), a.reps),
            "marching_cubes_ms": wall(lambda: marching_cubes(field, level), a.reps),
            "implicit_to_mesh_ms": wall(lambda: implicit_to_mesh(m, x, DIMS, level, path, ri), a.reps),
            "export_obj_ms": wall(lambda: export_obj(hv, hf, path), a.reps),
            "obj_bytes": os.path.getsize(path),
        }
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
