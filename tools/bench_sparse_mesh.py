"""Dense against block-sparse implicit_to_mesh on the random-weight IFNet and the 3 % occupied input
of tools/bench_mesh.py, at the inference lattices 139 x 104 x 112 and 278 x 208 x 224 and block edges 4, 8, 16.  One
process; every repetition runs the dense path and then each block edge, and the medians are reported.  One JSON object per
lattice on stdout (--out FILE: also written there).

Per block edge: implicit_to_mesh and lattice-evaluation wall time, the evaluated fraction (points the network was queried
on / lattice points, coarse points included), rounds, per-round leak counts, host reads, and -- from one more run with HIP
events around every library call and every query -- the time of the svr_sl_* kernels apart from the queries.
`expected_grid_ms` = dense lattice time x evaluated fraction + bookkeeping: what the sparse lattice evaluation should cost
if a query's price per point did not change; the host reads (one per round) come on top.

--input shell: a sphere-shell occupancy instead of the random 3 % (a surface-like pyramid; the weights stay random)."""
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
from svr_amd.model import IFNet, evaluate_network_on_grid_device, evaluate_network_on_grid_sparse, implicit_to_mesh  # noqa: E402
from svr_amd.util.visualize import marching_cubes  # noqa: E402

DIMS = (139, 104, 112)
BLOCKS = (4, 8, 16)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--input", choices=("random", "shell"), default="random")
    a = ap.parse_args()
    m = IFNet(net_res=128)
    m.load_state_dict(O.name_seeded_state(128), strict=False)
    m = m.cuda().eval()
    if a.input == "random":
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(1, 1, *DIMS, generator=g) < 0.03).float().cuda()
    else:
        ax = [torch.arange(n, dtype=torch.float64) - (n - 1) / 2 for n in DIMS]
        d = torch.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
        x = ((d - 36.0).abs() < 0.8).float().reshape(1, 1, *DIMS).cuda()
    rows = []
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "m.obj")
    for ri in (1, 2):
        dense = 1 - evaluate_network_on_grid_device(m, x, DIMS, ri)
        level = 0.5
        dv, df = marching_cubes(dense, level)
        if df.shape[0] == 0:           # random weights: use a level that gives a surface (tools/bench_mesh.py does the same)
            level = float(dense.view(-1)[::97].median())
            dv, df = marching_cubes(dense, level)
        runs = {"dense": lambda: implicit_to_mesh(m, x, DIMS, level, path, ri, block=0),
                "dense_grid": lambda: evaluate_network_on_grid_device(m, x, DIMS, ri)}
        for s in BLOCKS:
            runs[f"s{s}"] = lambda s=s: implicit_to_mesh(m, x, DIMS, level, path, ri, block=s)
            runs[f"s{s}_grid"] = lambda s=s: evaluate_network_on_grid_sparse(m, x, DIMS, level, ri, block=s)
        for fn in runs.values():       # warm-up: allocator pools, lazy kernel loads
            fn()
        ts = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                ts[k].append(timed(fn))
        r = {"input": a.input, "lattice": list(dense.shape), "points": dense.numel(), "level": level, "V": int(dv.shape[0]),
             "F": int(df.shape[0]), "reps": a.reps, "dense_implicit_to_mesh_ms": median(ts["dense"]),
             "dense_grid_ms": median(ts["dense_grid"]), "blocks": {}}
        for s in BLOCKS:
            res = evaluate_network_on_grid_sparse(m, x, DIMS, level, ri, block=s, profile=True)
            sv, sf = marching_cubes(res.field, level)
            ev = res.state != 0
            frac = res.evaluated_fraction
            book = res.timings.get("bookkeeping_ms", 0.0)
            r["blocks"][str(s)] = {
                "implicit_to_mesh_ms": median(ts[f"s{s}"]), "grid_ms": median(ts[f"s{s}_grid"]),
                "evaluated_fraction": frac, "blocks_evaluated": int(ev.sum()), "blocks_total": ev.numel(), "rounds": res.rounds,
                "leaks": res.leaks, "fell_back": res.fell_back, "host_reads": res.timings["host_reads"],
                "bookkeeping_kernels_ms": book, "queries_ms": res.timings.get("query_ms", 0.0),
                "expected_grid_ms": median(ts["dense_grid"]) * frac + book,
                "sides_equal_dense": bool(torch.equal(res.field.double() < level, dense.double() < level)),
                "mesh_equals_dense": bool(sv.shape == dv.shape and sf.shape == df.shape and torch.equal(sv, dv) and torch.equal(sf, df)),
                "V": int(sv.shape[0]), "F": int(sf.shape[0])}
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
