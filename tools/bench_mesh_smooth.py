"""Mesh-smoothing timings and quality on the meshes tools/bench_mesh.py and tools/bench_mesh_simplify.py
time: marching cubes of the random-weight IFNet's lattice at res_increase 1 (139 x 104 x 112) and 2 (278 x 208 x 224), 3 %
occupied input.  Per mesh, with and without `fix_boundary`: the device time of svr_mesh_smooth through the C ABI at 0, 1, 10
and 30 iterations (0 is the index build alone: prepare, count, scan, fill, classify, finish), the time of one pass derived
from the 10- and 30-iteration figures ((t30 - t10) / 40: the default weights run two passes per iteration), the four state
counts, ``smooth_mesh`` on the host clock (allocations and the counts' read-back included), and a bit-for-bit check against the
numpy oracle at 10 iterations; for scale, marching cubes and the .obj write of the same mesh.  Quality: radial RMS error,
normal consistency and enclosed volume before and after 10 default iterations, and after 10 plain Laplacian ones (mu = 0), on
the binary spheres of radius 8 on 24^3 and 11.3 on 32^3 meshed on the device at level 0.5.  Writes profiles/mesh_smooth.json.

Device times: HIP events around `batch` back-to-back calls, divided by `batch`; the median, minimum and maximum over `reps`
batches, after a warm-up batch; one process.

    python tools/bench_mesh_smooth.py [--reps 30] [--batch 20] [--out profiles/mesh_smooth.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import svr_amd  # noqa: E402,F401
from svr_amd import _lib  # noqa: E402
from svr_amd._lib import check, ptr, stream  # noqa: E402
from svr_amd.util.mesh_smooth import smooth_mesh  # noqa: E402
from svr_amd.util.visualize import export_obj, marching_cubes  # noqa: E402

DIMS = (139, 104, 112)
ITERATIONS = (0, 1, 10, 30)
LAM, MU = 0.5, -0.53
SPHERES = ((24, 8.0), (32, 11.3))


def _stats(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def _wall_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return _stats(out)


def _events_ms(fn, reps, batch):
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / batch)
    return _stats(out)


def measure(v, f, fix_boundary, reps, batch):
    from tests import mesh_smooth_oracle as O
    l = _lib.lib()
    V, F = int(v.shape[0]), int(f.shape[0])
    ws_bytes = int(l.svr_mesh_smooth_workspace_bytes(V, F))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    out, state = torch.empty((V, 3), device="cuda"), torch.empty(V, device="cuda", dtype=torch.uint8)
    counts = torch.empty(4, device="cuda", dtype=torch.int64)

    def call(n):
        check(l.svr_mesh_smooth(ptr(v), V, ptr(f), F, n, LAM, MU, fix_boundary, ptr(ws), ws_bytes, ptr(out), ptr(state), ptr(counts), stream()),
              "mesh_smooth")

    res = {"fix_boundary": bool(fix_boundary), "V": V, "F": F, "workspace_bytes": ws_bytes, "reps": reps, "batch": batch, "lam": LAM, "mu": MU}
    for n in ITERATIONS:
        res[f"events_ms_n{n}"] = _events_ms(lambda: call(n), reps, batch)
    res["states_moved_isolated_fixed_bad"] = counts.tolist()
    res["index_build_ms"] = res["events_ms_n0"]["median"]
    res["per_pass_ms"] = (res["events_ms_n30"]["median"] - res["events_ms_n10"]["median"]) / 40.0
    res["smooth_mesh_wall_ms_n10"] = _wall_ms(lambda: smooth_mesh(v, f, 10, LAM, MU, bool(fix_boundary)), reps)
    got = smooth_mesh(v, f, 10, LAM, MU, bool(fix_boundary))
    t = time.perf_counter()
    want = O.smooth(v.cpu().numpy(), f.cpu().numpy(), 10, LAM, MU, bool(fix_boundary))
    res["numpy_oracle_ms_n10"] = (time.perf_counter() - t) * 1e3
    res["equal_to_oracle"] = bool(np.array_equal(got.vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32))
                                  and np.array_equal(got.state.cpu().numpy(), want.state)
                                  and [got.moved, got.isolated, got.fixed, got.bad] == want.counts.tolist())
    return res


def quality(n, r):
    from tests import mc_oracle
    from tests import mesh_smooth_oracle as O
    field = torch.from_numpy((mc_oracle.sphere(n, r) > 0).astype(np.float32)).cuda()
    v, f = marching_cubes(field, 0.5)
    c = ((n - 1) / 2.0,) * 3
    hf = f.cpu().numpy()
    as_dict = lambda q: {"radial_rms": q.rms, "normal_consistency": q.normal_consistency, "volume": q.volume}   # noqa: E731
    row = {"lattice": n, "radius": r, "level": 0.5, "V": int(v.shape[0]), "F": int(f.shape[0]), "iterations": 10,
           "before": as_dict(O.sphere_quality(v.cpu().numpy(), hf, c, r))}
    for name, mu in (("taubin", MU), ("laplacian_mu0", 0.0)):
        got = smooth_mesh(v, f, 10, LAM, mu)
        row[name] = as_dict(O.sphere_quality(got.vertices.cpu().numpy(), hf, c, r))
        row[name]["volume_change"] = row[name]["volume"] / row["before"]["volume"] - 1.0
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_mesh_smooth needs a GPU"
    from oracle import ifnet_oracle as IO
    from svr_amd.model import IFNet, evaluate_network_on_grid_device
    m = IFNet(net_res=128)
    m.load_state_dict(IO.name_seeded_state(128), strict=False)
    m = m.cuda().eval()
    x = (torch.rand(1, 1, *DIMS, generator=torch.Generator().manual_seed(0)) < 0.03).float().cuda()
    rows = []
    tmp = tempfile.mkdtemp()
    for ri in (1, 2):
        with torch.no_grad():
            field = 1 - evaluate_network_on_grid_device(m, x, DIMS, ri)
        level = 0.5
        v, f = marching_cubes(field, level)
        if f.shape[0] == 0:            # random weights: the level tools/bench_mesh.py falls back to
            level = float(field.view(-1)[::97].median())
            v, f = marching_cubes(field, level)
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        path = os.path.join(tmp, "mesh.obj")
        row = {"lattice": list(field.shape), "res_increase": ri, "level": level, "V": int(v.shape[0]), "F": int(f.shape[0]),
               "marching_cubes_wall_ms": _wall_ms(lambda: marching_cubes(field, level), a.reps),
               "export_obj_ms": _wall_ms(lambda: export_obj(hv, hf, path), max(3, a.reps // 6), warmup=1), "modes": []}
        for fix in (1, 0):
            r = measure(v, f, fix, a.reps, a.batch)
            row["modes"].append(r)
            print(json.dumps({"res_increase": ri, **r}), flush=True)
        rows.append(row)
    spheres = [quality(n, r) for n, r in SPHERES]
    for s in spheres:
        print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"meshes": rows, "spheres": spheres,
                   "not_measured": "one step-kernel form only (a thread per vertex, 32-byte rows); no hardware counters; no mesh beyond 10^5 vertices"},
                  fh, indent=1)
    return 0 if all(r["equal_to_oracle"] for row in rows for r in row["modes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
