"""Vertex-clustering timings on the meshes tools/bench_mesh.py times: marching cubes of the random-weight
IFNet's lattice at res_increase 1 (139 x 104 x 112) and 2 (278 x 208 x 224), 3 % occupied input.  Per lattice and per cell
of 1, 2 and 4 grid cells (multiplied by res_increase, as Reconstruction.simplify does): V and F before and after; the device
time of svr_mesh_simplify_count + svr_mesh_simplify_emit through the C ABI with the wave-folded and with the per-lane sums
path; ``simplify_mesh`` on the host clock (workspace and output allocation and the totals' read-back included); the .obj write
time and file size before and after; and, for scale, marching cubes on the same lattice.  Also checks the device result
against the numpy oracle bit for bit.  Writes profiles/mesh_simplify.json.

Device times: HIP events around `batch` back-to-back count + emit pairs, divided by `batch` (one pair is tens of
microseconds of kernels, less than an event pair resolves); the two paths alternate batch by batch inside one loop, after a
warm-up of both; the median, minimum and maximum over `reps` batches are kept.

    python tools/bench_mesh_simplify.py [--reps 30] [--batch 20] [--out profiles/mesh_simplify.json]
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
from svr_amd.util.mesh_simplify import simplify_mesh  # noqa: E402
from svr_amd.util.visualize import export_obj, marching_cubes  # noqa: E402

DIMS = (139, 104, 112)
CELLS = (1.0, 2.0, 4.0)


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


def _alternating_events_ms(fns, reps, batch):
    """{name: stats of ms per call}: per repetition one batch of each function, in turn."""
    for fn in fns.values():
        for _ in range(batch):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / batch)
    return {name: _stats(t) for name, t in out.items()}


def measure(v, f, cell, reps, batch, tmp):
    from tests import mesh_simplify_oracle as O
    l = _lib.lib()
    V, F = int(v.shape[0]), int(f.shape[0])
    ws_bytes = int(l.svr_mesh_simplify_workspace_bytes(V, F))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    totals = torch.empty(3, device="cuda", dtype=torch.int64)

    def count(uniform):
        check(l.svr_mesh_simplify_count(ptr(v), V, ptr(f), F, cell, ptr(ws), ws_bytes, uniform, ptr(totals), stream()), "count")

    count(1)
    nv, nf, bad = totals.tolist()
    ov, of = torch.empty((nv, 3), device="cuda"), torch.empty((nf, 3), device="cuda", dtype=torch.int32)
    oc, osz = torch.empty(V, device="cuda", dtype=torch.int32), torch.empty(nv, device="cuda", dtype=torch.int32)

    def both(uniform):
        count(uniform)
        check(l.svr_mesh_simplify_emit(ptr(v), V, ptr(f), F, ptr(ws), ws_bytes, ptr(ov), ptr(of), ptr(oc), ptr(osz), stream()), "emit")

    res = {"cell": cell, "V": V, "F": F, "V_after": nv, "F_after": nf, "bad": bad, "workspace_bytes": ws_bytes, "reps": reps, "batch": batch}
    ev = _alternating_events_ms({"wave_folded": lambda: both(1), "per_lane": lambda: both(0), "count_only_wave_folded": lambda: count(1)},
                                reps, batch)
    res["count_emit_wave_folded_events_ms"], res["count_emit_per_lane_events_ms"] = ev["wave_folded"], ev["per_lane"]
    res["count_wave_folded_events_ms"] = ev["count_only_wave_folded"]
    res["simplify_mesh_wall_ms"] = _wall_ms(lambda: simplify_mesh(v, f, cell), reps)

    got = simplify_mesh(v, f, cell)
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    t = time.perf_counter()
    want = O.simplify(hv, hf, cell)
    res["numpy_oracle_ms"] = (time.perf_counter() - t) * 1e3
    res["equal_to_oracle"] = bool(
        np.array_equal(got.vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32))
        and np.array_equal(got.faces.cpu().numpy(), want.faces) and np.array_equal(got.vertex_cluster.cpu().numpy(), want.vertex_cluster)
        and np.array_equal(got.cluster_size.cpu().numpy(), want.cluster_size) and got.bad == want.bad)
    sv, sf = got.vertices.cpu().numpy(), got.faces.cpu().numpy()
    path = os.path.join(tmp, "after.obj")
    res["export_obj_after_ms"] = _wall_ms(lambda: export_obj(sv, sf, path), max(3, reps // 6), warmup=1)
    res["obj_bytes_after"] = os.path.getsize(path)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_mesh_simplify needs a GPU"
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
        path = os.path.join(tmp, "before.obj")
        row = {"lattice": list(field.shape), "res_increase": ri, "level": level, "V": int(v.shape[0]), "F": int(f.shape[0]),
               "marching_cubes_wall_ms": _wall_ms(lambda: marching_cubes(field, level), a.reps),
               "export_obj_before_ms": _wall_ms(lambda: export_obj(hv, hf, path), max(3, a.reps // 6), warmup=1),
               "obj_bytes_before": os.path.getsize(path), "cells": []}
        for cells in CELLS:
            r = measure(v, f, cells * ri, a.reps, a.batch, tmp)
            r["grid_cells"] = cells
            row["cells"].append(r)
            print(json.dumps({"res_increase": ri, **r}), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
    return 0 if all(r["equal_to_oracle"] for row in rows for r in row["cells"]) else 1


if __name__ == "__main__":
    sys.exit(main())
