"""Ray-caster timings at the real shape: the reference sample's mesh (tests/golden/scene_mesh_00000.npz, 45 172 faces)
seen at 240 x 320 through the default intrinsic.  HIP events around the phases of data_processing.render_view -- the face
rectangles, the count + scan, the emit of the candidate lists and the exact kernel -- for tile 8 and 16, medians of 9
passes after a warm-up pass, with the candidate-list statistics (mean / max per tile, total bytes); the brute-force
baseline (cull=False: the exact kernel with every face as a candidate of every tile) beside them, and whether the two
agree bit for bit.  Writes profiles/render_view.json.

    python tools/bench_render.py [--reps 9] [--out profiles/render_view.json]
    python tools/bench_render.py --mode resources      # the compiler's register report only: no GPU needed
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import svr_amd  # noqa: E402,F401
from svr_amd import _lib  # noqa: E402
from svr_amd._lib import check, ptr, stream  # noqa: E402
from svr_amd.data_processing import render_view as R  # noqa: E402
from svr_amd.data_processing.mesh_to_df import plan_batches, triangle_table  # noqa: E402

SIZE = (240, 320)
MAPS = ("depth", "face", "distance", "normal", "shade")


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _maps():
    H, W = SIZE
    return [torch.empty((H, W), device="cuda", dtype=torch.float32), torch.empty((H, W), device="cuda", dtype=torch.int32),
            torch.empty((H, W), device="cuda", dtype=torch.float32), torch.empty((H, W, 3), device="cuda", dtype=torch.float32),
            torch.empty((H, W), device="cuda", dtype=torch.uint8)]


def _eval(l, tri, kc, tile, offsets, lst, b0, b1, maps):
    H, W = SIZE
    check(l.svr_raycast_eval(ptr(tri), tri.shape[0], kc, H, W, tile, 0.0, float("inf"), 0.0, ptr(offsets), ptr(lst), b0, b1,
                             *[ptr(m) for m in maps], stream()), "eval")


def culled_once(tri, kc, tile, budget):
    """One pass of the driver's loop with events between the phases -> (phase ms, list statistics, maps)."""
    l = _lib.lib()
    H, W = SIZE
    F = tri.shape[0]
    nt = int(l.svr_raycast_tiles(H, W, tile))
    ws_bytes = int(l.svr_raycast_workspace_bytes(H, W, tile))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    rects = torch.empty((F, 4), device="cuda", dtype=torch.int32)
    offsets = torch.empty(nt + 1, device="cuda", dtype=torch.int64)
    maps = _maps()
    e0 = _event()
    check(l.svr_raycast_face_bounds(ptr(tri), F, kc, ptr(rects), stream()), "face_bounds")
    e1 = _event()
    check(l.svr_raycast_count(ptr(rects), F, H, W, tile, ptr(ws), ws_bytes, ptr(offsets), stream()), "count")
    e2 = _event()
    host_off = offsets.cpu().numpy()
    ms = {"face_bounds": e0.elapsed_time(e1), "count_scan": e1.elapsed_time(e2), "emit": 0.0, "exact": 0.0}
    batches = plan_batches(host_off, budget)
    marks = []
    for b0, b1 in batches:
        n = int(host_off[b1] - host_off[b0])
        lst = torch.empty(max(n, 1), device="cuda", dtype=torch.int32)
        a = _event()
        check(l.svr_raycast_emit(ptr(rects), F, H, W, tile, ptr(offsets), b0, b1, ptr(lst), n, stream()), "emit")
        b = _event()
        _eval(l, tri, kc, tile, offsets, lst, b0, b1, maps)
        marks.append((a, b, _event()))
    torch.cuda.synchronize()
    for a, b, c in marks:
        ms["emit"] += a.elapsed_time(b)
        ms["exact"] += b.elapsed_time(c)
    per = np.diff(host_off)
    lists = {"tiles": nt, "mean_per_tile": float(per.mean()), "max_per_tile": int(per.max()), "total_entries": int(host_off[-1]),
             "total_bytes": int(host_off[-1]) * 4, "batches": len(batches), "every_tile_faces": int((rects[:, 0] == -(1 << 30)).sum().item()),
             "exact_pair_tests": int(host_off[-1]) * tile * tile}              # partial tiles counted whole
    return ms, lists, maps


def brute_once(tri, kc, tile):
    l = _lib.lib()
    nt = int(l.svr_raycast_tiles(*SIZE, tile))
    maps = _maps()
    e0 = _event()
    _eval(l, tri, kc, tile, None, None, 0, nt, maps)
    e1 = _event()
    e1.synchronize()
    return e0.elapsed_time(e1), maps


def median_of(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def load_mesh():
    z = np.load(os.path.join(ROOT, "tests", "golden", "scene_mesh_00000.npz"))
    return z["vertices"], z["faces"]


def mode_run(a):
    V, F = load_mesh()
    tri = torch.from_numpy(triangle_table((V, F))).cuda()
    kc = (C.c_float * 12)(*[float(v) for v in R.view_consts()])
    out = {"size": list(SIZE), "faces": int(tri.shape[0]), "pixels": SIZE[0] * SIZE[1], "list_budget_bytes": a.budget, "reps": a.reps,
           "pair_tests_brute_force": SIZE[0] * SIZE[1] * int(tri.shape[0])}
    kept = {}
    for tile in (8, 16):
        culled_once(tri, kc, tile, a.budget)                                   # warm-up: code objects, allocator
        rows = []
        for _ in range(a.reps):
            ms, lists, maps = culled_once(tri, kc, tile, a.budget)
            rows.append(ms)
        med = median_of(rows)
        med["total"] = sum(med.values())
        brute_once(tri, kc, tile)
        times = []
        for _ in range(a.brute_reps):
            t, bmaps = brute_once(tri, kc, tile)
            times.append(t)
        same = all(torch.equal(x, y) for x, y in zip(maps, bmaps))
        t0 = time.perf_counter()
        R.render_depth((V, F), size=SIZE, tile=tile, return_distance=True)
        torch.cuda.synchronize()
        out[f"tile{tile}"] = {"phase_ms": med, "lists": lists, "brute_force_ms": float(np.median(times)),
                              "speedup": float(np.median(times)) / med["total"], "culled_equals_brute_force": bool(same),
                              "render_depth_wall_ms": (time.perf_counter() - t0) * 1e3}
        kept[tile] = maps
        print(json.dumps({f"tile{tile}": out[f"tile{tile}"]}), flush=True)
    out["tile8_equals_tile16"] = all(torch.equal(x, y) for x, y in zip(kept[8], kept[16]))
    out["culled_equals_brute_force"] = bool(out["tile8"]["culled_equals_brute_force"] and out["tile16"]["culled_equals_brute_force"])
    depth, face = kept[R.DEFAULT_TILE][0], kept[R.DEFAULT_TILE][1]
    hit = face >= 0
    out["hit_share"] = float(hit.float().mean())
    out["depth_min_max"] = [float(depth[hit].min()), float(depth[hit].max())]
    return out


def mode_resources():
    """The compiler's register / scratch report of csrc/raycast.hip's kernels (build.resource_usage(): no GPU needed)."""
    import importlib
    b = importlib.import_module("single-view-3d-reconstruction_amd.build")
    short = {"rc_face_bounds_kernel": "rc_face_bounds_kernel", "rc_count_kernel": "rc_count_kernel", "rc_emit_kernel": "rc_emit_kernel",
             "rc_eval_kernelILi8E": "rc_eval_kernel<8>", "rc_eval_kernelILi16E": "rc_eval_kernel<16>"}
    out = {}
    for name, v in b.resource_usage().items():
        for k, label in short.items():
            if v["file"] == "raycast.hip" and k in name:
                out[label] = {x: v[x] for x in ("vgprs", "agprs", "scratch", "occupancy") if x in v}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("run", "resources"), default="run")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--brute_reps", type=int, default=3)
    ap.add_argument("--budget", type=int, default=R.DEFAULT_LIST_BUDGET)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_view.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    if a.mode == "resources":
        doc["kernel_resources"] = mode_resources()
    else:
        assert torch.cuda.is_available(), "bench_render needs a GPU"
        doc.update(mode_run(a))
    doc["default_tile"] = R.DEFAULT_TILE
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
