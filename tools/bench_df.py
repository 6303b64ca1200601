"""Distance-field timings at the real shape: the reference sample's mesh (tests/golden/scene_mesh_00000.npz, 45 172
faces) on the 139 x 104 x 112 lattice.  HIP events around the three phases of data_processing.mesh_to_df -- the cull sweep
(svr_mesh_df_count: dmin, counts, scan), the emit of the candidate lists and the exact kernel -- for brick 4 and 8, with
the candidate-list statistics (mean / max per brick, total bytes, batches); and the brute-force baseline (cull=False: the
exact kernel with every face as a candidate of every brick), on the full lattice or on its 1/8 sub-lattice
(70 x 52 x 56).  Results are merged into one JSON file (default profiles/mesh_df.json), one key per mode, so the modes
can run as separate commands, each under its own time limit:

    python tools/bench_df.py --mode culled
    python tools/bench_df.py --mode brute --lattice sub
    python tools/bench_df.py --mode brute --lattice full      # limit: the sub-lattice time x 8 (the pair-count ratio) x 3
"""
import argparse
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
from svr_amd.data_processing import mesh_to_df as M  # noqa: E402

DIMS = (139, 104, 112)
SUB = (70, 52, 56)


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def culled_once(tri, host_tri, dims, brick, budget):
    """One pass of the driver's loop with events between the phases -> (phase ms, list statistics, field)."""
    l = _lib.lib()
    X, Y, Z = dims
    F = tri.shape[0]
    nb = int(l.svr_mesh_df_bricks(X, Y, Z, brick))
    ws_bytes = int(l.svr_mesh_df_workspace_bytes(X, Y, Z, brick))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    offsets = torch.empty(nb + 1, device="cuda", dtype=torch.int64)
    field = torch.empty(dims, device="cuda", dtype=torch.float32)
    slack = M.cull_slack(host_tri, dims)
    ms = {"cull_sweep": 0.0, "emit": 0.0, "exact": 0.0}
    e0 = _event()
    check(l.svr_mesh_df_count(ptr(tri), F, X, Y, Z, brick, 0.0, slack, ptr(ws), ws_bytes, ptr(offsets), stream()), "count")
    e1 = _event()
    host_off = offsets.cpu().numpy()
    ms["cull_sweep"] = e0.elapsed_time(e1)
    batches = M.plan_batches(host_off, budget)
    marks = []
    for b0, b1 in batches:
        n = int(host_off[b1] - host_off[b0])
        lst = torch.empty(max(n, 1), device="cuda", dtype=torch.int32)
        a = _event()
        check(l.svr_mesh_df_emit(ptr(tri), F, X, Y, Z, brick, ptr(ws), ptr(offsets), b0, b1, ptr(lst), n, stream()), "emit")
        b = _event()
        check(l.svr_mesh_df_eval(ptr(tri), F, X, Y, Z, brick, 0.0, ptr(offsets), ptr(lst), b0, b1, ptr(field), None, stream()), "eval")
        marks.append((a, b, _event()))
    torch.cuda.synchronize()
    for a, b, c in marks:
        ms["emit"] += a.elapsed_time(b)
        ms["exact"] += b.elapsed_time(c)
    per = np.diff(host_off)
    lists = {"bricks": nb, "mean_per_brick": float(per.mean()), "max_per_brick": int(per.max()), "total_entries": int(host_off[-1]),
             "total_bytes": int(host_off[-1]) * 4, "batches": len(batches),
             "exact_pair_tests": int(host_off[-1]) * brick ** 3}           # partial bricks counted whole
    return ms, lists, field


def median_of(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def load_mesh():
    z = np.load(os.path.join(ROOT, "tests", "golden", "scene_mesh_00000.npz"))
    host_tri = M.triangle_table((z["vertices"], z["faces"]))
    return host_tri, torch.from_numpy(host_tri).cuda()


def mode_culled(a):
    host_tri, tri = load_mesh()
    out = {"lattice": list(DIMS), "faces": int(tri.shape[0]), "points": int(np.prod(DIMS)), "list_budget_bytes": a.budget, "reps": a.reps}
    fields = {}
    for brick in (4, 8):
        culled_once(tri, host_tri, DIMS, brick, a.budget)                      # warm-up: code objects, allocator
        rows = []
        for _ in range(a.reps):
            ms, lists, field = culled_once(tri, host_tri, DIMS, brick, a.budget)
            rows.append(ms)
        med = median_of(rows)
        med["total"] = sum(med.values())
        t0 = time.perf_counter()
        M.mesh_distance_field(vertices_and_faces(), DIMS, brick=brick)
        torch.cuda.synchronize()
        out[f"brick{brick}"] = {"phase_ms": med, "lists": lists, "mesh_distance_field_wall_ms": (time.perf_counter() - t0) * 1e3}
        fields[brick] = field
        print(json.dumps({f"brick{brick}": out[f"brick{brick}"]}), flush=True)
    out["brick4_equals_brick8"] = bool(torch.equal(fields[4], fields[8]))
    out["field_min_max"] = [float(fields[8].min()), float(fields[8].max())]
    return out


def vertices_and_faces():
    z = np.load(os.path.join(ROOT, "tests", "golden", "scene_mesh_00000.npz"))
    return z["vertices"], z["faces"]


def mode_brute(a):
    host_tri, tri = load_mesh()
    dims = SUB if a.lattice == "sub" else DIMS
    l = _lib.lib()
    F = tri.shape[0]
    rows = {}
    fields = {}
    for brick in ((8,) if a.lattice == "full" else (8, 4)):
        nb = int(l.svr_mesh_df_bricks(*dims, brick))
        field = torch.empty(dims, device="cuda", dtype=torch.float32)
        run = lambda: check(l.svr_mesh_df_eval(ptr(tri), F, *dims, brick, 0.0, None, None, 0, nb, ptr(field), None, stream()), "eval")  # noqa: E731
        if a.lattice == "sub":
            run()                                                              # warm-up (the full lattice runs once, cold)
        e0 = _event()
        run()
        e1 = _event()
        e1.synchronize()
        rows[f"brick{brick}_ms"] = e0.elapsed_time(e1)
        fields[brick] = field
    # the culled run at the same shape: the same bits, and the time to compare with
    ms, lists, culled = culled_once(tri, host_tri, dims, 8, a.budget)
    ms, lists, culled = culled_once(tri, host_tri, dims, 8, a.budget)
    rows.update({"lattice": list(dims), "pair_tests": int(np.prod(dims)) * F, "culled_brick8_phase_ms": ms,
                 "culled_brick8_total_ms": sum(ms.values()), "culled_equals_brute_force": bool(torch.equal(culled, fields[8]))})
    rows["speedup_brick8"] = rows["brick8_ms"] / rows["culled_brick8_total_ms"]
    print(json.dumps(rows), flush=True)
    return rows


def mode_resources():
    """The compiler's register / scratch report of csrc/mesh_df.hip's kernels (build.resource_usage(): no GPU needed)."""
    import importlib
    b = importlib.import_module("single-view-3d-reconstruction_amd.build")
    short = {"df_valid_kernel": "df_valid_kernel", "df_cull_count_kernel": "df_cull_count_kernel", "df_emit_kernel": "df_emit_kernel",
             "df_eval_kernelILi8ELi256ELi2": "df_eval_kernel<8, 256, 2>", "df_eval_kernelILi4ELi64ELi1": "df_eval_kernel<4, 64, 1>"}
    out = {}
    for name, v in b.resource_usage().items():
        for k, label in short.items():
            if v["file"] == "mesh_df.hip" and k in name:
                out[label] = {x: v[x] for x in ("vgprs", "agprs", "scratch", "occupancy") if x in v}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("culled", "brute", "resources"), default="culled")
    ap.add_argument("--lattice", choices=("sub", "full"), default="sub")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=int, default=M.DEFAULT_LIST_BUDGET)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_df.json"))
    a = ap.parse_args()
    if a.mode == "resources":
        key, res = "kernel_resources", mode_resources()
    else:
        assert torch.cuda.is_available(), "bench_df needs a GPU"
        key = "culled" if a.mode == "culled" else f"brute_force_{a.lattice}"
        res = mode_culled(a) if a.mode == "culled" else mode_brute(a)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc[key] = res
    doc["default_brick"] = M.DEFAULT_BRICK
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
