"""Vertex-colour timings at the real shape: the reference sample's mesh (tests/golden/scene_mesh_00000.npz, 22 588
vertices, 45 172 faces) seen at 240 x 320 through the default intrinsic, coloured from a random image of that size.
The sample kernel (HIP events), the spread to its fixed point for several read-back intervals (host clock: the call ends
in a stream synchronise), the spread's kernels alone (events around exactly the changing passes, no read-back), the whole
``Reconstruction.colorize()`` (render included), each a median after a warm-up, and the numpy oracle's time on the same
box for orientation.  Also checks the device result against the oracle bit for bit.  Writes profiles/vertex_color.json.

    python tools/bench_vertex_color.py [--reps 30] [--out profiles/vertex_color.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
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
from svr_amd.reconstruct import Reconstruction  # noqa: E402
from svr_amd.util import mesh_color  # noqa: E402

SIZE = (240, 320)
INTERVALS = (1, 2, 4, 8, 16, 64)


def _median_ms(fn, reps, warmup=3):
    """Host clock around fn() + synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def _median_events_ms(fn, reps, warmup=3, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    out = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_color.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_vertex_color needs a GPU"
    z = np.load(os.path.join(ROOT, "tests", "golden", "scene_mesh_00000.npz"))
    V, F = z["vertices"].astype(np.float32), z["faces"].astype(np.int32)
    consts = R.view_consts()
    image = np.random.default_rng(0).integers(0, 256, size=SIZE + (3,), dtype=np.uint8)
    v, f, img = torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda(), torch.from_numpy(image).cuda()
    depth = R.render_depth((V, F), size=SIZE, consts=consts)
    l = _lib.lib()
    nV, nF = len(V), len(F)
    kc = (C.c_float * 12)(*[float(x) for x in consts])
    pm, fill = (C.c_double * 4)(1.0, 0.0, 1.0, 0.0), (C.c_uint8 * 3)(128, 128, 128)
    bias = 1.0 / float(consts[7])
    colors0 = torch.empty((nV, 3), device="cuda", dtype=torch.uint8)
    state0 = torch.empty((nV,), device="cuda", dtype=torch.uint8)

    def sample():
        check(l.svr_vertex_color_sample(ptr(v), nV, kc, ptr(depth), SIZE[0], SIZE[1], bias, ptr(img), SIZE[0], SIZE[1], pm, fill,
                                        ptr(colors0), ptr(state0), stream()), "sample")

    res = {"mesh": "tests/golden/scene_mesh_00000.npz", "vertices": nV, "faces": nF, "size": list(SIZE), "reps": a.reps,
           "bias_m": bias}
    res["sample_kernel_ms"] = dict(zip(("median", "min", "max"), _median_events_ms(sample, a.reps)))
    n = np.bincount(state0.cpu().numpy(), minlength=3)
    res["seen"], res["hidden_after_sample"] = int(n[1]), int(n[0])

    ws_bytes = int(l.svr_vertex_color_workspace_bytes(nV))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    colors, state = colors0.clone(), state0.clone()
    passes = C.c_int64(0)

    def reset():
        colors.copy_(colors0)
        state.copy_(state0)

    def spread(limit, every):
        check(l.svr_vertex_color_spread(ptr(f), nF, nV, ptr(colors), ptr(state), ptr(ws), ws_bytes, limit, every, C.byref(passes),
                                        stream()), "spread")

    reset()
    spread(-1, 1)
    changing = int(passes.value) - 1
    n = np.bincount(state.cpu().numpy(), minlength=3)
    res["spread"] = {"changing_passes": changing, "spread_vertices": int(n[2]), "unreached": int(n[0]), "by_interval": {}}
    for every in INTERVALS:
        times = []
        for i in range(a.reps + 3):
            reset()
            torch.cuda.synchronize()
            t = time.perf_counter()
            spread(-1, every)
            torch.cuda.synchronize()
            if i >= 3:
                times.append((time.perf_counter() - t) * 1e3)
        res["spread"]["by_interval"][str(every)] = {"passes_launched": int(passes.value), "wall_ms_median": statistics.median(times),
                                                    "wall_ms_min": min(times), "wall_ms_max": max(times)}
    # the kernels alone: exactly the changing passes, max_passes set, so the host never reads the counter back
    med, lo, hi = _median_events_ms(lambda: spread(changing, 10 ** 6), a.reps, before=reset)
    res["spread"]["kernels_only_ms"] = {"median": med, "min": lo, "max": hi, "passes": changing, "per_pass_ms": med / max(changing, 1)}
    final_c, final_s = colors.cpu().numpy(), state.cpu().numpy()

    rec = Reconstruction(torch.ones(SIZE, device="cuda"), None, None, v, f, 1, 1, [float(x) for x in consts[3:9]], None, img)
    res["colorize_wall_ms"] = dict(zip(("median", "min", "max"), _median_ms(lambda: rec.colorize(), a.reps)))
    res["render_depth_wall_ms"] = dict(zip(("median", "min", "max"), _median_ms(lambda: rec.render_depth(), a.reps)))
    res["readback_interval_default"] = mesh_color.READBACK_INTERVAL
    same_api = bool(np.array_equal(rec.colors.cpu().numpy(), final_c) and np.array_equal(rec.color_state.cpu().numpy(), final_s))

    from tests import vertex_color_oracle as O
    d = depth.cpu().numpy()
    t = time.perf_counter()
    oc, os_ = O.sample(V, consts, d, bias, image)
    t1 = time.perf_counter()
    oc, os_, opasses = O.spread(F, oc, os_)
    t2 = time.perf_counter()
    res["numpy_oracle_ms"] = {"sample": (t1 - t) * 1e3, "spread": (t2 - t1) * 1e3, "changing_passes": opasses}
    res["equal_to_oracle"] = bool(np.array_equal(oc, final_c) and np.array_equal(os_, final_s) and opasses == changing)
    res["colorize_equals_direct_calls"] = same_api
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0 if res["equal_to_oracle"] and same_api else 1


if __name__ == "__main__":
    sys.exit(main())
