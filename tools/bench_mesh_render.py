"""Mesh-preview timings: a marching-cubes sphere meshed on the device at 128^3 (radius 48 cells), seen whole at 240 x 320, at
ssaa 1 and 2.  HIP events around 20 back-to-back calls of each entry point through the C ABI, divided by 20, medians of `reps`
such batches after a warm-up: svr_mesh_vertex_normals (its memset and three kernels), svr_mesh_shade on the ray caster's face
map (flat, smooth, smooth with colours) and svr_box_downsample_rgb8; ``render_mesh`` end to end on the host clock beside them.
Writes profiles/mesh_render.json.

    python tools/bench_mesh_render.py [--reps 15] [--out profiles/mesh_render.json]
    python tools/bench_mesh_render.py --mode resources      # the compiler's register report only: no GPU needed
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
from svr_amd.data_processing.render_view import render_depth  # noqa: E402
from svr_amd.util import mesh_render as M  # noqa: E402
from svr_amd.util.visualize import marching_cubes  # noqa: E402

SIZE = (240, 320)
N, RADIUS, DEPTH = 128, 48.0, 6.0                  # lattice edge, sphere radius in cells, camera distance in metres
CALLS = 20


def sphere_mesh():
    g = torch.arange(N, device="cuda", dtype=torch.float32) - (N - 1) / 2
    field = torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) - RADIUS
    return marching_cubes(field.contiguous(), 0.0)


def camera():
    """The default scale (20 cells per metre), the sphere's centre on the optical axis at DEPTH metres."""
    c = (N - 1) / 2
    return np.array([0.9 * SIZE[1], (SIZE[1] - 1) / 2, (SIZE[0] - 1) / 2, 20.0, c, 20.0, c, 20.0, c - 20.0 * DEPTH, 0, 0, 0], dtype=np.float32)


def timed(fn, reps):
    """Median over `reps` batches of CALLS back-to-back calls, per call, in ms."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / CALLS)
    return float(np.median(out))


def mode_run(a):
    l = _lib.lib()
    v, f = sphere_mesh()
    V, F = int(v.shape[0]), int(f.shape[0])
    consts = camera()
    out = {"lattice": N, "radius_cells": RADIUS, "vertices": V, "faces": F, "size": list(SIZE), "reps": a.reps, "calls_per_batch": CALLS}
    ws_bytes = int(l.svr_mesh_vertex_normals_workspace_bytes(V, F))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    normals = torch.empty((V, 3), device="cuda", dtype=torch.float32)
    state = torch.empty(V, device="cuda", dtype=torch.uint8)
    counts = torch.empty(3, device="cuda", dtype=torch.int64)
    out["vertex_normals_ms"] = timed(lambda: check(l.svr_mesh_vertex_normals(ptr(v), V, ptr(f), F, ptr(ws), ws_bytes, ptr(normals), ptr(state),
                                                                           ptr(counts), stream()), "normals"), a.reps)
    out["normal_states"] = counts.tolist()
    colors = torch.randint(0, 256, (V, 3), device="cuda", dtype=torch.uint8, generator=torch.Generator(device="cuda").manual_seed(1))
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    albedo, background = (C.c_uint8 * 3)(200, 200, 200), (C.c_uint8 * 3)(255, 255, 255)
    for s in (1, 2):
        k = M.ssaa_consts(consts, s)
        H, W = SIZE[0] * s, SIZE[1] * s
        _, face, tri = render_depth((hv, hf), size=(H, W), consts=k, return_face=True, return_tri=True)
        kc = (C.c_float * 12)(*[float(x) for x in k])
        rgb = torch.empty((H, W, 3), device="cuda", dtype=torch.uint8)
        row = {"fine_size": [H, W], "hit_share": float((face >= 0).float().mean())}
        for label, n, c in (("flat", None, None), ("smooth", normals, None), ("smooth_colors", normals, colors)):
            row[f"shade_{label}_ms"] = timed(lambda: check(l.svr_mesh_shade(ptr(tri), ptr(f), F, V, ptr(face), kc, H, W, ptr(n), ptr(c), albedo,
                                                                          background, 0.25, ptr(rgb), stream()), "shade"), a.reps)
        small = torch.empty((*SIZE, 3), device="cuda", dtype=torch.uint8)
        row["downsample_ms"] = timed(lambda: check(l.svr_box_downsample_rgb8(ptr(rgb), SIZE[0], SIZE[1], s, ptr(small), stream()), "downsample"),
                                     a.reps)
        walls = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            img = M.render_mesh(v, f, consts=consts, size=SIZE, ssaa=s, colors=colors)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        row["render_mesh_wall_ms"] = float(np.median(walls[1:]))
        row["render_mesh_equals_the_phases"] = bool(torch.equal(img, small if s > 1 else rgb))
        out[f"ssaa{s}"] = row
        print(json.dumps({f"ssaa{s}": row}), flush=True)
    return out


def mode_resources():
    """The compiler's register / scratch report of the two units' kernels (build.resource_usage(): no GPU needed)."""
    import importlib
    b = importlib.import_module("single-view-3d-reconstruction_amd.build")
    out = {}
    for name, v in b.resource_usage().items():
        if v["file"] in ("mesh_normals.hip", "mesh_shade.hip"):
            label = next(k for k in ("mn_zero_kernel", "mn_face_kernel", "mn_vertex_kernel", "ms_shade_kernel", "ms_downsample_kernel") if k in name)
            out[label] = {x: v[x] for x in ("vgprs", "agprs", "scratch", "occupancy") if x in v}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("run", "resources"), default="run")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    if a.mode == "resources":
        doc["kernel_resources"] = mode_resources()
    else:
        assert torch.cuda.is_available(), "bench_mesh_render needs a GPU"
        doc.update(mode_run(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
