"""Mesh output timings at the inference lattices (139 x 104 x 112 and res_increase 2: 278 x 208 x 224): the dense-grid
evaluation, marching cubes on the device, implicit_to_mesh end to end and the .obj write, with V and F.  One JSON
object per lattice on stdout (--out FILE: also written there).  Random-weight IFNet, 3 % occupied input.

The kernel / scan split comes from a run under `rocprofv3 --kernel-trace --stats -- python tools/bench_mesh.py`.

--voxel: the voxel-box mesher instead, on the real 139 x 104 x 112 depth grid of
tests/golden/ref_depth_grid.npz and on project()'s blurred occupancy of the same points: V / F, per-kernel times (HIP
events around each C-ABI phase: classify + scan, emit), `voxel_mesh` and `visualize_grid` wall time, and the numpy
oracle's host time on the same grid (the stand-in for the reference's host path: trimesh is not installed)."""
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


def event_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def voxel_rows(reps):
    import ctypes as C

    import numpy as np
    from svr_amd import _lib
    from svr_amd.model.projection import project
    from svr_amd.util.visualize import marching_cubes as mc, visualize_grid, voxel_mesh
    from tests import voxel_mesh_oracle as V
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    grid = np.load(os.path.join(root, "tests", "golden", "ref_depth_grid.npz"))["grid"].astype(np.float32)
    real = torch.from_numpy(grid).cuda()
    pts = torch.nonzero(real >= 0.5).float()
    proj = project(torch.tensor(DIMS), [3, 3, 3], torch.tensor([1.5, 1.5, 1.5])).cuda()
    with torch.no_grad():
        d = torch.tensor(DIMS, device="cuda", dtype=torch.float32)
        blurred = proj(((pts - d / 2) / d).unsqueeze(0)).reshape(DIMS).contiguous()
    l = _lib.lib()
    tmp = tempfile.mkdtemp()
    rows = []
    for name, field in (("ref_depth_grid", real), ("project(ref_depth_grid points)", blurred)):
        v, f = voxel_mesh(field)
        ws_bytes = int(l.svr_voxel_mesh_workspace_bytes(*DIMS))
        ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
        totals = torch.empty(2, device="cuda", dtype=torch.int64)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
        count = lambda: l.svr_voxel_mesh_count(p(field), *DIMS, 0.5, p(ws), ws_bytes, p(totals), s)      # noqa: E731
        emit = lambda: l.svr_voxel_mesh_emit(p(field), *DIMS, 0.5, p(ws), p(v), p(f), s)                # noqa: E731
        host = field.cpu().numpy()
        t0 = time.perf_counter()
        ov, of = V.voxel_mesh(host)
        oracle_ms = (time.perf_counter() - t0) * 1e3
        assert ov.shape == tuple(v.shape) and of.shape == tuple(f.shape)
        path = os.path.join(tmp, "g.obj")
        r = {"grid": name, "lattice": list(DIMS), "occupied": int((field >= 0.5).sum()), "V": int(v.shape[0]), "F": int(f.shape[0]),
             "count_classify_scan_ms": event_ms(count, reps), "emit_ms": event_ms(emit, reps),
             "voxel_mesh_ms": wall(lambda: voxel_mesh(field), reps), "visualize_grid_ms": wall(lambda: visualize_grid(field, path), reps),
             "marching_cubes_same_lattice_ms": wall(lambda: mc(field, 0.5), reps),
             "numpy_oracle_host_ms": oracle_ms, "obj_bytes": os.path.getsize(path)}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--voxel", action="store_true", help="time the voxel-box mesher instead (DESIGN.md section 12)")
    a = ap.parse_args()
    if a.voxel:
        rows = voxel_rows(a.reps)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(rows, fh, indent=1)
        return
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
