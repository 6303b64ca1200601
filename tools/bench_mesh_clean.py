"""Connected-components timings on two meshes: the reference sample's (tests/golden/scene_mesh_00000.npz,
22 588 vertices / 45 172 faces) and the marching-cubes mesh of the inf_res = 2 lattice of a random-weight IFNet, made as
tools/bench_mesh.py makes its own (about 99 k / 195 k).  Per mesh, in one process and after a warm-up: HIP-event medians of
the three stages through the C ABI (label; statistics with the wave-uniform path and with per-lane atomics; filter count +
emit, keeping the largest component), the host-clock median of ``clean_mesh(keep_largest=True)`` (two read-backs included),
and the numpy oracle's time on the same box for orientation.  Also checks the device result against the oracle bit for bit.
Writes profiles/mesh_clean.json.

    python tools/bench_mesh_clean.py [--reps 50] [--out profiles/mesh_clean.json]
"""
import argparse
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
from svr_amd.util import mesh_clean as M  # noqa: E402

DIMS = (139, 104, 112)


def _stats(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def _events_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return _stats(out)


def _wall_ms(fn, reps, warmup=5):
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


def lattice_mesh():
    """tools/bench_mesh.py's second row: the res_increase = 2 lattice of the name-seeded IFNet on a 3 % occupied input."""
    from oracle import ifnet_oracle as O
    from svr_amd.model import IFNet, evaluate_network_on_grid_device
    from svr_amd.util.visualize import marching_cubes
    m = IFNet(net_res=128)
    m.load_state_dict(O.name_seeded_state(128), strict=False)
    m = m.cuda().eval()
    x = (torch.rand(1, 1, *DIMS, generator=torch.Generator().manual_seed(0)) < 0.03).float().cuda()
    field = 1 - evaluate_network_on_grid_device(m, x, DIMS, 2)
    v, f = marching_cubes(field, 0.5)
    if f.shape[0] == 0:
        v, f = marching_cubes(field, float(field.view(-1)[::97].median()))
    return v, f


def measure(name, v, f, reps):
    from tests import mesh_components_oracle as O
    l = _lib.lib()
    V, F = int(v.shape[0]), int(f.shape[0])
    ws_bytes = int(l.svr_mesh_components_workspace_bytes(V, F))
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    vl, fl = torch.empty(V, device="cuda", dtype=torch.int32), torch.empty(F, device="cuda", dtype=torch.int32)
    count, totals = torch.empty(1, device="cuda", dtype=torch.int64), torch.empty(2, device="cuda", dtype=torch.int64)

    def label():
        check(l.svr_mesh_components_label(ptr(f), F, V, ptr(ws), ws_bytes, ptr(vl), ptr(fl), ptr(count), stream()), "label")

    label()
    n = int(count.item())
    ints = [torch.empty(n, device="cuda", dtype=torch.int32) for _ in range(4)]
    boxes = [torch.empty((n, 3), device="cuda", dtype=torch.float32) for _ in range(2)]

    def stats(uniform):
        check(l.svr_mesh_components_stats(ptr(v), V, ptr(vl), ptr(fl), F, None, n, ptr(ws), ws_bytes, *(ptr(t) for t in ints + boxes),
                                          uniform, stream()), "stats")

    res = {"mesh": name, "vertices": V, "faces": F, "components": n, "reps": reps, "workspace_bytes": ws_bytes}
    res["label_events_ms"] = _events_ms(label, reps)
    res["stats_wave_uniform_events_ms"] = _events_ms(lambda: stats(1), reps)
    res["stats_per_lane_events_ms"] = _events_ms(lambda: stats(0), reps)
    stats(1)
    comps = M.MeshComponents(vl, fl, *ints, *boxes, n)
    keep = M.select_components(comps, keep_largest=True).to(torch.uint8)
    res["face_counts_largest_first"] = sorted(ints[2].tolist(), reverse=True)[:8]

    def filter_count():
        check(l.svr_mesh_filter_count(ptr(f), F, V, ptr(vl), ptr(keep), n, ptr(ws), ws_bytes, ptr(totals), stream()), "filter_count")

    filter_count()
    nv, nf = totals.tolist()
    ov, of, oi = (torch.empty((nv, 3), device="cuda"), torch.empty((nf, 3), device="cuda", dtype=torch.int32),
                  torch.empty(nv, device="cuda", dtype=torch.int32))

    def filter_both():
        filter_count()
        check(l.svr_mesh_filter_emit(ptr(v), V, ptr(f), F, ptr(ws), ws_bytes, ptr(ov), ptr(of), ptr(oi), stream()), "filter_emit")

    res["kept_vertices"], res["kept_faces"] = nv, nf
    res["filter_count_events_ms"] = _events_ms(filter_count, reps)
    res["filter_count_emit_events_ms"] = _events_ms(filter_both, reps)
    res["clean_mesh_wall_ms"] = _wall_ms(lambda: M.clean_mesh(v, f, keep_largest=True), reps)
    res["select_components_wall_ms"] = _wall_ms(lambda: M.select_components(comps, keep_largest=True), reps)
    # a synchronising read of one word, for scale: what each of clean_mesh's two read-backs costs at least
    res["one_word_readback_wall_ms"] = _wall_ms(lambda: count.item(), reps)

    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    t = time.perf_counter()
    want = O.clean(hv, hf, keep_largest=True)
    res["numpy_oracle_ms"] = (time.perf_counter() - t) * 1e3
    got = M.clean_mesh(v, f, keep_largest=True)
    res["equal_to_oracle"] = bool(
        np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].cpu().numpy(), want[1])
        and np.array_equal(got[2].cpu().numpy(), want[2]) and np.array_equal(got[3].vertex_label.cpu().numpy(), want[3].vertex_label)
        and np.array_equal(got[3].face_count.cpu().numpy(), want[3].face_count)
        and np.array_equal(got[3].bbox_min.cpu().numpy(), want[3].bbox_min) and np.array_equal(got[3].bbox_max.cpu().numpy(), want[3].bbox_max))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_mesh_clean needs a GPU"
    z = np.load(os.path.join(ROOT, "tests", "golden", "scene_mesh_00000.npz"))
    rows = [measure("tests/golden/scene_mesh_00000.npz", torch.from_numpy(z["vertices"].astype(np.float32)).cuda(),
                    torch.from_numpy(z["faces"].astype(np.int32)).cuda(), a.reps)]
    print(json.dumps(rows[-1]), flush=True)
    with torch.no_grad():
        v, f = lattice_mesh()
    rows.append(measure("marching cubes of the inf_res = 2 lattice (random-weight IFNet, tools/bench_mesh.py)", v, f, a.reps))
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
    return 0 if all(r["equal_to_oracle"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
