"""Mesh evaluation timings on a marching-cubes mesh pair at the 139 x 104 x 112 inference
lattice: face table + upload, surface sampling, the exact nearest-neighbour search 100 000 x 100 000 per direction (with
pair updates per second and the share of the float32 vector rate), the two 1 M-point containment passes, and eval_mesh
end to end at n_points = 100 000.  Each GPU phase is synchronised and timed, median of --reps.  If scipy is importable
the CPU route (cKDTree build + query, workers=16: the stand-in for the reference's pykdtree) is timed on the same clouds;
if not, the JSON says so.  One JSON object on stdout (--out FILE: also written there).

Kernel times come from a run under `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import svr_amd  # noqa: E402,F401
from svr_amd.data_processing.implicit_waterproofing import implicit_waterproofing  # noqa: E402
from svr_amd.util import evaluate as EV  # noqa: E402
from svr_amd.util.visualize import marching_cubes  # noqa: E402

DIMS = (139, 104, 112)
VALU_OPS_PER_PAIR = 8            # 3 subtractions, 3 products, 2 sums, none fused (the compare / selects not counted)
F32_VECTOR_OPS_PER_S = 78.6e12   # the 157 TFLOPS vector line of MI355X counted as operations (an FMA is 2 FLOPs)


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


def blob_field(scale):
    """A smooth multi-blob implicit on the lattice (negative inside): a scene-sized closed surface."""
    ax = [torch.arange(d, dtype=torch.float32, device="cuda") for d in DIMS]
    g = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1)
    c = torch.tensor([[60., 50., 55.], [85., 60., 50.], [50., 40., 70.], [75., 45., 75.]], device="cuda")
    r = torch.tensor([30., 22., 18., 20.], device="cuda") * scale
    d = ((g[..., None, :] - c) ** 2).sum(-1).sqrt() - r
    return d.min(dim=-1).values.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n_points", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n_points
    pred, gt = marching_cubes(blob_field(0.95), 0.0), marching_cubes(blob_field(1.0), 0.0)
    bb_min, bb_max = 0.0, float(max(DIMS))
    g = torch.Generator(device="cuda").manual_seed(0)
    mp, mg = EV.EvalMesh(pred), EV.EvalMesh(gt)
    up, ug, ub = EV.eval_mesh_draws(n, g)
    pc_p, _, n_p = EV.sample_with_uniforms(mp, up)
    pc_g, _, n_g = EV.sample_with_uniforms(mg, ug)
    box = ub * (bb_max - bb_min) + bb_min
    r = {"lattice": list(DIMS), "n_points": n, "reps": a.reps,
         "V_pred": int(pred[0].shape[0]), "F_pred": int(pred[1].shape[0]), "V_gt": int(gt[0].shape[0]), "F_gt": int(gt[1].shape[0])}
    hv, hf = gt[0].cpu().numpy(), gt[1].cpu().numpy()
    r["face_table_upload_ms"] = wall(lambda: EV.EvalMesh((hv, hf)), a.reps)
    r["sample_ms"] = wall(lambda: EV.sample_with_uniforms(mg, ug), a.reps)
    r["nn_ms_per_direction"] = wall(lambda: EV.nn_search(pc_p, pc_g), a.reps)
    # a longer window for the rate: 10 searches back to back behind one synchronise
    r["nn_ms_per_direction_x10"] = wall(lambda: [EV.nn_search(pc_p, pc_g) for _ in range(10)], a.reps) / 10
    pairs = float(n) * float(n)
    r["nn_pairs_per_s"] = pairs / (r["nn_ms_per_direction_x10"] * 1e-3)
    r["nn_share_of_f32_vector_rate"] = r["nn_pairs_per_s"] * VALU_OPS_PER_PAIR / F32_VECTOR_OPS_PER_S
    r["distance_p2p_ms"] = wall(lambda: EV._distance_p2p_device(pc_p, pc_g, n_p, n_g), a.reps)
    r["eval_pointcloud_ms"] = wall(lambda: EV._eval_pointcloud_device(pc_p, pc_g, n_p, n_g), a.reps)
    r["containment_2x%d_points_ms" % box.shape[0]] = wall(lambda: (implicit_waterproofing(mp, box), implicit_waterproofing(mg, box)),
                                                          a.reps)
    r["eval_mesh_ms"] = wall(lambda: EV.eval_mesh(pred, gt, bb_min, bb_max, n_points=n, generator=g), a.reps)
    r["eval_mesh"] = EV.eval_mesh(pred, gt, bb_min, bb_max, n_points=n, generator=g)
    # smaller and larger searches: where all-pairs stops being the right choice
    scale_rows = []
    for m in (10000, 30000, 100000, 300000):
        q = (torch.rand((m, 3), device="cuda", generator=g) - 0.5).contiguous()
        t = (torch.rand((m, 3), device="cuda", generator=g) - 0.5).contiguous()
        ms = wall(lambda: EV.nn_search(q, t), 3)
        scale_rows.append({"Q": m, "T": m, "ms": ms, "pairs_per_s": float(m) * m / (ms * 1e-3)})
    r["nn_scaling"] = scale_rows
    try:
        from scipy.spatial import cKDTree
        hp, hg = pc_p.cpu().numpy(), pc_g.cpu().numpy()

        def cpu_nn():
            cKDTree(hg).query(hp, workers=16)

        ts = []
        for _ in range(max(3, a.reps // 2)):
            t0 = time.perf_counter()
            cpu_nn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        r["cpu_ckdtree_build_query_ms_per_direction"] = ts[len(ts) // 2]
        r["cpu_note"] = "scipy.spatial.cKDTree build + query(workers=16): stand-in for the reference's pykdtree"
        _, ci = cKDTree(hg).query(hp, workers=16)
        di = EV.nn_search(pc_p, pc_g)[1].cpu().numpy()
        r["idx_agreement_with_ckdtree"] = float((ci == di).mean())
    except ImportError:
        r["cpu_ckdtree_build_query_ms_per_direction"] = None
        r["cpu_note"] = "scipy is not importable here: the CPU route was not timed"
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(r, fh, indent=1)


if __name__ == "__main__":
    main()
