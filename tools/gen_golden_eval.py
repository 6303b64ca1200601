"""Generate tests/golden/eval_pointcloud.npz by running the REFERENCE's util/evaluate.py (eval_pointcloud,
distance_p2p) on the CPU.  Needs a checkout of the reference (--reference DIR or $SVR_REFERENCE) and scipy; no test does.

THE TREE IS A STAND-IN.  The reference queries pykdtree.kdtree.KDTree; that package (and trimesh) is not installed
where this is run, so `trimesh` and `data_processing.implicit_waterproofing` are stubbed as empty modules (eval_pointcloud
and distance_p2p use neither) and `pykdtree.kdtree.KDTree` is a thin wrapper over scipy.spatial.cKDTree.  The golden
therefore pins the reference's AGGREGATION -- the normalisation of the normals, the abs, the means,
chamfer_l2 = 0.5 * completeness2 + 0.5 * accuracy2 -- and exact float64 nearest neighbours, not pykdtree's rounding.

Stored: two clustered clouds of 8 192 points with (unnormalised) normals, float32; the reference's eval_pointcloud
dictionary (ref_<key>); dist (float64) and idx (int32) of both directions; and `min_relative_gap`.  The inputs are
re-seeded until, for every query in both directions, the second-nearest float64 distance exceeds the nearest by more than
1e-5 relative (query(k=2)): then an exact float32 search (d2 rounded to <= 3 * 2^-24 relative) must return the same index,
and index equality is a fair demand on every point.  Nothing of the reference's text is stored; only these arrays are."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

N = 8192
GAP = 1e-5
KEYS = ("completeness", "accuracy", "normals completeness", "normals accuracy", "normals", "completeness2", "accuracy2",
        "chamfer_l2", "iou")


def load_reference(ref):
    from scipy.spatial import cKDTree

    class KDTree:                                   # pykdtree.kdtree.KDTree(data).query(pts) -> (dist, idx), k = 1
        def __init__(self, data):
            self._tree = cKDTree(np.asarray(data))

        def query(self, pts, k=1):
            return self._tree.query(np.asarray(pts), k=k)

    stubs = {"trimesh": types.ModuleType("trimesh"), "pykdtree": types.ModuleType("pykdtree"),
             "pykdtree.kdtree": types.ModuleType("pykdtree.kdtree"), "data_processing": types.ModuleType("data_processing"),
             "data_processing.implicit_waterproofing": types.ModuleType("data_processing.implicit_waterproofing")}
    stubs["pykdtree.kdtree"].KDTree = KDTree
    stubs["data_processing.implicit_waterproofing"].implicit_waterproofing = None
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_reference_evaluate", os.path.join(ref, "util", "evaluate.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def clouds(seed):
    """Two draws from the same clustered surface distribution: blobs of very different density on a bumpy sphere."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(7, 3))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    spread = np.array([0.02, 0.05, 0.08, 0.12, 0.2, 0.3, 0.5])
    out = []
    for _ in range(2):
        k = rng.choice(7, size=N, p=[0.3, 0.2, 0.15, 0.12, 0.1, 0.08, 0.05])
        d = centres[k] + spread[k, None] * rng.normal(size=(N, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = 0.35 * (1 + 0.1 * np.sin(5 * d[:, 0]) * np.cos(4 * d[:, 1]))
        p = d * r[:, None] + 0.002 * rng.normal(size=(N, 3))
        n = (d + 0.15 * rng.normal(size=(N, 3))) * rng.uniform(0.2, 3.0, size=(N, 1))      # not unit, some flipped
        n[rng.random(N) < 0.1] *= -1
        out.append((p.astype(np.float32), n.astype(np.float32)))
    return out


def min_gap(queries, targets):
    from scipy.spatial import cKDTree
    d, _ = cKDTree(targets.astype(np.float64)).query(queries.astype(np.float64), k=2)
    with np.errstate(divide="ignore"):
        return float(np.min(np.where(d[:, 0] > 0, (d[:, 1] - d[:, 0]) / d[:, 0], np.where(d[:, 1] > 0, np.inf, 0.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVR_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "eval_pointcloud.npz"))
    a = ap.parse_args()
    assert a.reference and os.path.isdir(a.reference), "--reference DIR (or SVR_REFERENCE): a checkout of the reference"
    ref = load_reference(a.reference)
    seed = 0
    while True:
        (pp, npred), (pg, ngt) = clouds(seed)
        gap = min(min_gap(pp, pg), min_gap(pg, pp))
        if gap > GAP:
            break
        seed += 1
    from scipy.spatial import cKDTree
    res = ref.eval_pointcloud(pp, pg, npred, ngt)
    c_dist, c_idx = cKDTree(pp).query(pg)          # completeness: gt -> pred, as distance_p2p builds and queries it
    a_dist, a_idx = cKDTree(pg).query(pp)
    assert set(res) == set(KEYS)
    # the dictionary really is the aggregation of these distances
    assert res["completeness"] == c_dist.mean() and res["accuracy2"] == (a_dist ** 2).mean()
    arrays = {"pred": pp, "gt": pg, "normals_pred": npred, "normals_gt": ngt,
              "completeness_dist": c_dist, "completeness_idx": c_idx.astype(np.int32),
              "accuracy_dist": a_dist, "accuracy_idx": a_idx.astype(np.int32),
              "min_relative_gap": np.float64(gap), "seed": np.int64(seed),
              "note": np.array("reference util/evaluate.py eval_pointcloud with pykdtree.kdtree.KDTree replaced by a "
                               "scipy.spatial.cKDTree stand-in: pins the aggregation, not pykdtree's rounding")}
    for k in KEYS:
        arrays["ref_" + k.replace(" ", "_")] = np.float64(res[k])
    np.savez_compressed(a.out, **arrays)
    print(f"seed {seed}, min relative gap {gap:.3e}, {os.path.getsize(a.out)} bytes -> {a.out}")
    for k in KEYS:
        print(f"  {k}: {res[k]!r}")


if __name__ == "__main__":
    main()
