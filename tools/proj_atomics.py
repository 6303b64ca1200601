"""CPU model of the atomic projected scatter (gather.hip, gather_bwd_proj_kernel): what an item order costs, without a GPU.

For one level and one item order it counts, under the kernel's own rules,
  runs           maximal stretches of equal (sample, displacement, cell) inside one wave's chunk of 256 sorted items
  atomic bytes   every run end adds its in-volume corners (256 floats each) to dP with float atomics; a run whose
                 successor IN THE SAME CHUNK is the +x neighbour cell of the same (sample, displacement) keeps its +x face
                 in registers (the hand-over) and flushes only the other 4 corners
  row fetches    a wave reads the dh row of every item of its chunk; the 7 displacements of a point share one row, so
                 (sum over chunks of the distinct points in the chunk) / (distinct points) says how often a row is fetched:
                 1 = all 7 items of every point in one chunk, 7 = no reuse at all
The order is svr_gather_item_order_xblock's: (sample, z, y, x / K, j, x % K); K = 1 is the (cell, j) order.

  python tools/proj_atomics.py --dims 16 16 16 --N 50000 --B 2 --K 1 3 4 6 9
numpy only (the `surface` distribution is bench.synth_batch's and imports bench.py, hence torch, on the CPU).
"""
import argparse
import os
import sys

import numpy as np

CHUNK = 256          # items per wave: 2 x 64 lanes x kProjReps
ROW_BYTES = 256 * 4  # one (voxel, displacement) row of dP


def item_cells(points, dims, align_corners, displacement):
    """Base cell of every item, as sample_corner / pull_cell compute it in float32.
    points (B, N, 3) float32 in (z, y, x) order -> b, j, z, y, x (lattice coordinates base + 1) and the in-volume mask,
    each of shape (B*N*7,), item id = (b*N + n)*7 + j."""
    pts = np.asarray(points, dtype=np.float32)
    B, N, _ = pts.shape
    D, H, W = dims
    d = np.float32(displacement)
    g = np.float32(2.0) * pts[:, :, None, ::-1]                      # (B, N, 1, xyz) grid coordinates
    g = np.repeat(g, 7, axis=2).copy()
    for j in range(1, 7):
        g[:, :, j, (j - 1) // 2] += (-d if (j & 1) else d)
    out = []
    for a, S in ((0, W), (1, H), (2, D)):
        v = g[..., a]
        if align_corners:
            i = ((v + np.float32(1)) / np.float32(2)) * np.float32(S - 1)
        else:
            i = ((v + np.float32(1)) * np.float32(S) - np.float32(1)) / np.float32(2)
        out.append(np.floor(i).astype(np.int64).reshape(-1))
    x0, y0, z0 = out
    ok = (z0 >= -1) & (z0 < D) & (y0 >= -1) & (y0 < H) & (x0 >= -1) & (x0 < W)
    b = np.repeat(np.arange(B, dtype=np.int64), N * 7)
    j = np.tile(np.arange(7, dtype=np.int64), B * N)
    return b, j, z0 + 1, y0 + 1, x0 + 1, ok


def xblock_keys(b, j, z, y, x, ok, dims, K):
    """Sort key of svr_gather_item_order_xblock; items that touch no voxel get the key count (they sort last)."""
    D, H, W = dims
    nb = (W + 1 + K - 1) // K
    key = ((((b * (D + 1) + z) * (H + 1) + y) * nb + x // K) * 8 + j) * K + x % K
    nkeys = (int(b.max()) + 1 if b.size else 0) * (D + 1) * (H + 1) * nb * 8 * K
    return np.where(ok, key, nkeys)


def count(points, dims, align_corners=False, displacement=0.0722, K=1, order=None):
    """Counts for one launch.  order: an explicit item order (a permutation of the item ids) instead of the x-block order."""
    D, H, W = dims
    b, j, z, y, x, ok = item_cells(points, dims, align_corners, displacement)
    T = b.size
    if order is None:
        order = np.argsort(xblock_keys(b, j, z, y, x, ok, dims, K), kind="stable")
    b, j, z, y, x, ok = (a[order] for a in (b, j, z, y, x, ok))
    pn = np.asarray(order) // 7
    chunk = np.arange(T) // CHUNK
    # the walk skips items that touch no voxel: runs are found among the others, in order
    idx = np.nonzero(ok)[0]
    cb, cj, cz, cy, cx, cc = b[idx], j[idx], z[idx], y[idx], x[idx], chunk[idx]
    cell = (cz * 1024 + cy) * 1024 + cx                              # the kernel's own key
    bb = cb * 8 + cj
    same = (cell[1:] == cell[:-1]) & (bb[1:] == bb[:-1]) & (cc[1:] == cc[:-1])
    start = np.concatenate(([True], ~same)) if idx.size else np.zeros(0, bool)
    s = np.nonzero(start)[0]                                         # first item of every run
    rz, ry, rx, rcell, rbb, rc = cz[s], cy[s], cx[s], cell[s], bb[s], cc[s]
    # corners of a run: base voxel = lattice - 1, corner k at base + (k >> 2, (k >> 1) & 1, k & 1)
    inz = [(rz - 1 + dz >= 0) & (rz - 1 + dz < D) for dz in (0, 1)]
    iny = [(ry - 1 + dy >= 0) & (ry - 1 + dy < H) for dy in (0, 1)]
    inx = [(rx - 1 + dx >= 0) & (rx - 1 + dx < W) for dx in (0, 1)]
    nyz = (inz[0].astype(np.int64) + inz[1]) * (iny[0].astype(np.int64) + iny[1])
    hand = np.zeros(s.size, bool)
    if s.size > 1:
        hand[:-1] = (rcell[1:] == rcell[:-1] + 1) & (rbb[1:] == rbb[:-1]) & (rc[1:] == rc[:-1])
    rows = nyz * (inx[0].astype(np.int64) + np.where(hand, 0, inx[1]))
    # dh rows: distinct points per chunk over distinct points
    pc = np.unique(chunk * (pn.max() + 1 if T else 1) + pn).size if T else 0
    return {"K": K, "items": int(T), "runs": int(s.size), "handed": int(hand.sum()),
            "atomic_bytes": int(rows.sum()) * ROW_BYTES,
            "row_fetches_per_row": pc / max(np.unique(pn).size, 1) if T else 0.0}


def make_points(dist, B, N, seed, D=128):
    if dist == "uniform":
        return (np.random.default_rng(seed).random((B, N, 3), dtype=np.float32) - np.float32(0.5))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    return bench.synth_batch(seed, B, 8, N, "cpu", dist="surface")["points"].numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--dims", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--align-corners", action="store_true")
    ap.add_argument("--displacement", type=float, default=0.0722)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 2, 3, 4, 6, 9, 17])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dist", choices=["uniform", "surface"], default="uniform")
    ap.add_argument("--scale-to-batch", type=int, default=8, help="also print the bytes scaled from B to this batch")
    a = ap.parse_args()
    pts = make_points(a.dist, a.B, a.N, a.seed)
    print(f"B={a.B} N={a.N} dims={tuple(a.dims)} align_corners={a.align_corners} displacement={a.displacement} "
          f"dist={a.dist} seed={a.seed}")
    print(f"{'K':>3} {'runs':>9} {'handed':>9} {'atomic GB/launch':>17} {'GB at batch ' + str(a.scale_to_batch):>15} "
          f"{'dh row fetches/row':>19}")
    for K in a.K:
        if K < 1 or K > a.dims[2] + 1:
            continue
        r = count(pts, tuple(a.dims), a.align_corners, a.displacement, K)
        gb = r["atomic_bytes"] / 1e9
        print(f"{K:>3} {r['runs']:>9} {r['handed']:>9} {gb:>17.4f} {gb * a.scale_to_batch / a.B:>15.3f} "
              f"{r['row_fetches_per_row']:>19.2f}")


if __name__ == "__main__":
    main()
