"""numpy float32 restatement of the ORDERED splat's summation order (include/svr_hip.h, svr_voxelize_splat_fwd_ordered):

  * base voxel i = floor((p + 0.5) * (D - 1)), fraction r = that product minus its floor, per axis, in float32;
    valid <=> every coordinate strictly inside (-0.5 + 1e-6, 0.5 - 1e-6) compared in float32 (NaN: invalid);
  * weight of corner (k, j, l): (w0[k] * w1[j]) * w2[l] with w[0] = 1 - r, w[1] = r;
  * voxel (z, y, x) holds eight partial sums P[k][j][l] = the float32 sum, from +0 and in ASCENDING POINT INDEX, of the
    corner-(k, j, l) weights of the valid points of its sample whose base voxel is (z - k, y - j, x - l);
  * acc = ((P000 + P001) + (P010 + P011)) + ((P100 + P101) + (P110 + P111)).

``np.add.at`` applies its updates one after the other in index order and in the array's dtype, which is exactly the
sequential float32 sum of a partial (a partial of a voxel only ever receives from one base cell)."""
import numpy as np

F = np.float32


def splat_terms(pts, dims):
    """pts (B, N, 3) -> valid (B, N) bool, base (B, N, 3) int64 (zeros for NaN points, like the kernel), r (B, N, 3) f32."""
    p = np.asarray(pts, dtype=F)
    hi, lo = F(0.5 - 1e-6), F(-0.5 + 1e-6)
    nan = np.isnan(p).any(-1)
    with np.errstate(invalid="ignore"):
        valid = ((p < hi) & (p > lo)).all(-1) & ~nan
        g = (p + F(0.5)) * (np.asarray(dims, dtype=F) - F(1.0))
        f = np.floor(g)
        r = (g - f).astype(F)
        base = np.clip(np.nan_to_num(f, nan=0.0), -2.0e9, 2.0e9).astype(np.int64)
    base[nan] = 0
    return valid, base, r


def splat_ordered(pts, dims):
    """-> acc (B, D0, D1, D2) float32 in the fixed order above, valid, base."""
    dims = tuple(int(d) for d in dims)
    valid, base, r = splat_terms(pts, dims)
    B, N = valid.shape
    b_idx = np.broadcast_to(np.arange(B)[:, None], (B, N))
    w = np.stack([F(1.0) - r, r], axis=0).astype(F)          # w[c][b, n, axis]
    P = np.zeros((2, 2, 2, B) + dims, dtype=F)
    for k in range(2):
        for j in range(2):
            for l in range(2):
                z, y, x = base[..., 0] + k, base[..., 1] + j, base[..., 2] + l
                m = valid & (z >= 0) & (z < dims[0]) & (y >= 0) & (y < dims[1]) & (x >= 0) & (x < dims[2])
                wt = ((w[k][..., 0] * w[j][..., 1]).astype(F) * w[l][..., 2]).astype(F)
                # row-major flattening of (b, n) keeps ascending point index inside every sample
                np.add.at(P[k, j, l], (b_idx[m], z[m], y[m], x[m]), wt[m])
    acc = ((P[0, 0, 0] + P[0, 0, 1]) + (P[0, 1, 0] + P[0, 1, 1])) + ((P[1, 0, 0] + P[1, 0, 1]) + (P[1, 1, 0] + P[1, 1, 1]))
    return acc.astype(F), valid, base


def clamp8(acc):
    """pc_voxels' x8 alias quirk and clamp: clamp(8 * acc, 0, 1) in float32."""
    return np.clip(acc.astype(F) * F(8.0), F(0.0), F(1.0)).astype(F)
