"""Numpy oracle of the mesh evaluation kernels (test helper, not product code): the rules of include/svr_hip.h
("Mesh evaluation") restated as array code -- face table, surface sampler, all-pairs nearest neighbour in float32,
distance_p2p / eval_pointcloud / IoU with the reference's aggregation.  numpy only."""
import numpy as np

KEYS = ("completeness", "accuracy", "normals completeness", "normals accuracy", "normals", "completeness2", "accuracy2",
        "chamfer_l2", "iou")


def face_table(vertices, faces):
    """-> (unit normals (F,3) float64, cum_area (F,) float64): one rounding per operation, areas summed sequentially."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = B - A, C - A
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = ln > 0.0
    normals = np.zeros_like(n)
    normals[ok] = n[ok] / ln[ok, None]
    area = np.where(ok, 0.5 * ln, 0.0)
    return normals, np.cumsum(area)             # np.cumsum of a 1-D float64 array adds in index order


def sample(vertices, faces, cum_area, uniforms, return_exact=False):
    """-> (points (n,3) float32, face index (n,) int32) for uniforms (n,3) float64; `return_exact`: also the float64
    points and the two barycentric weights."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    u = np.asarray(uniforms, dtype=np.float64)
    total = cum_area[-1]
    x = u[:, 0] * total
    j = np.searchsorted(cum_area, x, side="right")                  # first j with cum[j] > x
    over = j >= len(cum_area)
    j[over] = min(np.searchsorted(cum_area, total, side="left"), len(cum_area) - 1)
    w1, w2 = u[:, 1].copy(), u[:, 2].copy()
    refl = w1 + w2 > 1.0
    w1[refl], w2[refl] = 1.0 - w1[refl], 1.0 - w2[refl]
    A, B, C = v[f[j, 0]], v[f[j, 1]], v[f[j, 2]]
    p = (A + w1[:, None] * (B - A)) + w2[:, None] * (C - A)
    if return_exact:
        return p.astype(np.float32), j.astype(np.int32), p, w1, w2
    return p.astype(np.float32), j.astype(np.int32)


def nn_search(queries, targets, rows=None, chunk=None):
    """All pairs in float32 by the header's rule -> (dist (Q,) float32, idx (Q,) int32); `rows`: only these queries."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    t = np.ascontiguousarray(targets, dtype=np.float32)
    if rows is not None:
        q = q[rows]
    Q, T = len(q), len(t)
    dist = np.empty(Q, dtype=np.float32)
    idx = np.empty(Q, dtype=np.int32)
    chunk = chunk or max(1, (1 << 24) // max(T, 1))
    tx, ty, tz = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, Q, chunk):
            c = q[s:s + chunk]
            dx, dy, dz = c[:, 0:1] - tx, c[:, 1:2] - ty, c[:, 2:3] - tz
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            bits = np.ascontiguousarray(d2).view(np.uint32).copy()          # d2 >= +0: the bits order like the values
            bits[np.isnan(d2)] = 0xFFFFFFFF                                 # a NaN never wins against a number
            j = bits.argmin(axis=1)                                         # first minimum = lowest index
            b = bits[np.arange(len(c)), j]
            win = d2[np.arange(len(c)), j]
            none = b > 0x7F800000
            dist[s:s + chunk] = np.where(none, np.float32(np.nan), np.sqrt(win.astype(np.float64)).astype(np.float32))
            idx[s:s + chunk] = np.where(none, -1, j)
    return dist, idx


def normals_dot(normals_q, normals_t, idx):
    def unit(n):
        n = np.asarray(n).astype(np.float64)
        return n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    a, b = unit(normals_q), unit(normals_t)[idx]
    return np.abs((b[:, 0] * a[:, 0] + b[:, 1] * a[:, 1]) + b[:, 2] * a[:, 2])


def distance_p2p(pointcloud_pred, pointcloud_gt, normals_pred, normals_gt):
    """-> (dist float32, |dot| float64 or None, idx)."""
    dist, idx = nn_search(pointcloud_pred, pointcloud_gt)
    if normals_pred is None:
        return dist, None, idx
    return dist, normals_dot(normals_pred, normals_gt, idx), idx


def eval_pointcloud(pointcloud_pred, pointcloud_gt, normals_pred=None, normals_gt=None):
    """The reference's aggregation: means of the distances, of their squares, of |dot| in both directions;
    chamfer_l2 = 0.5 * completeness2 + 0.5 * accuracy2; normals = the mean of the two normal entries."""
    c_dist, c_dot, _ = distance_p2p(pointcloud_gt, pointcloud_pred, normals_gt, normals_pred)
    a_dist, a_dot, _ = distance_p2p(pointcloud_pred, pointcloud_gt, normals_pred, normals_gt)
    c_dist, a_dist = c_dist.astype(np.float64), a_dist.astype(np.float64)
    out = {"completeness": c_dist.mean(), "accuracy": a_dist.mean(),
           "completeness2": (c_dist ** 2).mean(), "accuracy2": (a_dist ** 2).mean()}
    out["chamfer_l2"] = 0.5 * out["completeness2"] + 0.5 * out["accuracy2"]
    if normals_pred is not None:
        out["normals completeness"], out["normals accuracy"] = c_dot.mean(), a_dot.mean()
        out["normals"] = 0.5 * out["normals completeness"] + 0.5 * out["normals accuracy"]
    else:
        out["normals completeness"] = out["normals accuracy"] = out["normals"] = np.nan
    out["iou"] = np.nan
    return {k: float(out[k]) for k in KEYS}


def iou(occ_a, occ_b):
    a, b = np.asarray(occ_a, dtype=bool), np.asarray(occ_b, dtype=bool)
    union = int((a | b).sum())
    return int((a & b).sum()) / union if union else float("nan")


def eval_mesh(mesh_pred, mesh_gt, bb_min, bb_max, u_pred, u_gt, u_box, contains):
    """eval_mesh from the same uniforms; meshes are (vertices, faces) pairs; `contains(vertices, faces, points) -> bool
    array` labels the box samples (oracle.mesh_oracle.implicit_waterproofing's first output)."""
    clouds = []
    for (v, f), u in ((mesh_pred, u_pred), (mesh_gt, u_gt)):
        normals, cum = face_table(v, f)
        pts, face = sample(v, f, cum, u)
        clouds.append((pts, normals[face]))
    out = eval_pointcloud(clouds[0][0], clouds[1][0], clouds[0][1], clouds[1][1])
    box = np.asarray(u_box, dtype=np.float64) * (bb_max - bb_min) + bb_min
    out["iou"] = iou(contains(mesh_pred[0], mesh_pred[1], box), contains(mesh_gt[0], mesh_gt[1], box))
    return out
