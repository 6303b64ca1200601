"""numpy float64 restatement of the distance-field rule of include/svr_hip.h (svr_mesh_df_*): brute force over
points x faces, every region computed and selected with np.where in the header's order.  It knows nothing of bricks,
candidate lists or batches; numpy rounds every operation once, as the kernels (built with -ffp-contract=off) do, so the
device result must equal this one bit for bit."""
import numpy as np


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def triangle_table(vertices, faces):
    """(F, 9) float64: a, b, c per face."""
    v = np.asarray(vertices, dtype=np.float64)
    return v[np.asarray(faces, dtype=np.int64)].reshape(-1, 9)


def has_area(tri):
    """(F,) bool: ab x ac is not exactly (0, 0, 0)."""
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    abx, aby, abz = t[:, 3] - t[:, 0], t[:, 4] - t[:, 1], t[:, 5] - t[:, 2]
    acx, acy, acz = t[:, 6] - t[:, 0], t[:, 7] - t[:, 1], t[:, 8] - t[:, 2]
    nx, ny, nz = aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx
    return ~((nx == 0.0) & (ny == 0.0) & (nz == 0.0))


def pair_dd(points, tri):
    """(P, F) float64 squared distances of points (P, 3) to the faces of tri (F, 9)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    px, py, pz = p[:, 0, None], p[:, 1, None], p[:, 2, None]
    ax, ay, az, bx, by, bz, cx, cy, cz = (t[None, :, i] for i in range(9))
    with np.errstate(all="ignore"):
        abx, aby, abz = bx - ax, by - ay, bz - az
        acx, acy, acz = cx - ax, cy - ay, cz - az
        apx, apy, apz = px - ax, py - ay, pz - az
        bpx, bpy, bpz = px - bx, py - by, pz - bz
        cpx, cpy, cpz = px - cx, py - cy, pz - cz
        d1, d2 = _dot(abx, aby, abz, apx, apy, apz), _dot(acx, acy, acz, apx, apy, apz)
        d3, d4 = _dot(abx, aby, abz, bpx, bpy, bpz), _dot(acx, acy, acz, bpx, bpy, bpz)
        d5, d6 = _dot(abx, aby, abz, cpx, cpy, cpz), _dot(acx, acy, acz, cpx, cpy, cpz)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        den = (va + vb) + vc
        v, w = vb / den, vc / den                                     # 7. face interior
        w6 = e43 / (e43 + e56)
        conds = [
            ((va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0), 1.0 - w6, w6),                    # 6. edge bc
            ((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), 0.0, d2 / (d2 - d6)),               # 5. edge ac
            ((d6 >= 0.0) & (d5 <= d6), 0.0, 1.0),                                         # 4. vertex c
            ((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), d1 / (d1 - d3), 0.0),               # 3. edge ab
            ((d3 >= 0.0) & (d4 <= d3), 1.0, 0.0),                                         # 2. vertex b
            ((d1 <= 0.0) & (d2 <= 0.0), 0.0, 0.0),                                        # 1. vertex a
        ]
        for cond, cv, cw in conds:                                    # applied last to first: the FIRST true line wins
            v = np.where(cond, cv, v)
            w = np.where(cond, cw, w)
        ex = px - ((ax + v * abx) + w * acx)
        ey = py - ((ay + v * aby) + w * acy)
        ez = pz - ((az + v * abz) + w * acz)
        return _dot(ex, ey, ez, ex, ey, ez)


class EmptyMesh(ValueError):
    pass


def distance_at(points, tri, truncate=None, chunk=256):
    """-> (field (P,) float32, face (P,) int32) at arbitrary points (the lattice rule at p = the point)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    keep = np.nonzero(has_area(t))[0]
    if keep.size == 0:
        raise EmptyMesh("no face with area")
    t = t[keep]
    field = np.empty(p.shape[0], dtype=np.float32)
    face = np.empty(p.shape[0], dtype=np.int32)
    for s in range(0, p.shape[0], chunk):
        dd = pair_dd(p[s:s + chunk], t)
        # strict `<` in ascending face order: the first occurrence of the minimum; a NaN never wins
        dd = np.where(np.isnan(dd), np.inf, dd)
        j = np.argmin(dd, axis=1)
        best = dd[np.arange(dd.shape[0]), j]
        f = np.where(np.isinf(best), -1, keep[j]).astype(np.int32)
        with np.errstate(all="ignore"):
            val = np.sqrt(best).astype(np.float32)
        field[s:s + chunk], face[s:s + chunk] = val, f
    if truncate is not None and truncate > 0:
        T = np.float32(truncate)
        over = field > T
        field = np.where(over, T, field).astype(np.float32)
        face = np.where(over, -1, face).astype(np.int32)
    return field, face


def lattice_points(dims):
    X, Y, Z = dims
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), axis=-1)
    return g.reshape(-1, 3).astype(np.float64)


def distance_field(vertices, faces, dims, truncate=None):
    """-> (field (X, Y, Z) float32, face (X, Y, Z) int32)."""
    field, face = distance_at(lattice_points(dims), triangle_table(vertices, faces), truncate)
    return field.reshape(dims), face.reshape(dims)
