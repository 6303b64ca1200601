"""numpy float64 restatement of the ray-casting rule of include/svr_hip.h (svr_raycast_*): brute force over pixels x
faces, Moeller-Trumbore with every operation written out in the header's order.  It knows nothing of tiles, candidate
lists or batches; numpy rounds every operation once, as the kernels (built with -ffp-contract=off) do, so the device
result must equal this one bit for bit.  ``face_rects`` restates svr_raycast_face_bounds, the culling's only input."""
import numpy as np

DEFAULT_OFFSETS = (69.0655, 51.745, -8.0)


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def _cross(ux, uy, uz, vx, vy, vz):
    return uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx


def make_consts(H, W, f=None, cx=None, cy=None, scale=20.0, offsets=DEFAULT_OFFSETS):
    """The 12 constants as float32: by default f = 0.9 max(H, W), the principal point at the image centre, the default
    camera -> grid affine."""
    f = 0.9 * max(H, W) if f is None else f
    cx = (W - 1) / 2 if cx is None else cx
    cy = (H - 1) / 2 if cy is None else cy
    return np.array([f, cx, cy, scale, offsets[0], scale, offsets[1], scale, offsets[2], 0, 0, 0], dtype=np.float32)


def camera_to_grid(points, consts):
    """Camera-space points (x right, y up, z forward, metres) -> grid index space, in float64 (test placement only)."""
    k = np.asarray(consts, dtype=np.float32).astype(np.float64)
    p = np.asarray(points, dtype=np.float64)
    return np.stack([k[3] * p[:, 0] + k[4], k[5] * p[:, 1] + k[6], k[7] * p[:, 2] + k[8]], axis=1)


def triangle_table(vertices, faces):
    """(F, 9) float64: a, b, c per face."""
    v = np.asarray(vertices, dtype=np.float64)
    return v[np.asarray(faces, dtype=np.int64)].reshape(-1, 9)


def ray_directions(u, v, consts):
    """d (P, 3) float64 of the rays through pixels (u = column, v = row), and the shared origin o (3,)."""
    k = np.asarray(consts, dtype=np.float32).astype(np.float64)
    f, cx, cy, s00, t0, s11, t1, s22, t2 = k[:9]
    u = np.asarray(u).astype(np.float64)
    v = np.asarray(v).astype(np.float64)
    d = np.stack([s00 * ((u - cx) / f), -(s11 * ((v - cy) / f)), np.full(u.shape, s22)], axis=-1)
    return np.array([t0, t1, t2]), d


def pair_z(o, d, tri, near=0.0, far=np.inf):
    """(P, F): the accepted depth of every (ray, face) pair, NaN where the pair is rejected or skipped."""
    return pair_details(o, d, tri, near, far)[0]


def pair_details(o, d, tri, near=0.0, far=np.inf, pairwise=False):
    """-> z (P, F) (NaN = not accepted), det, bu, bv (P, F) as the rule computes them.  `pairwise`: ray i against face i
    only (P == F; near / far may be arrays), every result (P,)."""
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    if pairwise:
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        ax, ay, az, bx, by, bz, cx, cy, cz = (t[:, i] for i in range(9))
    else:
        dx, dy, dz = d[:, 0, None], d[:, 1, None], d[:, 2, None]
        ax, ay, az, bx, by, bz, cx, cy, cz = (t[None, :, i] for i in range(9))
    with np.errstate(all="ignore"):
        e1x, e1y, e1z = bx - ax, by - ay, bz - az
        e2x, e2y, e2z = cx - ax, cy - ay, cz - az
        px, py, pz = _cross(dx, dy, dz, e2x, e2y, e2z)
        det = _dot(e1x, e1y, e1z, px, py, pz)
        inv = 1.0 / det
        sx, sy, sz = o[0] - ax, o[1] - ay, o[2] - az
        bu = _dot(sx, sy, sz, px, py, pz) * inv
        qx, qy, qz = _cross(sx, sy, sz, e1x, e1y, e1z)
        bv = _dot(dx, dy, dz, qx, qy, qz) * inv
        z = _dot(e2x, e2y, e2z, qx, qy, qz) * inv
        ok = ~(det == 0.0) & (bu >= 0.0) & (bu <= 1.0) & (bv >= 0.0) & (bu + bv <= 1.0) & (near < z) & (z <= far)
    return np.where(ok, z, np.nan), det, bu, bv


def cast(tri, consts, u, v, near=0.0, far=None, chunk=64):
    """Rays through pixels (u, v) (1-D arrays) -> (best z (P,) float64, +inf for a miss; face (P,) int32, -1 for a miss)."""
    far = np.inf if far is None else float(far)
    o, d = ray_directions(u, v, consts)
    best = np.empty(d.shape[0], dtype=np.float64)
    face = np.empty(d.shape[0], dtype=np.int32)
    for s in range(0, d.shape[0], chunk):
        z = pair_z(o, d[s:s + chunk], tri, near, far)
        z = np.where(np.isnan(z), np.inf, z)
        j = np.argmin(z, axis=1)               # the first occurrence of the minimum: the lowest index wins a tie
        b = z[np.arange(z.shape[0]), j]
        best[s:s + chunk] = b
        face[s:s + chunk] = np.where(np.isinf(b), -1, j)
    return best, face


def distance_factor(H, W, f, rows, cols):
    """float32: sqrt((float)(r*r + c*c) / (f*f) + 1), r = row - H/2, c = col - W/2 (integer division)."""
    f = np.float32(f)
    r = np.asarray(rows, dtype=np.int64) - H // 2
    c = np.asarray(cols, dtype=np.int64) - W // 2
    rc = (r * r + c * c).astype(np.float32)
    return np.sqrt(rc / (f * f) + np.float32(1.0))


def distance_to_depth(distance, H, W, f, rows, cols):
    """svr_distance_to_depth's rule at the given pixels, float32."""
    f = np.float32(f)
    r = np.asarray(rows, dtype=np.int64) - H // 2
    c = np.asarray(cols, dtype=np.int64) - W // 2
    rc = (r * r + c * c).astype(np.float32)
    d = np.asarray(distance, dtype=np.float32)
    return np.sqrt(d * d / (rc / (f * f) + np.float32(1.0)))


def maps_at(tri, consts, H, W, rows, cols, near=0.0, far=None, miss=0.0):
    """The rule's outputs at the given pixels: {"depth" f32, "face" i32, "distance" f32, "normal" (P, 3) f32, "shade" u8}."""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    consts = np.asarray(consts, dtype=np.float32)
    rows, cols = np.asarray(rows), np.asarray(cols)
    best, face = cast(tri, consts, cols, rows, near, far)
    hit = face >= 0
    depth = np.where(hit, best, 0.0).astype(np.float32)
    depth = np.where(hit, depth, np.float32(miss)).astype(np.float32)
    distance = (depth * distance_factor(H, W, consts[0], rows, cols)).astype(np.float32)
    _, d = ray_directions(cols, rows, consts)
    t = tri[np.maximum(face, 0)]
    with np.errstate(all="ignore"):
        e1, e2 = t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3]
        nx, ny, nz = _cross(e1[:, 0], e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1], e2[:, 2])
        ln = np.sqrt(_dot(nx, ny, nz, nx, ny, nz))
        m = np.stack([nx / ln, ny / ln, nz / ln], axis=1)
        flip = _dot(m[:, 0], m[:, 1], m[:, 2], d[:, 0], d[:, 1], d[:, 2]) > 0.0
        m = np.where(flip[:, None], -m, m)
        m = np.where(hit[:, None], m, 0.0)
        g = np.rint((255.0 * np.abs(_dot(m[:, 0], m[:, 1], m[:, 2], d[:, 0], d[:, 1], d[:, 2])))
                    / np.sqrt(_dot(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])))
        shade = np.where(g >= 0.0, np.minimum(np.where(np.isnan(g), 0.0, g), 255.0), 0.0).astype(np.uint8)
    return {"depth": depth, "face": face, "distance": distance, "normal": m.astype(np.float32), "shade": shade}


def render(vertices, faces, consts, size, near=0.0, far=None, miss=0.0):
    """All maps of an (H, W) image, shaped (H, W[, 3])."""
    H, W = size
    rows, cols = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    out = maps_at(triangle_table(vertices, faces), consts, H, W, rows, cols, near, far, miss)
    return {k: a.reshape((H, W) + a.shape[1:]) for k, a in out.items()}


def transform_vertices(vertices, M):
    """x' = ((M00*x + M01*y) + M02*z) + M03 per row of the 4x4 float64 mesh -> grid affine."""
    v = np.asarray(vertices, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], axis=1)


RECT_MAX = 1 << 30
MIN_DEPTH = 2.0 ** -20
MAX_DEPTH_RATIO = 1024.0


def face_rects(tri, consts):
    """svr_raycast_face_bounds: (F, 4) int32 {x0, x1, y0, y1}, inclusive; an "every tile" face gets +-2^30."""
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    k = np.asarray(consts, dtype=np.float32).astype(np.float64)
    f, cx, cy, s00, t0, s11, t1, s22, t2 = k[:9]
    with np.errstate(all="ignore"):
        zc = (t[:, :, 2] - t2) / s22
        u = cx + (f * (t[:, :, 0] - t0)) / (s00 * zc)
        v = cy - (f * (t[:, :, 1] - t1)) / (s11 * zc)
        ok = ((zc > MIN_DEPTH) & (np.abs(u) <= float(RECT_MAX)) & (np.abs(v) <= float(RECT_MAX))).all(axis=1)
        ok &= zc.max(1) <= MAX_DEPTH_RATIO * zc.min(1)
        lim = float(RECT_MAX)
        sides = [np.floor(u.min(1)) - 1.0, np.ceil(u.max(1)) + 1.0, np.floor(v.min(1)) - 1.0, np.ceil(v.max(1)) + 1.0]
        sides = [np.where(ok, np.clip(s, -lim, lim), e) for s, e in zip(sides, (-lim, lim, -lim, lim))]
    return np.stack(sides, axis=1).astype(np.int32)
