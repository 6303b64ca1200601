"""numpy restatement of the mesh-preview rules of include/svr_hip.h (svr_mesh_vertex_normals, svr_mesh_shade,
svr_box_downsample_rgb8), written from the header's text: int64 sums that wrap like the kernels' unsigned atomics, float64 with
one rounding per operation for the shader.  The device results must equal these bit for bit.  ``transform_normals`` and
``orbit`` restate the two host-side formulas of util/mesh_render.py's docstrings."""
from types import SimpleNamespace

import numpy as np

from tests import raycast_oracle as R

HAS_NORMAL, NO_NORMAL, BAD = 0, 1, 3
LIMIT = np.float32(65536.0)


def usable(vertices):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(v) < LIMIT).all(axis=1)


def valid_faces(vertices, faces):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    ok[ok] = usable(v)[f[ok]].all(axis=1)
    return ok


def vertex_normals(vertices, faces):
    """-> SimpleNamespace(normals (V, 3) float32, state (V,) uint8, counts [state 0, 1, 3], sums (V, 3) int64)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok_v = usable(v)
    q = np.zeros(v.shape, dtype=np.int64)
    q[ok_v] = np.rint(v[ok_v].astype(np.float64) * 1024.0).astype(np.int64)
    g = f[valid_faces(v, f)]
    a, b, c = q[g[:, 0]], q[g[:, 1]], q[g[:, 2]]
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    sums = np.zeros(v.shape, dtype=np.int64)
    with np.errstate(over="ignore"):
        for k in range(3):
            np.add.at(sums, g[:, k], n)                      # int64: wraps modulo 2^64
    x, y, z = (sums[:, k].astype(np.float64) for k in range(3))
    length = np.sqrt((x * x + y * y) + z * z)
    has = ok_v & (length > 0.0)
    safe = np.where(has, length, 1.0)
    normals = np.stack([np.where(has, t / safe, 0.0) for t in (x, y, z)], axis=1).astype(np.float32)
    state = np.where(~ok_v, BAD, np.where(has, HAS_NORMAL, NO_NORMAL)).astype(np.uint8)
    counts = [int((state == s).sum()) for s in (HAS_NORMAL, NO_NORMAL, BAD)]
    return SimpleNamespace(normals=normals, state=state, counts=counts, sums=sums)


def shade_bytes(x):
    """rint, half to even, clamped to [0, 255]; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        r = np.rint(x)
        return np.where(r >= 0.0, np.minimum(np.where(np.isnan(r), 0.0, r), 255.0), 0.0).astype(np.uint8)


def shade_pixels(tri, faces, n_vertices, face, u, v, consts, normals=None, colors=None, ambient=0.25, albedo=(200, 200, 200),
                 background=(255, 255, 255)):
    """The rule at pixels (u = column, v = row) whose face-map entries are `face` -> (P, 3) uint8."""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 9)
    F, V = len(tri), int(n_vertices)
    face = np.asarray(face, dtype=np.int64).reshape(-1)
    o, d = R.ray_directions(np.asarray(u).reshape(-1), np.asarray(v).reshape(-1), consts)
    on = (face >= 0) & (face < F)
    fi = np.where(on, face, 0)
    t = tri[fi] if F else np.zeros((len(face), 9))
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az, bx, by, bz, cx, cy, cz = (t[:, i] for i in range(9))
    with np.errstate(all="ignore"):
        e1x, e1y, e1z = bx - ax, by - ay, bz - az
        e2x, e2y, e2z = cx - ax, cy - ay, cz - az
        px, py, pz = R._cross(dx, dy, dz, e2x, e2y, e2z)
        det = R._dot(e1x, e1y, e1z, px, py, pz)
        inv = 1.0 / det
        sx, sy, sz = o[0] - ax, o[1] - ay, o[2] - az
        bu = R._dot(sx, sy, sz, px, py, pz) * inv
        qx, qy, qz = R._cross(sx, sy, sz, e1x, e1y, e1z)
        bv = R._dot(dx, dy, dz, qx, qy, qz) * inv
        w0 = (1.0 - bu) - bv
        on &= ~(det == 0.0)
        # the face's own normal, turned against the ray
        nx, ny, nz = R._cross(e1x, e1y, e1z, e2x, e2y, e2z)
        ln = np.sqrt(R._dot(nx, ny, nz, nx, ny, nz))
        m = np.stack([nx / ln, ny / ln, nz / ln], axis=1)
        flip = R._dot(m[:, 0], m[:, 1], m[:, 2], dx, dy, dz) > 0.0
        N = np.where(flip[:, None], -m, m)
        corners = np.zeros(len(face), dtype=bool)
        idx = np.zeros((len(face), 3), dtype=np.int64)
        if (normals is not None or colors is not None) and F:
            idx = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[fi]
            corners = ((idx >= 0) & (idx < V)).all(axis=1)
            idx = np.where(corners[:, None], idx, 0)
        if normals is not None and V:
            nn = np.asarray(normals, dtype=np.float32).astype(np.float64)
            S = np.stack([(w0 * nn[idx[:, 0], a] + bu * nn[idx[:, 1], a]) + bv * nn[idx[:, 2], a] for a in range(3)], axis=1)
            sl = np.sqrt(R._dot(S[:, 0], S[:, 1], S[:, 2], S[:, 0], S[:, 1], S[:, 2]))
            smooth = corners & (sl > 0.0)
            N = np.where(smooth[:, None], S / sl[:, None], N)
        c = np.abs(R._dot(N[:, 0], N[:, 1], N[:, 2], dx, dy, dz)) / np.sqrt(R._dot(dx, dy, dz, dx, dy, dz))
        a = np.float64(np.float32(ambient))
        I = a + (1.0 - a) * c
        base = np.broadcast_to(np.asarray(albedo, dtype=np.float64), (len(face), 3)).copy()
        if colors is not None and V:
            cc = np.asarray(colors, dtype=np.uint8).astype(np.float64)
            mixed = np.stack([(w0 * cc[idx[:, 0], k] + bu * cc[idx[:, 1], k]) + bv * cc[idx[:, 2], k] for k in range(3)], axis=1)
            base = np.where(corners[:, None], mixed, base)
        out = shade_bytes(base * I[:, None])
    return np.where(on[:, None], out, np.asarray(background, dtype=np.uint8)[None, :]).astype(np.uint8)


def render(vertices, faces, consts, size, normals=None, colors=None, face_map=None, **kw):
    """The (H, W, 3) image: the ray-casting oracle's face map of the (already transformed) mesh, then the shader.  `vertices`
    are the positions the camera sees, float64 or float32; `normals` / `colors` per vertex or None."""
    H, W = size
    rows, cols = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    tri = R.triangle_table(vertices, faces)
    if face_map is None:
        _, face_map = R.cast(tri, consts, cols, rows)
    return shade_pixels(tri, faces, len(vertices), face_map, cols, rows, consts, normals, colors, **kw).reshape(H, W, 3)


def ssaa_consts(consts, s):
    k = np.asarray(consts, dtype=np.float32).copy()
    f, cx, cy = k[:3].astype(np.float64)
    k[0], k[1], k[2] = s * f, s * cx + (s - 1) / 2, s * cy + (s - 1) / 2     # the assignment rounds to float32
    return k


def box_downsample(rgb, s):
    a = np.asarray(rgb, dtype=np.uint8)
    H, W = a.shape[0] // s, a.shape[1] // s
    total = a.reshape(H, s, W, s, 3).astype(np.int64).sum(axis=(1, 3))
    return ((total + (s * s) // 2) // (s * s)).astype(np.uint8)


def render_ssaa(vertices, faces, consts, size, s, **kw):
    fine = render(vertices, faces, ssaa_consts(consts, s), (size[0] * s, size[1] * s), **kw)
    return fine if s == 1 else box_downsample(fine, s)


def transform_normals(normals, M):
    """Cofactor matrix of the linear part times the normal, renormalised in float64, rounded to float32."""
    L = np.asarray(M, dtype=np.float64)[:3, :3]
    cof = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            r, c = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            cof[i, j] = (-1) ** (i + j) * (L[r[0], c[0]] * L[r[1], c[1]] - L[r[0], c[1]] * L[r[1], c[0]])
    n = np.asarray(normals, dtype=np.float32).astype(np.float64)
    m = [(cof[i, 0] * n[:, 0] + cof[i, 1] * n[:, 1]) + cof[i, 2] * n[:, 2] for i in range(3)]
    length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    ok = length > 0.0
    return np.stack([np.where(ok, a / np.where(ok, length, 1.0), 0.0) for a in m], axis=1).astype(np.float32)
