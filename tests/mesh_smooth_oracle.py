"""The Taubin smoothing rule of include/svr_hip.h (svr_mesh_smooth) restated in plain numpy: what csrc/mesh_smooth.hip must
reproduce bit for bit.  Written the way the rule reads -- a list of (next, prev) entries per vertex, sorted by owner once, and
integer sums over it -- not the way the kernels work (they fill the lists with atomics, in whatever order those land).
Also the quality measures DESIGN.md section 24 quotes: radial RMS error, normal consistency and enclosed volume on a sphere."""
from types import SimpleNamespace

import numpy as np

COORD_LIMIT = 2.0 ** 16
ONE = 65536                                              # the fixed point of the positions and of the step weights
Q_LIMIT = 2 ** 33
MAX_ITERATIONS, MAX_FACES = 1024, 2 ** 28
MOVABLE, ISOLATED, FIXED, BAD = 0, 1, 2, 3


def weights(lam, mu):
    """(L_lambda, L_mu) as Python ints, or ValueError: 0 < L_lambda <= 65536 and -65536 <= L_mu <= 0 after the rounding."""
    with np.errstate(invalid="ignore"):
        L = [np.rint(np.float64(np.float32(x)) * ONE) for x in (lam, mu)]
    if not (1 <= L[0] <= ONE and -ONE <= L[1] <= 0):     # written so that a NaN fails it
        raise ValueError(f"lam={lam} mu={mu}")
    return int(L[0]), int(L[1])


def usable(vertices):
    """(V,) bool: three finite coordinates, each |v_a| < 2^16."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(v) & (np.abs(v) < np.float32(COORD_LIMIT))).all(axis=1)


def entries(vertices, faces):
    """-> owner, next, prev (int64, 3 per valid face, sorted by owner; the order inside a list is the faces') and m (V,)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3).astype(np.int64)
    V = len(v)
    ok = usable(v)
    in_range = ((f >= 0) & (f < V)).all(axis=1)
    valid = in_range & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    valid[valid] = ok[f[valid]].all(axis=1)              # the indices first, then what they name
    a, b, c = f[valid, 0], f[valid, 1], f[valid, 2]
    owner = np.concatenate([a, b, c])
    nxt = np.concatenate([b, c, a])
    prv = np.concatenate([c, a, b])
    order = np.argsort(owner, kind="stable")
    return owner[order], nxt[order], prv[order], np.bincount(owner, minlength=V).astype(np.int64)


def interior(owner, nxt, prv, V):
    """(V,) bool: the multiset of i's `next` equals the multiset of its `prev` (true for a vertex without entries)."""
    by_next = np.lexsort((nxt, owner))
    by_prev = np.lexsort((prv, owner))
    differs = nxt[by_next] != prv[by_prev]               # both are sorted by owner first: list against list, element by element
    out = np.ones(V, dtype=bool)
    out[owner[by_next][differs]] = False
    return out


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
    """-> namespace of vertices (V, 3) float32, state (V,) uint8, counts (4,) int64, and for the tests q (V, 3) int64: the
    fixed-point positions after the last pass (rows of unusable vertices hold 0)."""
    n = int(iterations)
    if not 0 <= n <= MAX_ITERATIONS or n != iterations:
        raise ValueError(f"iterations={iterations}")
    L_lam, L_mu = weights(lam, mu)
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    if len(f) > MAX_FACES:
        raise ValueError(f"F={len(f)}")
    V = len(v)
    ok = usable(v)
    owner, nxt, prv, m = entries(v, f)
    state = np.full(V, MOVABLE, dtype=np.uint8)
    if fix_boundary:
        state[~interior(owner, nxt, prv, V)] = FIXED
    state[m == 0] = ISOLATED
    state[~ok] = BAD
    q = np.zeros((V, 3), dtype=np.int64)
    q[ok] = np.rint(v[ok].astype(np.float64) * float(ONE)).astype(np.int64)
    has = np.flatnonzero(m > 0)                          # owner is sorted: the lists of these vertices, one after the other
    starts = (np.cumsum(m) - m)[has]
    movable = state[has] == MOVABLE
    rows, mm = has[movable], m[has][movable][:, None]
    for _ in range(n):
        for L in (L_lam, L_mu):
            if L == 0 or len(rows) == 0:
                continue
            S = np.add.reduceat(q[nxt] + q[prv], starts, axis=0)[movable]
            mean = (S + mm) // (2 * mm)                  # floor division
            step = (L * (mean - q[rows]) + 32768) >> 16  # arithmetic shift: floor
            new = np.clip(q[rows] + step, -Q_LIMIT, Q_LIMIT)
            q = q.copy()
            q[rows] = new
    out = v.copy()
    if n > 0:
        moved = state == MOVABLE
        out[moved] = (q[moved].astype(np.float64) / float(ONE)).astype(np.float32)
    return SimpleNamespace(vertices=out, state=state, counts=np.bincount(state, minlength=4).astype(np.int64), q=q)


# ---- quality on a sphere ------------------------------------------------------------------------------------------------------
def sphere_quality(vertices, faces, centre, radius):
    """Radial RMS error of the vertices, area-weighted mean of |face normal . analytic normal at the centroid|'s signed value
    (the faces' orientation against the outward radius, whichever sign the mesher uses: the absolute value of the mean), and
    the enclosed volume (absolute)."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    c = np.asarray(centre, dtype=np.float64)
    rms = float(np.sqrt(np.mean((np.linalg.norm(v - c, axis=1) - radius) ** 2)))
    a, b, d = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = np.cross(b - a, d - a)                         # its length is twice the area
    out = (a + b + d) / 3 - c
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    consistency = abs(float((nrm * out).sum() / np.linalg.norm(nrm, axis=1).sum()))
    volume = abs(float((a * np.cross(b, d)).sum() / 6.0))
    return SimpleNamespace(rms=rms, normal_consistency=consistency, volume=volume)
