"""Numpy oracle of the block-sparse lattice evaluation (test helper, not product code): the rule of include/svr_hip.h
(svr_sl_*) stated over a DENSE field -- "evaluating" a point is reading the dense value -- with whole-lattice masks instead
of the kernels' per-block face walks.  Also the analytic fields the CPU and GPU tests share."""
from types import SimpleNamespace

import numpy as np


def axis_blocks(n, s):
    """-> (nb, owner (n,), coarse (nb+1,)) for an axis of n points and blocks of s cells."""
    nb = -(-(n - 1) // s)
    owner = np.minimum(np.arange(n) // s, nb - 1)
    coarse = np.minimum(np.arange(nb + 1) * s, n - 1)
    return nb, owner, coarse


def inside(v, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(v).astype(np.float64) < level          # NaN: False


def point_list(shape, s, blocks):
    """Lattice indices (n, 3) of the owned points of `blocks` (flat block indices, ascending), block by block, C order."""
    ax = [axis_blocks(n, s) for n in shape]
    nb = [a[0] for a in ax]
    out = []
    for b in blocks:
        bc = np.unravel_index(b, nb)
        own = [np.nonzero(ax[a][1] == bc[a])[0] for a in range(3)]
        out.append(np.stack(np.meshgrid(*own, indexing="ij"), axis=-1).reshape(-1, 3))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def sparse_field(dense, level, s, max_rounds=32):
    """-> namespace(field, state, n_points, rounds, leaks, fell_back, evaluated (bool mask of the lattice))."""
    dense = np.ascontiguousarray(dense, dtype=np.float32)
    shape = dense.shape
    assert len(shape) == 3 and min(shape) >= 2 and s >= 2 and max_rounds >= 1
    ax = [axis_blocks(n, s) for n in shape]
    nb = tuple(a[0] for a in ax)
    own = np.ix_(*[a[1] for a in ax])                             # lattice point -> its owner block
    C = dense[np.ix_(*[a[2] for a in ax])]
    field = C[:-1, :-1, :-1][own].copy()                          # fill: the coarse value at the block's minimum corner
    flags = inside(C, level)
    n_in = sum(flags[dx:nb[0] + dx, dy:nb[1] + dy, dz:nb[2] + dz].astype(np.int64)
               for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
    selected = (n_in != 0) & (n_in != 8)
    state = np.zeros(nb, dtype=np.uint8)
    n_points, rounds, leaks, fell_back = C.size, 0, [], False
    while selected.any():
        r = rounds + 1
        if r > max_rounds:
            selected = state == 0
            fell_back = True
        pts = selected[own]
        field[pts] = dense[pts]
        n_points += int(pts.sum())
        state[selected] = r
        rounds = r
        # leak check: edges between a point of this round's blocks and a point of a block never evaluated
        now, never = state[own] == r, state[own] == 0
        side = inside(field, level)
        nxt = np.zeros(nb, dtype=bool)
        count = 0
        for a in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[a], hi[a] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            differ = side[lo] != side[hi]
            for p, q in ((lo, hi), (hi, lo)):
                leak = differ & now[p] & never[q]
                count += int(leak.sum())
                idx = np.nonzero(leak)
                if len(idx[0]):
                    full = np.stack(idx, axis=1)
                    if q is hi:
                        full[:, a] += 1
                    nxt[ax[0][1][full[:, 0]], ax[1][1][full[:, 1]], ax[2][1][full[:, 2]]] = True
        leaks.append(count)
        selected = nxt
        if fell_back:
            break
    return SimpleNamespace(field=field, state=state, n_points=n_points, rounds=rounds, leaks=leaks, fell_back=fell_back,
                           evaluated=(state != 0)[own])


def leak_free(field, evaluated, level):
    """No lattice edge with differing sides has an unevaluated endpoint."""
    side = inside(field, level)
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        if ((side[lo] != side[hi]) & ~(evaluated[lo] & evaluated[hi])).any():
            return False
    return True


# ---- analytic fields on the lattice of make_3d_grid: p in [-0.5, 0.5]^3, negative inside, level 0 -------------------------
NORMAL = np.array([0.3, 0.5, 0.81]) / np.linalg.norm([0.3, 0.5, 0.81])


def lattice_points(shape):
    return np.stack(np.meshgrid(*[np.linspace(-0.5, 0.5, n) for n in shape], indexing="ij"), axis=-1)


def sphere(p, r=0.3, c=(0.0, 0.0, 0.0)):
    return np.sqrt(((p - np.asarray(c)) ** 2).sum(-1)) - r


def torus(p, R=0.28, r=0.11):
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return np.sqrt(q ** 2 + p[..., 2] ** 2) - r


def slab(p):
    return np.abs(p @ NORMAL - 0.03) - 0.02


def plane(p):
    return p @ NORMAL - 0.03


def speck(p):
    return sphere(p, 0.02, (0.31, 0.29, 0.33))


FIELDS = {"sphere": sphere, "torus": torus, "slab": slab, "plane": plane, "speck": speck}


def dense_field(name, shape):
    return FIELDS[name](lattice_points(shape)).astype(np.float32)
