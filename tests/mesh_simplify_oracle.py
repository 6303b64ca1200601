"""The vertex-clustering rule of include/svr_hip.h (svr_mesh_simplify_*) restated in plain numpy: what csrc/mesh_simplify.hip
must reproduce bit for bit.  Written the way the rule reads -- clusters numbered by ascending root, faces mapped to cluster
numbers -- not the way the kernels work (they name a cluster by its root and never number the dropped ones)."""
from types import SimpleNamespace

import numpy as np

CELL_MIN, CELL_MAX, COORD_LIMIT = 2.0 ** -10, 2.0 ** 16, 2.0 ** 16


def clusterable(vertices):
    """(V,) bool: three finite coordinates, each |v_a| < 2^16."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(v) & (np.abs(v) < np.float32(COORD_LIMIT))).all(axis=1)


def cells(vertices, cell):
    """(V, 3) int64: floor(v / cell) in float64 (rows of unclusterable vertices hold 0 and mean nothing)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    ok = clusterable(v)
    q = np.zeros(v.shape, dtype=np.int64)
    q[ok] = np.floor(v[ok].astype(np.float64) / np.float64(np.float32(cell))).astype(np.int64)
    return q


def canonical(triples):
    """Each row rotated so that its smallest number comes first (rows whose numbers differ)."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    k = np.argmin(t, axis=1)
    rows = np.arange(len(t))
    return np.stack([t[rows, k], t[rows, (k + 1) % 3], t[rows, (k + 2) % 3]], axis=1)


def simplify(vertices, faces, cell):
    """-> namespace of vertices (V', 3) float32, faces (F', 3) int32, vertex_cluster (V,) int32, cluster_size (V',) int32, bad,
    and for the tests face_index (F',): the input face each kept face was."""
    cell = np.float32(cell)
    if not (np.isfinite(cell) and CELL_MIN <= cell <= CELL_MAX):
        raise ValueError(f"cell={cell}")
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V = len(v)
    ok = clusterable(v)
    ids = np.flatnonzero(ok)
    q = cells(v, cell)[ids]
    # 3. root = the smallest member index (np.unique returns each row's first occurrence); numbered by ascending root
    _, first, inverse = np.unique(q, axis=0, return_index=True, return_inverse=True)
    root_of = ids[first[np.asarray(inverse).reshape(-1)]] if len(ids) else np.zeros(0, dtype=np.int64)
    roots = np.unique(root_of)
    C = len(roots)
    number = np.full(V, -1, dtype=np.int64)
    number[ids] = np.searchsorted(roots, root_of)
    # 4. fixed-point sums in int64, one division in float64, rounded once to float32
    s = np.rint(v[ids].astype(np.float64) * 65536.0).astype(np.int64)
    S = np.zeros((C, 3), dtype=np.int64)
    np.add.at(S, number[ids], s)
    n = np.bincount(number[ids], minlength=C).astype(np.int64)
    pos = ((S.astype(np.float64) / n[:, None].astype(np.float64)) / 65536.0).astype(np.float32) if C else np.zeros((0, 3), np.float32)
    single = n == 1
    pos[single] = v[roots[single]]                                   # the words of the one member (-0.0 stays -0.0)
    # 5. valid: the indices first, then what they name
    f64 = f.astype(np.int64)
    in_range = ((f64 >= 0) & (f64 < V)).all(axis=1)
    valid = in_range.copy()
    valid[in_range] = ok[f64[in_range]].all(axis=1)
    mapped = np.full(f.shape, -1, dtype=np.int64)
    mapped[valid] = number[f64[valid]]
    live = valid & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0])
    # 6. of equal canonical triples the smallest face index stays
    live_ids = np.flatnonzero(live)
    if len(live_ids):
        _, first_face = np.unique(canonical(mapped[live_ids]), axis=0, return_index=True)
        kept_faces = np.sort(live_ids[first_face])
    else:
        kept_faces = np.zeros(0, dtype=np.int64)
    # 7. the clusters the kept faces name, in their order
    used = np.zeros(C, dtype=bool)
    used[mapped[kept_faces].reshape(-1)] = True
    new = np.cumsum(used) - 1
    vertex_cluster = np.full(V, -1, dtype=np.int32)
    named = ids[used[number[ids]]]
    vertex_cluster[named] = new[number[named]]
    return SimpleNamespace(vertices=np.ascontiguousarray(pos[used]), faces=new[mapped[kept_faces]].astype(np.int32).reshape(-1, 3),
                           vertex_cluster=vertex_cluster, cluster_size=n[used].astype(np.int32), bad=int((~ok).sum()),
                           face_index=kept_faces)


def directed_edges(faces):
    """(3 F, 2) int64: a -> b, b -> c, c -> a of every face."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed(faces):
    """Every directed edge has its opposite: a -> b occurs as often as b -> a (the surface has no boundary).  Once each on a
    manifold; where clustering folds a thin feature, an edge can carry four faces and occur twice each way."""
    e = directed_edges(faces)
    if len(e) == 0:
        return False
    there, n_there = np.unique(e, axis=0, return_counts=True)
    back, n_back = np.unique(e[:, ::-1], axis=0, return_counts=True)
    return bool(np.array_equal(there, back) and np.array_equal(n_there, n_back))
