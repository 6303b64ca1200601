"""The connected-components rule of include/svr_hip.h (svr_mesh_components_*, svr_mesh_filter_*) restated in plain numpy:
what csrc/mesh_components.hip must reproduce bit for bit (the box: by value).  No scipy in here; tests/test_mesh_components_cpu.py
checks this file against scipy.sparse.csgraph where scipy imports."""
from types import SimpleNamespace

import numpy as np


def valid_faces(faces, V):
    """(F,) bool: all three indices in [0, V)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def _roots(V, faces):
    """root[i] = the smallest vertex index of i's component.  Rounds of: every tree's root takes the smallest root among the
    trees its edges touch, then pointer jumping until every vertex names its root; a tree with an edge to another merges in
    each round, so the rounds are logarithmic in V."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    e0 = np.concatenate([f[:, 0], f[:, 1]])
    e1 = np.concatenate([f[:, 1], f[:, 2]])
    root = np.arange(V, dtype=np.int64)
    while True:
        r0, r1 = root[e0], root[e1]
        m = np.minimum(r0, r1)
        new = root.copy()
        np.minimum.at(new, r0, m)
        np.minimum.at(new, r1, m)
        while True:
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, root):
            return root
        root = new


def components(vertices, faces, mark=None):
    """-> namespace of vertex_label (V,), face_label (F,), root, vertex_count, face_count, marked_count (C,) int32,
    bbox_min, bbox_max (C, 3) float32, count."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V = len(v)
    root_of = _roots(V, f)
    roots = np.flatnonzero(root_of == np.arange(V))                 # ascending: the numbering
    vertex_label = np.searchsorted(roots, root_of).astype(np.int32)
    ok = valid_faces(f, V)
    face_label = np.full(len(f), -1, dtype=np.int32)
    face_label[ok] = vertex_label[f[ok, 0]]
    C = len(roots)
    marked = np.zeros(V, dtype=bool) if mark is None else np.asarray(mark).reshape(-1) != 0
    bbox_min = np.full((C, 3), np.inf, dtype=np.float32)
    bbox_max = np.full((C, 3), -np.inf, dtype=np.float32)
    np.fmin.at(bbox_min, vertex_label, v)                           # fmin / fmax skip NaN
    np.fmax.at(bbox_max, vertex_label, v)
    return SimpleNamespace(vertex_label=vertex_label, face_label=face_label, root=roots.astype(np.int32),
                           vertex_count=np.bincount(vertex_label, minlength=C).astype(np.int32),
                           face_count=np.bincount(face_label[ok], minlength=C).astype(np.int32),
                           marked_count=np.bincount(vertex_label[marked], minlength=C).astype(np.int32),
                           bbox_min=bbox_min, bbox_max=bbox_max, count=C)


def select(comps, keep_largest=False, min_faces=0, min_extent=0.0, require_mark=False):
    """(C,) bool: the host's selection rule."""
    keep = np.zeros(comps.count, dtype=bool)
    best = None
    for c in range(comps.count):
        lo, hi = comps.bbox_min[c].astype(np.float64), comps.bbox_max[c].astype(np.float64)
        extent = float(np.sqrt(sum(float(hi[k] - lo[k]) ** 2 for k in range(3) if hi[k] > lo[k])))     # an axis without a value: 0
        ok = comps.face_count[c] >= max(1, min_faces) and extent >= min_extent and (not require_mark or comps.marked_count[c] >= 1)
        keep[c] = ok
        if ok and (best is None or comps.face_count[c] > comps.face_count[best]):                    # ties: the lowest label
            best = c
    if keep_largest:
        keep[:] = False
        if best is not None:
            keep[best] = True
    return keep


def filter_mesh(vertices, faces, comps, keep):
    """-> (vertices (V', 3) float32, faces (F', 3) int32, vertex_index (V',) int32)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    keep = np.asarray(keep).astype(bool).reshape(-1)
    assert keep.shape == (comps.count,)
    ok = valid_faces(f, len(v))
    face_kept = ok.copy()
    face_kept[ok] = keep[comps.face_label[ok]]
    in_face = np.zeros(len(v), dtype=bool)
    in_face[f[ok].reshape(-1)] = True
    vertex_kept = in_face & (keep[comps.vertex_label] if len(v) else np.zeros(0, dtype=bool))
    vertex_index = np.flatnonzero(vertex_kept).astype(np.int32)
    new = np.cumsum(vertex_kept) - 1
    return v[vertex_index], new[f[face_kept]].astype(np.int32).reshape(-1, 3), vertex_index


def clean(vertices, faces, mark=None, **criteria):
    comps = components(vertices, faces, mark)
    keep = select(comps, **criteria)
    return (*filter_mesh(vertices, faces, comps, keep), comps, keep)


def edge_counts(faces):
    """{(low, high): how many faces hold the edge}: a closed surface has 2 everywhere."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    pairs, n = np.unique(e, axis=0, return_counts=True)
    return pairs, n
