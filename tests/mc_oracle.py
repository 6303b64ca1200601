"""Numpy oracle of the marching-cubes kernels (test helper, not product code): the same semantics, written as vectorised
array code over the whole lattice, with the case table read from the library (svr_mc_case_table) -- so the GPU tests
can compare vertices bit for bit and faces element for element.  Also: topology / geometry helpers for meshes."""
import ctypes

import numpy as np

# corner c of a cell: offset (c & 1, c >> 1 & 1, c >> 2 & 1) along axes (0, 1, 2)
CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=np.int64)


def case_table():
    """(256, 16) int8 from the library: 3 edge ids per triangle, -1 padded."""
    import svr_amd
    out = np.zeros(256 * 16, dtype=np.int8)
    assert svr_amd._lib.lib().svr_mc_case_table(out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out.reshape(256, 16)


def edge_endpoints(e):
    """Edge id -> (axis, offset (3,) of its lower endpoint in the cell)."""
    ax = e >> 2
    u, v = [a for a in range(3) if a != ax]
    off = np.zeros(3, dtype=np.int64)
    off[u] = e & 1
    off[v] = (e >> 1) & 1
    return ax, off


def marching_cubes(field, level, table=None):
    """-> (vertices (V,3) float32, faces (F,3) int32) with the kernels' rules (include/svr_hip.h)."""
    table = case_table() if table is None else table
    f = np.ascontiguousarray(field, dtype=np.float32)
    X, Y, Z = f.shape
    if X < 2 or Y < 2 or Z < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    d = f.astype(np.float64)
    inside = d < level                                   # NaN: False
    own = np.zeros((X, Y, Z, 3), dtype=bool)             # owned crossing edges (+axis) per lattice point
    own[:-1, :, :, 0] = inside[:-1] != inside[1:]
    own[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    own[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = own.reshape(-1)
    vid = np.full(flat.shape, -1, dtype=np.int64)
    nz = np.nonzero(flat)[0]                             # point-major, then axis: the kernels' vertex order
    vid[nz] = np.arange(len(nz))
    vid = vid.reshape(X, Y, Z, 3)
    pt, ax = nz // 3, nz % 3
    ijk = np.stack(np.unravel_index(pt, (X, Y, Z)), axis=1)
    a = d.reshape(-1)[pt]
    step = np.array([Y * Z, Z, 1])[ax]
    b = d.reshape(-1)[pt + step]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.fmin(np.fmax((level - a) / (b - a), 0.0), 1.0)
    verts = ijk.astype(np.float32)
    verts[np.arange(len(nz)), ax] = (ijk[np.arange(len(nz)), ax].astype(np.float64) + t).astype(np.float32)
    # cases of the cells (C order of the minimum corner)
    cs = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        cs |= inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << c
    cs = cs.reshape(-1)
    ntri = (table >= 0).sum(axis=1) // 3
    nt = ntri[cs]
    cell = np.repeat(np.arange(len(cs)), nt)
    slot = np.arange(len(cell)) - np.repeat(np.cumsum(nt) - nt, nt)
    cijk = np.stack(np.unravel_index(cell, (X - 1, Y - 1, Z - 1)), axis=1)
    faces = np.zeros((len(cell), 3), dtype=np.int64)
    for m in range(3):
        e = table[cs[cell], 3 * slot + m].astype(np.int64)
        for eid in np.unique(e):
            sel = e == eid
            axis, off = edge_endpoints(int(eid))
            q = cijk[sel] + off
            faces[sel, m] = vid[q[:, 0], q[:, 1], q[:, 2], axis]
    assert (faces >= 0).all()
    return verts, faces.astype(np.int32)


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed(faces):
    """Every directed edge is matched by its reverse exactly once (and occurs once itself)."""
    de = directed_edges(faces)
    if len(de) == 0:
        return True
    key = lambda e: e[:, 0] * (1 << 32) + e[:, 1]
    fw, bw = key(de), key(de[:, ::-1])
    if len(np.unique(fw)) != len(fw):
        return False
    return np.array_equal(np.sort(fw), np.sort(bw))


def euler_characteristic(verts, faces):
    de = directed_edges(faces)
    und = np.unique(np.sort(de, axis=1), axis=0)
    return len(np.unique(np.asarray(faces).reshape(-1))) - len(und) + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def sphere(n=24, r=8.0, c=None):
    c = (n - 1) / 2.0 if c is None else c
    g = np.stack(np.meshgrid(*([np.arange(n, dtype=np.float64)] * 3), indexing="ij"), axis=-1)
    return (np.sqrt(((g - c) ** 2).sum(-1)) - r).astype(np.float32)


def torus(shape=(40, 40, 24), R=10.0, r=4.0):
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    c = (np.array(shape) - 1) / 2.0 + np.array([0.13, -0.21, 0.07])    # off-lattice centre: no value exactly at 0
    p = g - c
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return (np.sqrt(q ** 2 + p[..., 2] ** 2) - r).astype(np.float32)
