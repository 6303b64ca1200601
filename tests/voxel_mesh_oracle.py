"""Numpy oracle of the voxel-box mesher (test helper, not product code), written independently of the kernels'
formulation: the kernels gather neighbours per corner-lattice point; this builds all six quads of every occupied box,
cancels the quads that occur twice (coincident and opposite: the face shared by two boxes), and welds what is left by
corner index.  Semantics as in include/svr_hip.h: occupied iff v >= threshold (NaN is not); voxel (i, j, k) is the cube
[i-1/2, i+1/2]^3-shifted; vertices are corner-lattice points in C order; faces by voxel (C order), then direction
-x, +x, -y, +y, -z, +z, each quad q0 q1 q2 q3 as the triangles (q0, q1, q2), (q0, q2, q3).  Also: geometry checks and a
stdlib decoder for the 8-bit grayscale PNG files of svr_write_png_gray8."""
import struct
import zlib

import numpy as np

# direction -> (axis, sign) and the quad's 4 corners as (x, y, z) offsets from the voxel's minimum corner,
# counter-clockwise seen from outside (the header's table, typed out once more)
DIRECTIONS = [(0, -1), (0, +1), (1, -1), (1, +1), (2, -1), (2, +1)]
QUADS = np.array([
    [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],      # -x
    [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)],      # +x
    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],      # -y
    [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],      # +y
    [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],      # -z
    [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],      # +z
], dtype=np.int64)


def occupancy(grid, threshold=0.5):
    with np.errstate(invalid="ignore"):
        return np.asarray(grid, dtype=np.float32).astype(np.float64) >= threshold        # NaN: False


def voxel_mesh(grid, threshold=0.5):
    """-> (vertices (V,3) float32, faces (F,3) int32)."""
    occ = occupancy(grid, threshold)
    X, Y, Z = occ.shape
    vox = np.argwhere(occ)                                            # occupied voxels, C order
    cdims = (X + 1, Y + 1, Z + 1)
    # all six quads of every box: (n, 6, 4) corner-lattice indices
    corners = vox[:, None, None, :] + QUADS[None]                     # (n, 6, 4, 3)
    cidx = np.ravel_multi_index((corners[..., 0], corners[..., 1], corners[..., 2]), cdims).reshape(-1, 4)
    # two boxes that share a face each bring a quad on the same 4 corners (in opposite order): both go
    # (an axis-aligned unit square is named by its smallest and largest corner index)
    srt = np.sort(cidx, axis=1)
    key = srt[:, 0] * int(np.prod(cdims)) + srt[:, 3]
    _, inverse, count = np.unique(key, return_inverse=True, return_counts=True)
    assert (count <= 2).all()
    keep = count[inverse.reshape(-1)] == 1
    quads = cidx[keep]
    # weld: the corners in use, ascending corner index
    used = np.unique(quads)
    remap = np.full(int(np.prod(cdims)), -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    verts = (np.stack(np.unravel_index(used, cdims), axis=1).astype(np.float32) - np.float32(0.5)).reshape(-1, 3)
    q = remap[quads]
    faces = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return verts, faces


def face_directions(grid, threshold=0.5):
    """The direction index (0..5) of every triangle voxel_mesh emits, by the rule 'the neighbour across is empty'."""
    occ = occupancy(grid, threshold)
    pad = np.pad(occ, 1)
    X, Y, Z = occ.shape
    exposed = np.zeros((X, Y, Z, 6), dtype=bool)
    for d, (ax, sg) in enumerate(DIRECTIONS):
        sl = [slice(1, X + 1), slice(1, Y + 1), slice(1, Z + 1)]
        sl[ax] = slice(1 + sg, occ.shape[ax] + 1 + sg)
        exposed[..., d] = occ & ~pad[tuple(sl)]
    return np.repeat(np.nonzero(exposed.reshape(-1))[0] % 6, 2)


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def triangle_normals(verts, faces):
    """Unnormalised (b - a) x (c - a): a unit-square half has length 1."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def area(verts, faces):
    return float(np.linalg.norm(triangle_normals(verts, faces), axis=1).sum() / 2.0)


def edges_balanced(faces):
    """Every directed edge occurs as often as its reverse (at an edge or corner where two boxes only touch, an edge is
    used twice in each direction: the surface of a union of boxes is closed but not always a manifold)."""
    f = np.asarray(faces, dtype=np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fw = np.sort(de[:, 0] * (1 << 32) + de[:, 1])
    bw = np.sort(de[:, 1] * (1 << 32) + de[:, 0])
    return np.array_equal(fw, bw)


def check_surface(grid, verts, faces, threshold=0.5):
    """The four properties every voxel_mesh output has; all exact in float64 (coordinates are multiples of 1/2)."""
    occ = occupancy(grid, threshold)
    dirs = face_directions(grid, threshold)
    assert len(faces) == len(dirs) and len(faces) % 2 == 0
    assert signed_volume(verts, faces) == float(occ.sum())
    assert area(verts, faces) == len(faces) / 2
    assert edges_balanced(faces)
    expect = np.zeros((len(dirs), 3))
    for d, (ax, sg) in enumerate(DIRECTIONS):
        expect[dirs == d, ax] = sg
    assert np.array_equal(triangle_normals(verts, faces), expect)
    if len(faces):
        assert np.array_equal(np.unique(faces), np.arange(len(verts)))       # welded: every vertex used, none twice
        assert len(np.unique(np.asarray(verts), axis=0)) == len(verts)


def decode_png_gray8(blob):
    """PNG bytes -> (H, W) uint8, checking the signature, the IHDR fields, every chunk's CRC, the chunk sequence
    IHDR / IDAT / IEND and filter type 0 on every scanline."""
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        (n,) = struct.unpack(">I", blob[pos:pos + 4])
        typ, data = blob[pos + 4:pos + 8], blob[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + data) & 0xffffffff, typ
        chunks.append((typ, data))
        pos += 12 + n
    assert pos == len(blob)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 0, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == H * (W + 1)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, W + 1)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:]
