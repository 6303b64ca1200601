"""numpy float64 restatement of the vertex-colour rule of include/svr_hip.h (svr_vertex_color_sample, svr_vertex_color_spread)
and a reader for the PLY files svr_write_ply writes.  numpy rounds every operation once, as the kernels (built with
-ffp-contract=off) do, and the spread is integer arithmetic, so the device result must equal this one bit for bit.
``exact_visibility`` is NOT part of the rule: it is the ground truth the rule's depth-map test approximates."""
import numpy as np

from tests import raycast_oracle as R

IDENTITY = (1.0, 0.0, 1.0, 0.0)
FILL = (128, 128, 128)


def _widened(vertices):
    """The kernel's input is float32, widened; float64 vertices are taken as they are (the CPU tests' ground-truth runs)."""
    g = np.asarray(vertices)
    return (g if g.dtype == np.float64 else g.astype(np.float32).astype(np.float64)).reshape(-1, 3)


def project(vertices, consts):
    """-> zc, u, v (V,) float64: svr_raycast_face_bounds' projection of the vertices in grid index space."""
    g = _widened(vertices)
    k = np.asarray(consts, dtype=np.float32).astype(np.float64)
    f, cx, cy, s00, t0, s11, t1, s22, t2 = k[:9]
    with np.errstate(all="ignore"):
        zc = (g[:, 2] - t2) / s22
        u = cx + (f * (g[:, 0] - t0)) / (s00 * zc)
        v = cy - (f * (g[:, 1] - t1)) / (s11 * zc)
    return zc, u, v


def pad_map(Hi, Wi):
    """The pixel map of a (Hi, Wi) image behind SquarePad + resize, for the 240 x 320 depth map (reconstruct.input_pixel_map)."""
    m = max(Hi, Wi)
    pad_y, pad_x = (m - Hi) // 2, (m - Wi) // 2
    ay, ax = (Hi + 2 * pad_y) / 320, (Wi + 2 * pad_x) / 320
    return (ax, 0.5 * ax - 0.5 - pad_x, ay, 40.5 * ay - 0.5 - pad_y)


def sample(vertices, consts, depth, bias, image, pixel_map=IDENTITY, fill=FILL):
    """svr_vertex_color_sample -> colors (V, 3) uint8, state (V,) uint8."""
    depth = np.asarray(depth, dtype=np.float32)
    image = np.asarray(image, dtype=np.uint8)
    H, W = depth.shape
    Hi, Wi = image.shape[:2]
    ax, bx, ay, by = (float(x) for x in pixel_map)
    bias = float(bias)
    zc, u, v = project(vertices, consts)
    V = zc.shape[0]
    with np.errstate(all="ignore"):
        frame = (zc > 0.0) & (u >= -0.5) & (u <= W - 0.5) & (v >= -0.5) & (v <= H - 0.5)
        iu = np.where(frame, np.floor(u), 0.0).astype(np.int64)
        iv = np.where(frame, np.floor(v), 0.0).astype(np.int64)
        seen = np.zeros(V, dtype=bool)
        for b in (0, 1):
            for a in (0, 1):
                pc, pr = iu + a, iv + b
                inside = (pc >= 0) & (pc < W) & (pr >= 0) & (pr < H)
                D = depth[np.clip(pr, 0, H - 1), np.clip(pc, 0, W - 1)]
                seen |= inside & (D > np.float32(0.0)) & (zc <= D.astype(np.float64) + bias)
        x = ax * u + bx
        y = ay * v + by
        inside = (x >= -0.5) & (x <= Wi - 0.5) & (y >= -0.5) & (y <= Hi - 0.5)
        ok = frame & seen & inside
        x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
        x0, y0 = np.floor(x), np.floor(y)
        wx, wy = x - x0, y - y0
        c0, c1 = np.clip(x0.astype(np.int64), 0, Wi - 1), np.clip(x0.astype(np.int64) + 1, 0, Wi - 1)
        r0, r1 = np.clip(y0.astype(np.int64), 0, Hi - 1), np.clip(y0.astype(np.int64) + 1, 0, Hi - 1)
        p00, p10 = image[r0, c0].astype(np.float64), image[r0, c1].astype(np.float64)
        p01, p11 = image[r1, c0].astype(np.float64), image[r1, c1].astype(np.float64)
        top = p00 + wx[:, None] * (p10 - p00)
        bot = p01 + wx[:, None] * (p11 - p01)
        val = top + wy[:, None] * (bot - top)
        col = np.rint(val).astype(np.uint8)
    colors = np.where(ok[:, None], col, np.array(fill, dtype=np.uint8)[None, :]).astype(np.uint8)
    return colors, ok.astype(np.uint8)


PAIRS = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))


def spread_pass(faces, colors, state):
    """One pass of svr_vertex_color_spread -> (colors, state, vertices changed); the inputs are left as they are."""
    V = state.shape[0]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < V)).all(axis=1)]
    total = np.zeros((V, 3), dtype=np.uint32)
    count = np.zeros(V, dtype=np.uint32)
    for s, d in PAIRS:
        take = (state[f[:, s]] != 0) & (state[f[:, d]] == 0)
        np.add.at(total, f[take, d], colors[f[take, s]].astype(np.uint32))
        np.add.at(count, f[take, d], np.uint32(1))
    hit = count > 0
    colors, state = colors.copy(), state.copy()
    c = count[hit].astype(np.uint32)[:, None]
    colors[hit] = ((np.uint32(2) * total[hit] + c) // (np.uint32(2) * c)).astype(np.uint8)
    state[hit] = 2
    return colors, state, int(hit.sum())


def spread(faces, colors, state, max_passes=None):
    """svr_vertex_color_spread -> (colors, state, passes that changed a vertex)."""
    colors, state = np.array(colors, dtype=np.uint8), np.array(state, dtype=np.uint8)
    passes = 0
    while max_passes is None or passes < max_passes:
        colors, state, changed = spread_pass(faces, colors, state)
        if not changed:
            break
        passes += 1
    return colors, state, passes


def vertex_colors(vertices, faces, image, depth, consts, pixel_map=IDENTITY, bias=None, do_spread=True, fill=FILL, max_passes=None):
    """util.mesh_color.vertex_colors -> colors, state."""
    k = np.asarray(consts, dtype=np.float32)
    bias = 1.0 / float(k[7]) if bias is None else bias
    colors, state = sample(vertices, consts, depth, bias, image, pixel_map, fill)
    if do_spread:
        colors, state, _ = spread(faces, colors, state, max_passes)
    return colors, state


def exact_visibility(vertices, faces, consts, eps=1e-9):
    """(V,) bool: False where a face that does not contain the vertex is accepted, by the ray caster's own pair rule, on the
    ray from the camera through the vertex at a depth z < zc - eps.  The ray's third component is s22, as a pixel ray's, so
    its parameter is the depth in metres and the vertex lies at zc."""
    g = _widened(vertices)
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    k = np.asarray(consts, dtype=np.float32).astype(np.float64)
    o = np.array([k[4], k[6], k[8]])
    zc = (g[:, 2] - k[8]) / k[7]
    d = (g - o) / zc[:, None]
    tri = R.triangle_table(g, F)
    visible = np.ones(g.shape[0], dtype=bool)
    for s in range(0, g.shape[0], 64):
        z = R.pair_z(o, d[s:s + 64], tri)                                   # (n, F), NaN = not accepted
        own = (F[None, :, :] == np.arange(s, min(s + 64, g.shape[0]))[:, None, None]).any(axis=2)
        with np.errstate(invalid="ignore"):
            visible[s:s + 64] = ~((z < (zc[s:s + 64] - eps)[:, None]) & ~own).any(axis=1)
    return visible


HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
          "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {nf}\n"
          "property list uchar int vertex_indices\nend_header\n")


def read_ply(path):
    """-> vertices (V, 3) float32, colors (V, 3) uint8, faces (F, 3) int32, the header text.  Accepts exactly the layout
    svr_write_ply documents and refuses a file with bytes missing or left over."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii")
    lines = header.split("\n")
    nv = int([l for l in lines if l.startswith("element vertex ")][0].split()[2])
    nf = int([l for l in lines if l.startswith("element face ")][0].split()[2])
    assert header == HEADER.format(nv=nv, nf=nf), header
    assert len(data) == end + 15 * nv + 13 * nf, (len(data), end, nv, nf)
    vt = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    assert vt.itemsize == 15 and ft.itemsize == 13
    v = np.frombuffer(data, dtype=vt, count=nv, offset=end)
    f = np.frombuffer(data, dtype=ft, count=nf, offset=end + 15 * nv)
    assert (f["n"] == 3).all()
    return v["xyz"].reshape(nv, 3).copy(), v["rgb"].reshape(nv, 3).copy(), f["idx"].reshape(nf, 3).copy(), header
