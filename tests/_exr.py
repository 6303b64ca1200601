"""A small OpenEXR writer and reader in numpy + zlib for the tests: independent of the library's C++ code, it produces the
files the reader is tested on (every supported compression / pixel type / line order / data-window origin) and decodes
what the library's writer produces."""
import struct
import zlib

import numpy as np

UINT, HALF, FLOAT = 0, 1, 2
NONE, ZIPS, ZIP, PIZ = 0, 2, 3, 4
_NP = {UINT: np.dtype("<u4"), HALF: np.dtype("<f2"), FLOAT: np.dtype("<f4")}
_LINES = {NONE: 1, ZIPS: 1, ZIP: 16}


def _attr(name, typ, payload):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload


def _pack(raw):
    """the ZIP(S) transform: split into even / odd bytes, delta code, deflate"""
    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int64)
    d = np.concatenate([t[:1], (t[1:] - t[:-1] + 128 + 256) % 256]).astype(np.uint8)
    return zlib.compress(d.tobytes(), 6)


def _unpack(packed, raw_size):
    d = np.frombuffer(zlib.decompress(packed), np.uint8).astype(np.int64)
    assert d.size == raw_size
    t = (np.cumsum(np.concatenate([d[:1], d[1:] - 128])) % 256).astype(np.uint8)
    half = (raw_size + 1) // 2
    u = np.empty(raw_size, np.uint8)
    u[0::2], u[1::2] = t[:half], t[half:]
    return u.tobytes()


def write_exr(path, channels, compression=ZIP, origin=(0, 0), line_order=0, version=2, sampling=None, tiles=False):
    """channels: {name: (H, W) array of dtype uint32 / float16 / float32}, written in alphabetical order.
    -> {"table": offset of the offset table, "offsets": block offsets in table (increasing y) order, "stored_raw": how many
    blocks deflate did not shrink}.  `version`, `sampling` ({name: (xs, ys)}) and `tiles` only doctor the header."""
    names = sorted(channels)
    arrs = []
    for n in names:
        a = np.asarray(channels[n])
        code = {np.dtype("uint32"): UINT, np.dtype("float16"): HALF, np.dtype("float32"): FLOAT}[a.dtype]
        arrs.append((code, np.ascontiguousarray(a.astype(_NP[code]))))
    H, W = arrs[0][1].shape
    x0, y0 = origin
    chlist = b""
    for n, (code, _) in zip(names, arrs):
        xs, ys = (sampling or {}).get(n, (1, 1))
        chlist += n.encode() + b"\0" + struct.pack("<iB3xii", code, 0, xs, ys)
    box = struct.pack("<4i", x0, y0, x0 + W - 1, y0 + H - 1)
    head = struct.pack("<II", 20000630, version)
    head += _attr("channels", "chlist", chlist + b"\0") + _attr("compression", "compression", bytes([compression]))
    head += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box)
    head += _attr("lineOrder", "lineOrder", bytes([line_order])) + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    head += _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0)) + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    if tiles:
        head += _attr("tiles", "tiledesc", struct.pack("<IIB", 32, 32, 0))
    head += b"\0"
    lines = _LINES.get(compression, 1)
    blocks, stored_raw = [], 0
    for r0 in range(0, H, lines):
        nl = min(lines, H - r0)
        raw = b"".join(a[r0 + l].tobytes() for l in range(nl) for _, a in arrs)
        data = raw
        if compression in (ZIPS, ZIP):
            packed = _pack(raw)
            if len(packed) < len(raw):
                data = packed
            else:
                stored_raw += 1
        blocks.append(struct.pack("<ii", y0 + r0, len(data)) + data)
    order = range(len(blocks)) if line_order == 0 else reversed(range(len(blocks)))     # where each block lies in the file
    offsets, pos = [0] * len(blocks), len(head) + 8 * len(blocks)
    body = b""
    for k in order:
        offsets[k] = pos
        body += blocks[k]
        pos += len(blocks[k])
    with open(path, "wb") as f:
        f.write(head + struct.pack(f"<{len(blocks)}Q", *offsets) + body)
    return {"table": len(head), "offsets": offsets, "stored_raw": stored_raw}


def read_exr(path):
    """{name: (H, W) array in the channel's own dtype} + the header facts, for single-part scanline NONE / ZIPS / ZIP files."""
    b = open(path, "rb").read()
    assert struct.unpack("<II", b[:8]) == (20000630, 2)
    p, attrs = 8, {}
    while b[p] != 0:
        e = b.index(0, p)
        name = b[p:e].decode()
        p = b.index(0, e + 1) + 1
        size = struct.unpack("<i", b[p:p + 4])[0]
        attrs[name] = b[p + 4:p + 4 + size]
        p += 4 + size
    p += 1
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"])
    W, H = x1 - x0 + 1, y1 - y0 + 1
    chans, c, q = [], attrs["channels"], 0
    while c[q] != 0:
        e = c.index(0, q)
        chans.append((c[q:e].decode(), struct.unpack("<i", c[e + 1:e + 5])[0]))
        q = e + 17
    comp = attrs["compression"][0]
    lines = _LINES[comp]
    nblk = -(-H // lines)
    out = {n: np.zeros((H, W), _NP[t]) for n, t in chans}
    line_bytes = sum(W * _NP[t].itemsize for _, t in chans)
    for off in struct.unpack(f"<{nblk}Q", b[p:p + 8 * nblk]):
        y, size = struct.unpack("<ii", b[off:off + 8])
        data = b[off + 8:off + 8 + size]
        nl = min(lines, H - (y - y0))
        if comp and size < nl * line_bytes:
            data = _unpack(data, nl * line_bytes)
        assert len(data) == nl * line_bytes
        q = 0
        for l in range(nl):
            for n, t in chans:
                out[n][y - y0 + l] = np.frombuffer(data[q:q + W * _NP[t].itemsize], _NP[t])
                q += W * _NP[t].itemsize
    return out, {"origin": (x0, y0), "compression": comp, "channels": chans, "attrs": attrs}
