"""Native readers for the sample wire formats: thin numpy-level wrappers over the C ABI's host
functions (svr_df_*, svr_npz_member_*, svr_exr_*: plain C++ + zlib, csrc/io_df.cpp / io_npz.cpp / io_exr.cpp, linked into
libsvr_hip.so; no GPU involved) and the device-side helpers of csrc/sample_io.hip
(transpose / cast / row subset).  `out=` lets the caller pass a pinned buffer so the H2D copy can be asynchronous."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream

_NP = {0: np.float32, 1: np.float64, 2: np.bool_, 3: np.uint8, 4: np.int32, 5: np.int64}
_CODE = {torch.float32: 0, torch.float64: 1, torch.bool: 2, torch.uint8: 3, torch.int32: 4, torch.int64: 5}


def _path(p):
    return os.fspath(p).encode()


def df_dims(path):
    dims = (C.c_int64 * 3)()
    check(_lib.lib().svr_df_dims(_path(path), dims), "df_dims")
    return tuple(int(d) for d in dims)


def df_read_payload(path, out=None):
    """The raw float32 payload (x fastest) of a .df file as a flat array; `out`: a flat float32 numpy array (e.g. the
    numpy view of a pinned tensor) of the right length."""
    X, Y, Z = df_dims(path)
    n = X * Y * Z
    if out is None:
        out = np.empty(n, dtype=np.float32)
    assert out.dtype == np.float32 and out.size == n and out.flags["C_CONTIGUOUS"]
    check(_lib.lib().svr_df_read(_path(path), out.ctypes.data_as(C.c_void_p), n), "df_read")
    return out, (X, Y, Z)


def grid_to_df(grid):
    """(X, Y, Z) array (host, or a device tensor: copied to the host) -> the flat float32 payload of a .df file, x fastest:
    the inverse of df_to_grid, on the host."""
    if torch.is_tensor(grid):
        grid = grid.detach().cpu().numpy()
    grid = np.asarray(grid, dtype=np.float32)
    if grid.ndim != 3:
        raise ValueError(f"grid_to_df: an (X, Y, Z) array, got shape {grid.shape}")
    return np.ascontiguousarray(grid.reshape(-1, order="F"))


def df_write(path, grid):
    """Write a host or device (X, Y, Z) array as a .df file: three little-endian uint64 extents, then the float32 values
    with x fastest (what df_dims / df_read_payload parse).  Raises on a failed open or write."""
    payload = grid_to_df(grid)
    X, Y, Z = grid.shape
    check(_lib.lib().svr_df_write(_path(path), payload.ctypes.data_as(C.c_void_p), X, Y, Z), "df_write")
    return path


def npz_member_info(path, member):
    dt, nd, fo = C.c_int32(), C.c_int32(), C.c_int32()
    shape = (C.c_int64 * 8)()
    check(_lib.lib().svr_npz_member_info(_path(path), member.encode(), C.byref(dt), C.byref(nd), shape, C.byref(fo)),
          "npz_member_info")
    return _NP[dt.value], tuple(int(shape[i]) for i in range(nd.value)), bool(fo.value)


def npz_load(path, member, out=None):
    """np.load(path)[member] through the native reader (stored or deflated member)."""
    dtype, shape, fortran = npz_member_info(path, member)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if out is None:
        out = np.empty(n, dtype=dtype)
    assert out.dtype == dtype and out.size == n and out.flags["C_CONTIGUOUS"]
    check(_lib.lib().svr_npz_member_read(_path(path), member.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes),
          "npz_member_read")
    return out.reshape(shape, order="F" if fortran else "C")


EXR_PIXEL_TYPES = {0: "UINT", 1: "HALF", 2: "FLOAT"}
EXR_COMPRESSIONS = {0: "NONE", 2: "ZIPS", 3: "ZIP"}


def exr_info(path):
    """Header of a single-part scanline OpenEXR file (the subset of include/svr_hip.h): {"width", "height", "origin": the
    data window's (x, y) minimum, "channels": [(name, "UINT" | "HALF" | "FLOAT")] in the file's order, "compression":
    "NONE" | "ZIPS" | "ZIP", "line_order"}.  Anything outside the subset raises with the reason."""
    w, h, n, comp, lo = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    origin = (C.c_int32 * 2)()
    names = C.create_string_buffer(1 << 16)
    types = (C.c_int32 * 1024)()
    check(_lib.lib().svr_exr_info(_path(path), C.byref(w), C.byref(h), origin, C.byref(n), names, len(names), types, 1024,
                                  C.byref(comp), C.byref(lo)), "exr_info")
    nm = names.raw.split(b"\0")[:n.value]
    return {"width": w.value, "height": h.value, "origin": (origin[0], origin[1]),
            "channels": [(nm[i].decode(), EXR_PIXEL_TYPES[types[i]]) for i in range(n.value)],
            "compression": EXR_COMPRESSIONS[comp.value], "line_order": lo.value}


def exr_read(path, channel="R", out=None):
    """One channel as an (H, W) float32 array, top scanline first (pyexr.open(path).get(channel)[:, :, 0]); `out`: a
    float32 numpy array of H * W values, e.g. the numpy view of a pinned tensor."""
    info = exr_info(path)
    H, W = info["height"], info["width"]
    if out is None:
        out = np.empty(H * W, dtype=np.float32)
    assert out.dtype == np.float32 and out.size == H * W and out.flags["C_CONTIGUOUS"]
    check(_lib.lib().svr_exr_read_channel(_path(path), channel.encode(), out.ctypes.data_as(C.c_void_p), H * W), "exr_read_channel")
    return out.reshape(H, W)


def exr_write(path, channels):
    """{name: (H, W) array} -> an uncompressed FLOAT scanline file (what visualize_depthmap's .exr output needs)."""
    names = list(channels)
    planes = np.ascontiguousarray(np.stack([np.asarray(channels[k], dtype=np.float32) for k in names]))
    assert planes.ndim == 3, "exr_write: every channel is an (H, W) array"
    check(_lib.lib().svr_exr_write(_path(path), planes.ctypes.data_as(C.c_void_p), planes.shape[1], planes.shape[2],
                                   b"\0".join(k.encode() for k in names) + b"\0", len(names)), "exr_write")


# ---- device side -------------------------------------------------------------------------------------------------
def df_to_grid(payload, dims):
    """device float32 payload (x fastest) -> (X, Y, Z) C-order float32 tensor."""
    X, Y, Z = dims
    out = torch.empty(X, Y, Z, device=payload.device, dtype=torch.float32)
    check(_lib.lib().svr_df_to_grid(ptr(payload), ptr(out), X, Y, Z, stream()), "df_to_grid")
    return out


def cast_to_f32(t):
    t = t.contiguous()
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    check(_lib.lib().svr_cast_to_f32(ptr(t), _CODE[t.dtype], ptr(out), t.numel(), stream()), "cast_to_f32")
    return out


def subsample_rows(rows, idx):
    """out[i] = float32(rows[idx[i]]) for a (n_rows, cols) or (n_rows,) device tensor of float64 / float32 / bool."""
    rows = rows.contiguous()
    cols = 1 if rows.dim() == 1 else rows.shape[1]
    idx = idx.to(device=rows.device, dtype=torch.int64).contiguous()
    out = torch.empty((idx.numel(),) if rows.dim() == 1 else (idx.numel(), cols), device=rows.device, dtype=torch.float32)
    bad = torch.zeros(1, device=rows.device, dtype=torch.int32)
    check(_lib.lib().svr_subsample_rows(ptr(rows), _CODE[rows.dtype], rows.shape[0], cols, ptr(idx), idx.numel(), ptr(out),
                                        ptr(bad), stream()), "subsample_rows")
    return out, bad


ROW_SEGMENT_WORDS = 6      # sizeof(svr_row_segment) / 8: rows, n_rows, idx_offset, n_idx, out_offset, (dtype | cols << 32)


def pack_row_segments(segments, n_index, n_out, pin=True):
    """The host side of svr_subsample_rows_batched: ONE int64 buffer ``[elem_prefix (S + 1) | svr_row_segment table (6 S) |
    indices (n_index)]`` (pinned by default), so that prefix, table and indices cross in a single copy.

    `segments`: S tuples ``(rows, idx_offset, n_idx, out_offset)``; `rows` a contiguous device tensor (n_rows, cols) or
    (n_rows,) of float32 / float64 / bool / uint8, the offsets in elements of the shared index buffer (`n_index` entries)
    and of the shared float32 output (`n_out` entries).  Every range is checked here, on the host: the kernel trusts the
    table.  Returns ``(buffer, indices, total)``: `indices` is the numpy view of the buffer's index part, for the caller to
    fill; `total` the number of output elements."""
    S = len(segments)
    buf = torch.empty((S + 1) + ROW_SEGMENT_WORDS * S + n_index, dtype=torch.int64, pin_memory=pin)
    a = buf.numpy()
    table = a[S + 1:S + 1 + ROW_SEGMENT_WORDS * S].reshape(S, ROW_SEGMENT_WORDS)
    total, taken = 0, []
    a[0] = 0
    for s, (rows, idx_offset, n_idx, out_offset) in enumerate(segments):
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.is_contiguous() and rows.dim() in (1, 2)):
            raise ValueError("subsample_rows_batched: rows must be a contiguous (n_rows, cols) or (n_rows,) device tensor")
        if rows.dtype not in (torch.float32, torch.float64, torch.bool, torch.uint8):
            raise ValueError(f"subsample_rows_batched: dtype {rows.dtype}")
        cols = 1 if rows.dim() == 1 else int(rows.shape[1])
        n_rows, n_idx, idx_offset, out_offset = int(rows.shape[0]), int(n_idx), int(idx_offset), int(out_offset)
        if n_idx < 0 or (n_idx > 0 and (cols <= 0 or n_rows <= 0)):
            raise ValueError("subsample_rows_batched: empty source")
        if idx_offset < 0 or idx_offset + n_idx > n_index or out_offset < 0 or out_offset + n_idx * cols > n_out:
            raise ValueError(f"subsample_rows_batched: segment {s} reaches outside the index buffer or the output")
        if n_idx:
            taken.append((out_offset, out_offset + n_idx * cols))
        table[s] = (rows.data_ptr(), n_rows, idx_offset, n_idx, out_offset, _CODE[rows.dtype] | (max(cols, 1) << 32))
        total += n_idx * cols
        a[s + 1] = total
    taken.sort()
    if any(taken[i][1] > taken[i + 1][0] for i in range(len(taken) - 1)):
        raise ValueError("subsample_rows_batched: output ranges overlap")
    return buf, a[S + 1 + ROW_SEGMENT_WORDS * S:], total


def subsample_rows_batched(packed, n_segments, total, out, bad=None):
    """One launch for every segment of `packed` (the DEVICE copy of pack_row_segments' buffer, which also fixed `total`):
    out[out_offset + i * cols + c] = float32(rows[idx[idx_offset + i], c]).  `out`: the contiguous float32 device tensor the
    table was checked against; `bad` (optional int32 (1,) device tensor) is set to 1 by a row outside [0, n_rows), which
    writes 0.  No segments or no indices: nothing is launched."""
    if n_segments <= 0 or total <= 0:
        return out
    if not (packed.is_cuda and packed.dtype == torch.int64 and packed.is_contiguous() and out.is_cuda
            and out.dtype == torch.float32 and out.is_contiguous()):
        raise RuntimeError("subsample_rows_batched needs a device int64 table and a contiguous float32 device output")
    base = packed.data_ptr()
    table = base + 8 * (n_segments + 1)
    check(_lib.lib().svr_subsample_rows_batched(C.c_void_p(table), C.c_void_p(base), n_segments, total,
                                                C.c_void_p(table + 8 * ROW_SEGMENT_WORDS * n_segments),
                                                ptr(out), ptr(bad), stream()), "subsample_rows_batched")
    return out
