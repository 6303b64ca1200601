"""Damaged .exr / .npz files, each built once from an intact one: the named damages tests/test_exr_reader.py and
tests/test_sample_io.py check message by message through ctypes, and tests/test_fileio_host.py feeds, with its byte sweeps,
to the stand-alone driver.  Every entry is (name, bytes of the damaged file, ...)."""
import struct

import numpy as np

from tests import _exr as X

W, H = 37, 23                      # 37 x 23 pixels: under ZIP one block of 16 scanlines and a last block of 7


def smooth_exr(path, **kw):
    """A two-channel ramp written by the tests' own writer -> (what write_exr returns, the ramp)."""
    a = np.add.outer(np.arange(H), np.arange(W)).astype(np.float32)
    return X.write_exr(path, {"R": a, "G": a}, **kw), a


def exr_damages(whole, made, a):
    """whole / made / a: the bytes, the write_exr record and the ramp of smooth_exr(compression=ZIP).
    -> [(name, bytes, the message svr_exr_read_channel gives, whether svr_exr_info gives it too)]"""
    assert len(made["offsets"]) == 2
    out = [("cut_table", whole[:made["table"] + 8 + 3], "truncated offset table", True),        # ends in the middle of the second offset
           ("cut_header", whole[:40], "truncated header", True)]                               # ends inside the attribute list
    last = max(made["offsets"])
    size = struct.unpack("<i", whole[last + 4:last + 8])[0]
    out.append(("cut_block", whole[:last + 8 + size // 2], "is truncated", False))             # ends in the middle of the last block's payload
    out.append(("cut_block_header", whole[:last + 5], "beyond the file", False))               # ... and in the middle of its 8-byte block header
    t = made["table"] + 8
    out.append(("far_offset", whole[:t] + struct.pack("<Q", len(whole) + 1000) + whole[t + 8:], "beyond the file", False))   # second table entry points past the end
    out.append(("wrapping_offset", whole[:t] + struct.pack("<Q", (1 << 64) - 4) + whole[t + 8:], "beyond the file", False))  # ... and one that would wrap a sum
    out.append(("twice", whole[:t] + struct.pack("<Q", made["offsets"][0]) + whole[t + 8:], "appears twice", False))         # two table entries name the same block
    # a block whose deflate stream is sound but inflates to the wrong size (4 bytes short, then 4 bytes long)
    assert last == made["offsets"][-1] and last + 8 + size == len(whole)       # the last block ends the file
    nl = H - 16
    raw = b"".join(a[16 + l].tobytes() * 2 for l in range(nl))
    assert X._unpack(whole[last + 8:], len(raw)) == raw
    for tag, wrong in (("short", raw[:-4]), ("long", raw + b"\0\0\0\0")):
        packed = X._pack(wrong)
        out.append(("inflates_" + tag, whole[:last] + struct.pack("<ii", 16, len(packed)) + packed, "wrong inflated size", False))
    out.append(("no_deflate_stream", whole[:last + 8] + bytes(size), "corrupt deflate stream", False))      # zeros are no deflate stream
    return out


def npz_cuts(raw):
    return (0, 10, 30, len(raw) // 3, len(raw) // 2, len(raw) - 40, len(raw) - 22, len(raw) - 1)


def npz_damages(raw):
    """raw: the bytes of an .npz.  -> [(name, bytes)]: truncations at every region of the file, a central directory whose
    size / offset fields point past the file, an entry whose name length runs past the directory."""
    out = [(f"cut_{cut}", raw[:cut]) for cut in npz_cuts(raw)]
    eocd = raw.rfind(b"PK\x05\x06")
    assert eocd > 0
    for off, val in ((12, 0x7FFFFFF0), (16, 0x7FFFFFF0), (12, 0xFFFFFFFE)):      # cd_size / cd_offset far past the file
        b = bytearray(raw)
        b[eocd + off: eocd + off + 4] = int(val).to_bytes(4, "little")
        out.append((f"eocd_{off}_{val:x}", bytes(b)))
    cd = raw.find(b"PK\x01\x02")
    b = bytearray(raw)
    b[cd + 28: cd + 30] = (0xFFFF).to_bytes(2, "little")                          # file-name length past the directory
    out.append(("name_length", bytes(b)))
    return out


def npy_header_without_fortran_value(r):
    """r: the bytes of a STORED .npz.  -> the same with nothing but spaces behind 'fortran_order': in its first member"""
    k = r.find(b"'fortran_order': False")
    assert k > 0
    hdr_end = r.find(b"\n", k)
    b = bytearray(r)
    b[k + len(b"'fortran_order':"): hdr_end] = b" " * (hdr_end - k - len(b"'fortran_order':"))
    return bytes(b)
