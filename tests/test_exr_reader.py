"""CPU: the library's OpenEXR subset reader / writer (csrc/io_exr.cpp through data_processing.sample_io) against the real
distance map of the reference's sample and against a numpy + zlib writer / reader of the tests' own (tests/_exr.py)."""
import os

import numpy as np
import pytest

from tests import _damage as D
from tests import _exr as X

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = D.W, D.H                    # 37 x 23 pixels: under ZIP one block of 16 scanlines and a last block of 7


@pytest.fixture(scope="module")
def io():
    import __graft_entry__ as ge
    ge.build()
    from svr_amd.data_processing import sample_io
    return sample_io


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _special_floats(rng, shape):
    a = rng.standard_normal(shape).astype(np.float32)
    f = a.reshape(-1).view(np.uint32)
    f[:8] = [0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff]   # NaN payloads, +-inf, -0.0, denormals, max
    return a


def test_golden_distance_map(io):
    path = os.path.join(GOLD, "raw_distance.exr")
    info = io.exr_info(path)
    assert (info["width"], info["height"], info["origin"]) == (320, 240, (0, 0))
    assert info["channels"] == [("B", "FLOAT"), ("G", "FLOAT"), ("R", "FLOAT")] and info["compression"] == "ZIP" and info["line_order"] == 0
    want = np.load(os.path.join(GOLD, "raw_sample.npz"))["distance"]
    r = io.exr_read(path, "R")
    assert r.shape == (240, 320) and r.dtype == np.float32 and np.array_equal(_bits(r), _bits(want))
    assert np.array_equal(_bits(io.exr_read(path, "G")), _bits(r)) and np.array_equal(_bits(io.exr_read(path, "B")), _bits(r))
    assert np.array_equal(_bits(io.exr_read(path)), _bits(r))                      # the default channel is R
    own, _ = X.read_exr(path)                                                      # and the tests' decoder agrees
    assert np.array_equal(_bits(own["R"]), _bits(want))


@pytest.mark.parametrize("compression", [X.NONE, X.ZIPS, X.ZIP], ids=["NONE", "ZIPS", "ZIP"])
@pytest.mark.parametrize("ptype", ["HALF", "FLOAT", "UINT"])
def test_round_trip(io, tmp_path, compression, ptype):
    """37 x 23 pixels: under ZIP a full block of 16 scanlines and a last block of 7 (23 is no multiple of 16); the odd width
    gives HALF scanlines an odd number of 16-bit words."""
    rng = np.random.default_rng(1)
    smooth = np.add.outer(np.arange(H), np.arange(W)).astype(np.float32) / 8
    if ptype == "FLOAT":
        chans = {"R": _special_floats(rng, (H, W)), "A": smooth}
    elif ptype == "HALF":
        h = rng.integers(0, 1 << 16, (H, W), dtype=np.uint16)                      # every class of half: denormals, inf, NaN
        chans = {"R": h.view(np.float16), "A": smooth.astype(np.float16)}
    else:
        chans = {"R": rng.integers(0, 1 << 32, (H, W), dtype=np.uint32), "A": np.arange(H * W, dtype=np.uint32).reshape(H, W)}
    path = tmp_path / "a.exr"
    X.write_exr(path, chans, compression=compression)
    info = io.exr_info(path)
    assert (info["width"], info["height"]) == (W, H)
    assert info["channels"] == [("A", ptype), ("R", ptype)] and info["compression"] == {0: "NONE", 2: "ZIPS", 3: "ZIP"}[compression]
    for name, a in chans.items():
        got = io.exr_read(path, name)
        want = a.astype(np.float32)                                                 # numpy's float16 -> float32 for HALF
        assert got.shape == (H, W) and np.array_equal(_bits(got), _bits(want)), name


def test_four_channels_mixed_types_origin_and_decreasing_line_order(io, tmp_path):
    rng = np.random.default_rng(2)
    chans = {"Z": _special_floats(rng, (H, W)), "B": rng.standard_normal((H, W)).astype(np.float16),
             "id": rng.integers(0, 1 << 24, (H, W), dtype=np.uint32), "G": np.full((H, W), 0.25, np.float32)}
    for comp in (X.NONE, X.ZIPS, X.ZIP):
        path = tmp_path / f"b{comp}.exr"
        X.write_exr(path, chans, compression=comp, origin=(5, -3), line_order=1)
        info = io.exr_info(path)
        assert info["origin"] == (5, -3) and info["line_order"] == 1 and (info["width"], info["height"]) == (W, H)
        assert info["channels"] == [("B", "HALF"), ("G", "FLOAT"), ("Z", "FLOAT"), ("id", "UINT")]      # byte order: upper case first
        for name, a in chans.items():
            assert np.array_equal(_bits(io.exr_read(path, name)), _bits(a.astype(np.float32))), (comp, name)


def test_blocks_that_deflate_did_not_shrink_are_read_raw(io, tmp_path):
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 1 << 32, (H, W), dtype=np.uint32).view(np.float32)     # incompressible: stored raw by the writer
    flat = np.zeros((H, W), np.float32)
    for comp in (X.ZIPS, X.ZIP):
        path = tmp_path / f"n{comp}.exr"
        made = X.write_exr(path, {"R": noise}, compression=comp)
        assert made["stored_raw"] == len(made["offsets"])                           # every block of this file is raw
        assert np.array_equal(_bits(io.exr_read(path, "R")), _bits(noise))
    # a file that mixes deflated and raw blocks
    mixed = np.concatenate([flat[:16], noise[16:]])
    made = X.write_exr(tmp_path / "m.exr", {"R": mixed}, compression=X.ZIP)
    assert 0 < made["stored_raw"] < len(made["offsets"])
    assert np.array_equal(_bits(io.exr_read(tmp_path / "m.exr", "R")), _bits(mixed))


def _smooth_file(tmp_path, name="r.exr", **kw):
    path = tmp_path / name
    made, a = D.smooth_exr(path, **kw)
    return path, made, a


def test_refusals_name_the_reason(io, tmp_path):
    path, _, _ = _smooth_file(tmp_path, "tiled.exr", version=2 | 0x200, tiles=True)
    with pytest.raises(RuntimeError, match="tiled files are not supported"):
        io.exr_info(path)
    with pytest.raises(RuntimeError, match="tiled files are not supported"):
        io.exr_read(path, "R")
    path, _, _ = _smooth_file(tmp_path, "multi.exr", version=2 | 0x1000)
    with pytest.raises(RuntimeError, match="multi-part files are not supported"):
        io.exr_read(path, "R")
    path, _, _ = _smooth_file(tmp_path, "deep.exr", version=2 | 0x800)
    with pytest.raises(RuntimeError, match="deep files are not supported"):
        io.exr_read(path, "R")
    path, _, _ = _smooth_file(tmp_path, "piz.exr", compression=X.PIZ)
    with pytest.raises(RuntimeError, match=r"compression 4 \(PIZ\) is not supported"):
        io.exr_read(path, "R")
    path, _, _ = _smooth_file(tmp_path, "sub.exr", sampling={"G": (2, 1)})
    with pytest.raises(RuntimeError, match=r"channel 'G' is subsampled \(2 x 1\)"):
        io.exr_read(path, "R")
    path, _, _ = _smooth_file(tmp_path, "ok.exr")
    with pytest.raises(RuntimeError, match="has no channel 'Z'"):
        io.exr_read(path, "Z")
    with pytest.raises(RuntimeError, match="cannot open"):
        io.exr_info(tmp_path / "missing.exr")
    (tmp_path / "junk.exr").write_bytes(b"not an exr file at all")
    with pytest.raises(RuntimeError, match="bad magic"):
        io.exr_info(tmp_path / "junk.exr")


def test_damaged_files_are_errors_not_wild_reads(io, tmp_path):
    """The named damages of tests/_damage.py (a cut offset table, attribute list, block payload and block header; table
    entries past the end, wrapping, and naming a block twice; blocks that inflate to the wrong size or not at all)."""
    path, made, a = _smooth_file(tmp_path, "whole.exr", compression=X.ZIP)
    whole = path.read_bytes()
    assert np.array_equal(io.exr_read(path, "R"), a)
    damages = D.exr_damages(whole, made, a)
    assert [d[2] for d in damages] == ["truncated offset table", "truncated header", "is truncated", "beyond the file", "beyond the file",
                                       "beyond the file", "appears twice", "wrong inflated size", "wrong inflated size",
                                       "corrupt deflate stream"]
    for name, data, message, info_too in damages:
        bad = tmp_path / (name + ".exr")
        bad.write_bytes(data)
        with pytest.raises(RuntimeError, match=message):
            io.exr_read(bad, "R")
        if info_too:
            with pytest.raises(RuntimeError, match=message):
                io.exr_info(bad)
    assert np.array_equal(io.exr_read(path, "R"), a)       # the process is alive and well


def test_writer_round_trips_through_the_tests_decoder(io, tmp_path):
    rng = np.random.default_rng(4)
    z = _special_floats(rng, (H, W))
    conf = rng.random((H, W), dtype=np.float32)
    path = tmp_path / "w.exr"
    io.exr_write(path, {"Z": z, "A": conf})                # given out of order: written alphabetically
    got, head = X.read_exr(path)
    assert head["channels"] == [("A", X.FLOAT), ("Z", X.FLOAT)] and head["compression"] == X.NONE and head["origin"] == (0, 0)
    assert np.array_equal(_bits(got["Z"]), _bits(z)) and np.array_equal(_bits(got["A"]), _bits(conf))
    assert np.array_equal(_bits(io.exr_read(path, "Z")), _bits(z))             # and through the library's own reader
    info = io.exr_info(path)
    assert (info["width"], info["height"], info["compression"]) == (W, H, "NONE")
    with pytest.raises(RuntimeError, match="exr_write: cannot open"):
        io.exr_write(tmp_path / "no_such_dir" / "w.exr", {"Z": z})
