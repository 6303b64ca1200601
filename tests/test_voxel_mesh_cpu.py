"""CPU: the voxel-mesher ABI is exported and refuses oversized lattices, the numpy oracle the GPU tests compare against
(tests/voxel_mesh_oracle.py) produces closed outward surfaces of the right volume and area, and the two host writers
(svr_write_png_gray8, svr_write_obj_points) write exactly what a PNG decoder / the reference's format expression expect."""
import ctypes

import numpy as np
import pytest

from tests import voxel_mesh_oracle as V


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import svr_amd
    return svr_amd._lib.lib()


def test_abi_symbols_and_lattice_limit(lib):
    import svr_amd
    raw = ctypes.CDLL(svr_amd._lib.LIB_PATH)
    for name in ("svr_voxel_mesh_workspace_bytes", "svr_voxel_mesh_count", "svr_voxel_mesh_emit", "svr_depth_minmax",
                 "svr_depth_planes", "svr_write_png_gray8", "svr_write_obj_points"):
        assert hasattr(raw, name) and name in svr_amd._lib.SIGNATURES, name
    assert lib.svr_voxel_mesh_workspace_bytes(139, 104, 112) > 17 * 140 * 105 * 113
    assert lib.svr_voxel_mesh_workspace_bytes(0, 5, 5) > 0
    # the corner lattice has (X+1)(Y+1)(Z+1) points and must stay below 2^31
    assert lib.svr_voxel_mesh_workspace_bytes(2047, 1023, 1023) == -2            # 2048 * 1024 * 1024 = 2^31
    assert lib.svr_voxel_mesh_workspace_bytes(2046, 1023, 1023) > 0              # 2047 * 2^20 < 2^31
    assert lib.svr_voxel_mesh_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == -2
    assert lib.svr_voxel_mesh_workspace_bytes(-1, 4, 4) == -2
    assert b"2^31" in lib.svr_last_error()


def _two(shape, a, b):
    g = np.zeros(shape, dtype=np.float32)
    g[a] = 1
    g[b] = 1
    return g


ORACLE_CASES = {
    "single": (np.ones((1, 1, 1), dtype=np.float32), 8, 12),
    "face_adjacent": (_two((2, 1, 1), (0, 0, 0), (1, 0, 0)), 12, 20),
    "edge_touching": (_two((2, 2, 1), (0, 0, 0), (1, 1, 0)), 14, 24),
    "corner_touching": (_two((2, 2, 2), (0, 0, 0), (1, 1, 1)), 15, 24),
    "full_3x4x5": (np.ones((3, 4, 5), dtype=np.float32), None, 2 * 2 * (3 * 4 + 4 * 5 + 3 * 5)),
    "random_7x6x5": ((np.random.default_rng(7).random((7, 6, 5)) < 0.4).astype(np.float32), None, None),
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_oracle_surfaces_are_closed_outward_and_exact(name):
    grid, nv, nf = ORACLE_CASES[name]
    v, f = V.voxel_mesh(grid)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape[1] == 3 and f.shape[1] == 3
    if nv is not None:
        assert len(v) == nv
    if nf is not None:
        assert len(f) == nf
    occ = V.occupancy(grid)
    assert V.signed_volume(v, f) == float(occ.sum())                   # exact: coordinates are multiples of 1/2
    assert V.area(v, f) == len(f) / 2                                  # one unit square per emitted quad
    assert V.edges_balanced(f)
    V.check_surface(grid, v, f)                                        # + every triangle's normal is its face direction
    # vertices ascend in corner C order, faces in (voxel C order, direction) order
    cidx = np.ravel_multi_index(tuple((v + 0.5).astype(np.int64).T), tuple(s + 1 for s in grid.shape))
    assert (np.diff(cidx) > 0).all()


def test_oracle_threshold_and_nan():
    g = np.array([[[0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, 1.0]]], dtype=np.float32)
    assert V.occupancy(g).tolist() == [[[True, False, False, True]]]
    v, f = V.voxel_mesh(g)
    assert len(v) == 16 and len(f) == 24


# ---- svr_write_png_gray8 ------------------------------------------------------------------------------------------
def _png_images():
    rng = np.random.default_rng(3)
    ramp = (np.arange(240 * 320, dtype=np.int64).reshape(240, 320) * 255 // (240 * 320 - 1)).astype(np.uint8)
    return {"1x1": np.array([[137]], dtype=np.uint8), "3x5": rng.integers(0, 256, (3, 5)).astype(np.uint8),
            "240x320_ramp": ramp, "240x320_noise": rng.integers(0, 256, (240, 320)).astype(np.uint8)}


@pytest.mark.parametrize("name", ["1x1", "3x5", "240x320_ramp", "240x320_noise"])
def test_write_png_gray8(lib, tmp_path, name):
    img = np.ascontiguousarray(_png_images()[name])
    p = tmp_path / "a.png"
    assert lib.svr_write_png_gray8(str(p).encode(), img.ctypes.data_as(ctypes.c_void_p), img.shape[0], img.shape[1]) == 0
    assert np.array_equal(V.decode_png_gray8(p.read_bytes()), img)


@pytest.mark.parametrize("name", ["1x1", "3x5", "240x320_ramp", "240x320_noise"])
def test_write_png_gray8_decodes_with_pil(lib, tmp_path, name):
    Image = pytest.importorskip("PIL.Image")
    img = np.ascontiguousarray(_png_images()[name])
    p = tmp_path / "a.png"
    assert lib.svr_write_png_gray8(str(p).encode(), img.ctypes.data_as(ctypes.c_void_p), img.shape[0], img.shape[1]) == 0
    with Image.open(p) as im:
        assert im.mode == "L" and im.size == (img.shape[1], img.shape[0])
        assert np.array_equal(np.asarray(im), img)


def test_write_png_gray8_refuses_bad_arguments(lib, tmp_path):
    img = np.zeros((2, 2), dtype=np.uint8)
    ptr = img.ctypes.data_as(ctypes.c_void_p)
    assert lib.svr_write_png_gray8(str(tmp_path / "a.png").encode(), ptr, 0, 2) == -2
    assert lib.svr_write_png_gray8(str(tmp_path / "a.png").encode(), None, 2, 2) == -1
    assert lib.svr_write_png_gray8(str(tmp_path / "no" / "dir.png").encode(), ptr, 2, 2) == -5


# ---- svr_write_obj_points -----------------------------------------------------------------------------------------
def _reference_point_lines(grid):
    """util/visualize.py:14-20 of the reference, its format expression typed out (grid: float32 rows, so numpy 2 adds the 0.5 in
    float32)."""
    out = []
    for i in range(grid.shape[0]):
        x, y, z = grid[i, 0], grid[i, 1], grid[i, 2]
        c = [1, 1, 1]
        out.append('v %f %f %f %f %f %f\n' % (x + 0.5, y + 0.5, z + 0.5, c[0], c[1], c[2]))
    return "".join(out)


def test_write_obj_points_matches_the_reference_format(lib, tmp_path):
    rng = np.random.default_rng(11)
    pts = (rng.standard_normal((1000, 3)) * 10.0 ** rng.integers(-3, 3, (1000, 1))).astype(np.float32)
    # values whose sixth decimal sits on a rounding edge, negatives, integers (voxel indices), zero
    pts[:6] = [[0.0000005, -0.5000005, 1.0000015], [-0.5, -1.5, 2.5], [137.0, 103.0, 111.0], [0.0, -0.0, 1e-7],
               [0.1234565, -0.1234565, 0.0000025], [-3.4999995, 2.4999995, -0.0000005]]
    p = tmp_path / "pc.obj"
    assert lib.svr_write_obj_points(str(p).encode(), pts.ctypes.data_as(ctypes.c_void_p), len(pts)) == 0
    assert p.read_bytes() == _reference_point_lines(pts).encode()
    # through the Python surface, from an int64 point list
    import svr_amd  # noqa: F401
    from svr_amd.util.visualize import to_point_list, visualize_point_list
    grid = (rng.random((5, 4, 3)) < 0.3).astype(np.float32)
    pl = to_point_list(grid)
    assert pl.dtype == np.int64 and np.array_equal(pl, np.stack(np.where(grid >= 0.5), axis=1))
    visualize_point_list(pl, tmp_path / "pl.obj")
    assert (tmp_path / "pl.obj").read_bytes() == _reference_point_lines(pl.astype(np.float32)).encode()


def test_write_obj_points_empty_and_io_error(lib, tmp_path):
    p = tmp_path / "empty.obj"
    assert lib.svr_write_obj_points(str(p).encode(), None, 0) == 0
    assert p.read_bytes() == b""
    assert lib.svr_write_obj_points(str(tmp_path / "no" / "dir.obj").encode(), None, 0) == -5
    assert lib.svr_write_obj_points(str(p).encode(), None, 3) == -1


def test_device_functions_refuse_cpu_tensors():
    import torch
    import svr_amd  # noqa: F401
    from svr_amd.util.visualize import to_point_list, visualize_depthmap, voxel_mesh
    with pytest.raises(RuntimeError):
        voxel_mesh(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError):
        to_point_list(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError):
        visualize_depthmap(torch.ones(4, 4), "nowhere")
