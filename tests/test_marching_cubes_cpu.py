"""CPU: the marching-cubes case table the kernels use (svr_mc_case_table, built from a rule in csrc/mc_table.h), the numpy
oracle the GPU tests compare against, and the host .obj writer (svr_write_obj) read back by the repository's load_obj."""
import ctypes
import math

import numpy as np
import pytest

from tests import mc_oracle as M


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as ge
    ge.build()
    return M.case_table()


def _crossing_edges(case):
    out = set()
    for e in range(12):
        ax, off = M.edge_endpoints(e)
        c0 = int(off[0] | off[1] << 1 | off[2] << 2)
        c1 = c0 | (1 << ax)
        if ((case >> c0) & 1) != ((case >> c1) & 1):
            out.add(e)
    return out


def test_case_table_shape_and_edges(table):
    assert table.shape == (256, 16)
    counts = []
    for case in range(256):
        row = table[case]
        n = int((row >= 0).sum())
        assert n % 3 == 0 and (row[:n] >= 0).all() and (row[n:] == -1).all(), case
        assert n // 3 <= 5, case
        counts.append(n // 3)
        cross = _crossing_edges(case)
        assert set(row[:n].tolist()) == cross, case          # only (and every one of) the case's crossing edges
    assert counts[0] == 0 and counts[255] == 0
    assert sum(counts) == 820


@pytest.mark.parametrize("case", range(1, 255))
def test_every_case_alone_gives_a_closed_outward_mesh(table, case):
    f = np.full((4, 4, 4), 1.0, dtype=np.float32)            # outside everywhere but the cell's inside corners
    for c, off in enumerate(M.CORNERS):
        if (case >> c) & 1:
            f[1 + off[0], 1 + off[1], 1 + off[2]] = -1.0
    v, fa = M.marching_cubes(f, 0.0, table)
    assert len(fa) > 0 and M.is_closed(fa), case
    assert M.signed_volume(v, fa) > 0, case


def test_oracle_sphere_topology_and_volume(table):
    v, f = M.marching_cubes(M.sphere(24, 8.0), 0.0, table)
    assert M.is_closed(f) and M.euler_characteristic(v, f) == 2
    vol = M.signed_volume(v, f)
    assert abs(vol - 4.0 / 3.0 * math.pi * 8.0 ** 3) < 0.02 * 4.0 / 3.0 * math.pi * 8.0 ** 3


def test_oracle_torus_topology(table):
    v, f = M.marching_cubes(M.torus(), 0.0, table)
    assert M.is_closed(f) and M.euler_characteristic(v, f) == 0 and M.signed_volume(v, f) > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_random_noise_is_closed(table, seed):
    rng = np.random.default_rng(seed)
    f = np.ones((14, 12, 10), dtype=np.float32)
    f[1:-1, 1:-1, 1:-1] = rng.standard_normal((12, 10, 8)).astype(np.float32)   # bounded by an outside shell
    v, fa = M.marching_cubes(f, 0.0, table)
    assert len(fa) > 100 and M.is_closed(fa) and M.signed_volume(v, fa) > 0


@pytest.mark.parametrize("n", [0, 1, 7, 5000])
def test_write_obj_round_trip(tmp_path, n):
    import __graft_entry__ as ge
    ge.build()
    import svr_amd
    from svr_amd.data_processing.mesh_occupancies import load_obj
    rng = np.random.default_rng(n)
    v = (rng.standard_normal((n, 3)) * 10.0 ** rng.integers(-6, 6, (n, 1))).astype(np.float32)
    if n:
        v[0] = [np.float32(1 / 3), np.nextafter(np.float32(2), np.float32(3)), np.float32(1e-38)]
    f = rng.integers(0, max(n, 1), (2 * n, 3)).astype(np.int32)
    p = tmp_path / "m.obj"
    rc = svr_amd._lib.lib().svr_write_obj(str(p).encode(), v.ctypes.data_as(ctypes.c_void_p), n,
                                          f.ctypes.data_as(ctypes.c_void_p), len(f))
    assert rc == 0
    m = load_obj(str(p))
    assert m.vertices.shape == (n, 3) and m.faces.shape == (2 * n, 3)
    assert np.array_equal(m.vertices.astype(np.float32).view(np.uint32), v.view(np.uint32))
    assert np.array_equal(m.faces, f)


def test_write_obj_reports_io_errors(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    import svr_amd
    from svr_amd.util.visualize import export_obj
    assert svr_amd._lib.lib().svr_write_obj(str(tmp_path / "no" / "such" / "dir.obj").encode(), None, 0, None, 0) == -5
    with pytest.raises(RuntimeError):
        export_obj(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), tmp_path / "no" / "dir.obj")


def test_marching_cubes_refuses_cpu_tensors():
    import torch
    import svr_amd  # noqa: F401
    from svr_amd.util.visualize import marching_cubes
    with pytest.raises(RuntimeError):
        marching_cubes(torch.zeros(4, 4, 4), 0.5)
