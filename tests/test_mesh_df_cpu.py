"""CPU: the distance-field oracle (tests/df_oracle.py, the numpy restatement of include/svr_hip.h's svr_mesh_df_* rule)
against an independent routine and an analytic bound, the .df writer, and process_sample's new argument."""
import ctypes
import inspect
import os
import struct

import numpy as np
import pytest

from tests import df_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps


def _mesh(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z["vertices"].astype(np.float64), z["faces"].astype(np.int32)


def _segment_dd(p, a, b):
    ab = b - a
    t = np.clip(((p - a) * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    e = p - (a + t[..., None] * ab)
    return (e * e).sum(-1)


def _independent_dd(points, tri):
    """(P, F): project the point onto the face's plane; accept the projection when its barycentric coordinates are in
    range, otherwise the minimum over the three segments.  None of the oracle's d1..d6 / va, vb, vc."""
    p = points[:, None, :]
    a, b, c = tri[None, :, 0:3], tri[None, :, 3:6], tri[None, :, 6:9]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    h = ((p - a) * n).sum(-1) / nn                     # signed plane distance over |n|
    q = p - h[..., None] * n
    # barycentric coordinates of q from the sub-triangle normals
    wa = (np.cross(b - q, c - q) * n).sum(-1) / nn
    wb = (np.cross(c - q, a - q) * n).sum(-1) / nn
    wc = (np.cross(a - q, b - q) * n).sum(-1) / nn
    inside = (wa >= 0) & (wb >= 0) & (wc >= 0)
    plane = h * h * nn
    edges = np.minimum(np.minimum(_segment_dd(p, a, b), _segment_dd(p, b, c)), _segment_dd(p, c, a))
    return np.where(inside, plane, edges)


@pytest.mark.parametrize("name", ["mesh_sphere", "mesh_torus", "mesh_openbox"])
def test_oracle_agrees_with_an_independent_routine(name):
    """300 random points per committed mesh; |dd_oracle - dd_independent| <= 64 * eps * max(1, scale^2), scale the largest
    coordinate magnitude of points and vertices.  The factor comes from the operation count, not from a measurement: each
    routine reaches its dd through a chain of at most ~15 rounded float64 operations (differences, a dot product, one
    division, the closest point, a difference, a dot product) on quantities bounded by a few scale^2, i.e. at most
    ~16 eps scale^2 each once the growth through the division by a well-conditioned denominator is counted; two routines
    give 32, and a point on a region border, where the two pick different but adjacent formulas for the same closest
    point, doubles that.  The measured maximum is printed; on these meshes it is a few eps."""
    V, F = _mesh(name)
    tri = O.triangle_table(V, F)
    assert O.has_area(tri).all()
    rng = np.random.default_rng(11)
    lo, hi = V.min(0), V.max(0)
    pts = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), size=(300, 3))
    scale = max(np.abs(pts).max(), np.abs(V).max())
    a, b = O.pair_dd(pts, tri), _independent_dd(pts, tri)
    err = np.abs(a - b).max()
    bound = 64 * EPS * max(1.0, scale * scale)
    print(f"{name}: max |dd - dd'| = {err:.3e} = {err / EPS:.1f} eps, bound {bound:.3e}")
    assert err <= bound
    # and the per-point minimum picks the same distance
    field, face = O.distance_at(pts, tri)
    assert np.abs(field.astype(np.float64) ** 2 - b.min(axis=1)).max() <= bound + 2 ** -23 * b.min(axis=1).max()
    assert (face >= 0).all() and (face < len(F)).all()


def test_oracle_sphere_bound():
    """Icosphere with centre c0, circumradius R, inradius r_in (the minimum plane distance of a face from c0): the surface
    lies in the shell r_in <= |x - c0| <= R and every ray from c0 crosses it, so | d(p) - | |p - c0| - R | | <= R - r_in."""
    V, F = _mesh("mesh_sphere")
    c0 = 0.5 * (V.min(0) + V.max(0))
    rad = np.linalg.norm(V - c0, axis=1)
    R = rad.max()
    assert rad.min() > R * (1 - 1e-6), "not an icosphere about the centre of its bounding box"
    tri = O.triangle_table(V, F)
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    n = np.cross(b - a, c - a)
    r_in = (np.abs(((a - c0) * n).sum(-1)) / np.linalg.norm(n, axis=1)).min()
    assert 0 < r_in < R
    rng = np.random.default_rng(5)
    pts = np.concatenate([c0 + rng.uniform(-2 * R, 2 * R, size=(600, 3)), c0[None], V[:20]])
    field, _ = O.distance_at(pts, tri)
    gap = np.abs(field.astype(np.float64) - np.abs(np.linalg.norm(pts - c0, axis=1) - R))
    print(f"sphere: R={R:.6f} r_in={r_in:.6f} max gap {gap.max():.6f} of {R - r_in:.6f}")
    assert gap.max() <= (R - r_in) + 1e-6 * R          # float32 output: 2^-24 relative, far inside the margin


def test_oracle_tie_and_zero_area_rules():
    a, b, c = [0.0, 0, 0], [4.0, 0, 0], [0.0, 4, 0]
    V = np.array([a, b, c, [9.0, 9, 9]])
    dims = (3, 3, 3)
    one, f1 = O.distance_field(V, [[0, 1, 2]], dims)
    two, f2 = O.distance_field(V, [[0, 1, 2], [0, 1, 2]], dims)
    assert np.array_equal(one.view(np.int32), two.view(np.int32)) and (f2 == 0).all()
    mixed, f3 = O.distance_field(V, [[0, 0, 1], [3, 3, 3], [0, 1, 2]], dims)
    assert np.array_equal(one.view(np.int32), mixed.view(np.int32)) and (f3 == 2).all()
    assert one[1, 1, 2] == 2.0 and one[0, 0, 0] == 0.0
    with pytest.raises(O.EmptyMesh):
        O.distance_field(V, [[0, 0, 1], [3, 3, 3]], dims)
    t, ft = O.distance_field(V, [[0, 1, 2]], dims, truncate=1.5)
    assert t.max() == 1.5 and np.array_equal(ft == -1, one > 1.5) and np.array_equal(t, np.minimum(one, np.float32(1.5)))


def test_df_write_round_trip(tmp_path):
    import svr_amd
    from svr_amd.data_processing import sample_io
    from svr_amd.data_processing.volume_reader import read_df, write_df
    ramp = np.arange(5 * 3 * 4, dtype=np.float32).reshape(5, 3, 4) * np.float32(0.25) - np.float32(1.0)
    payload = ramp.reshape(-1, order="F")
    assert np.array_equal(sample_io.grid_to_df(ramp), payload)
    want = struct.pack("<3Q", 5, 3, 4) + payload.tobytes()
    for k, writer in enumerate((sample_io.df_write, write_df)):
        path = tmp_path / f"ramp{k}.df"
        writer(str(path), ramp)
        assert path.read_bytes() == want
        back = read_df(str(path))
        assert back.shape == (5, 3, 4) and back.dtype == np.float32 and np.array_equal(back.view(np.int32), ramp.view(np.int32))
        assert sample_io.df_dims(path) == (5, 3, 4)
        dims = (ctypes.c_int64 * 3)()
        assert svr_amd._lib.lib().svr_df_dims(str(path).encode(), dims) == 0 and tuple(dims) == (5, 3, 4)
    with pytest.raises(RuntimeError, match="cannot open"):
        sample_io.df_write(str(tmp_path / "no_such_dir" / "x.df"), ramp)
    with pytest.raises(ValueError):
        sample_io.df_write(str(tmp_path / "flat.df"), ramp.reshape(-1))
    assert svr_amd._lib.lib().svr_df_write(str(tmp_path / "no_such_dir" / "x.df").encode(), payload.ctypes.data, 5, 3, 4) == -5


def test_process_sample_scene_mesh_defaults_to_none():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import process_sample as P
    for fn in (P.process_sample, P.process_sample_pipeline):
        assert inspect.signature(fn).parameters["scene_mesh"].default is None


def test_host_checks_and_batch_plan_need_no_device():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import mesh_to_df as M
    from svr_amd.data_processing.process_sample import EmptyMeshError
    V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert M.triangle_table((V, np.array([[0, 1, 2]]))).shape == (1, 9)
    with pytest.raises(ValueError, match="outside the 3 vertices"):
        M.triangle_table((V, np.array([[0, 1, 3]])))
    with pytest.raises(ValueError, match="outside the 3 vertices"):
        M.triangle_table((V, np.array([[0, -1, 2]])))
    bad = V.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        M.triangle_table((bad, np.array([[0, 1, 2]])))
    with pytest.raises(EmptyMeshError):
        M.triangle_table((V, np.zeros((0, 3), dtype=np.int32)))
    # batches: consecutive, covering, within the budget unless a single brick is larger
    off = np.array([0, 3, 3, 10, 11, 40, 41])
    assert M.plan_batches(off, 4 * 1000) == [(0, 6)]
    assert M.plan_batches(off, 4 * 10) == [(0, 3), (3, 4), (4, 5), (5, 6)]
    assert M.plan_batches(off, 4) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
