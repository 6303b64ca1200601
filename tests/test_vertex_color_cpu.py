"""CPU: what the vertex-colour rule (include/svr_hip.h, restated by tests/vertex_color_oracle.py) MEANS -- its visibility test
against exact per-vertex visibility, its image geometry, the spread's properties -- and the PLY writer, which is host code."""
import os

import numpy as np
import pytest
import torch

from tests import _vertex_color_cases as K
from tests import vertex_color_oracle as O


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["placed_f64", "rounded_f32"])
@pytest.mark.parametrize("mesh", ["sphere", "torus"])
def test_depth_map_visibility_against_exact_visibility(mesh, dtype):
    """At (240, 320), bias one cell: no occluded vertex is seen, and at most 5 % of the mesh's vertices are visible but not
    seen (the price of the bias-and-four-pixels test at grazing angles).  Measured: false-seen 0 in all
    four runs; false-hidden 3 of 162 (sphere, both) and 15 of 640 (torus as placed in float64) -- rounding the torus to
    float32, the kernels' input, tips its 15 silhouette-ring vertices behind their neighbours: visible 320, all seen."""
    size = (240, 320)
    V, F, consts, depth = K.case(size, mesh, "in_view", dtype)
    _, state = O.sample(V, consts, depth, K.one_cell(consts), K.random_image(size, 1))
    visible = O.exact_visibility(V, F, consts)
    seen = state == 1
    false_seen, false_hidden = int((seen & ~visible).sum()), int((~seen & visible).sum())
    print(f"{mesh}: V={len(V)} visible={int(visible.sum())} seen={int(seen.sum())} false_seen={false_seen} false_hidden={false_hidden}")
    assert 0.2 * len(V) < visible.sum() < 0.8 * len(V)            # a closed surface: part of it faces away
    assert false_seen == 0
    assert false_hidden <= 0.05 * len(V)


@pytest.mark.parametrize("image_size,mapped", [((48, 64), False), ((100, 150), True), ((150, 100), True), ((240, 256), True)])
def test_a_seen_vertex_takes_the_colour_at_its_own_position(image_size, mapped):
    """Red and green encode column and row: the bilinear sample of a ramp is the position itself (clamped at the border,
    at most 0.5 away), then rounded (0.5 more)."""
    size = (240, 320) if mapped else image_size
    consts = O.R.make_consts(*size)
    V, _ = K.placed("torus", "in_view", size, consts)
    if mapped:                                                     # spread the vertices so that some fall into the pad
        V = V.copy()
        V[:, :2] = (V[:, :2] - V[:, :2].mean(0)) * 2.2 + V[:, :2].mean(0)
    pm = O.pad_map(*image_size) if mapped else O.IDENTITY
    depth = np.full(size, 1e9, dtype=np.float32)                  # everything in the frame is seen: geometry only
    colors, state = O.sample(V, consts, depth, 0.0, K.ramp_image(*image_size), pm)
    _, u, v = O.project(V, consts)
    x, y = pm[0] * u + pm[1], pm[2] * v + pm[3]
    inside = (x >= -0.5) & (x <= image_size[1] - 0.5) & (y >= -0.5) & (y <= image_size[0] - 0.5)
    in_frame = (u >= -0.5) & (u <= size[1] - 0.5) & (v >= -0.5) & (v <= size[0] - 0.5)
    assert np.array_equal(state == 1, inside & in_frame) and (state == 1).sum() > 100
    if max(image_size) == 150:
        assert (in_frame & ~inside).sum() > 0                       # some vertices do fall into the pad
    s = state == 1
    assert (np.abs(colors[s, 0].astype(np.float64) - x[s]) <= 1.0).all() and (np.abs(colors[s, 1].astype(np.float64) - y[s]) <= 1.0).all()
    assert (colors[s, 2] == 7).all() and (colors[~s] == np.array(O.FILL, dtype=np.uint8)).all()


def test_the_pad_map_is_the_identity_at_the_networks_own_size():
    assert O.pad_map(240, 320) == O.IDENTITY
    import svr_amd  # noqa: F401
    from svr_amd.reconstruct import input_pixel_map
    assert input_pixel_map(240, 320, True) == O.IDENTITY and input_pixel_map(7, 5, False) == O.IDENTITY
    for shape in ((7, 5), (300, 200), (240, 320), (201, 300)):
        assert input_pixel_map(*shape, True) == O.pad_map(*shape)


@pytest.mark.parametrize("mesh,most", [("torus", 5), ("sphere", 6)])
def test_spread_properties(mesh, most):
    size = (48, 64)
    V, F, consts, depth = K.case(size, mesh, "in_view")
    c0, s0 = O.sample(V, consts, depth, K.one_cell(consts), K.random_image(size, 2))
    assert 0 < (s0 == 1).sum() < len(V)
    colors, state, passes = O.spread(F, c0, s0)
    assert 1 <= passes <= most <= len(V), passes
    assert (state != 0).all() and np.array_equal(state == 1, s0 == 1) and np.array_equal(colors[s0 == 1], c0[s0 == 1])
    lo, hi = c0[s0 == 1].min(0), c0[s0 == 1].max(0)
    assert (colors >= lo).all() and (colors <= hi).all()
    again_c, again_s, again = O.spread(F, colors, state)                      # the fixed point: a second run changes nothing
    assert again == 0 and np.array_equal(again_c, colors) and np.array_equal(again_s, state)
    c, s = c0, s0
    for k in range(passes + 2):                                               # max_passes = k is the first k passes of the full run
        ck, sk, pk = O.spread(F, c0, s0, max_passes=k)
        assert pk == min(k, passes) and np.array_equal(ck, c) and np.array_equal(sk, s), k
        c, s, _ = O.spread_pass(F, c, s)
    assert np.array_equal(c, colors) and np.array_equal(s, state)


def test_spread_mean_rounds_half_up_and_counts_shared_edges_twice():
    """Two faces share the edge (0, 1) with 0 coloured: vertex 1 hears of 0 twice and of 3 once; vertex 2 of 0 once."""
    F = np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32)
    colors = np.array([[10, 0, 255], [0, 0, 0], [0, 0, 0], [13, 1, 0]], dtype=np.uint8)
    state = np.array([1, 0, 0, 1], dtype=np.uint8)
    c, s, n = O.spread_pass(F, colors, state)
    assert n == 2 and s.tolist() == [1, 2, 2, 1]
    assert c[1].tolist() == [11, 0, 170] and c[2].tolist() == [10, 0, 255]      # (33 / 3, 1 / 3 -> 0, 510 / 3)
    c, s, _ = O.spread_pass(np.array([[0, 1, 3]], dtype=np.int32), colors, state)
    assert c[1].tolist() == [12, 1, 128]                                       # 11.5 -> 12, 0.5 -> 1, 127.5 -> 128: half up


def _write_and_read(tmp_path, V, F, C, name):
    import __graft_entry__ as ge
    ge.build()
    from svr_amd.util.visualize import export_ply
    path = tmp_path / name
    export_ply(V, F, C, path)
    return path, O.read_ply(path)


@pytest.mark.parametrize("nv,nf", [(0, 0), (5, 0), (162, 320), (70000, 3)])
def test_export_ply_round_trip(tmp_path, nv, nf):
    rng = np.random.default_rng(nv + nf)
    V = rng.standard_normal((nv, 3)).astype(np.float32)
    if nv:
        V[0] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38)]
    F = rng.integers(0, max(nv, 1), size=(nf, 3)).astype(np.int32)
    C = rng.integers(0, 256, size=(nv, 3), dtype=np.uint8)
    path, (v, c, f, header) = _write_and_read(tmp_path, V, F, C, "m.ply")
    assert header == O.HEADER.format(nv=nv, nf=nf)
    assert os.path.getsize(path) == len(header) + 15 * nv + 13 * nf
    assert np.array_equal(v.view(np.uint32), V.view(np.uint32)) and np.array_equal(c, C) and np.array_equal(f, F)


def test_export_ply_reports_a_failed_open_and_mismatched_colours(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    from svr_amd import _lib
    from svr_amd.util.visualize import export_ply
    V, F, C = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32), np.zeros((3, 3), np.uint8)
    with pytest.raises(RuntimeError, match="write_ply"):
        export_ply(V, F, C, tmp_path / "no_such_dir" / "m.ply")
    import ctypes as C_
    rc = _lib.lib().svr_write_ply(os.fsencode(tmp_path / "no_such_dir" / "m.ply"), V.ctypes.data_as(C_.c_void_p),
                                  C.ctypes.data_as(C_.c_void_p), 3, F.ctypes.data_as(C_.c_void_p), 1)
    assert rc == -5                                                            # SVR_E_IO
    with pytest.raises(ValueError):
        export_ply(V, F, C[:2], tmp_path / "m.ply")


def test_vertex_colors_refuses_cpu_tensors():
    import svr_amd  # noqa: F401
    from svr_amd.util.mesh_color import vertex_colors
    consts = O.R.make_consts(4, 4)
    args = (torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(4, 4, 3, dtype=torch.uint8), torch.ones(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vertex_colors(*args, consts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vertex_colors(*(a.numpy() for a in args), consts)
