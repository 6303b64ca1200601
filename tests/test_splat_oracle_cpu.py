"""CPU: tests/splat_oracle.py -- the numpy restatement of the ordered splat's summation order that
tests/test_gpu_scene_deterministic.py holds the kernel to bit for bit -- is itself pinned against the reference-derived
oracle (oracle/projection_oracle.py) on the inputs of the project_cube / project_half fixtures: voxels within the 1e-5
rel_err gate tests/test_gpu_projection_parity.py applies to the raw voxels, validity mask and base indices equal."""
import numpy as np
import pytest

from oracle import projection_oracle as P
from tests import _golden as G
from tests import splat_oracle as SO


@pytest.mark.parametrize("case", ["cube", "half"])
def test_ordered_splat_oracle_matches_the_projection_oracle(case):
    z = G.load("project_" + case)
    depth, _, dims, _, _, scale = G.project_inputs(z)
    pts = P.norm_grid_space(P.depthmap_to_gridspace(depth, scale), dims)
    acc, valid, base = SO.splat_ordered(pts.numpy(), dims)
    ref = P.pc_voxels(pts, dims).numpy()
    assert acc.dtype == np.float32 and acc.shape == ref.shape
    assert G.rel_err(SO.clamp8(acc), ref) < 1e-5
    v_ref, b_ref, _ = P.splat_indices(pts, dims)
    assert 0 < int(v_ref.sum()) and np.array_equal(valid, v_ref.numpy())
    assert np.array_equal(base[valid], b_ref.numpy()[valid])
    assert np.array_equal(np.packbits(valid.astype(np.uint8)), z["valid_bits"])          # ... and the reference's own mask


def test_ordered_splat_oracle_order_and_edges():
    """The order is what the docstring says: a cell's points are added one after the other in ascending point index (a
    float32 sum that differs from the reversed one), out-of-range and NaN points add nothing, corners outside the grid are
    dropped."""
    dims = (3, 3, 3)
    rng = np.random.default_rng(5)
    cell = (rng.random((1, 40, 3), dtype=np.float32) * np.float32(0.4) - np.float32(0.45)).astype(np.float32)     # base voxel (0, 0, 0)
    acc, valid, base = SO.splat_ordered(cell, dims)
    assert valid.all() and (base == 0).all()
    g = (cell[0] + np.float32(0.5)) * np.float32(2.0)
    w = ((np.float32(1.0) - g[:, 0]) * (np.float32(1.0) - g[:, 1])).astype(np.float32) * (np.float32(1.0) - g[:, 2])
    seq = np.float32(0.0)
    for v in w:
        seq = np.float32(seq + v)
    assert acc[0, 0, 0, 0] == seq                                   # only P000 is non-zero at voxel (0, 0, 0)
    bad = np.array([[[0.6, 0.0, 0.0], [np.nan, 0.0, 0.0], [-0.5, 0.1, 0.1], [0.4999995, 0.0, 0.0]]], dtype=np.float32)
    acc, valid, _ = SO.splat_ordered(bad, (5, 6, 7))
    assert not valid.any() and not acc.any()
    one = np.array([[[0.0, 0.0, 0.0]]], dtype=np.float32)
    want = np.zeros((1, 1, 4, 4), dtype=np.float32)                  # D0 = 1: the k = 1 corners fall outside the grid
    want[0, 0, 1:3, 1:3] = 0.25                                      # base (0, 1, 1), fractions (0, 0.5, 0.5)
    assert np.array_equal(SO.splat_ordered(one, (1, 4, 4))[0], want)
