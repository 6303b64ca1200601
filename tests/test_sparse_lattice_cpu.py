"""CPU: the rule of the block-sparse lattice evaluation (include/svr_hip.h, svr_sl_*) as stated by
tests/sparse_lattice_oracle.py, on analytic fields: what it guarantees (leak-free exit, evaluated points carry the dense
values), where it reproduces the dense mesh exactly, and where it cannot (a speck between the coarse points)."""
import numpy as np
import pytest

from tests import mc_oracle as M
from tests import sparse_lattice_oracle as S

EXACT = [("sphere", (64, 64, 64), 4), ("torus", (64, 64, 64), 4), ("slab", (64, 64, 64), 4), ("plane", (64, 64, 64), 4),
         ("slab", (37, 30, 23), 8)]
OTHER = [("torus", (37, 30, 23), 8), ("speck", (64, 64, 64), 4), ("sphere", (19, 18, 17), 3)]


@pytest.fixture(scope="module")
def table():
    import svr_amd  # noqa: F401
    return M.case_table()


def test_axis_partition():
    for n, s in ((64, 4), (37, 8), (23, 8), (17, 8), (19, 3), (18, 2), (2, 2), (3, 2), (9, 16), (65, 4)):
        nb, owner, coarse = S.axis_blocks(n, s)
        assert nb == int(np.ceil((n - 1) / s)) and len(coarse) == nb + 1
        assert coarse[0] == 0 and coarse[-1] == n - 1 and (np.diff(coarse) >= 1).all() and (np.diff(coarse) <= s).all()
        counts = np.bincount(owner, minlength=nb)
        assert (counts[:-1] == s).all() and 2 <= counts[-1] <= s + 1 and owner[-1] == nb - 1
        assert (coarse[:-1] == np.arange(nb) * s).all()            # a block's minimum corner is its first owned point


@pytest.mark.parametrize("name,shape,s", EXACT + OTHER)
def test_exit_is_leak_free_and_evaluated_points_are_dense(name, shape, s):
    dense = S.dense_field(name, shape)
    r = S.sparse_field(dense, 0.0, s)
    assert S.leak_free(r.field, r.evaluated, 0.0)
    assert np.array_equal(r.field[r.evaluated], dense[r.evaluated])
    assert len(r.leaks) == r.rounds and (r.rounds == 0 or r.leaks[-1] == 0) and not r.fell_back
    assert all(c > 0 for c in r.leaks[:-1])
    assert r.state.max() == r.rounds
    nb = [S.axis_blocks(n, s)[0] for n in shape]
    assert r.n_points == (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1) + int(r.evaluated.sum())
    # the list of a round: every owned point of its blocks once
    for rnd in range(1, r.rounds + 1):
        pts = S.point_list(shape, s, np.nonzero(r.state.reshape(-1) == rnd)[0])
        mask = np.zeros(shape, dtype=bool)
        mask[pts[:, 0], pts[:, 1], pts[:, 2]] = True
        assert int(mask.sum()) == len(pts) and np.array_equal(mask, (r.state == rnd)[np.ix_(*[S.axis_blocks(n, s)[1] for n in shape])])


@pytest.mark.parametrize("name,shape,s", EXACT)
def test_exact_cases_give_the_dense_mesh(name, shape, s, table):
    dense = S.dense_field(name, shape)
    r = S.sparse_field(dense, 0.0, s)
    assert np.array_equal(S.inside(r.field, 0.0), S.inside(dense, 0.0))
    want = M.marching_cubes(dense, 0.0, table)
    got = M.marching_cubes(r.field, 0.0, table)
    assert len(want[1]) > 100
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    if shape == (64, 64, 64):
        assert r.rounds == 2 and 0.115 <= r.n_points / dense.size <= 0.215


def test_slab_follows_the_surface_for_several_rounds_and_falls_back_when_capped():
    dense = S.dense_field("slab", (37, 30, 23))
    r = S.sparse_field(dense, 0.0, 8)
    assert r.rounds >= 3 and not r.fell_back
    capped = S.sparse_field(dense, 0.0, 8, max_rounds=2)
    assert capped.fell_back and capped.rounds == 3 and capped.leaks[-1] == 0 and capped.leaks[1] > 0
    assert capped.evaluated.all() and (capped.state != 0).all() and np.array_equal(capped.field, dense)
    assert np.array_equal(capped.state <= 2, (r.state <= 2) & (r.state > 0))      # the first two rounds are the uncapped ones


def test_coarse_torus_is_missed_entirely():
    """The documented limit: at 37 x 30 x 23 with blocks of 8 cells no coarse point lies inside the torus."""
    dense = S.dense_field("torus", (37, 30, 23))
    assert S.inside(dense, 0.0).any()
    r = S.sparse_field(dense, 0.0, 8)
    assert r.rounds == 0 and r.leaks == [] and not r.evaluated.any() and not S.inside(r.field, 0.0).any()


def test_speck_gives_the_pure_fill_and_an_empty_mesh(table):
    dense = S.dense_field("speck", (64, 64, 64))
    assert S.inside(dense, 0.0).sum() >= 1 and len(M.marching_cubes(dense, 0.0, table)[1]) > 0
    r = S.sparse_field(dense, 0.0, 4)
    assert r.rounds == 0 and not r.state.any() and r.n_points == 17 ** 3
    own = np.minimum(np.arange(64) // 4, 15) * 4
    assert np.array_equal(r.field, dense[np.ix_(own, own, own)])
    v, f = M.marching_cubes(r.field, 0.0, table)
    assert len(v) == 0 and len(f) == 0


def test_nan_is_outside():
    dense = S.dense_field("sphere", (19, 18, 17))
    dense[:, :, 9:] = np.nan
    r = S.sparse_field(dense, 0.0, 3)
    assert r.rounds >= 1 and S.leak_free(r.field, r.evaluated, 0.0)
    same = r.evaluated
    assert np.array_equal(np.isnan(r.field[same]), np.isnan(dense[same]))
    assert np.array_equal(S.inside(r.field, 0.0), S.inside(dense, 0.0))


def test_inference_block_setting():
    """INFERENCE_BLOCK: 0 (dense, the default) or an integer >= 2, from SVR_INF_BLOCK; anything else raises at import."""
    import os
    import subprocess
    import sys
    import svr_amd  # noqa: F401
    from svr_amd.model import ifnet
    assert ifnet.INFERENCE_BLOCK == int(os.environ.get("SVR_INF_BLOCK", "0"))
    assert [ifnet._inference_block(v) for v in (0, "0", 2, "8", 16)] == [0, 0, 2, 8, 16]
    for bad in (1, -4, "1", "x", "", None, "2.5"):
        with pytest.raises(ValueError):
            ifnet._inference_block(bad)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, sys.argv[1]); import svr_amd; from svr_amd.model import ifnet; print('BLOCK', ifnet.INFERENCE_BLOCK)"
    ok = subprocess.run([sys.executable, "-c", code, repo], env=dict(os.environ, SVR_INF_BLOCK="8"), capture_output=True, text=True)
    assert ok.returncode == 0 and "BLOCK 8" in ok.stdout, ok.stderr[-1000:]
    bad = subprocess.run([sys.executable, "-c", code, repo], env=dict(os.environ, SVR_INF_BLOCK="1"), capture_output=True, text=True)
    assert bad.returncode != 0 and "inference block must be 0" in bad.stderr


def test_sparse_path_refuses_cpu_tensors():
    import svr_amd  # noqa: F401
    import torch
    from svr_amd.model import IFNet, evaluate_network_on_grid_sparse
    from svr_amd.util.sparse_grid import sparse_lattice_field
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate_network_on_grid_sparse(IFNet(net_res=128), torch.zeros(1, 1, 16, 16, 16), (16, 16, 16), 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        sparse_lattice_field(lambda p: p[:, 0], (16, 16, 16), 0.0, 4, device="cpu")
    from svr_amd import _lib
    l = _lib.lib()
    assert l.svr_sl_workspace_bytes(16, 16, 16, 4) > 0
    for X, Y, Z, s in ((16, 16, 16, 1), (1, 16, 16, 4), (16, 16, 1, 4), (2048, 2048, 512, 4)):
        assert l.svr_sl_workspace_bytes(X, Y, Z, s) == -2          # SVR_E_BADSHAPE
