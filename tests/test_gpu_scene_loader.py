"""GPU: svr_subsample_rows_batched against numpy fancy indexing, and DeviceSceneLoader against default_collate over
scene_net_data -- bit for bit, first visit and cached visit -- and a training step on the loader's batch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._scene_tree import build_tree

pytestmark = pytest.mark.gpu
N_ROWS = (37, 64, 4505)
NP_DTYPES = {"f64_bool": (np.float64, np.bool_), "f32_u8": (np.float32, np.uint8)}


def _sources(pair, seed=3):
    """Per item and sigma: (points (n_rows, 3), occupancies (n_rows,)) in the pair's dtypes; the two sigmas of an item differ."""
    rng = np.random.default_rng(seed)
    pd, od = NP_DTYPES[pair]
    out = []
    for n_rows in N_ROWS:
        item = []
        for _ in range(2):
            occ = (rng.random(n_rows) < 0.4).astype(od) if od is np.bool_ else rng.integers(0, 256, n_rows).astype(od)
            item.append((rng.uniform(-0.5, 0.5, size=(n_rows, 3)).astype(pd), occ))
        out.append(item)
    return out


def _launch(sources, draws, n, poison=None):
    """One batched launch for 3 items x 2 sigmas x (points, occupancies); the segments interleave into one (3, 2n, 3) /
    (3, 2n) pair carved from one float32 block.  Returns (points, occupancies, bad flag, the sentinel-filled tail)."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    B = len(sources)
    dev = [[(torch.from_numpy(p).cuda(), torch.from_numpy(o).cuda()) for p, o in item] for item in sources]
    occ_base, tail = B * 2 * n * 3, 64
    out = torch.full((B * 2 * n * 4 + tail,), -7.0, device="cuda")
    segments = []
    for b in range(B):
        for k in range(2):
            at = (b * 2 + k) * n
            segments.append((dev[b][k][0], at, n, at * 3))
            segments.append((dev[b][k][1], at, n, occ_base + at))
    packed, index_view, total = sample_io.pack_row_segments(segments, B * 2 * n, out.numel() - tail)
    assert total == B * 2 * n * 4 and packed.is_pinned() and packed.dtype == torch.int64
    index_view[:] = draws.reshape(-1)
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    sample_io.subsample_rows_batched(packed.cuda(), len(segments), total, out, bad)
    torch.cuda.synchronize()
    return (out[:occ_base].view(B, 2 * n, 3).cpu().numpy(), out[occ_base:occ_base + B * 2 * n].view(B, 2 * n).cpu().numpy(),
            int(bad.item()), out[B * 2 * n * 4:].cpu().numpy())


def _expected(sources, draws, n):
    pts = np.stack([np.concatenate([item[k][0][draws[b, k]] for k in range(2)]).astype(np.float32) for b, item in enumerate(sources)])
    occ = np.stack([np.concatenate([item[k][1][draws[b, k]] for k in range(2)]).astype(np.float32) for b, item in enumerate(sources)])
    return pts, occ


# n = 5: 120 output elements, one partly filled block that holds all twelve segments; n = 300: 7200 elements in 29 blocks,
# segment boundaries every 900 / 300 elements, so blocks straddle two segments and the last block is partly filled
@pytest.mark.parametrize("n", [5, 300])
@pytest.mark.parametrize("pair", list(NP_DTYPES))
def test_batched_row_subset_equals_numpy_fancy_indexing(pair, n):
    sources = _sources(pair)
    rng = np.random.default_rng(n)
    draws = np.stack([np.stack([rng.integers(0, n_rows, n) for _ in range(2)]) for n_rows in N_ROWS]).astype(np.int64)
    draws[2, 1, -1] = N_ROWS[2] - 1                                            # the last row of the longest source
    draws[0, 0, 0] = 0
    pts, occ, bad, tail = _launch(sources, draws, n)
    want_pts, want_occ = _expected(sources, draws, n)
    assert bad == 0 and (tail == -7.0).all()
    assert pts.dtype == np.float32 and np.array_equal(pts.view(np.int32), want_pts.view(np.int32))
    assert np.array_equal(occ.view(np.int32), want_occ.view(np.int32))


@pytest.mark.parametrize("row", [-1, 64])
def test_batched_row_subset_out_of_range_row_gives_zeros_and_sets_the_flag(row):
    n = 5
    sources = _sources("f64_bool")
    rng = np.random.default_rng(9)
    draws = np.stack([np.stack([rng.integers(0, n_rows, n) for _ in range(2)]) for n_rows in N_ROWS]).astype(np.int64)
    good = draws.copy()
    draws[1, 1, 2] = row                                                       # item 1 has 64 rows: -1 and 64 are outside
    good[1, 1, 2] = 0
    pts, occ, bad, tail = _launch(sources, draws, n)
    want_pts, want_occ = _expected(sources, good, n)
    want_pts[1, n + 2] = 0
    want_occ[1, n + 2] = 0
    assert bad == 1 and (tail == -7.0).all()
    assert np.array_equal(pts.view(np.int32), want_pts.view(np.int32)) and np.array_equal(occ.view(np.int32), want_occ.view(np.int32))


def test_batched_row_subset_empty_table_and_empty_segments_do_nothing():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    out = torch.full((32,), -7.0, device="cuda")
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    packed, index_view, total = sample_io.pack_row_segments([], 0, out.numel())
    assert total == 0 and index_view.size == 0
    sample_io.subsample_rows_batched(packed.cuda(), 0, total, out, bad)
    rows = torch.ones(4, 3, device="cuda", dtype=torch.float64)
    packed, index_view, total = sample_io.pack_row_segments([(rows, 0, 0, 0), (rows, 0, 0, 8)], 0, out.numel())
    assert total == 0
    sample_io.subsample_rows_batched(packed.cuda(), 2, total, out, bad)
    # the C entry itself: no segments / no elements return before any pointer is looked at
    lib = svr_amd._lib.lib()
    assert lib.svr_subsample_rows_batched(None, None, 0, 0, None, None, None, None) == 0
    assert lib.svr_subsample_rows_batched(None, None, 3, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all() and bad.item() == 0


def test_pack_row_segments_refuses_ranges_outside_the_buffers():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    rows = torch.ones(4, 3, device="cuda", dtype=torch.float64)
    for segments in ([(rows, 0, 5, 0)],                      # 15 outputs into 12
                     [(rows, 2, 3, 0)],                      # indices 2..5 of 4
                     [(rows, 0, 2, 0), (rows, 2, 2, 3)],     # outputs 0..6 and 3..9 overlap
                     [(rows.cpu(), 0, 1, 0)], [(rows.int(), 0, 1, 0)], [(rows.t(), 0, 1, 0)]):
        with pytest.raises(ValueError):
            sample_io.pack_row_segments(segments, 4, 12)


# ---- DeviceSceneLoader --------------------------------------------------------------------------------------------------
NAMES = ["scene0/0", "scene0/1", "scene1/0"]
ROWS = {"scene0/0": (4505, 3001), "scene0/1": (300, 777), "scene1/0": (1037, 64)}
TENSORS = ("rgb", "points", "occupancies", "depthmap_target")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return build_tree(tmp_path_factory.mktemp("scene_loader"), {"train": NAMES}, rows=ROWS, seed=4)


def _dataset(tree, n=250, **kw):
    import svr_amd  # noqa: F401
    from svr_amd.dataset import scene_net_data
    cfg = dict(W=64, resize_input=True, precision=32)
    cfg.update(kw)
    return scene_net_data("train", tree / "data", n, "tiny", SimpleNamespace(**cfg), splits_root=tree / "splits")


def _same(got, want):
    assert list(got) == list(want)
    assert got["name"] == want["name"] and got["mesh"] == want["mesh"] and isinstance(got["name"], list)
    for k in TENSORS:
        assert got[k].is_cuda and got[k].dtype == want[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k


@pytest.mark.parametrize("resize", [True, False])
def test_loader_batch_equals_default_collate_of_the_dataset(tree, resize):
    from svr_amd.dataset import DeviceSceneLoader
    ds = _dataset(tree, resize_input=resize)
    order = [2, 0, 1]
    want = []
    for seed in (21, 22):
        np.random.seed(seed)
        want.append(torch.utils.data.default_collate([ds[i] for i in order]))
    assert tuple(want[0]["points"].shape) == (3, 500, 3) and tuple(want[0]["rgb"].shape) == ((3, 3, 64, 64) if resize else (3, 3, 240, 320))
    assert not torch.equal(want[0]["points"], want[1]["points"])
    loader = DeviceSceneLoader(ds)
    np.random.seed(21)
    first = loader.batch(order)                     # decodes the three views
    _same(first, want[0])
    assert sorted(loader.cache) == sorted(NAMES)
    resident = {k: v.data_ptr() for k, v in loader.cache["scene1/0"].items() if torch.is_tensor(v)}
    np.random.seed(22)
    second = loader.batch(order)                    # served from the cache: no file is read, the same device arrays
    _same(second, want[1])
    assert resident == {k: v.data_ptr() for k, v in loader.cache["scene1/0"].items() if torch.is_tensor(v)}
    _same(first, want[0])                           # the first batch was not written over by the second
    assert not loader.bad_rows()
    # stored dtypes stay as they are on the device
    s = loader.cache["scene0/0"]
    assert s[("0.10", "points")].dtype == torch.float64 and s[("0.10", "occupancies")].dtype == torch.bool
    assert tuple(s[("0.10", "points")].shape) == (4505, 3) and tuple(s[("0.01", "occupancies")].shape) == (3001,)


def test_loader_serves_cached_views_without_the_files(tree, tmp_path):
    import shutil
    from svr_amd.dataset import DeviceSceneLoader
    copy = tmp_path / "copy"
    shutil.copytree(tree, copy)
    ds = _dataset(copy)
    loader = DeviceSceneLoader(ds)
    np.random.seed(5)
    loader.batch([0, 1, 2])
    torch.cuda.synchronize()
    np.random.seed(6)
    want = torch.utils.data.default_collate([ds[i] for i in (1, 1, 2)])
    shutil.rmtree(copy / "data")
    np.random.seed(6)
    _same(loader.batch([1, 1, 2]), want)            # an item twice in a batch: two draws, as the dataset's
    uncached = DeviceSceneLoader(_dataset(tree), cache=False)
    np.random.seed(6)
    got = uncached.batch([1, 1, 2])
    assert uncached.cache is None
    for k in TENSORS:
        assert torch.equal(got[k], want[k]), k


def test_loader_refuses_other_precisions(tree):
    from svr_amd.dataset import DeviceSceneLoader
    for precision in (16, 64):
        with pytest.raises(ValueError, match="precision"):
            DeviceSceneLoader(_dataset(tree, precision=precision))


def test_loader_batch_drives_the_scene_trainer(tree):
    from oracle import ifnet_oracle as O
    from svr_amd.dataset import DeviceSceneLoader
    from svr_amd.trainer import SceneNetTrainer, default_hparams
    loader = DeviceSceneLoader(_dataset(tree, n=256))
    np.random.seed(1)
    batch = loader.batch([0, 2])
    tr = SceneNetTrainer(default_hparams(skip_unet=True, scale_factor=2))
    tr.ifnet.load_state_dict(O.name_seeded_state(128), strict=False)
    loss = tr.cuda().train().training_step(batch, 0)["loss"]
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in tr.ifnet.parameters())
