"""CPU: the host side of the fit loops -- command-line flags, top-k checkpoint bookkeeping, rank sharding, mesh
normalisation.  No kernel runs here."""
import numpy as np
import pytest


def test_parse_arguments_defaults_are_the_references():
    import svr_amd  # noqa: F401
    from svr_amd.util import arguments
    assert not hasattr(arguments, "args")                      # nothing parsed at import time
    a = arguments.parse_arguments([], timestamp=False)
    seed = vars(a).pop("seed")
    assert 0 <= seed <= 999                                    # -1 -> randint(0, 999)
    assert vars(a) == dict(
        num_workers=0, gpu=0, sanity_steps=2, resume=None, splitsdir="overfit", datasetdir="data", val_check_percent=0.5,
        val_check_interval=0.25, max_epoch=100, save_epoch=1, lr=0.0001, batch_size=16, experiment="scenes_net", W=256,
        sigma=[1.5, 1.5, 1.5], kernel_size=[3, 3, 3], num_points=2048, net_res=128, inf_res=1, precision=32, profiler=None,
        version=None, resize_input=False, pretrain_unet=None, visualize=False, min_z=0.1953997164964676, max_z=7.0,
        scale_factor=1, subsample_points=0, skip_unet=False, no_depth_sup=False, test=None)
    assert arguments.parse_arguments(["--seed", "7"], timestamp=False).seed == 7


def test_parse_arguments_post_processing(tmp_path):
    import re
    import svr_amd  # noqa: F401
    from svr_amd.util.arguments import parse_arguments
    a = parse_arguments(["--sigma", "2.5", "--kernel_size", "5"], timestamp=False)
    assert a.sigma == [2.5, 2.5, 2.5] and a.kernel_size == [5, 5, 5]
    a = parse_arguments(["--sigma", "1", "2", "3", "--kernel_size", "3", "5", "7"], timestamp=False)
    assert a.sigma == [1.0, 2.0, 3.0] and a.kernel_size == [3, 5, 7]
    a = parse_arguments(["--val_check_interval", "2.7"], timestamp=False)
    assert a.val_check_interval == 2 and isinstance(a.val_check_interval, int)
    a = parse_arguments(["--val_check_interval", "1.0"], timestamp=False)
    assert a.val_check_interval == 1.0 and isinstance(a.val_check_interval, float)
    assert re.fullmatch(r"\d{8}_name", parse_arguments(["--experiment", "name"]).experiment)      # %d%m%H%M_
    assert parse_arguments(["--experiment", "name"], timestamp=False).experiment == "name"
    ckpt = tmp_path / "runs" / "12031455_scene" / "last.ckpt"
    for stamp in (True, False):
        a = parse_arguments(["--resume", str(ckpt), "--experiment", "other"], timestamp=stamp)
        assert a.experiment == "12031455_scene" and a.resume == str(ckpt)
    flags = parse_arguments(["--resize_input", "--visualize", "--skip_unet", "--no_depth_sup", "--test", "m.ckpt"], timestamp=False)
    assert flags.resize_input and flags.visualize and flags.skip_unet and flags.no_depth_sup and flags.test == "m.ckpt"


def test_top_k_keeper_holds_the_best_two_and_deletes_the_rest(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.trainer import TopKCheckpoints
    keeper = TopKCheckpoints(2, "val_ce_loss")
    paths = [tmp_path / f"epoch=0-step={i}.ckpt" for i in range(4)]
    kept = []
    for value, path in zip((0.5, 0.3, 0.4, 0.2), paths):
        kept.append(keeper.offer(value, path))
        if kept[-1]:
            path.write_bytes(b"checkpoint")
    assert kept == [True, True, True, True]
    assert keeper.best == [(0.2, str(paths[3])), (0.3, str(paths[1]))]
    assert (keeper.best_value, keeper.best_path) == (0.2, str(paths[3]))
    assert sorted(p.name for p in tmp_path.iterdir()) == [paths[1].name, paths[3].name]
    assert not keeper.offer(0.35, tmp_path / "worse.ckpt") and not keeper.offer(float("nan"), tmp_path / "nan.ckpt")
    assert not keeper.offer(float("inf"), tmp_path / "inf.ckpt")
    assert keeper.best == [(0.2, str(paths[3])), (0.3, str(paths[1]))] and paths[1].exists() and paths[3].exists()
    other = TopKCheckpoints(2, "val_ce_loss")
    other.load_state(keeper.state())
    assert other.best == keeper.best and keeper.state()["monitor"] == "val_ce_loss"
    assert other.offer(0.25, tmp_path / "new.ckpt") and not paths[1].exists() and paths[3].exists()


def test_checkpoint_with_optimizer_state_passes_the_restricted_unpickler(tmp_path):
    import argparse
    import torch
    import svr_amd  # noqa: F401
    from svr_amd.trainer import TopKCheckpoints, load_checkpoint, save_checkpoint
    module = torch.nn.Linear(3, 2)
    module.hparams = argparse.Namespace(lr=1e-3, sigma=[1.5] * 3)
    opt = torch.optim.Adam(module.parameters(), lr=1e-3)
    module(torch.ones(1, 3)).sum().backward()
    opt.step()
    keeper = TopKCheckpoints(2)
    keeper.offer(0.5, tmp_path / "a.ckpt")
    path = save_checkpoint(module, tmp_path / "last.ckpt", epoch=1, global_step=9, optimizer_states=[opt.state_dict()],
                           checkpoint_callback=keeper.state(), val_ce_loss=0.5)
    ck = load_checkpoint(path)
    assert (ck["epoch"], ck["global_step"], ck["val_ce_loss"]) == (1, 9, 0.5)
    assert ck["checkpoint_callback"]["best_k"] == [[0.5, str(tmp_path / "a.ckpt")]]
    state = ck["optimizer_states"][0]["state"]
    assert float(state[0]["step"]) == 1 and torch.equal(state[0]["exp_avg"], opt.state_dict()["state"][0]["exp_avg"])
    fresh = torch.optim.Adam(torch.nn.Linear(3, 2).parameters(), lr=1.0)
    fresh.load_state_dict(ck["optimizer_states"][0])
    assert fresh.param_groups[0]["lr"] == 1e-3


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_sharding_covers_every_batch_exactly_once(world):
    import svr_amd  # noqa: F401
    from svr_amd.trainer import shard_batches
    for n in (0, 1, 2, 3, 7, 12):
        shards = [shard_batches(n, rank, world) for rank in range(world)]
        assert sorted(b for s in shards for b in s) == list(range(n))
        for rank, s in enumerate(shards):
            assert s == list(range(rank, n, world))
        padded = [shard_batches(n, rank, world, pad=True) for rank in range(world)]
        assert {len(s) for s in padded} == {-(-n // world)}                    # every rank joins every all-reduce
        for s, p in zip(shards, padded):
            assert p[:len(s)] == s and all(0 <= b < n for b in p)


def test_epoch_batches_follow_the_dataloader_rules():
    import torch
    import svr_amd  # noqa: F401
    from svr_amd.trainer.fit import epoch_batches
    assert epoch_batches(5, 2, shuffle=False, drop_last=False) == [[0, 1], [2, 3], [4]]
    assert epoch_batches(5, 2, shuffle=False, drop_last=True) == [[0, 1], [2, 3]]
    torch.manual_seed(3)
    got = epoch_batches(7, 3, shuffle=True, drop_last=True)
    assert len(got) == 2 and len({i for b in got for i in b}) == 6 and all(0 <= i < 7 for b in got for i in b)


@pytest.mark.parametrize("scale_factor", [1, 2])
def test_normalize_meshes_is_the_float64_formula_rounded_once(tmp_path, scale_factor):
    import __graft_entry__ as ge
    ge.build()
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.convert_to_scaled_obj import normalize_meshes
    from svr_amd.data_processing.mesh_occupancies import load_obj
    verts = np.array([[0.0, 0.0, 0.0], [139.0, 104.0, 112.0], [17.3125, 51.7, 99.000007], [69.5, 0.1, 33.333332]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    lines = [f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}" for v in verts] + [f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}" for f in faces]
    (tmp_path / "a_predicted.obj").write_text("\n".join(lines) + "\n")
    (tmp_path / "a_voxelized.obj").write_text("\n".join(lines) + "\n")          # not matched by the pattern
    written = normalize_meshes(tmp_path, scale_factor=scale_factor)
    assert written == [str(tmp_path / "a_predicted_normed.obj")]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a_predicted.obj", "a_predicted_normed.obj", "a_voxelized.obj"]
    dims = np.array([139, 104, 112], dtype=np.float64) / scale_factor          # 69.5, 52, 56 at 2: not rounded to 70
    want = ((verts.astype(np.float64) - dims / 2) / dims).astype(np.float32)
    got = load_obj(written[0])
    assert np.array_equal(got.faces, faces)
    assert np.array_equal(got.vertices.astype(np.float32).view(np.int32), want.view(np.int32))
