"""The fit loops' overhead over the bare step, and DeviceSceneLoader against default_collate over scene_net_data
(DESIGN.md section 14).  Builds its own synthetic dataset tree (8 views, 110 000 float64 points per occupancy file,
128^3 grids) in a temporary directory.

usage: python tools/bench_fit.py [--what loader,ifnet,scene] [--steps K] [--warmup W] [--out FILE]   -> one JSON line

  loader : per-batch host time and device launches (kernels + copies, from torch.profiler) at B = 8, 2 x 2048 points:
           default_collate over scene_net_data (every item decodes its files), DeviceSceneLoader cold (first touch) and
           cached; the batched kernel + its index copy against the per-segment launches they replace (HIP events).
  ifnet  : train_implicit_refinement at bench.py's shapes (128^3, batch 8, 2 x 25 000 points) against the bare step on one
           resident batch through the same DataParallelTrainer.
  scene  : train_scene_net at tools/bench_scene.py's shapes (batch 4, 2 x 25 000 points, 256 x 256 input; the lattice is the
           dataset's 139 x 104 x 112, not the benchmark's 128^3) against the bare step likewise.
Step times are the median interval between the starts of consecutive DataParallelTrainer.step calls: with at most two
steps in flight the host waits for the GPU, so in steady state that interval is the GPU's time per step."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import svr_amd  # noqa: E402,F401
from oracle.dataset_oracle import make_sample, write_df  # noqa: E402  (write process_sample.py's file formats)
from svr_amd import dp  # noqa: E402
from svr_amd.data_processing import sample_io  # noqa: E402
from svr_amd.dataset import DeviceSceneLoader, scene_net_data  # noqa: E402
from svr_amd.trainer import ImplicitRefinementTrainer, SceneNetTrainer, train_implicit_refinement, train_scene_net  # noqa: E402
from svr_amd.util.arguments import parse_arguments  # noqa: E402
from tests import _exr  # noqa: E402  (EXR writer of the test suite)

VIEWS, ROWS = 8, 110000


def build_tree(root, grid):
    rng = np.random.default_rng(0)
    names = [f"{i:05d}" for i in range(VIEWS)]
    for k, name in enumerate(names):
        raw, processed = root / "data" / "raw" / "overfit_bench" / name, root / "data" / "processed" / "overfit_bench" / name
        raw.mkdir(parents=True)
        Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(raw / "rgb.png")
        _exr.write_exr(raw / "distance.exr", {"R": (2.0 + 2.0 * rng.random((240, 320))).astype(np.float32)}, compression=_exr.ZIPS)
        make_sample(processed, dims=(grid,) * 3, n_pts=ROWS, seed=k)
        # the run's closing validation pass meshes the target's level-1 surface: none in a constant field, instead of
        # millions of triangles in make_sample's noise
        write_df(processed / "target.df", np.full((grid,) * 3, 2.0, dtype=np.float32))
    (root / "splits" / "overfit_bench").mkdir(parents=True)
    for split, items in (("train", names), ("val", names[:1]), ("test", names[:1])):
        (root / "splits" / "overfit_bench" / f"{split}.txt").write_text("\n".join(items) + "\n")


def arguments(root, **kw):
    a = parse_arguments(["--splitsdir", "overfit_bench", "--datasetdir", str(root / "data"), "--sanity_steps", "0",
                         "--val_check_interval", "1.0", "--seed", "1", "--max_epoch", "1"], timestamp=False)
    a.splits_root = str(root / "splits")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def launches(fn):
    """Device launches (kernels, copies, memsets) one call of `fn` enqueues."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    torch.cuda.synchronize()
    return {"median": statistics.median(out), "min": min(out), "max": max(out), "reps": reps}


def event_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def bench_loader(root):
    args = arguments(root, num_points=2048, resize_input=True)
    ds = scene_net_data("test", args.datasetdir, args.num_points, args.splitsdir, args, splits_root=args.splits_root)
    ds.data = [f"{i:05d}" for i in range(VIEWS)]                     # every view once (the train split repeats them x50)
    order = list(range(VIEWS))

    def collate():
        return torch.utils.data.default_collate([ds[i] for i in order])

    collate()                                                       # library start-up, file cache
    res = {"batch": VIEWS, "num_points": 2048, "rows_per_file": ROWS,
           "default_collate_ms": host_ms(lambda: (collate(), torch.cuda.synchronize()), 5),
           "default_collate_launches": launches(collate)}
    cold = []
    for _ in range(3):
        loader = DeviceSceneLoader(ds)
        torch.cuda.synchronize()
        t = time.perf_counter()
        loader.batch(order)
        torch.cuda.synchronize()
        cold.append((time.perf_counter() - t) * 1e3)
    res["loader_cold_ms"] = {"median": statistics.median(cold), "min": min(cold), "max": max(cold), "reps": 3}
    loader.batch(order)
    res["loader_cached_host_ms"] = host_ms(lambda: loader.batch(order), 50)                   # enqueue only
    res["loader_cached_ms"] = host_ms(lambda: (loader.batch(order), torch.cuda.synchronize()), 50)
    res["loader_cached_launches"] = launches(lambda: loader.batch(order))
    # the one kernel + one index copy against the per-segment launches they replace (same resident sources, same draws)
    samples = [loader.cache[n] for n in ds.data]
    n = 2048
    out = torch.empty(VIEWS * 2 * n * 4, device="cuda")
    segments, occ_base = [], VIEWS * 2 * n * 3
    for b, s in enumerate(samples):
        for k, sigma in enumerate(("0.10", "0.01")):
            at = (b * 2 + k) * n
            segments += [(s[(sigma, "points")], at, n, at * 3), (s[(sigma, "occupancies")], at, n, occ_base + at)]
    packed, draws, total = sample_io.pack_row_segments(segments, VIEWS * 2 * n, out.numel())
    draws[:] = np.random.randint(0, ROWS, draws.size)
    device_packed = packed.cuda()
    idx = [torch.from_numpy(draws[i * n:(i + 1) * n].copy()).cuda() for i in range(VIEWS * 2)]
    res["batched_kernel_us"] = event_us(lambda: sample_io.subsample_rows_batched(device_packed, len(segments), total, out), 200)
    res["batched_kernel_and_copy_us"] = event_us(
        lambda: sample_io.subsample_rows_batched(packed.to("cuda", non_blocking=True), len(segments), total, out), 200)
    res["index_copy_bytes"] = packed.numel() * 8

    def per_segment():
        for i, (rows, _, _, _) in enumerate(segments):
            sample_io.subsample_rows(rows, idx[i // 2])

    res["per_segment_kernels_us"] = event_us(per_segment, 50)
    res["per_segment_launches"] = launches(per_segment)
    return res


class StepClock:
    """Start times of DataParallelTrainer.step calls."""

    def __enter__(self):
        self.t, self.orig = [], dp.DataParallelTrainer.step
        clock, orig = self, self.orig

        def step(driver, batch, batch_idx=0):
            clock.t.append(time.perf_counter())
            return orig(driver, batch, batch_idx)

        dp.DataParallelTrainer.step = step
        return self

    def __exit__(self, *exc):
        dp.DataParallelTrainer.step = self.orig

    def intervals_ms(self, warmup):
        d = [(b - a) * 1e3 for a, b in zip(self.t, self.t[1:])][warmup:]
        s = sorted(d)
        return {"median": statistics.median(d), "min": s[0], "max": s[-1], "p90": s[int(0.9 * (len(s) - 1))], "steps": len(d)}


def bench_loop(root, which, steps, warmup):
    if which == "ifnet":
        args = arguments(root, num_points=25000, batch_size=8, experiment="bench_ifnet")
        train, cls = train_implicit_refinement, ImplicitRefinementTrainer
    else:
        args = arguments(root, num_points=25000, batch_size=4, resize_input=True, experiment="bench_scene")
        train, cls = train_scene_net, SceneNetTrainer
    res = {"batch": args.batch_size, "num_points": args.num_points, "steps": steps, "warmup": warmup}
    # bare step: one resident batch through the same driver
    torch.manual_seed(1)
    model = cls(args).cuda().train()
    np.random.seed(1)
    loader = model.device_loader("train")
    batch = loader.batch(list(range(args.batch_size)))
    if which == "ifnet":
        # what the loop's batch costs beside the subset kernel and that the bare step, with its resident batch, does not
        # have: the stacks of the items' `input` and `target` grids
        held = [loader.cache[n] for n in loader.ds.data[:args.batch_size]]
        res["stack_input_and_target_us"] = event_us(
            lambda: (torch.stack([s["input"].unsqueeze(0) for s in held]), torch.stack([s["target"].unsqueeze(0) for s in held])), 50)
        res["stack_bytes"] = 2 * sum(s["input"].numel() * 4 for s in held)
        np.random.seed(1)
        res["loader_batch_us"] = event_us(lambda: loader.batch(list(range(args.batch_size))), 50)
    driver = dp.DataParallelTrainer(model)
    with StepClock() as clock:
        for i in range(warmup + steps + 1):
            driver.step(batch, i)
        torch.cuda.synchronize()
    res["bare_step_ms"] = clock.intervals_ms(warmup)
    del model, driver, batch
    torch.cuda.empty_cache()
    # the loop; its first epoch decodes the 8 views once (inside the warm-up steps), then every batch is cached
    with StepClock() as clock:
        out = train(args, steps=warmup + steps + 1, output_root=str(root / "runs"))
        torch.cuda.synchronize()
    res["loop_step_ms"] = clock.intervals_ms(warmup)
    res["loop_minus_bare_ms"] = res["loop_step_ms"]["median"] - res["bare_step_ms"]["median"]
    res["history_keys"] = sorted(out["history"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="loader,ifnet,scene")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=12, help="decoding, the step arena, MIOpen's solver search, the scatter-form lag")
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = Path(tempfile.mkdtemp(prefix="bench_fit_"))
    try:
        t = time.perf_counter()
        build_tree(root, a.grid)
        res = {"tree_build_s": time.perf_counter() - t, "device": torch.cuda.get_device_name(0)}
        for what in a.what.split(","):
            res[what] = bench_loader(root) if what == "loader" else bench_loop(root, what, a.steps, a.warmup)
            print(f"# {what} done", file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
