"""One UNet depth pre-training step (forward, backward, Adam) for `Unet` at B = 16, 256 x 256 -> 240 x 320 depth, timed with
HIP events: 5 warm-up and 20 timed steps, the median.  Two heads behind the same network:

  fused : ops.depth_head (csrc/depth_head.hip)
  chain : the stock torch ops typed out below (F.interpolate(size=320), crop of rows 40:280, sigmoid, renormalise, mse_loss)

The two are timed in the same process, step by step in alternation, each on its own copy of the network and its own Adam.  On
a tree without ops.depth_head (the commit before the head existed) only the chain runs: that run is the baseline.

The head alone is bracketed too: forward + backward of the head on a fixed UNet output, `--head-reps` calls inside one event
pair (one call is tens of microseconds: a single bracketed call would measure the launch), 20 brackets, the median per call.

One JSON object on stdout; --out FILE --label NAME stores it under NAME in FILE (other labels in the file are kept)."""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import svr_amd  # noqa: E402,F401
from svr_amd import ops  # noqa: E402
from svr_amd.model import Unet  # noqa: E402

MIN_Z, MAX_Z = 0.1953997164964676, 7.0
HAVE_FUSED = hasattr(ops, "depth_head")


def chain_loss(raw, target):
    logits = F.interpolate(raw, size=320, mode="bilinear")[:, :, 40:280, :]
    depth = torch.sigmoid(logits) * (MAX_Z - MIN_Z) + MIN_Z
    return F.mse_loss(depth, target, reduction="mean")


def fused_loss(raw, target):
    return ops.depth_head(raw, target, size=320, rows=(40, 280), min_z=MIN_Z, max_z=MAX_Z)[1]


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def bracket(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--head-reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing of this step"
    B = a.batch
    g = torch.Generator().manual_seed(0)
    rgb = (torch.rand(B, 3, 256, 256, generator=g) * 2 - 1).cuda()
    target = (5 * torch.rand(B, 1, 240, 320, generator=g) + 0.5).cuda()
    torch.manual_seed(0)
    base = Unet(channels_in=3, channels_out=1)
    heads = ([("fused", fused_loss)] if HAVE_FUSED else []) + [("chain", chain_loss)]
    runs = {}
    for name, fn in heads:
        net = copy.deepcopy(base).cuda().train()
        runs[name] = (net, torch.optim.Adam(net.parameters(), lr=1e-4), fn, [])

    def step(net, opt, fn):
        opt.zero_grad(set_to_none=True)
        loss = fn(net(rgb), target)
        loss.backward()
        opt.step()
        return loss

    losses = {}
    for i in range(a.warmup + a.steps):
        for name, (net, opt, fn, ts) in runs.items():          # alternate the variants: both see the same machine state
            out = []
            t = bracket(lambda: out.append(step(net, opt, fn)))
            if i >= a.warmup:
                ts.append(t)
            losses[name] = out[0].item()

    # the head alone, on a fixed UNet output
    with torch.no_grad():
        raw0 = runs[heads[0][0]][0](rgb).contiguous()
    head = {}
    for name, fn in heads:
        def one():
            r = raw0.clone().requires_grad_(True)
            fn(r, target).backward()
        ts = []
        for i in range(a.warmup + a.steps):
            t = bracket(lambda: [one() for _ in range(a.head_reps)])
            if i >= a.warmup:
                ts.append(t / a.head_reps)
        head[name] = ts

    res = {"workload": f"Unet depth pre-training step, B={B}, 256x256 -> 240x320, forward + backward + Adam",
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps, "head_reps": a.head_reps,
           "fused_available": HAVE_FUSED}
    for name, (_, _, _, ts) in runs.items():
        res[f"step_ms_{name}"] = {"median": median(ts), "min": min(ts), "max": max(ts)}
        res[f"head_us_{name}"] = {"median": 1e3 * median(head[name]), "min": 1e3 * min(head[name]), "max": 1e3 * max(head[name]),
                                  "note": "forward + backward of the head per call, incl. a clone of its input"}
        res[f"final_loss_{name}"] = losses[name]
    line = json.dumps(res)
    print(line)
    if a.out:
        data = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                data = json.load(f)
        data[a.label] = res
        with open(a.out, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
