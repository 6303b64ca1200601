"""Times behind DESIGN.md section 17, on a tree of --views random 240 x 320 PNGs (tests/_scene_tree.py's layout):

  decode_rgb : DeviceSceneLoader._decode_rgb per view, device_rgb False against True, with and without the input resize:
               `host` = the call's own wall time (what the loading thread pays), `done` = until the copy stream has drained.
  reconstruct: a randomly initialised SceneNetTrainer at scale_factor 1, inf_res 1 (the full 139 x 104 x 112 lattice), one
               view at a time, dense and with block 8: preprocess / UNet + depth head / project / lattice + marching cubes,
               a device synchronisation behind every stage, and reconstruct(path) end to end (PNG decode included).
               The mesh stage depends on the surface the network draws: the untrained network's output bias is moved to
               its median logit, which puts an arbitrary, noisy level set through the lattice (vertex / face counts are in
               the output) -- large next to a trained network's surface, so the block-8 figure is on the high side.

Medians over the views after one warm-up pass.  Numbers only, no threshold.  One JSON object on stdout and in --out."""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import svr_amd  # noqa: E402,F401
from svr_amd.dataset import DeviceSceneLoader, scene_net_data  # noqa: E402
from svr_amd.model.ifnet import evaluate_network_on_grid_device  # noqa: E402
from svr_amd.reconstruct import Reconstructor  # noqa: E402
from svr_amd.trainer.trainer_scene_net import SceneNetTrainer, default_hparams  # noqa: E402
from tests._scene_tree import build_tree  # noqa: E402


def median(ts):
    ts = sorted(ts)
    return round(ts[len(ts) // 2], 3)


def decode_rgb(tree, names, resize_input, device_rgb):
    kw = SimpleNamespace(W=256, resize_input=resize_input, precision=32)
    ds = scene_net_data("test", tree / "data", 16, "tiny", kw, splits_root=tree / "splits")
    loader = DeviceSceneLoader(ds, cache=False, device_rgb=device_rgb)
    host, done = [], []
    for rep in range(2):                                   # the first pass warms files, tables and the allocator
        for name in names:
            path = tree / "data" / "raw" / "tiny" / name / "rgb.png"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = loader._decode_rgb(path)
            t1 = time.perf_counter()
            loader.copy_stream.synchronize()
            t2 = time.perf_counter()
            del keep
            if rep:
                host.append((t1 - t0) * 1e3)
                done.append((t2 - t0) * 1e3)
    return {"host_ms": median(host), "done_ms": median(done)}


def shifted_model(tree, names):
    """A randomly initialised network draws no surface at p = 0.5 (its logits sit on one side of 0): move fc_out's bias by
    the median logit over the first view's lattice, so that the level set passes through the lattice."""
    torch.manual_seed(0)
    hparams = default_hparams(resize_input=True, scale_factor=1, inf_res=1)
    probe = Reconstructor(SceneNetTrainer(hparams))
    view = probe.reconstruct(tree / "data" / "raw" / "tiny" / names[0] / "rgb.png")
    vox = view.voxel_occupancy
    p = evaluate_network_on_grid_device(probe.model.ifnet, vox.reshape(1, 1, *vox.shape[-3:]), probe.model.dims.tolist(), 1)
    state = {k: v.detach().clone() for k, v in probe.model.state_dict().items()}
    state["ifnet.fc_out.bias"] -= torch.logit(p.double()).median().float()
    model = SceneNetTrainer(hparams)
    model.load_state_dict(state)
    return model


def reconstruct(tree, names, block):
    rec = Reconstructor(shifted_model(tree, names), block=block)
    model = rec.model
    stages = {k: [] for k in ("preprocess", "unet_depth", "project", "mesh", "end_to_end")}
    sizes = []

    def tick(key, t0, rep):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if rep:
            stages[key].append((t1 - t0) * 1e3)
        return t1

    for rep in range(2):
        for name in names:
            path = tree / "data" / "raw" / "tiny" / name / "rgb.png"
            with Image.open(path) as im:
                pixels = torch.from_numpy(np.array(im.convert("RGB"))).cuda().unsqueeze(0)
            with torch.no_grad():
                torch.cuda.synchronize()
                t = time.perf_counter()
                x = rec.preprocess(pixels)
                t = tick("preprocess", t, rep)
                depth = model._predict_depth(x)
                t = tick("unet_depth", t, rep)
                point_cloud, vox = model._voxels_from_depth(depth)
                t = tick("project", t, rep)
                (view,) = rec._views(depth, point_cloud, vox)
                t = tick("mesh", t, rep)
            view = rec.reconstruct(path)
            tick("end_to_end", t, rep)
            if rep:
                sizes.append((int(view.vertices.shape[0]), int(view.faces.shape[0])))
    out = {k + "_ms": median(v) for k, v in stages.items()}
    out["vertices_faces"] = sizes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reconstruct_bench.json"))
    a = ap.parse_args()
    names = [f"{i:05d}" for i in range(a.views)]
    tree = build_tree(Path(tempfile.mkdtemp()), {"test": names}, rows={n: (64, 64) for n in names}, seed=5)
    res = {"views": a.views, "torch_threads": torch.get_num_threads(), "decode_rgb": {},
           "reconstruct": {}}
    for resize_input in (True, False):
        for device_rgb in (False, True):
            res["decode_rgb"][f"resize_input={resize_input} device_rgb={device_rgb}"] = decode_rgb(tree, names, resize_input, device_rgb)
    for block in (0, 8):
        res["reconstruct"]["dense" if not block else f"block={block}"] = reconstruct(tree, names, block)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
