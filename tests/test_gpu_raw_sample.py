"""GPU: raw view -> training sample (csrc/raw_sample.hip, data_processing/distance_to_depth.py, process_sample.py,
dataset/scene_net_data.py) against the reference's own outputs for its one real sample (tests/golden/raw_sample.npz,
raw_sample_coords.npz, ref_depth_grid.npz: tools/gen_golden_raw.py) and against float32 numpy restatements written here."""
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _exr as X

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
INTRINSIC_TXT = ("[[277.1281435,   0.       , 159.5,  0.],\n[  0.       , 277.1281435, 119.5,  0.],\n"
                 "[  0.       ,   0.       ,   1. ,  0.],\n[  0.       ,   0.       ,   0. ,  1.]]")
FOCAL = F32(277.1281435)


# ---- float32 restatements (numpy rounds every operation on its own) ---------------------------------------------------
def np_depth(d, f):
    H, W = d.shape[-2:]
    rc = ((np.arange(H)[:, None] - H // 2) ** 2 + (np.arange(W)[None, :] - W // 2) ** 2).astype(F32)
    return np.sqrt(d * d / (rc / (F32(f) * F32(f)) + F32(1)))


def np_coords(z, c):
    f, cx, cy, s0, t0, s1, t1, s2, t2 = (F32(v) for v in c[:9])
    H, W = z.shape
    u, v = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
    with np.errstate(invalid="ignore"):                    # inf - inf in the edge test
        Xc = (u * z - cx * z) / f
        Yc = -((v * z - cy * z) / f)
        return np.stack([s0 * Xc + t0, s1 * Yc + t1, s2 * z + t2], -1).reshape(-1, 3)


def np_mark(coords, dims):
    """-> (grid uint8, out-of-range count): np.round, NaN / inf and every index outside [0, dim) skipped and counted"""
    with np.errstate(invalid="ignore"):
        r = np.round(coords)
        ok = (np.isfinite(r) & (r >= 0) & (r <= np.array(dims, F32) - 1)).all(1)
    grid = np.zeros(dims, np.uint8)
    i = r[ok].astype(np.int32)
    grid[i[:, 0], i[:, 1], i[:, 2]] = 1
    return grid, int((~ok).sum())


def grid_consts(scale):
    """f, cx, cy and camera2frustum's diagonal / offsets as the reference computes them (distance_to_depth.py:30-75), in
    torch float32 on the CPU: a restatement of its own, not the package's _camera_to_grid."""
    K = torch.tensor([[float(FOCAL), 0, 159.5, 0], [0, float(FOCAL), 119.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    pts = torch.tensor([[u * d, v * d, d, 1.0] for d in (0.4, 6.0) for (u, v) in ((0, 0), (0, 240), (320, 240), (320, 0))]).transpose(1, 0)
    fr = torch.mm(torch.inverse(K), pts).transpose(1, 0)[:, :3]
    vs = 0.05 * scale
    off = [-(torch.min(fr[:, a]) / vs) for a in range(3)]
    inv = torch.tensor(1.0 / vs)
    return [float(K[0, 0]), 159.5, 119.5, float(inv), float(off[0]), float(inv), float(off[1]), float(inv), float(off[2])]


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.fixture(scope="module")
def gold():
    z = dict(np.load(os.path.join(GOLD, "raw_sample.npz")))
    z["coords"] = np.load(os.path.join(GOLD, "raw_sample_coords.npz"))["coords"]
    z["grid"] = np.load(os.path.join(GOLD, "ref_depth_grid.npz"))["grid"]
    return z


# ---- 1. distance -> depth --------------------------------------------------------------------------------------------
def test_distance_to_depth(gold):
    """The golden map: <= 1 float32 ulp from the reference's depth, and bit for bit the float32 restatement of the rule.
    WHICH BOUND AND WHY: the reference's own CPU result is not the one-division rule of include/svr_hip.h.  It hands torch
    `ndarray ** 2 / Tensor`, which numpy defers to Tensor.__rtruediv__ = reciprocal() * other, and divides an integer
    tensor by a 0-d tensor, which ATen turns into a multiplication by the reciprocal: extra roundings.  Measured on the
    CPU (tools/gen_golden_raw.py): the separately rounded float32 restatement differs from the reference's depth in 8 647
    of 76 800 pixels, by 1 ulp at most.  So the bound against the reference is 1 ulp, and the kernel is pinned bit for bit
    against the restatement."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.distance_to_depth import FromDistanceToDepth
    d = gold["distance"]
    got = FromDistanceToDepth(FOCAL)(torch.from_numpy(d).cuda())
    assert got.is_cuda and got.shape == (240, 320) and got.dtype == torch.float32
    got = got.cpu().numpy()
    u = ulps(got, gold["depth"])
    print(f"depth vs reference: {int((u != 0).sum())} of {u.size} differ, max {int(u.max())} ulp")
    assert u.max() <= 1
    assert np.array_equal(got.view(np.int32), np_depth(d, FOCAL).view(np.int32))
    assert np.array_equal(FromDistanceToDepth(FOCAL)(d).cpu().numpy().view(np.int32), got.view(np.int32))     # numpy in: uploaded
    # odd shape, batch of 3: rows - 5 // 2, cols - 7 // 2
    rng = np.random.default_rng(0)
    b = (rng.random((3, 5, 7), dtype=F32) * 6 + F32(0.3)).astype(F32)
    for f in (FOCAL, F32(3.0)):
        out = FromDistanceToDepth(f)(torch.from_numpy(b).cuda()).cpu().numpy()
        assert out.shape == (3, 5, 7) and np.array_equal(out.view(np.int32), np_depth(b, f).view(np.int32))
    with pytest.raises(RuntimeError):
        FromDistanceToDepth(FOCAL)(torch.from_numpy(d))                                                      # CPU tensor: refused


# ---- 2. the real depth grid ------------------------------------------------------------------------------------------
def test_real_depth_grid(gold, tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import sample_io
    from svr_amd.data_processing.distance_to_depth import depth_grid, depth_to_gridspace, depthmap_to_gridspace
    exr = os.path.join(GOLD, "raw_distance.exr")
    intrinsic = tmp_path / "intrinsic.txt"
    intrinsic.write_text(str(gold["intrinsic_txt"]))
    pc = depth_to_gridspace(exr, intrinsic)
    assert pc.is_cuda and tuple(pc.shape) == (76800, 3) and pc.dtype == torch.float32
    got, want = pc.cpu().numpy(), gold["coords"]
    err = np.abs(got - want).max()
    print(f"grid-space coordinates vs reference: max |diff| {err:.3g}")
    assert err <= 6.1e-5                                    # 8 float32 ulps at magnitude 64 - 128
    assert np.array_equal(np.round(got), np.round(want))    # all 230 400 rounded indices, no exclusions
    # a leading batch axis -> (B, H*W, 3); the default intrinsic is this sample's
    depth = torch.from_numpy(np_depth(gold["distance"], FOCAL)).cuda()
    pcb = depthmap_to_gridspace(torch.stack([depth, depth * 0.5]))
    assert tuple(pcb.shape) == (2, 76800, 3) and torch.equal(pcb[0], pc)
    # the fused marking: the reference's own depth_grid.npz, nothing out of range, coordinates as above, repeatable
    dist = sample_io.exr_read(exr, "R")
    grid, count, coords = depth_grid(dist, (139, 104, 112), intrinsic, return_coords=True)
    assert grid.dtype == torch.uint8 and tuple(grid.shape) == (139, 104, 112) and int(count) == 0
    assert int(grid.sum()) == int(gold["n_ones"]) == 5466
    assert np.array_equal(grid.cpu().numpy().astype(np.float64), gold["grid"])
    assert torch.equal(coords, pc)
    grid2, count2 = depth_grid(dist, (139, 104, 112), intrinsic)
    assert torch.equal(grid2, grid) and int(count2) == 0
    grid3, count3 = depth_grid(depth, (139, 104, 112), intrinsic, is_distance=False)        # from the depth map: same grid
    assert torch.equal(grid3, grid) and int(count3) == 0


# ---- 3. edges of the marking kernel ----------------------------------------------------------------------------------
def test_marking_edges():
    """4 x 4 map, 7 x 5 x 6 grid, constants chosen so that the coordinates are gx = u*z, gy = 4 - 0.5*v*z, gz = z."""
    import ctypes as C
    import svr_amd  # noqa: F401
    from svr_amd import _lib
    nan, inf = float("nan"), float("inf")
    z = np.array([[2.5, 3.5, 2.5, 2.25],       # (0,4,2) tie 2.5 -> 2 | (4,4,4) ties 3.5 -> 4 | (5,4,2) | gx 6.75 -> 7 = dim: out
                  [5.4, 5.5, nan, inf],        # (0,1,5) dim-1 | gz 5.5 -> 6 = dim: out | NaN: out | inf: out
                  [4.4, 4.6, 2.5, -0.2],       # gy -0.4 -> -0 -> 0: (0,0,4) | gy -0.6 -> -1: out, not wrapped | (5,2,2) | gx -0.6 -> -1: out
                  [2.5, 2.5, 1.25, 1.6]], F32)  # (0,0,2) | gx tie 2.5 -> 2: (2,0,2) | (2,2,1) | (5,2,2) again: two pixels, one voxel
    dims = (7, 5, 6)
    c = [1.0, 0.0, 0.0, 1.0, 0.0, 0.5, 4.0, 1.0, 0.0, 7.0, 5.0, 6.0]
    want_coords = np_coords(z, c)
    want_grid, want_out = np_mark(want_coords, dims)
    assert want_out == 6 and int(want_grid.sum()) == 9
    for v in ((0, 4, 2), (4, 4, 4), (5, 4, 2), (0, 1, 5), (0, 0, 4), (5, 2, 2), (0, 0, 2), (2, 0, 2), (2, 2, 1)):
        assert want_grid[v] == 1, v
    zt = torch.from_numpy(z).cuda()
    grid = torch.zeros(dims, device="cuda", dtype=torch.uint8)
    count = torch.zeros(1, device="cuda", dtype=torch.int32)
    coords = torch.empty(16, 3, device="cuda")
    rc = _lib.lib().svr_depth_grid_mark(C.c_void_p(zt.data_ptr()), 0, 1.0, 4, 4, (C.c_float * 12)(*c), C.c_void_p(grid.data_ptr()),
                                        *dims, C.c_void_p(count.data_ptr()), C.c_void_p(coords.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert int(count) == 6 and np.array_equal(grid.cpu().numpy(), want_grid)
    assert np.array_equal(coords.cpu().numpy(), want_coords, equal_nan=True)         # (a NaN's sign / payload is not pinned)


# ---- synthetic raw sample --------------------------------------------------------------------------------------------
DIMS2 = (70, 52, 56)                       # round((139, 104, 112) / 2)
C_FULL = np.array([69.5, 51.5, 55.5])      # sphere centre in the 139 x 104 x 112 lattice; radius 20 voxels
C_HALF = (C_FULL - 0.5) / 2                # a 2 x 2 x 2 block mean sits at (2j + 0.5): the centre in the down-sampled lattice


def plane_distance():
    """A tilted plane z = 2 + 0.004 col + 0.003 row (2 .. 4: inside the frustum at every pixel) as a DISTANCE map."""
    depth = (F32(2) + F32(0.004) * np.arange(320, dtype=F32)[None, :] + F32(0.003) * np.arange(240, dtype=F32)[:, None]).astype(F32)
    rc = ((np.arange(240)[:, None] - 120) ** 2 + (np.arange(320)[None, :] - 160) ** 2).astype(F32)
    return (depth * np.sqrt(rc / (FOCAL * FOCAL) + F32(1))).astype(F32)


def write_view(folder, distance):
    folder.mkdir(parents=True)
    X.write_exr(folder / "distance.exr", {"R": distance, "G": distance, "B": distance}, compression=X.ZIP)
    (folder / "intrinsic.txt").write_text(INTRINSIC_TXT)
    g = np.indices((139, 104, 112)).astype(F32)
    r = np.sqrt(sum((g[a] - F32(C_FULL[a])) ** 2 for a in range(3)))
    df = np.abs(r - F32(20)).astype(F32)
    with open(folder / "distance_field.df", "wb") as f:
        f.write(struct.pack("<3Q", 139, 104, 112))
        f.write(np.asfortranarray(df).tobytes(order="F"))          # x fastest


@pytest.fixture(scope="module")
def processed(tmp_path_factory):
    """process_sample on one synthetic raw view, once for the module: down_scale_factor 2, 4096 surface samples."""
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.process_sample import process_sample
    root = tmp_path_factory.mktemp("raw_sample")
    distance = plane_distance()
    write_view(root / "raw" / "overfit" / "00000", distance)
    g = torch.Generator(device="cuda").manual_seed(3)
    process_sample(root, "overfit", "00000", down_scale_factor=2, sample_num=4096, generator=g)
    return root, distance


def test_process_sample_round_trip(processed, tmp_path):
    """Rows of the occupancy files: the reference's sample_points returns sample_num surface samples PLUS int(0.1 *
    sample_num) uniform ones (mesh_occupancies.py:9-22; 110 000 rows at its 100 000), so sample_num = 4096 gives 4505."""
    import svr_amd  # noqa: F401
    from oracle import ifnet_oracle as O
    from svr_amd.data_processing.mesh_occupancies import load_obj
    from svr_amd.data_processing.process_sample import process_sample
    from svr_amd.dataset import ImplicitDataset
    from svr_amd.trainer import ImplicitRefinementTrainer
    root, distance = processed
    raw, out = root / "raw" / "overfit" / "00000", root / "processed" / "overfit" / "00000"
    z = np.load(out / "depth_grid.npz")
    assert z.files == ["grid"] and z["grid"].dtype == np.float64 and z["grid"].shape == DIMS2
    want, n_out = np_mark(np_coords(np_depth(distance, FOCAL), grid_consts(2)), DIMS2)
    assert n_out == 0 and want.sum() > 1000 and np.array_equal(z["grid"], want.astype(np.float64))
    assert (out / "target.df").read_bytes() == (raw / "distance_field.df").read_bytes()
    mesh = load_obj(str(raw / "mesh.obj"))
    assert len(mesh.faces) > 1000
    e = np.sort(np.concatenate([mesh.faces[:, [0, 1]], mesh.faces[:, [1, 2]], mesh.faces[:, [2, 0]]]), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    assert (n == 2).all()                                                        # closed: every edge in two faces
    M = 4096 + int(0.1 * 4096)
    for sigma in ("0.01", "0.10"):
        o = np.load(out / f"occupancy_{sigma}.npz")
        assert sorted(o.files) == ["grid_coords", "occupancies", "points"]
        assert o["points"].shape == (M, 3) and o["occupancies"].shape == (M,) and o["grid_coords"].shape == (M, 3)
        assert o["points"].dtype == np.float64 and o["occupancies"].dtype == np.bool_ and o["grid_coords"].dtype == np.float64
        assert np.array_equal(o["grid_coords"], 2 * o["points"][:, ::-1])
        # analytic: the level-1.0 surface of |r - 20| is the pair of spheres r = 19, 21 (9.5 and 10.5 down-sampled voxels
        # around C_HALF); occupied = between them.  Every point farther than one voxel from both surfaces lies outside.
        # No point of the shell is that far from both, so the analytic sphere pins the outside only.  The shell is one
        # cell of the down-sampled lattice thick and marching cubes interpolates the block means linearly: along an axis
        # through the centre the means at r = 8.5, 9.5, 10.5 are 2.927, 0.934, 1.059, which puts the mesh at r = 9.47
        # and 10.03 -- so not even the band around r = 10 is inside everywhere, and what lies inside is only counted.
        r = np.linalg.norm(o["points"] * np.array(DIMS2) + np.array(DIMS2) / 2 - C_HALF, axis=1)
        far = np.minimum(np.abs(r - 9.5), np.abs(r - 10.5)) > 1.0
        assert far.sum() > 300 and not o["occupancies"][far].any(), sigma
        print(f"sigma {sigma}: {int(o['occupancies'].sum())} of {M} occupied, {int(far.sum())} far from the shell")
        assert o["occupancies"].any(), sigma                # a closed mesh has an inside, and samples of its surface + noise reach it
    # out-of-range depth: IndexError, before anything else is read
    bad = distance.copy()
    bad[100, 200] = F32(50.0)
    (root / "raw" / "overfit" / "bad").mkdir()
    X.write_exr(root / "raw" / "overfit" / "bad" / "distance.exr", {"R": bad}, compression=X.ZIPS)
    (root / "raw" / "overfit" / "bad" / "intrinsic.txt").write_text(INTRINSIC_TXT)
    with pytest.raises(IndexError, match="1 pixels unproject outside"):
        process_sample(root, "overfit", "bad", down_scale_factor=2, sample_num=64)
    # the IF-Net dataset loads the folder and a training step runs on it
    (tmp_path / "splits" / "overfit").mkdir(parents=True)
    (tmp_path / "splits" / "overfit" / "train.txt").write_text("00000\n")
    ds = ImplicitDataset("train", root, 300, "overfit", splits_root=tmp_path / "splits")
    np.random.seed(0)
    items = [ds[0], ds[1]]                                                        # (the overfit split repeats its sample)
    assert tuple(items[0]["input"].shape) == (1,) + DIMS2 and tuple(items[0]["points"].shape) == (600, 3)
    batch = {k: torch.stack([it[k] for it in items]).cuda() for k in ("input", "points", "occupancies")}
    tr = ImplicitRefinementTrainer(SimpleNamespace(lr=1e-4, net_res=128, scale_factor=2))
    tr.ifnet.load_state_dict(O.name_seeded_state(128), strict=False)
    loss = tr.cuda().train().training_step(batch, 0)["loss"]
    assert torch.isfinite(loss)


# ---- 5. pipeline quarantine ------------------------------------------------------------------------------------------
def test_pipeline_quarantines_the_out_of_range_view(tmp_path):
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.process_sample import process_sample_pipeline
    good, bad = plane_distance(), plane_distance()
    bad[0, 0] = F32(60.0)                                                        # far behind the frustum's 6 m
    write_view(tmp_path / "train" / "scene0" / "0", good)
    write_view(tmp_path / "train" / "scene0" / "1", bad)
    (tmp_path / "intrinsics.txt").write_text(INTRINSIC_TXT)
    moved = process_sample_pipeline(tmp_path, "train", down_scale_factor=2, sample_num=256)
    assert moved == [tmp_path / "quarantine" / "train" / "scene0" / "1"]
    assert not (tmp_path / "train" / "scene0" / "1").exists() and (moved[0] / "distance.exr").exists()
    assert not (moved[0] / "depth_grid.npz").exists()
    done = tmp_path / "train" / "scene0" / "0"
    assert sorted(p.name for p in done.iterdir()) == ["depth_grid.npz", "distance.exr", "distance_field.df", "intrinsic.txt", "mesh.obj",
                                                      "occupancy_0.01.npz", "occupancy_0.10.npz"]
    assert np.load(done / "depth_grid.npz")["grid"].sum() > 1000


# ---- 6. scene_net_data -----------------------------------------------------------------------------------------------
def test_scene_net_data_items_and_a_training_step(processed, gold, tmp_path):
    import shutil
    from PIL import Image, ImageOps
    import svr_amd  # noqa: F401
    from oracle import ifnet_oracle as O
    from svr_amd.dataset import scene_net_data
    from svr_amd.trainer import SceneNetTrainer, default_hparams
    root, _ = processed
    raw, out = tmp_path / "raw" / "overfit" / "00000", tmp_path / "processed" / "overfit" / "00000"
    raw.mkdir(parents=True)
    out.mkdir(parents=True)
    shutil.copyfile(os.path.join(GOLD, "raw_distance.exr"), raw / "distance.exr")
    for sigma in ("0.01", "0.10"):
        shutil.copyfile(root / "processed" / "overfit" / "00000" / f"occupancy_{sigma}.npz", out / f"occupancy_{sigma}.npz")
    rng = np.random.default_rng(5)
    png = rng.integers(1, 256, (240, 320, 3), dtype=np.uint8)                    # no 0: the pad is the only exact -1
    Image.fromarray(png).save(raw / "rgb.png")
    (tmp_path / "splits" / "overfit").mkdir(parents=True)
    (tmp_path / "splits" / "overfit" / "train.txt").write_text("00000\n")
    (tmp_path / "intrinsics.txt").write_text(str(gold["intrinsics_txt"]))

    def dataset(W, n=250):
        return scene_net_data("train", tmp_path, n, "overfit", SimpleNamespace(W=W, resize_input=True, precision=32),
                              splits_root=tmp_path / "splits", intrinsics_path=tmp_path / "intrinsics.txt")

    ds = dataset(320)                          # the padded square is 320 x 320: resizing to W = 320 changes no pixel
    assert len(ds) == 50
    np.random.seed(11)
    it = ds[0]
    assert sorted(it) == ["depthmap_target", "mesh", "name", "occupancies", "points", "rgb"]
    assert it["name"] == "00000" and it["mesh"] == str(raw / "mesh.obj")
    assert all(it[k].is_cuda and it[k].dtype == torch.float32 for k in ("depthmap_target", "occupancies", "points", "rgb"))
    # depthmap_target: test_distance_to_depth's result
    assert np.array_equal(it["depthmap_target"].cpu().numpy().view(np.int32), np_depth(gold["distance"], FOCAL).view(np.int32))
    # rgb: 40 pad rows above and below, exactly -1; the picture between them
    rgb = it["rgb"].cpu().numpy()
    assert rgb.shape == (3, 320, 320) and rgb.min() == -1 and rgb.max() <= 1
    assert (rgb[:, :40] == -1).all() and (rgb[:, 280:] == -1).all() and (rgb[:, 40:280] > -1).all()
    assert np.array_equal(rgb[:, 40:280], ((png.transpose(2, 0, 1).astype(F32) / F32(255)) - F32(0.5)) / F32(0.5))
    # points / occupancies: the same two randint draws, '0.10' first
    np.random.seed(11)
    pts, occ = [], []
    for sigma in ("0.10", "0.01"):
        o = np.load(out / f"occupancy_{sigma}.npz")
        idx = np.random.randint(0, o["points"].shape[0], 250)
        pts.append(o["points"][idx])
        occ.append(o["occupancies"][idx])
    assert np.array_equal(it["points"].cpu().numpy(), np.concatenate(pts).astype(F32))
    assert np.array_equal(it["occupancies"].cpu().numpy(), np.concatenate(occ).astype(F32))
    # W = 256: a direct PIL restatement (ImageOps.expand as the pad)
    small = dataset(256)[0]["rgb"].cpu().numpy()
    pil = ImageOps.expand(Image.fromarray(png), border=(0, 40, 0, 40), fill=0).resize((256, 256), Image.BILINEAR)
    assert small.shape == (3, 256, 256) and small.min() >= -1 and small.max() <= 1
    assert np.array_equal(small, ((np.asarray(pil).transpose(2, 0, 1).astype(F32) / F32(255)) - F32(0.5)) / F32(0.5))
    # a collated batch of 2 drives the scene trainer unchanged
    ds = dataset(256)
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert batch["mesh"] == [str(raw / "mesh.obj")] * 2 and tuple(batch["depthmap_target"].shape) == (2, 240, 320)
    tr = SceneNetTrainer(default_hparams(skip_unet=True))
    tr.ifnet.load_state_dict(O.name_seeded_state(128), strict=False)
    loss = tr.cuda().train().training_step(batch, 0)["loss"]
    assert torch.isfinite(loss)
