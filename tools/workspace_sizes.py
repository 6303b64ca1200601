#!/usr/bin/env python3
"""What every exported workspace size function (and svr_conv2d_planes_bytes) returns over a fixed shape table; host code only:
runs without a GPU.

    python tools/workspace_sizes.py [--lib PATH]       one JSON object {function: [[args..., bytes], ...]}
    python tools/workspace_sizes.py --ab PARENT_LIB    the A/B record of profiles/workspace_layout_sizes_ab.json: the table
                                                       through PARENT_LIB (tools/ab.sh prepare builds one in _ab/) and through
                                                       the tree's library, each in a process of its own, and the differences

The table: the benchmark's shapes (B 8, N 50000, grid 128 and its pyramid; the point MLP's M = 400000 with its (N, K); the
encoder's channel pairs; the UNet's convolutions; the 139 x 104 x 112 scene), 0 and 1 everywhere, sizes off the tile multiples
(63 / 64 / 65, K off 128, 1 and 257 vertices, lattices of 2 and 3 points) and the shapes the CPU tests expect to be refused."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BN = [(8, 50000), (0, 0), (1, 1), (1, 0), (0, 1), (3, 63), (2, 65), (1, 100000)]
PYRAMID = [128, 64, 32, 16, 8]
VOLUMES = [(8, d, d, d) for d in PYRAMID] + [(1, 139, 104, 112), (1, 1, 1, 1), (0, 1, 1, 1), (2, 3, 5, 7)]
NK = [(256, 2592), (256, 800), (256, 256), (1, 256), (63, 100), (64, 128), (65, 130), (128, 192), (0, 0), (1, 1)]
MNK = [(m, n, k) for m in (400000, 1, 63, 64, 65) for n, k in NK[:8]] + [(0, 256, 256), (1, 1, 1), (139 * 104 * 112, 32, 64)]
ENCODER = [(1, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (0, 0), (1, 1), (2, 16), (16, 1)]
ENCODER_AT = [(8, 64, 16, 32), (8, 64, 32, 32), (8, 32, 32, 64), (8, 32, 64, 64), (8, 16, 64, 128), (8, 16, 128, 128), (8, 8, 128, 128),
              (1, 1, 16, 16), (1, 3, 16, 32), (1, 2, 32, 16)]                # (B, D = H = W, Ci, Co)
LATTICES = [(128, 128, 128), (139, 104, 112), (256, 256, 256), (0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (2, 3, 257), (0, 5, 5),
            (2047, 1023, 1023), (2046, 1023, 1023), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (-1, 4, 4)]
BLOCKED = [(128, 128, 128, 8), (128, 128, 128, 4), (139, 104, 112, 8), (139, 104, 112, 4), (16, 16, 16, 4), (2, 2, 2, 2), (3, 3, 3, 2),
           (2, 3, 257, 8), (1, 1, 1, 4), (16, 16, 16, 1), (1, 16, 16, 4), (16, 16, 1, 4), (2048, 2048, 512, 4), (0, 0, 0, 8), (4, 4, 4, 5)]
MESHES = [(0, 0), (1, 1), (257, 1), (1, 257), (257, 257), (100000, 200000), (2 ** 31 - 1, 2 ** 31 - 1), (-1, 0), (0, 2 ** 31)]
# the UNet at 8 x 256 x 256 and UNetMini at 8 x 240 x 320: (H, W, C0, C1, k, stride, Cout); decoder inputs after the x2 upsample
UNET = [(256, 256, 3, 0, 4, 2, 32), (128, 128, 32, 0, 4, 2, 64), (64, 64, 64, 0, 4, 2, 128), (32, 32, 128, 0, 4, 2, 256),
        (16, 16, 256, 0, 4, 2, 256), (8, 8, 256, 0, 4, 2, 256), (4, 4, 256, 0, 4, 2, 256), (2, 2, 256, 0, 4, 2, 256),
        (2, 2, 256, 0, 3, 1, 256), (4, 4, 256, 256, 3, 1, 256), (8, 8, 256, 256, 3, 1, 256), (16, 16, 256, 256, 3, 1, 256),
        (32, 32, 256, 256, 3, 1, 128), (64, 64, 128, 128, 3, 1, 64), (128, 128, 64, 64, 3, 1, 32), (256, 256, 32, 32, 3, 1, 3),
        (256, 256, 32, 32, 3, 1, 1), (240, 320, 3, 0, 4, 2, 32), (120, 160, 32, 0, 4, 2, 64), (60, 80, 64, 0, 4, 2, 128),
        (30, 40, 128, 0, 4, 2, 256), (30, 40, 256, 0, 3, 1, 128), (60, 80, 128, 128, 3, 1, 64), (240, 320, 32, 32, 3, 1, 1)]
# pyramids of the fused gather -> fc_0: (channels, grid of each level), with (B, N, n_out)
PYRAMIDS = [([1, 16, 32, 64, 128, 128], [128, 128, 64, 32, 16, 8]), ([1, 64, 128, 128], [32, 32, 16, 8]), ([1, 16], [139, 104])]
FC0 = [(8, 50000, 256), (1, 1, 256), (0, 0, 256), (1, 63, 256), (1, 65, 256), (8, 50000, 1), (8, 50000, 0), (2, 100, 255)]


def table(L, ops):
    """-> [(function, ctypes arguments, the arguments as JSON)]"""
    rows = []

    def add(name, cases):
        rows.extend((name, list(c), list(c)) for c in cases)

    for name in ("svr_points_morton_order_workspace", "svr_gather_pull_plan_workspace", "svr_gather_project_plan_workspace"):
        add(name, BN)
    add("svr_gather_pull_plan_workspace_cells", VOLUMES)
    for chans, grids in PYRAMIDS:
        lay = ops.FeatureLayout(chans)
        for B, N, n_out in FC0:
            d = L.GatherDesc()
            d.n_levels, d.B, d.N, d.row_stride, d.align_corners, d.displacement = len(chans), B, N, lay.row_stride, 1, 0.0722
            for l, (c, g) in enumerate(zip(chans, grids)):
                d.level[l].C, d.level[l].D, d.level[l].H, d.level[l].W, d.level[l].col = c, g, g, g, lay.col[l]
            rows.append(("svr_gather_fc0_workspace", [C.byref(d), n_out], [chans, grids, B, N, n_out]))
    rows.append(("svr_gather_fc0_workspace", [None, 256], [None, 256]))
    for name in ("svr_linear_bwd_weight_workspace", "svr_linear_bwd_weight_bf16x3_workspace", "svr_linear_bwd_weight_f16x3_workspace"):
        add(name, MNK)
    for name in ("svr_linear_fwd_bf16x6_workspace", "svr_linear_fwd_f16x3_workspace", "svr_linear_bwd_data_bf16x3_workspace",
                 "svr_linear_bwd_data_f16x3_workspace"):
        add(name, NK)
    add("svr_fc_out_bwd_workspace", [(400000, 256), (0, 0), (1, 1), (63, 65)])
    add("svr_bce_ordered_workspace", [(8,), (0,), (1,), (400000,)])
    add("svr_conv3d_c1_fwd_stats_workspace", [v + (16,) for v in VOLUMES[:1] + VOLUMES[5:7]])
    for name in ("svr_conv3d_fwd_bf16x6_workspace", "svr_conv3d_fwd_f16x3_workspace", "svr_conv3d_bwd_data_bf16x3_workspace",
                 "svr_conv3d_bwd_data_f16x3_workspace"):
        add(name, ENCODER)
    for name in ("svr_conv3d_k3_bwd_weight_workspace", "svr_conv3d_k3_bwd_weight_bf16x3_workspace"):
        add(name, [(b, d, d, d, ci, co) for b, d, ci, co in ENCODER_AT])
    add("svr_bn_stats_workspace", [(8 * 128 ** 3, 16), (8 * 64 ** 3, 32), (400000, 256), (1, 1), (0, 1), (8 * 128 * 128, 64)])
    add("svr_stage1_workspace", VOLUMES[:1] + VOLUMES[5:7])
    add("svr_voxelize_splat_ordered_workspace", [(8, 50000, 128, 128, 128), (1, 100000, 139, 104, 112), (0, 0, 1, 1, 1), (1, 0, 1, 1, 1),
                                                 (1, 1, 1, 1, 1), (2, 63, 3, 5, 7), (8, 50000, 2047, 1023, 1023), (1, 2 ** 31 - 1, 4, 4, 4)])
    add("svr_blur_axis_bwd_ordered_workspace", [(8, 128, 128, 128, 5), (1, 139, 104, 112, 5), (1, 1, 1, 1, 1), (2, 3, 5, 7, 3)])
    for name in ("svr_conv2d_small_bwd_weight_workspace", "svr_conv2d_workspace_bytes", "svr_conv2d_bwd_weight_workspace"):
        for B in (8, 1):
            for H, W, C0, C1, k, stride, Cout in UNET:
                d = L.Conv2dDesc(None, None, B, H, W, C0, C1, k, stride, 0, 0)
                rows.append((name, [C.byref(d), Cout], [B, H, W, C0, C1, k, stride, Cout]))
        rows.append((name, [None, 32], [None, 32]))
    add("svr_conv2d_planes_bytes", sorted({(co, c0 + c1, k) for _, _, c0, c1, k, _, co in UNET}) + [(1, 1, 1), (0, 0, 3), (17, 15, 3)])
    add("svr_mc_workspace_bytes", LATTICES)
    add("svr_voxel_mesh_workspace_bytes", LATTICES)
    add("svr_sl_workspace_bytes", BLOCKED)
    add("svr_mesh_df_workspace_bytes", BLOCKED)
    add("svr_nn_search_workspace", [(5,), (0,), (-1,), (100000,), (1,)])
    add("svr_raycast_workspace_bytes", [(240, 320, 8), (240, 320, 16), (480, 640, 16), (1, 1, 8), (257, 63, 16), (32768, 32768, 8), (0, 0, 8),
                                        (8, 8, 7), (32769, 1, 8)])
    add("svr_vertex_color_workspace_bytes", [(0,), (1,), (257,), (100000,), (2 ** 31 - 1,), (-1,), (2 ** 31,)])
    add("svr_mesh_components_workspace_bytes", MESHES)
    add("svr_mesh_simplify_workspace_bytes", MESHES)
    add("svr_mesh_smooth_workspace_bytes", MESHES + [(100000, 2 ** 28), (0, 2 ** 28 + 1)])
    add("svr_depth_head_workspace", [(8, 256, 256), (8, 240, 320), (1, 1, 1)])
    return rows


def sizes(lib_path):
    from svr_amd import _lib as L, ops   # the binding's struct mirrors and signatures (the header is the same for both)
    lib = C.CDLL(lib_path or L.LIB_PATH)
    names = sorted(n for n, (res, _) in L.SIGNATURES.items() if "workspace" in n and res is L.I64)
    assert len(names) == 39, names
    names.append("svr_conv2d_planes_bytes")         # the UNet's weight planes: the one multi-piece buffer not called a workspace
    for n in names:
        getattr(lib, n).restype, getattr(lib, n).argtypes = L.SIGNATURES[n]
    out = {n: [] for n in names}
    for name, args, shown in table(L, ops):
        out[name].append(shown + [int(getattr(lib, name)(*args))])
    assert all(out.values()), [n for n in names if not out[n]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--ab", metavar="PARENT_LIB")
    a = ap.parse_args()
    if not a.ab:
        print(json.dumps(sizes(a.lib)))
        return
    run = lambda lib: json.loads(subprocess.run([sys.executable, __file__] + (["--lib", lib] if lib else []), check=True,  # noqa: E731
                                                capture_output=True, text=True).stdout.splitlines()[-1])
    parent, tree = run(os.path.abspath(a.ab)), run(a.lib)
    diff = [[n, p, t] for n in sorted(set(parent) | set(tree)) for p, t in zip(parent.get(n, []), tree.get(n, [])) if p != t]
    diff += [[n, len(parent.get(n, [])), len(tree.get(n, []))] for n in set(parent) | set(tree) if len(parent.get(n, [])) != len(tree.get(n, []))]
    print(json.dumps({"what": "every exported svr_*workspace* size function and svr_conv2d_planes_bytes over the shape table of tools/workspace_sizes.py, through the parent "
                              "commit's library and through this tree's, on the CPU; rows are [arguments..., returned bytes or error code]",
                      "functions": len(tree), "cases": sum(len(v) for v in tree.values()), "differences": len(diff), "differing": diff,
                      "parent": parent, "tree": tree}))
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
