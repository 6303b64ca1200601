"""The shapes of tests/test_gpu_wgrad_paths.py and the 3x3x3 weight-gradient kernel each one is there for.  Plain data, no GPU:
the CPU test (tests/test_capi_cpu.py) asks svr_conv3d_k3_bwd_weight_variant -- the function the launchers themselves call --
for every row and checks that the rows, together, reach every kernel the launchers can select; the GPU test asserts the same
tag before it runs a row.

Entry points (ops.WGRAD_VARIANT_OPS) and their kernel tags (ops.WGRAD_KERNELS):
  bwd_weight_f32 (svr_conv3d_k3_bwd_weight, csrc/conv3d.hip): "C1_CO16_LDS" = conv3d_c1_bwd_weight_co16_lds_kernel (Ci == 1,
    Co == 16, W <= 128), "C1_CO16" = conv3d_c1_bwd_weight_co16_kernel (wider rows), "C1" = conv3d_c1_bwd_weight_kernel (Ci == 1,
    other Co <= 32), "BRICK" = conv3d_bwd_weight_brick_kernel (Ci, Co % 4 == 0; min(cdiv(512, tile pairs), bricks) workgroups
    per 32 x 32 channel-tile pair);
  bwd_weight_f16x3s / bwd_weight_bf16x3 (csrc/conv3d_bwdw_bf16.hip, Ci, Co % 4 == 0): parts = min(cdiv(256, tile pairs), bricks)
    workgroups per tile pair; "WS_PAIR" (Ci <= 16) / "WS" = conv3d_bwd_weight_ws_kernel where bricks >= 8 parts, "X3" =
    conv3d_bwd_weight_x3_kernel otherwise.
A brick is 4 x 4 x 8 voxels (z, y, x); bricks = B cdiv(D, 4) cdiv(H, 4) cdiv(W, 8).  None = the entry point refuses the shape
(SVR_E_UNSUPPORTED, -4: the split kernels take no Ci == 1)."""

F32_OP = "bwd_weight_f32"
SPLIT_OPS = ("bwd_weight_f16x3s", "bwd_weight_bf16x3")
OPS = (F32_OP,) + SPLIT_OPS
UNSUPPORTED = -4      # SVR_E_UNSUPPORTED

# (name, B, dims, Ci, Co, gscale, f32 tag, split tag, bricks per workgroup of the f32 BRICK kernel: "1" / ">1" / None,
#  of the split kernel: "1" / ">1" / None)
CASES = [
    # ---- the split kernels ----------------------------------------------------------------------------------------------------
    # 16 x 16 x 8 = 2048 bricks on 256 parts: exactly the 8 bricks per workgroup the wave-specialised kernel asks for; partial
    # bricks on all three faces (61 = 15 x 4 + 1, 62 = 15 x 4 + 2, 63 = 7 x 8 + 7); paired-row tiles (Ci <= 16)
    ("pair_16_32", 1, (61, 62, 63), 16, 32, 1e-6, "BRICK", "WS_PAIR", ">1", ">1"),
    # the same volume with half-empty channel tiles: 8 of the 16 paired rows, 16 of the 32 columns live
    ("pair_8_16", 1, (61, 62, 63), 8, 16, 1e-5, "BRICK", "WS_PAIR", ">1", ">1"),
    # 2 x 16 x 8 x 8 = 2048 bricks over two samples, full 32-channel tiles
    ("ws_32_32_b2", 2, (61, 30, 63), 32, 32, 1e-4, "BRICK", "WS", ">1", ">1"),
    # 16 x 16 x 7 = 1792 bricks < 8 x 256: the 8-wave kernel with SEVEN bricks per workgroup, partial bricks among them
    ("x3_multi_16_32", 1, (61, 62, 55), 16, 32, 1e-3, "BRICK", "X3", ">1", ">1"),
    # 8 x 8 x 8 = 512 bricks, 4 tile pairs -> 64 parts of 8 bricks
    ("ws_64_64", 1, (29, 30, 61), 64, 64, 1e-2, "BRICK", "WS", ">1", ">1"),
    # padded channel tiles: 48 = 32 + 16 rows, 40 = 32 + 8 columns
    ("ws_48_40", 1, (29, 30, 61), 48, 40, 1e-1, "BRICK", "WS", ">1", ">1"),
    # 4 x 4 x 8 = 128 bricks, 16 tile pairs -> 16 parts of 8 bricks; the f32 BRICK kernel: 128 bricks on 32 parts (more bricks
    # than parts)
    ("ws_128_128", 1, (13, 14, 61), 128, 128, 1.0, "BRICK", "WS", ">1", ">1"),
    # the encoder's 8^3 layer at batch 2: 8 bricks, one per workgroup in both units (fewer bricks than parts)
    ("x3_128_128_b2", 2, (8, 8, 8), 128, 128, 30.0, "BRICK", "X3", "1", "1"),
    # Ci % 32 = 20 and Co % 32 = 12, both odd multiples of 4: the clamped last channel quad of the loads; 2 x 2 x 2 partial bricks
    ("x3_20_12", 1, (5, 6, 9), 20, 12, 1e-2, "BRICK", "X3", "1", "1"),
    # ---- Ci == 1 (conv_in; the f32 entry point only) --------------------------------------------------------------------------
    # W = 130 > 128: the scattered-load kernel, W % 32 = 2 (a last x group with two live voxels)
    ("c1_co16_w130", 2, (3, 2, 130), 1, 16, 1e-3, "C1_CO16", None, None, None),
    # the LDS kernel: one partial 16-row y block, odd sizes on every axis
    ("c1_lds_odd", 2, (9, 7, 11), 1, 16, 1e-4, "C1_CO16_LDS", None, None, None),
    # H = 17: a second y block of one row; W exactly at the W <= 128 limit of the LDS rows
    ("c1_lds_w128", 1, (2, 17, 128), 1, 16, 1.0, "C1_CO16_LDS", None, None, None),
    # the generic Ci == 1 kernel: all 32 columns, and 8 of them
    ("c1_co32", 2, (9, 7, 11), 1, 32, 1e-5, "C1", None, None, None),
    ("c1_co8", 2, (9, 7, 11), 1, 8, 1e-1, "C1", None, None, None),
]


def by_name(name):
    return next(c for c in CASES if c[0] == name)


def bricks(B, dims):
    return B * -(-dims[0] // 4) * -(-dims[1] // 4) * -(-dims[2] // 8)


def expected():
    """[(name, op, B, dims, Ci, Co, tag or None, bricks per workgroup "1" / ">1" / None)] for every (row, entry point)"""
    out = []
    for name, B, dims, Ci, Co, _, ftag, stag, fper, sper in CASES:
        out.append((name, F32_OP, B, dims, Ci, Co, ftag, fper))
        out += [(name, op, B, dims, Ci, Co, stag, sper) for op in SPLIT_OPS]
    return out


# every kernel the launchers can select, as (entry point, tag)
ALL_VARIANTS = ({(F32_OP, t) for t in ("C1_CO16_LDS", "C1_CO16", "C1", "BRICK")} |
                {(op, t) for op in SPLIT_OPS for t in ("WS_PAIR", "WS", "X3")})
