"""The shapes of tests/test_gpu_conv_paths.py and the kernel instantiation each one is there for.  Plain data, no GPU: the CPU
test (tests/test_capi_cpu.py) asks svr_conv3d_k3_variant for every entry and checks that the set still reaches every
instantiation the 3x3x3 launchers of csrc/conv3d_bf16.hip can produce; the GPU test asserts the same before it runs a case.

A variant is written as a tag:  "P" = conv3d_brick_p_kernel<16, ., 2> (persistent, 8x4x8 double bricks, 32 columns);
"VT2" = its one-brick-per-workgroup form conv3d_brick_x3_kernel<16, 1, 2, ., 2>;  "CK32TN2" etc. =
conv3d_brick_x3_kernel<CK, TN, 2, .> on 4x4x8 bricks.  `fwd` is the tag of the forward f16x3 entry point (output columns = Co,
reduction side = Ci), `bwd` the tag of BOTH backward-data entry points (f16x3s and bf16x3: columns = Ci, reduction = Co);
None = the entry point does not take the shape (forward needs Ci % 16 == 0; backward-data Co % 16 == 0 and Ci even)."""

FWD_OPS = ("fwd_f16x3",)
BWD_OPS = ("bwd_data_f16x3s", "bwd_data_bf16x3")


def tag(v):
    """variant dict of ops.conv3d_k3_variant -> tag"""
    if v["vt"] == 2:
        assert v["ck"] == 16 and v["tn"] == 1, v
        return "P" if v["persistent"] else "VT2"
    assert not v["persistent"], v
    return f"CK{v['ck']}TN{v['tn']}"


# (name, B, dims, Ci, Co, gscale, fwd tag, bwd tag)
ODD = (34, 26, 28)       # 9 x 7 x 4 bricks per sample: 756 at batch 3, 504 at batch 2 (420 / 280 double bricks)
CASES = [
    # 1. the encoder's layers at batch 8 (gscale: the magnitudes of tests/test_gpu_conv_wgrad.py REAL)
    ("real64_16_32", 8, (64, 64, 64), 16, 32, 1e-6, "P", "P"),                # backward-data: 16 of the 32 columns live
    ("real64_32_32", 8, (64, 64, 64), 32, 32, 1e-5, "P", "P"),
    ("real32_32_64", 8, (32, 32, 32), 32, 64, 1e-4, "CK32TN2", "P"),          # backward-data: 1024 double bricks
    ("real32_64_64", 8, (32, 32, 32), 64, 64, 1e-3, "CK32TN2", "CK32TN2"),
    ("real16_64_128", 8, (16, 16, 16), 64, 128, 1e-2, "CK32TN2", "CK32TN1"),  # 256 bricks: TN4 (and TN2 at 64 columns) fail the 512 rule
    ("real16_128_128", 8, (16, 16, 16), 128, 128, 1.0, "CK32TN2", "CK32TN2"),
    ("real8_128_128", 8, (8, 8, 8), 128, 128, 30.0, "CK32TN1", "CK32TN1"),    # 32 bricks
    # 2. partial bricks on the persistent path: D % 8 = 5 (37) and 3 (35: a lone 4-slice on top of the last double brick),
    #    H % 4 != 0, W % 8 != 0; backward-data with 16 and with 8 live columns of 32
    ("part37_16_32", 4, (37, 30, 61), 16, 32, 1e-4, "P", "P"),
    ("part37_32_32", 4, (37, 30, 61), 32, 32, 1e-3, "P", "P"),
    ("part35_16_32", 4, (35, 29, 59), 16, 32, 1e-5, "P", "P"),
    ("part35_8_16", 4, (35, 29, 59), 8, 16, 1e-2, None, "P"),
    # 3. TN4: 128 (and 96: last 32-column tile dead) columns at 756 bricks, CK32 and CK16 reduction sides
    ("tn4_128_128", 3, ODD, 128, 128, 1e-1, "CK32TN4", "CK32TN4"),
    ("tn4_48_128", 3, ODD, 48, 128, 1e-3, "CK16TN4", "CK32TN2"),              # backward-data: 48 columns, second tile half dead
    ("tn4_128_48", 3, ODD, 128, 48, 1e-5, "CK32TN2", "CK16TN4"),              # forward: 48 columns on a CK32 reduction
    ("tn4_32_96", 3, ODD, 32, 96, 1e-2, "CK32TN4", "CK32TN1"),
    ("tn4_96_16", 3, ODD, 96, 16, 1e-4, "CK32TN1", "CK16TN4"),
    # 4. TN2 at 756 bricks (64 and 48 columns) ...
    ("tn2_16_64", 3, ODD, 16, 64, 1e-6, "CK16TN2", "CK32TN1"),
    ("tn2_64_32", 3, ODD, 64, 32, 1.0, "CK32TN1", "CK32TN2"),
    ("tn2_48_16", 3, ODD, 48, 16, 1e-3, "CK16TN1", "CK16TN2"),
    ("tn2_32_48", 3, ODD, 32, 48, 1e-1, "CK32TN2", "CK16TN1"),
    #    ... and at 504 bricks with 96 / 128 columns (TN4 fails the 512 rule, TN2 passes it)
    ("tn2_128_128_b2", 2, ODD, 128, 128, 1e-2, "CK32TN2", "CK32TN2"),
    ("tn2_16_96_b2", 2, ODD, 16, 96, 1e-4, "CK16TN2", "CK32TN1"),
    ("tn2_96_16_b2", 2, ODD, 96, 16, 10.0, "CK32TN1", "CK16TN2"),
]
REAL = [c[0] for c in CASES[:7]]

# 5. SVR_CONV_PERSISTENT=0 (read once per process: a child process of the test): the one-brick VT2 form where "P" ran
NO_PERSISTENT = ["part37_16_32", "part35_8_16"]

# 6. the index limit of persistent_bricks(): D H W max(Ci, Co) < 2^30.  256 x 256 x 132 x 128 = 1.107e9 elements (over: VT2 in
#    this process), 256 x 256 x 127 x 128 = 1.065e9 (under: persistent).  (name, B, dims, Ci, Co, fwd tag, bwd tag)
LIMIT = [
    ("over_fwd", 1, (256, 256, 132), 128, 32, "VT2", None),
    ("under_fwd", 1, (256, 256, 127), 128, 32, "P", None),
    ("over_bwd", 1, (256, 256, 132), 32, 128, None, "VT2"),
    ("under_bwd", 1, (256, 256, 127), 32, 128, None, "P"),
]


def by_name(name):
    return next(c for c in CASES if c[0] == name)


def expected():
    """[(name, op, B, dims, Ci, Co, tag)] for every (case, entry point) that the GPU file runs in its own process"""
    out = []
    for name, B, dims, Ci, Co, *rest in CASES + [l[:5] + (None,) + l[5:] for l in LIMIT]:
        ftag, btag = rest[-2], rest[-1]
        out += [(name, op, B, dims, Ci, Co, ftag) for op in FWD_OPS if ftag]
        out += [(name, op, B, dims, Ci, Co, btag) for op in BWD_OPS if btag]
    return out


# every instantiation the three launchers can produce, as (entry point, tag)
ALL_VARIANTS = {(op, t) for op in FWD_OPS + BWD_OPS
                for t in ["P", "VT2"] + [f"CK{ck}TN{tn}" for ck in (16, 32) for tn in (1, 2, 4)]}
