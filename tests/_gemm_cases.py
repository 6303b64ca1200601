"""The shapes of tests/test_gpu_gemm_paths.py and the launcher branch each one is there for.  Plain data, no GPU: the CPU test
(tests/test_capi_cpu.py) asks ops.linear_variant (svr_linear_variant: the function the launchers of csrc/gemm*.hip call) for
every entry and checks that the set still reaches every (entry point, kernel, epilogue form, bias form) the launchers can
produce; the GPU test asserts the same tag before it runs a case.

In `ops` terms x is (M,K), w is (N,K), dy is (M,N).  A layout is (leading dimension, first column) of the operand inside a
wider buffer whose first element is 16-byte aligned; operands that are not named are contiguous.  A tag is
"kernel/epilogue" (forward, backward-data: "coal" = float4 rows through LDS, "lane" = one dword per lane) or "kernel/bias form"
(backward-weight, with db asked for), or "refuse" where the entry point answers with an SVR_E_* code (the op raises).  The kernel
names are ops.LINEAR_KERNELS: "nt" / "nn" / "tn" are the exact-f32 kernels, also where ops routes a split mode to them."""

FWD_MODES = ("f32", "f16x3", "bf16x6")
BWD_MODES = ("f32", "f16x3s", "bf16x3")
MODES = {"fwd": FWD_MODES, "bwd_data": BWD_MODES, "bwd_weight": BWD_MODES}


def _f(*tags):
    return dict(zip(FWD_MODES, tags))


def _b(*tags):
    return dict(zip(BWD_MODES, tags))


# (name, kind, M, N, K, {operand: (ld, col0)}, options, {mode: tag})
#   options: "gscale" (|dy|: 1 or 1e-6), "zero_mask" (mask <= 0 everywhere), "bias" (the want_bias values of backward-weight)
CASES = [
    # ---- forward: y = epi(x w^T), each with bias + ReLU, bias only and no bias
    ("f_1x32x16", "fwd", 1, 32, 16, {}, {}, _f("nt/lane", "nt64/lane", "nt_x6/lane")),            # one row, ONE k-step (klast = 0)
    ("f_129x64x48", "fwd", 129, 64, 48, {}, {}, _f("nt/lane", "nt64/lane", "nt_x6/lane")),        # N = 64 stays narrow; 3 k-steps (odd)
    ("f_200x72x32", "fwd", 200, 72, 32, {}, {}, _f("nt/lane", "nt128/coal", "nt_x6/lane")),       # partial column tile on the float4 epilogue
    ("f_130x160x64", "fwd", 130, 160, 64, {}, {}, _f("nt/lane", "nt128/coal", "nt_x6/lane")),     # two column tiles, the last 32 wide
    ("f_70x130x16", "fwd", 70, 130, 16, {}, {}, _f("nt/lane", "nt128/lane", "nt_x6/lane")),       # N % 4 != 0: per-lane epilogue, one k-step
    ("f_257x256x80_out", "fwd", 257, 256, 80, {"out": (288, 16)}, {}, _f("nt/lane", "nt128/coal", "nt_x6/lane")),    # 5 k-steps
    ("f_257x256x80_out1", "fwd", 257, 256, 80, {"out": (288, 17)}, {}, _f("nt/lane", "nt128/lane", "nt_x6/lane")),   # ... one column on
    ("f_130x96x48_xw", "fwd", 130, 96, 48, {"a": (80, 0), "b": (80, 16)}, {}, _f("nt/lane", "nt128/coal", "nt_x6/lane")),
    # ---- backward-data: dx = (dy w) [* (mask > 0)], each with and without the mask
    ("d_1x16x16", "bwd_data", 1, 16, 16, {}, {"gscale": 1.0}, _b("nn/lane", "nt128_bwd/coal", "nn/lane")),
    ("d_130x48x132", "bwd_data", 130, 48, 132, {}, {"gscale": 1e-6}, _b("nn/lane", "nt128_bwd/coal", "nn/lane")),   # last tile 4 wide
    ("d_130x48x130", "bwd_data", 130, 48, 130, {"out": (132, 0), "mask": (132, 0)}, {"gscale": 1.0},
     _b("refuse", "nt128_bwd/lane", "refuse")),                                                                     # K % 4 != 0
    ("d_129x32x36", "bwd_data", 129, 32, 36, {}, {"gscale": 1e-6}, _b("nn/lane", "nn_x3/coal", "nn_x3/coal")),      # N = 32: one k-step
    ("d_300x96x260", "bwd_data", 300, 96, 260, {}, {"gscale": 1.0}, _b("nn/lane", "nn_x3/coal", "nn_x3/coal")),     # last tile 4 wide
    ("d_200x256x64_w", "bwd_data", 200, 256, 64, {"b": (96, 16), "out": (96, 16), "mask": (96, 16)}, {"gscale": 1e-6},
     _b("nn/lane", "nn_x3/coal", "nn_x3/coal")),                                                  # column slices of the kept features
    ("d_129x32x36_out1", "bwd_data", 129, 32, 36, {"out": (40, 1)}, {"gscale": 1.0}, _b("nn/lane", "nn/lane", "nn/lane")),
    ("d_70x16x36_zero", "bwd_data", 70, 16, 36, {}, {"gscale": 1.0, "zero_mask": True}, _b("nn/lane", "nt128_bwd/coal", "nn/lane")),
    ("d_70x32x36_zero", "bwd_data", 70, 32, 36, {}, {"gscale": 1e-6, "zero_mask": True}, _b("nn/lane", "nn_x3/coal", "nn_x3/coal")),
    # ---- backward-weight: dw = dy^T x, db = column sums of dy; each with and without db
    ("w_1x4x4", "bwd_weight", 1, 4, 4, {}, {"gscale": 1.0}, _b("tn/colsum_vec", "tn_tr/kernel", "tn_tr/kernel")),              # 1 split
    ("w_33x8x36", "bwd_weight", 33, 8, 36, {}, {"gscale": 1e-6}, _b("tn/colsum_vec", "tn_tr/kernel", "tn_tr/kernel")),         # 2 splits, 1-row tail
    ("w_1100x72x132", "bwd_weight", 1100, 72, 132, {}, {"gscale": 1.0}, _b("tn/colsum_slow", "tn_tr/kernel", "tn_tr/kernel")), # 35 splits
    ("w_300x260x64", "bwd_weight", 300, 260, 64, {}, {"gscale": 1e-6}, _b("tn/colsum_slow", "tn_tr/kernel", "tn_tr/kernel")),  # N over 3 row tiles
    ("w_520x1792x128", "bwd_weight", 520, 1792, 128, {}, {"gscale": 1.0, "bias": (False,)}, _b("tn/none", "tn_tr/none", "tn_tr/none")),
    ("w_1152x32x16", "bwd_weight", 1152, 32, 16, {}, {"gscale": 1e-6, "bias": (False,), "modes": ("f32",)}, {"f32": "tn/none"}),
    ("w_100x8x6", "bwd_weight", 100, 8, 6, {}, {"gscale": 1.0, "modes": ("bf16x3",)}, {"bf16x3": "tn_prepass/kernel"}),        # K % 4 != 0
    ("w_1100x136x130", "bwd_weight", 1100, 136, 130, {}, {"gscale": 1e-6, "modes": ("bf16x3",)}, {"bf16x3": "tn_prepass/kernel"}),
    ("w_300x64x64_x66", "bwd_weight", 300, 64, 64, {"b": (66, 0)}, {"gscale": 1.0, "modes": ("bf16x3",)}, {"bf16x3": "tn_prepass/kernel"}),
    ("w_130x72x36_dy", "bwd_weight", 130, 72, 36, {"a": (136, 32)}, {"gscale": 1e-6}, _b("tn/colsum_slow", "tn_tr/kernel", "tn_tr/kernel")),
]


def by_name(name):
    return next(c for c in CASES if c[0] == name)


def modes(case):
    return case[6].get("modes", MODES[case[1]])


def layout(case, operand, cols):
    """(leading dimension, low four address bits, unit column stride) of `operand` ("a" / "b" / "out" / "mask"), as
    ops.operand_layout reports it for the tensors the GPU test builds; cols = its contiguous width."""
    ld, col0 = case[5].get(operand, (cols, 0))
    return (ld, (4 * col0) & 15, True)


def query(ops, case, mode, want_bias=True, masked=True, contiguous=False):
    """ops.linear_variant for the case in `mode` (contiguous: the same shape with every operand contiguous)."""
    name, kind, M, N, K, lays, opt, _ = case
    cols = {"fwd": (K, K, N, None), "bwd_data": (N, K, K, K), "bwd_weight": (N, K, K, None)}[kind]
    a, b, out, mask = [None if c is None else ((c, 0, True) if contiguous else layout(case, o, c))
                       for o, c in zip(("a", "b", "out", "mask"), cols)]
    if kind != "bwd_data" or not masked:
        mask = None
    return ops.linear_variant(kind, mode, M, N, K, a=a, b=b, out=out, mask=mask, epilogue=2 if kind == "fwd" else None,
                              want_bias=want_bias and kind == "bwd_weight")


def tag(kind, v):
    """variant dict of ops.linear_variant -> tag"""
    if v["status"] != 0:
        return "refuse"
    return f"{v['kernel']}/{v['bias']}" if kind == "bwd_weight" else f"{v['kernel']}/{'coal' if v['coalesced'] else 'lane'}"


# every (entry point, kernel, float4 epilogue, bias form) the launchers can produce
ALL_VARIANTS = (
    {("fwd_f32", "nt", False, "none"), ("fwd_bf16x6", "nt_x6", False, "none"), ("fwd_f16x3", "nt64", False, "none"),
     ("fwd_f16x3", "nt128", False, "none"), ("fwd_f16x3", "nt128", True, "none"),
     ("bwd_data_f32", "nn", False, "none"), ("bwd_data_bf16x3", "nn_x3", True, "none"), ("bwd_data_f16x3s", "nn_x3", True, "none"),
     ("bwd_data_f16x3s", "nt128_bwd", True, "none"), ("bwd_data_f16x3s", "nt128_bwd", False, "none"),
     ("bwd_weight_f32", "tn", False, "none"), ("bwd_weight_f32", "tn", False, "colsum_vec"), ("bwd_weight_f32", "tn", False, "colsum_slow")}
    | {(op, k, False, b) for op, k in (("bwd_weight_f16x3s", "tn_tr"), ("bwd_weight_bf16x3", "tn_tr"), ("bwd_weight_bf16x3", "tn_prepass"))
       for b in ("none", "kernel")})
