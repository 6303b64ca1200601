"""Cases of tests/test_gpu_conv2d_paths.py: plain data, one row per case with the launcher branches it is there for.  The tags
are what svr_conv2d_variant (the function the conv2d launchers themselves call) answers for the row; the CPU test
test_conv2d_variant_table_and_every_branch_is_reached (tests/test_capi_cpu.py) asserts every tag and that the rows, together,
reach every combination the launchers can produce.

A row: (name, (B, H, W, C0, C1, Cout, k, stride), misaligned, {op: tag}, extras)
  misaligned: names of the operands that start 4 bytes into their buffer ("src0", "src1", "dy"): the 16-byte loaders are off
  tag:    forward / backward-data GEMMs  "<family>/<v4|s>/c<classes>/<epilogue>"
          weight-gradient GEMM           "wgrad_tr/<v4|s>/<dy4|dy1>"
          small kernels                  "small/co<Cout>/k<k>/<v4|s>" (backward-data gathers dY per channel: "small/co<Cout>/k<k>")
  extras: regimes of a branch that the tag does not spell (see extras())."""
import itertools

OPS = ("fwd", "bwd_data", "bwd_weight")


def tag(v):
    vec = "v4" if v["vec4"] else "s"
    if v["family"] == "small":
        return f"small/co{v['co']}/k{v['kk']}" + ("" if v["op"] == "bwd_data" else "/" + vec)
    if v["family"] == "wgrad_tr":
        return f"wgrad_tr/{vec}/{'dy4' if v['dy_vec4'] else 'dy1'}"
    return f"{v['family']}/{vec}/c{v['classes']}/{v['epilogue']}"


def extras(v):
    """regimes inside a branch: loops that run more than once, second grid dimensions, caps"""
    e = set()
    op = v["op"]
    if v["family"] in ("igemm64", "igemm128"):
        if v["splits"] > 1 and v["split_stride"] > 1024 * v["reduce_grid"]:
            e.add(f"{op}:reduce_strides")                      # ig_reduce_kernel's grid-stride loop
        if v["splits"] == 1 and v["tiles"] >= 512:
            e.add(f"{op}:unsplit_by_tiles")
        if v["ksteps"] >= 512:
            e.add(f"{op}:ksteps>=512")
    elif v["family"] == "wgrad_tr":
        if v["splits"] > 4:
            e.add("wgrad:slabs>4")                             # every 64-lane group of conv_wgrad_reduce_kernel walks several slabs
        if v["splits"] >= 100:
            e.add("wgrad:slabs>=100")
        if v["rows_per_split"] > 128:
            e.add("wgrad:rows_per_split>128")
    else:
        if op != "bwd_weight" and v["capped"]:
            e.add(f"{op}:small_capped")
        if op == "bwd_weight":
            if v["grid_y"] > 1:
                e.add("small_wgrad:grid_y>1")
            if v["ipg"] == 1024 and v["groups"] == 1:
                e.add("small_wgrad:ipg1024")
            if v["rows_per_block"] > 64:
                e.add("small_wgrad:rows_per_block>64")
    return e


MIS = {"src0": "lo_src0", "src1": "lo_src1", "dy": "lo_dy"}


def query(ops, op, shape, mis=()):
    return ops.conv2d_variant(op, *shape, **{MIS[m]: 4 for m in mis})


# every (op, tag) the launchers can produce
_IG = [f"{fam}/{vec}/c{{}}/{epi}" for fam, epis in (("igemm64", ("lane", "reduce_v4", "reduce_scalar")),
                                                   ("igemm128", ("coal", "lane", "reduce_v4", "reduce_scalar")))
       for vec in ("v4", "s") for epi in epis]
ALL_VARIANTS = {("fwd", t.format(1)) for t in _IG} | {("bwd_data", t.format(c)) for t in _IG for c in (1, 4)} | \
    {("bwd_weight", t) for t in ("wgrad_tr/v4/dy4", "wgrad_tr/v4/dy1", "wgrad_tr/s/dy1")} | \
    {(op, f"small/co{co}/k{k}/{vec}") for op in ("fwd", "bwd_weight") for co, k, vec in itertools.product((1, 2, 3, 4), (3, 4), ("v4", "s"))} | \
    {("bwd_data", f"small/co{co}/k{k}") for co, k in itertools.product((1, 2, 3, 4), (3, 4))}
ALL_EXTRAS = {"fwd:reduce_strides", "fwd:unsplit_by_tiles", "bwd_data:unsplit_by_tiles", "fwd:ksteps>=512", "wgrad:slabs>4", "wgrad:slabs>=100",
              "wgrad:rows_per_split>128", "fwd:small_capped", "bwd_data:small_capped", "small_wgrad:grid_y>1", "small_wgrad:ipg1024",
              "small_wgrad:rows_per_block>64"}

def unet_layers(cls, B, H, W, nf=32, channels_in=3, channels_out=1):
    """[(layer name, (B, H, W, C0, C1, Cout, k, stride))] of a model/unet.py network as its convolutions see them: a decoder
    convolution reads the activated, upsampled, concatenated tensor conv2d_virtual wrote (one source, twice the side)."""
    out, c, h, w = [], channels_in, H, W
    for i, mult in enumerate(cls.ENC, start=1):
        out.append((f"conv{i}", (B, h, w, c, 0, nf * mult, 4, 2)))
        c, h, w = nf * mult, h // 2, w // 2
    for name, cin, cout, _ in cls.DEC:
        h, w = 2 * h, 2 * w
        out.append((name, (B, h, w, nf * cin, 0, channels_out if cout is None else nf * cout, 3, 1)))
    return out

CASES = [
    ('f64_unsplit', (2, 9, 7, 16, 0, 40, 3, 1), (), {'fwd': 'igemm64/v4/c1/lane', 'bwd_data': 'igemm64/v4/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('f128_coal_2src', (2, 9, 7, 8, 4, 72, 3, 1), (), {'fwd': 'igemm128/v4/c1/coal', 'bwd_data': 'igemm64/v4/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('n130_scalar', (1, 6, 5, 6, 0, 130, 3, 1), (), {'fwd': 'igemm128/s/c1/lane', 'bwd_data': 'igemm64/s/c1/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('all_odd', (1, 6, 5, 5, 3, 7, 3, 1), (), {'fwd': 'igemm64/s/c1/lane', 'bwd_data': 'igemm64/s/c1/lane', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('tiles547', (1, 700, 100, 16, 0, 96, 3, 1), (), {'fwd': 'igemm128/v4/c1/coal', 'bwd_data': 'igemm64/v4/c1/lane', 'bwd_weight': 'wgrad_tr/v4/dy4'}, ['bwd_data:unsplit_by_tiles', 'fwd:unsplit_by_tiles', 'wgrad:rows_per_split>128', 'wgrad:slabs>4', 'wgrad:slabs>=100']),
    ('reduce_stride', (1, 128, 128, 32, 0, 128, 3, 1), (), {'fwd': 'igemm128/v4/c1/reduce_v4', 'bwd_data': 'igemm64/v4/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, ['fwd:reduce_strides', 'wgrad:slabs>4', 'wgrad:slabs>=100']),
    ('m2_128_coal_split', (2, 6, 6, 96, 0, 64, 4, 2), (), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c4/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('m2_128_lane_unsplit', (1, 6, 6, 70, 0, 32, 4, 2), (), {'fwd': 'igemm64/s/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c4/lane', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('odd_s2_deep', (2, 5, 7, 128, 0, 256, 4, 2), (), {'fwd': 'igemm128/v4/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c4/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('odd_s2', (2, 5, 3, 24, 0, 48, 4, 2), (), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm64/v4/c4/lane', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('one_px_out', (1, 3, 3, 16, 0, 16, 4, 2), (), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm64/v4/c4/lane', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('ig_n3', (1, 4, 4, 512, 0, 3, 3, 1), (), {'fwd': 'igemm64/v4/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c1/coal', 'bwd_weight': 'wgrad_tr/v4/dy1'}, []),
    ('ig_n2', (1, 6, 6, 260, 0, 2, 4, 2), (), {'fwd': 'igemm64/v4/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c4/coal', 'bwd_weight': 'wgrad_tr/v4/dy1'}, []),
    ('ig_n1_k585', (1, 6, 6, 1040, 0, 1, 3, 1), (), {'fwd': 'igemm64/v4/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c1/coal', 'bwd_weight': 'wgrad_tr/v4/dy1'}, ['fwd:ksteps>=512']),
    ('small_8192', (1, 6, 6, 256, 0, 2, 4, 2), (), {'fwd': 'small/co2/k4/v4', 'bwd_data': 'small/co2/k4', 'bwd_weight': 'small/co2/k4/v4'}, ['small_wgrad:ipg1024']),
    ('small_gridy2', (1, 9, 9, 260, 0, 1, 4, 2), (), {'fwd': 'small/co1/k4/v4', 'bwd_data': 'small/co1/k4', 'bwd_weight': 'small/co1/k4/v4'}, ['small_wgrad:grid_y>1', 'small_wgrad:ipg1024']),
    ('small_cap_c4', (1, 260, 256, 4, 0, 1, 3, 1), (), {'fwd': 'small/co1/k3/v4', 'bwd_data': 'small/co1/k3', 'bwd_weight': 'small/co1/k3/v4'}, ['fwd:small_capped', 'small_wgrad:rows_per_block>64']),
    ('small_cap_c68', (1, 256, 258, 68, 0, 2, 3, 1), (), {'fwd': 'small/co2/k3/v4', 'bwd_data': 'small/co2/k3', 'bwd_weight': 'small/co2/k3/v4'}, ['bwd_data:small_capped', 'fwd:small_capped', 'small_wgrad:rows_per_block>64']),
    ('k1_one_src', (1, 40, 40, 16, 0, 16, 1, 1), (), {'fwd': 'igemm64/v4/c1/lane'}, []),
    ('k1_2src', (1, 9, 7, 8, 12, 24, 1, 1), (), {'fwd': 'igemm64/v4/c1/lane'}, []),
    ('mis_src0', (2, 9, 7, 16, 0, 40, 3, 1), ('src0',), {'fwd': 'igemm64/s/c1/lane', 'bwd_data': 'igemm64/v4/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('mis_src1', (2, 9, 7, 8, 4, 72, 3, 1), ('src1',), {'fwd': 'igemm128/s/c1/coal', 'bwd_data': 'igemm64/v4/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('mis_dy', (2, 9, 7, 16, 0, 40, 3, 1), ('dy',), {'fwd': 'igemm64/v4/c1/lane', 'bwd_data': 'igemm64/s/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('sm_co1_k3_s', (1, 6, 5, 3, 0, 1, 3, 1), (), {'fwd': 'small/co1/k3/s', 'bwd_data': 'small/co1/k3', 'bwd_weight': 'small/co1/k3/s'}, []),
    ('sm_co1_k4_s', (1, 6, 5, 3, 0, 1, 4, 2), (), {'fwd': 'small/co1/k4/s', 'bwd_data': 'small/co1/k4', 'bwd_weight': 'small/co1/k4/s'}, []),
    ('sm_co2_k3_s', (1, 6, 5, 3, 0, 2, 3, 1), (), {'fwd': 'small/co2/k3/s', 'bwd_data': 'small/co2/k3', 'bwd_weight': 'small/co2/k3/s'}, []),
    ('sm_co3_k3_s', (1, 6, 5, 3, 0, 3, 3, 1), (), {'fwd': 'small/co3/k3/s', 'bwd_data': 'small/co3/k3', 'bwd_weight': 'small/co3/k3/s'}, []),
    ('sm_co2_k4_s', (1, 6, 5, 3, 0, 2, 4, 2), (), {'fwd': 'small/co2/k4/s', 'bwd_data': 'small/co2/k4', 'bwd_weight': 'small/co2/k4/s'}, []),
    ('sm_co4_k3_s', (1, 6, 5, 3, 0, 4, 3, 1), (), {'fwd': 'small/co4/k3/s', 'bwd_data': 'small/co4/k3', 'bwd_weight': 'small/co4/k3/s'}, []),
    ('sm_co3_k3_v4', (1, 6, 5, 4, 0, 3, 3, 1), (), {'fwd': 'small/co3/k3/v4', 'bwd_data': 'small/co3/k3', 'bwd_weight': 'small/co3/k3/v4'}, []),
    ('sm_co3_k4_s', (1, 6, 5, 3, 0, 3, 4, 2), (), {'fwd': 'small/co3/k4/s', 'bwd_data': 'small/co3/k4', 'bwd_weight': 'small/co3/k4/s'}, []),
    ('sm_co4_k3_v4', (1, 6, 5, 4, 0, 4, 3, 1), (), {'fwd': 'small/co4/k3/v4', 'bwd_data': 'small/co4/k3', 'bwd_weight': 'small/co4/k3/v4'}, []),
    ('sm_co4_k4_s', (1, 6, 5, 3, 0, 4, 4, 2), (), {'fwd': 'small/co4/k4/s', 'bwd_data': 'small/co4/k4', 'bwd_weight': 'small/co4/k4/s'}, []),
    ('sm_co3_k4_v4', (1, 6, 5, 4, 0, 3, 4, 2), (), {'fwd': 'small/co3/k4/v4', 'bwd_data': 'small/co3/k4', 'bwd_weight': 'small/co3/k4/v4'}, []),
    ('sm_co4_k4_v4', (1, 6, 5, 4, 0, 4, 4, 2), (), {'fwd': 'small/co4/k4/v4', 'bwd_data': 'small/co4/k4', 'bwd_weight': 'small/co4/k4/v4'}, []),
    ('bwd64_s_c4_lane', (1, 6, 5, 3, 0, 6, 4, 2), (), {'fwd': 'igemm64/s/c1/reduce_scalar', 'bwd_data': 'igemm64/s/c4/lane', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd64_s_c4_reduce_scalar', (1, 6, 5, 3, 0, 66, 4, 2), (), {'fwd': 'igemm128/s/c1/reduce_scalar', 'bwd_data': 'igemm64/s/c4/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd64_v4_c4_reduce_scalar', (1, 6, 5, 3, 0, 72, 4, 2), (), {'fwd': 'igemm128/s/c1/reduce_v4', 'bwd_data': 'igemm64/v4/c4/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd64_s_c4_reduce_v4', (1, 6, 5, 4, 0, 66, 4, 2), (), {'fwd': 'igemm128/v4/c1/reduce_scalar', 'bwd_data': 'igemm64/s/c4/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy1'}, []),
    ('bwd64_v4_c1_reduce_scalar', (1, 6, 5, 3, 0, 24, 3, 1), (), {'fwd': 'igemm64/s/c1/lane', 'bwd_data': 'igemm64/v4/c1/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('fwd128_v4_c1_lane', (1, 6, 5, 4, 0, 66, 3, 1), (), {'fwd': 'igemm128/v4/c1/lane', 'bwd_data': 'igemm64/s/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy1'}, []),
    ('bwd128_s_c1_lane', (1, 6, 5, 68, 5, 6, 3, 1), (), {'fwd': 'igemm64/s/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c1/lane', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd64_v4_c4_reduce_v4', (1, 6, 5, 4, 0, 72, 4, 2), (), {'fwd': 'igemm128/v4/c1/reduce_v4', 'bwd_data': 'igemm64/v4/c4/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('bwd128_v4_c1_coal', (1, 6, 5, 68, 0, 8, 3, 1), (), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c1/coal', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('bwd128_v4_c1_lane', (1, 6, 5, 68, 5, 8, 3, 1), (), {'fwd': 'igemm64/s/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c1/lane', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd128_s_c4_lane', (1, 6, 5, 68, 5, 6, 4, 2), (), {'fwd': 'igemm64/s/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c4/lane', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd128_v4_c4_coal', (1, 6, 5, 132, 0, 4, 4, 2), (), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c4/coal', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('bwd128_v4_c1_reduce_v4', (1, 6, 5, 68, 0, 24, 3, 1), (), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy4'}, []),
    ('bwd128_s_c1_reduce_v4', (1, 6, 5, 68, 0, 24, 3, 1), ('dy',), {'fwd': 'igemm64/v4/c1/reduce_v4', 'bwd_data': 'igemm128/s/c1/reduce_v4', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd128_v4_c1_reduce_scalar', (1, 6, 5, 68, 5, 24, 3, 1), (), {'fwd': 'igemm64/s/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c1/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd128_s_c1_reduce_scalar', (1, 6, 5, 68, 5, 24, 3, 1), ('dy',), {'fwd': 'igemm64/s/c1/reduce_v4', 'bwd_data': 'igemm128/s/c1/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd128_s_c4_reduce_v4', (1, 6, 5, 68, 0, 66, 4, 2), (), {'fwd': 'igemm128/v4/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c4/reduce_v4', 'bwd_weight': 'wgrad_tr/v4/dy1'}, []),
    ('bwd128_s_c4_reduce_scalar', (1, 6, 5, 68, 5, 66, 4, 2), (), {'fwd': 'igemm128/s/c1/reduce_scalar', 'bwd_data': 'igemm128/s/c4/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
    ('bwd128_v4_c4_reduce_scalar', (1, 6, 5, 68, 5, 72, 4, 2), (), {'fwd': 'igemm128/s/c1/reduce_v4', 'bwd_data': 'igemm128/v4/c4/reduce_scalar', 'bwd_weight': 'wgrad_tr/s/dy1'}, []),
]


def by_name(name):
    return [c for c in CASES if c[0] == name][0]
