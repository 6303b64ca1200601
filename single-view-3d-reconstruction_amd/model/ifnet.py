"""IF-Net on MI355X: host-side mirror of the reference's model/ifnet.py.

Same public surface as the reference (model/ifnet.py:10-61,64-199,202-229): ``IFNet(hidden_dim)``
with ``forward(x (B,1,D,H,W), points (B,N,3)) -> logits (B,N)``, submodule / parameter names of
SURVEY.md App. A.1 (so Lightning checkpoints `ifnet.*` load), feature extractors
``IFNetFeatureExtractor128`` / ``IFNetFeatureExtractor`` and the inference helpers
``make_3d_grid`` / ``evaluate_network_on_grid`` / ``implicit_to_mesh``.  The one deliberate difference: the architecture
is a constructor argument (``net_res=128``) instead of a value parsed from sys.argv at import
(model/ifnet.py:8).

Every arithmetic step runs in the HIP kernels of libsvr_hip.so (include/svr_hip.h).  The
nn.Conv3d / nn.BatchNorm3d / nn.Conv1d submodules only HOLD the parameters and buffers; their
torch forward is never called.  There is no CPU fallback.
"""
import contextlib
import copy
import os

import torch
import torch.nn as nn

from .. import ops
from ..arena import StepArena

_ARCH = {
    # stages: ((conv attr names), bn attr name); channels per stage; gather displacement; align_corners
    128: dict(stages=[(("conv_in",), "conv_in_bn"), (("conv_0", "conv_0_1"), "conv0_1_bn"),
                      (("conv_1", "conv_1_1"), "conv1_1_bn"), (("conv_2", "conv_2_1"), "conv2_1_bn"),
                      (("conv_3", "conv_3_1"), "conv3_1_bn")],
              disp=0.0722, align_corners=False),
    32: dict(stages=[(("conv_1", "conv_1_1"), "conv1_1_bn"), (("conv_2", "conv_2_1"), "conv2_1_bn"),
                     (("conv_3", "conv_3_1"), "conv3_1_bn")],
             disp=0.035, align_corners=True),
}


def _displacements(d):
    rows = [[0.0, 0.0, 0.0]]
    for axis in range(3):
        for sign in (-1, 1):
            r = [0.0, 0.0, 0.0]
            r[axis] = sign * d
            rows.append(r)
    return torch.tensor(rows)


_side_streams = {}


def _get_side_stream(device, which=0):
    """Side stream `which` of a device (0: plans / orders in the forward and the kept-column branch of the backward;
    1: the kept columns' weight gradient)."""
    if os.environ.get("SVR_NO_SIDE_STREAM"):      # measurement switch: everything on the caller's stream
        return torch.cuda.current_stream(device)
    key = (torch.device(device).index, which)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


# Backward scatter form per level (gather.hip):
#   "auto"   (default) levels with C <= 64: atomic-free PULL form when the points are spread out (uniform-like: it is bound
#            by its longest serial walk), float atomics over the joint ITEM order when they are clustered (surface samples:
#            walks of thousands of items).  The statistic is the plan's `longest walk` of the PREVIOUS step, read without
#            synchronisation (pinned copy + event); the first step of a shape uses the item order.  C = 128: item order.
#   "pull"   force the pull form for C <= 64;  "items": item orders everywhere;  "atomic": the round-1 configuration
#            (per-displacement point orders for levels with >= ~0.15 points per voxel).
# Measured at config 3 (ms, levels 1/2/3): uniform points pull 0.56/0.38/0.57, items 1.07/0.99/0.45; points clustered on
# planes pull 1.72/1.81/3.53, items 0.65/0.56/0.49 -- longest walk 13/24/94 against 1409/1669/3282.
SCATTER_FORM = os.environ.get("SVR_SCATTER_FORM", "auto")
# Bit-reproducible training step (SVR_DETERMINISTIC=1, or set ifnet.DETERMINISTIC before the step): every scatter of the
# backward takes an atomic-free form -- pull plans for the levels with C <= 64 whatever the point distribution (level 0, the
# one-channel input grid, included when the input takes a gradient: the scene step), the two-pass form for the projected
# 128-channel levels -- and the BCE adds its block sums in block order, so no float atomic is left in the IF-Net step and two
# runs give the same bits.  The same switch covers the scene step's projection (ordered splat and blur-tap sums,
# model/projection.py) and depth head (trainer/trainer_scene_net.py): DESIGN.md section 16.  Measured on one box, configs[2], uniform points: 17.0 ms
# against 16.2 ms per step (the atomic forms win inside the backward's fork, and level 3's pull form is bound by its longest
# walk); with surface-clustered points the pull form is several times slower, so it is a mode, not
# the default.  A level that has no atomic-free form (C = 128 without the projection: the 32-architecture) raises.
DETERMINISTIC = os.environ.get("SVR_DETERMINISTIC") is not None
PULL_MAX_WALK = 64      # longest serial walk of a plan up to which the "auto" form takes the pull form
_pull_hint = {}       # (device, level, dims, C, B, N) -> {"use": last decision, "slots": [(pinned int32[2], event), ...]}


PULL_DECISION_LAG = 3   # steps between a plan's statistic and the decision that uses it


def _pull_decision(key, plan, side):
    """Use the pull form?  Decided from the plan statistic of the step PULL_DECISION_LAG steps back -- a FIXED lag, so the
    form a level takes in step s is a function of the data alone and not of how far the host happens to run ahead of the
    GPU (round 2 took "the most recent statistic that has arrived": two runs of the same workload could take different
    forms in the same step).  The statistic travels through a ring of pinned slots (queued behind the plan on the side
    stream); DataParallelTrainer keeps at most 2 steps in flight, so the slot read here has normally arrived long ago --
    if it has not (an unthrottled caller), the host waits for it.  The first steps of a shape use the item order."""
    h = _pull_hint.setdefault(key, {"use": False, "slots": [None] * (PULL_DECISION_LAG + 1), "seq": 0})
    if torch.cuda.is_current_stream_capturing():
        return h["use"]            # inside a HIP-graph capture: no event waits / pinned allocations; the decision of the
        #                            eager warm-up steps is baked into the graph
    seq, ring = h["seq"], h["slots"]
    old = ring[(seq - PULL_DECISION_LAG) % len(ring)] if seq >= PULL_DECISION_LAG else None
    if old is not None:
        old["event"].synchronize()
        h["use"] = 0 < int(old["host"][0]) <= PULL_MAX_WALK
    slot = ring[seq % len(ring)]
    if slot is None:
        slot = ring[seq % len(ring)] = {"host": torch.empty(2, dtype=torch.int32, pin_memory=True), "event": torch.cuda.Event()}
    slot["host"].copy_(plan.stats, non_blocking=True)
    slot["event"].record(side)
    h["seq"] = seq + 1
    return h["use"]


def _level_dims(D, H, W, l):
    """Resolution of pyramid level l: the input grid for levels 0 and 1, halved per stage behind them."""
    s = max(l - 1, 0)
    return (max(D >> s, 1), max(H >> s, 1), max(W >> s, 1))


def _level_orders_async(pts, D, H, W, n_levels, align, layout=None, disp=None, proj_levels=(), arena=None, need_level0=False):
    """Backward-scatter preparation that depends only on the points, computed on a side stream beside the encoder;
    returns (orders per level, pull plans per level, ready event).  Level l has the pyramid's resolution
    (D, H, W) >> (l - 1) for l >= 1 (level 0 is the input grid, one channel: neither).  See SCATTER_FORM.
    layout: the layout of the gradient rows the scatter will read (the full FeatureLayout, or the KeptLayout of the fused
    step).  arena: the step's StepArena -- the plans' arrays then live there (no allocator traffic on the side stream).
    need_level0: the input grid takes a gradient (the scene step: it is the projected voxel occupancy) -- under
    DETERMINISTIC level 0 (one channel) then gets a pull plan too; otherwise it keeps its float-atomic scatter."""
    B, N = pts.shape[0], pts.shape[1]
    orders = [None] * n_levels
    plans = [None] * n_levels
    main = torch.cuda.current_stream()
    side = _get_side_stream(pts.device)
    side.wait_stream(main)          # pts may have just been produced on the main stream
    if arena is None or not arena.owns(pts):
        # ... and must not return to the main stream's pool while the side stream reads it.  (Skipped only for points that
        # LIVE in the arena -- the Morton-sorted copy; with spatial_sort off or N == 1 pts is the caller's tensor even
        # under a lease, and a graph dropped without a backward would hand its block out again on main.)
        pts.record_stream(side)
    launched = False
    form = "pull" if DETERMINISTIC else SCATTER_FORM
    fits32 = layout is not None and N > 0 and 7 * B * N < 2 ** 31 and B * N * layout.row_stride < 2 ** 31
    with torch.cuda.stream(side):
        if DETERMINISTIC and need_level0 and N > 0:
            dhw = (D, H, W)
            if not (fits32 and layout.channels[0] == 1 and B * (D + 1) * (H + 1) * (W + 1) < 2 ** 31 - 1):
                raise RuntimeError(f"IF-Net HIP path, DETERMINISTIC: the input grid's gradient (level 0, {dhw}, batch {B}, {N} points) "
                                   "exceeds the pull plan's 32-bit cell / item / gradient offsets and has no other atomic-free scatter")
            plans[0] = ops.pull_plan(pts, dhw, 1, layout.col[0], layout.row_stride, disp, align, arena=arena, tag="L0.")
            plans[0].record_stream(main)
            launched = True
        for l in range(1, n_levels):
            dhw = _level_dims(D, H, W, l)
            C = layout.channels[l] if layout is not None else 0
            tag = f"L{l}."
            if l in proj_levels:                     # backward-only projection: items by (cell, displacement)
                if DETERMINISTIC:
                    orders[l] = ops.project_plan(pts, dhw, disp, align)      # two-pass form: no float atomics
                    orders[l].record_stream(main)
                else:
                    # atomic form: x-block order, so that x-neighbour runs hand their shared face over in registers
                    orders[l] = ops.item_order(pts, dhw, disp, align, arena=arena, tag=tag, x_block=ops.proj_x_block(N, dhw))
                    if arena is None:
                        orders[l].record_stream(main)
                launched = True
            elif form in ("auto", "pull") and fits32 and ops.pull_plan_supported(B, N, dhw, C, layout.row_stride):
                plan = ops.pull_plan(pts, dhw, C, layout.col[l], layout.row_stride, disp, align, arena=arena, tag=tag)
                plan.record_stream(main)
                if form == "pull" or _pull_decision((pts.device.index, l, dhw, C, B, N), plan, side):
                    plans[l] = plan
                else:
                    orders[l] = plan.items            # the plan's sorted item ids are this level's item order
                launched = True
            elif DETERMINISTIC and N > 0:
                raise RuntimeError(f"IF-Net HIP path, DETERMINISTIC: level {l} ({C} channels, {dhw}) has no atomic-free scatter "
                                   "(pull plans cover 16 / 32 / 64 channels, the projection the 128-channel levels of the "
                                   "128-architecture)")
            elif form in ("auto", "pull", "items") and fits32:
                orders[l] = ops.item_order(pts, dhw, disp, align, arena=arena, tag=tag)
                if arena is None:
                    orders[l].record_stream(main)
                launched = True
            elif N >= 0.15 * dhw[0] * dhw[1] * dhw[2] and N > 64:
                orders[l] = ops.voxel_order(pts, dhw, align)
                orders[l].record_stream(main)
                launched = True
        ready = None
        if launched:
            ready = torch.cuda.Event()
            ready.record(side)
    return orders, plans, ready


# Backward-only projection of the 128-channel levels (gather.hip, gather_bwd_proj_kernel): their 2 x 896 feature columns
# are 69 % of fc_0's K, and the scatter commutes with fc_0's product -- dh0 rows (256 wide) are scattered into
# dP_l[b][voxel][j][256], and two GEMMs over VOXELS (32 768 rows at level 4) give the level's gradient volume and its slice
# of dW0.  dX0 / dW0 of the point MLP then only cover the remaining 800 columns.  The forward pass is unchanged.
PROJECT_WIDE_LEVELS = os.environ.get("SVR_NO_PROJECTION") is None
# Fused gather -> fc_0 forward (gather_fc0.hip): the feature rows are never written to HBM; only the columns a backward
# still needs (the levels that are not projected) are kept.  SVR_NO_FUSED_FC0=1 restores the two separate kernels.
FUSE_FC0 = os.environ.get("SVR_NO_FUSED_FC0") is None
# ... and its bf16-storage variant for the query path's throughput mode (SVR_NO_FUSED_FC0_BF16=1: gather + fc_0 as two kernels)
FUSE_FC0_BF16 = os.environ.get("SVR_NO_FUSED_FC0_BF16") is None
# Fused + projected backward: the kept-column branch on the side stream beside the projected branch (SVR_NO_BWD_OVERLAP=1: serial)
OVERLAP_BACKWARD = os.environ.get("SVR_NO_BWD_OVERLAP") is None
# First stage of the 128-architecture (conv_in -> ReLU -> BatchNorm -> pool) with conv_in's activation recomputed instead
# of stored (stage1.hip): 3 of 5 forward and 5 of 7 backward passes over 1 GB tensors less.  SVR_NO_STAGE1=1: the separate
# conv / BatchNorm / weight-gradient kernels.
STAGE1_RECOMPUTE = os.environ.get("SVR_NO_STAGE1") is None
# Training step: the Morton sort of the points runs on the side stream beside the encoder (SVR_SORT_ON_MAIN=1: in front of it)
SORT_ON_SIDE_STREAM = os.environ.get("SVR_SORT_ON_MAIN") is None
# ... and so do the parameter-only preparations of the split-precision layers (SVR_NO_WEIGHT_PREP=1: in front of every layer)
PREPARE_WEIGHTS_AHEAD = os.environ.get("SVR_NO_WEIGHT_PREP") is None
# Level of the kept branch whose scatter runs on the third stream of the backward's fork
FORK_SPLIT_LEVEL = 3
# Per-level events instead of one join in front of the encoder's backward (SVR_NO_FORK_PIPELINE=1: the single join)
FORK_PIPELINED = os.environ.get("SVR_NO_FORK_PIPELINE") is None
# BatchNorm statistics of stages 2..5 from the epilogue of the stage's last convolution (SVR_NO_CONV_STATS=1: a separate pass)
STATS_IN_CONV_EPILOGUE = os.environ.get("SVR_NO_CONV_STATS") is None
# The step's large cross-stream buffers live in a per-module StepArena (arena.py); SVR_NO_ARENA=1: ordinary allocations
USE_ARENA = os.environ.get("SVR_NO_ARENA") is None


def _fc0_fusable(channels, B, dims, n_out):
    """Shapes gather_fc0.hip is built for (svr_gather_fc0_supported): 256 outputs, channel counts 1 (once), 16, 32 or
    multiples of 64, every level's volume below 2^30 elements (32-bit byte offsets)."""
    if n_out != 256 or sum(1 for c in channels if c == 1) > 1:
        return False
    D, H, W = dims
    for l, c in enumerate(channels):
        if not (c in (1, 16, 32) or c % 64 == 0):
            return False
        d, h, w = _level_dims(D, H, W, l)
        if B * d * h * w * c >= 2 ** 30:
            return False
    return True


def _stage1_applies(si, convs, inp):
    """First stage, one convolution from one input channel to 16 (the 128-architecture's conv_in), shapes stage1.hip covers."""
    return (STAGE1_RECOMPUTE and si == 0 and len(convs) == 1 and inp.is_cuda and tuple(convs[0].weight.shape[:2]) == (16, 1)
            and min(inp.shape[1:4]) >= 1 and ops.stage1_supported(inp, 16))


class _ProjLink:
    """Hand-over between the point MLP's backward (which runs first and produces dh0) and the encoder's."""

    def __init__(self, levels, layout):
        self.levels = tuple(levels)
        self.dh0 = None
        self.need_level0 = False
        cols = sorted((layout.col[l], layout.col[l] + 7 * layout.channels[l]) for l in levels)
        keep, start = [], 0
        for a, b in cols:                              # complement of the projected column ranges inside the row
            if a > start:
                keep.append((start, a))
            start = b
        if start < layout.row_stride:
            keep.append((start, layout.row_stride))
        # the raw-grid level (C == 1) gets a segment of its own, so that "its gradient is only needed for d(loss)/d(input)"
        # can never drop the columns of another kept level that happens to share a segment with it
        raw = [(layout.col[l], layout.col[l] + 7) for l, c in enumerate(layout.channels) if c == 1 and l not in levels]
        split = []
        for a, b in keep:
            cuts = sorted({a, b} | {c for r in raw for c in r if a < c < b})
            split += list(zip(cuts[:-1], cuts[1:]))
        self.keep = split                               # column segments dX0 / dW0 still have to cover
        self.raw = set(raw)                             # ... those of them that hold nothing but the raw-grid level


def _run_stages(ext, inp, training, for_backward):
    """The encoder's conv / ReLU / BatchNorm / pool stages over `inp` (B,D,H,W,1): (levels [inp, bn_1, ...], saved).
    for_backward (the autograd forward; encode_levels passes False): `saved` holds what _stages_bwd reads per stage, (inp,
    acts | ("stage1", wp), argmax, ss, mean), and in training mode the BatchNorm's statistics come out of the epilogue of
    the convolution in front of it; otherwise nothing is kept and the plain convolution kernels run."""
    levels, saved = [inp], []
    nst = len(ext._stages)
    for si, (convs, bn) in enumerate(ext._stages):
        bn_args = (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, training)
        bn_kw = dict(eps=bn.eps, momentum=bn.momentum, want_pool=(si + 1 < nst))
        if _stage1_applies(si, convs, inp):
            conv = convs[0]
            y, pooled, argmax, ss, mean, wp = ops.stage1_fwd(inp, conv.weight.detach(), conv.bias.detach(), *bn_args, **bn_kw)
            acts = ("stage1", wp)      # conv_in's activation is never stored
        else:
            acts = []
            cur = inp
            stats = None
            for conv in convs:
                w, b = conv.weight.detach(), conv.bias.detach()
                if for_backward and training and len(convs) == 1 and w.shape[1] == 1 and w.shape[0] in (16, 32):
                    # conv_in: the statistics of the BatchNorm that follows come out of the conv kernel's epilogue
                    cur, stats = ops.conv3d_c1_fwd_stats(cur, w, b, relu=True)
                elif for_backward and training and conv is convs[-1] and STATS_IN_CONV_EPILOGUE:
                    # the stage's last convolution: its epilogue also leaves the BatchNorm's partial sums (no statistics pass)
                    cur, stats = ops.conv3d_k3_fwd(cur, w, b, relu=True, want_stats=True)
                else:
                    cur = ops.conv3d_k3_fwd(cur, w, b, relu=True)
                if for_backward:
                    acts.append(cur)
            y, pooled, argmax, ss, mean = ops.bn_forward(cur, *bn_args, **bn_kw, stats=stats)
        levels.append(y)
        if for_backward:
            saved.append((inp, acts, argmax, ss, mean))
        inp = pooled
    return levels, saved


def _gvols(arena, levels, plans, proj):
    """Gradient volumes of the backward scatter for levels 1.. (None for level 0 and for the projected levels, whose
    volumes come out of a GEMM), from the step arena when there is one; zeroed unless a pull plan writes them by plain stores."""
    def one(l, like):
        if arena is None:
            return torch.zeros_like(like) if plans[l] is None else torch.empty_like(like)
        g = arena.get(f"gvol{l}", tuple(like.shape), like.dtype, like.device)
        return g.zero_() if plans[l] is None else g
    return [None] + [None if l in proj else one(l, v) for l, v in enumerate(levels) if l >= 1]


def _zero_fill_async(levels, orders, plans, proj, arena):
    """The zero-initialised gradient volumes of the backward scatter (1.45 GB of memset at config 3) and the zeroed
    (voxel, displacement, 256) slabs the projected levels' atomic scatter accumulates into, prepared on the side stream
    beside the point MLP instead of in front of the scatter.  Returns (gvols, dP slabs per level, ready event)."""
    x = levels[0]
    main, side = torch.cuda.current_stream(), _get_side_stream(x.device)
    with torch.cuda.stream(side):
        gvols = _gvols(arena, levels, plans, proj)
        dP = {}
        if arena is not None:
            for l in proj:
                if not isinstance(orders[l], ops.ProjPlan):      # (the two-pass form overwrites its own)
                    v = levels[l]
                    dP[l] = arena.get(f"dP{l}", (x.shape[0], v.shape[1] * v.shape[2] * v.shape[3], 7, 256), torch.float32,
                                      x.device).zero_()
        else:
            for g in gvols[1:]:
                if g is not None:
                    g.record_stream(main)
        ready = torch.cuda.Event()
        ready.record(side)
    return gvols, dP, ready


class _Fork:
    """Streams and events of the encoder backward's fork (fused forward + projection).  The kept columns' backward (dX0
    over 800 columns, then the scatter of levels 1-3) and the projected levels' (row scatter + voxel GEMMs) only share dh0
    and neither saturates the chip: the kept branch runs on the side stream `keep` beside the projected one on `main`, the
    leaf dW0 of the kept columns on the third stream `w`.
    split: the kept branch's last level (FORK_SPLIT_LEVEL) is scattered on `w`, behind dW0, as soon as dX0 is there (arena only).
    pipelined (FORK_PIPELINED): no join in front of the stages' backward -- every level's gradient volume gets an event and
    stage s only waits for level s + 1, so the deep stages (1.3 ms of small kernels) run while the fine levels are still
    scattered, one call per level, coarse to fine; the coarsest projected level gets a stream of its own, `p`.
    Not forking (`on` false; a captured step keeps the serial order): every stream is the caller's, nothing is waited for."""

    def __init__(self, on, main, device, arena, need_pts, skip, proj, n_levels):
        self.on = on
        self.main = main
        self.keep = _get_side_stream(device) if on else main
        self.w = _get_side_stream(device, 1) if on else main
        self.p = None
        s = FORK_SPLIT_LEVEL
        self.split = s if (on and arena is not None and not need_pts and s not in skip and s not in proj
                           and 0 < s < n_levels) else None
        self.pipelined = FORK_PIPELINED and self.split is not None
        self.dx0_done = self.keep_done = None
        self.level_done = {}

    def stream(self, s):      # context: run on stream s, or inline when not forking
        return torch.cuda.stream(s) if self.on else contextlib.nullcontext()

    def start(self, *held):
        """The side streams branch off main.  No record_stream on what they read: dh0, the kept rows, the gradient volumes
        ... and `held` stay referenced until backward() returns, behind join() -- or live in the step arena."""
        self.held = held
        if self.on:
            self.keep.wait_stream(self.main)
            self.w.wait_stream(self.main)

    def mark_level(self, l):
        self.level_done[l] = torch.cuda.current_stream().record_event()

    def wait_level(self, l):      # pipelined: main waits for level l's gradient volume, from whichever stream scattered it
        if self.pipelined and l in self.level_done:
            self.main.wait_event(self.level_done[l])

    def join(self):      # main waits for the leaves of the side streams (dW0's slices, db0) and everything that reads the arena
        self.main.wait_event(self.keep_done)
        self.main.wait_stream(self.w)
        if self.p is not None:
            self.main.wait_stream(self.p)


def _scatter_state(orders, plans, ready, gvols, ext, levels, pts, layout, proj, arena, need_x):
    """What the forward prepared for the scatter, or the same built now: (orders, plans, ready event, gradient volumes)."""
    if orders is None:
        orders, plans, ready = _level_orders_async(pts, *levels[0].shape[1:4], len(levels), ext._align, layout, ext._disp,
                                                   proj_levels=proj, arena=arena, need_level0=need_x)
    if ops.GATHER_FLAGS & ops._lib.GATHER_DETERMINISTIC:      # the serial test scatter accumulates into zeros
        plans = [None] * len(levels)
        gvols = None
    # the raw grid's: only for d(loss)/d(input); a level-0 pull plan (DETERMINISTIC) writes every voxel of it
    g0 = (torch.empty_like(levels[0]) if plans[0] is not None else torch.zeros_like(levels[0])) if need_x else None
    if gvols is None:
        gvols = _gvols(arena, levels, plans, proj)
    return orders, plans, ready, [g0] + gvols[1:]


def _fc0_kept_bwd(fork, dh0, feat, w0p, klay, arena):
    """Fused forward: fc_0's backward lives in the encoder's.  dh0 is dz0 (B*N, 256); dW0 / dX0 only over the kept
    columns, ONE product each over the compact kept-column matrix `feat`: (dW0, db0, the compact gradient rows)."""
    cols = klay.full_cols_on(w0p.device)
    w0k = w0p[:, cols]                           # (256, 800): fc_0's weights of the kept columns (zeros behind the padding)
    dw0_keep = torch.zeros_like(w0p)
    fork.start(w0k)
    with fork.stream(fork.w):
        dwk, db0 = ops.linear_bwd_weight(dh0, feat, want_bias=True)
        dw0_keep[:, cols[:klay.width]] = dwk[:, :klay.width]
        if fork.on:
            db0.record_stream(fork.main)
    with fork.stream(fork.keep):
        gfeat = arena.get("kept_grad", tuple(feat.shape), torch.float32, feat.device) if arena is not None else torch.empty_like(feat)
        ops.linear_bwd_data(dh0, w0k, out=gfeat)
        if fork.on:
            fork.dx0_done = torch.cuda.Event()
            fork.dx0_done.record(fork.keep)
    return dw0_keep, db0, gfeat


def _scatter_kept(fork, ext, levels, gvols, pts, gfeat, layout, orders, plans, ready, skip, proj, need_pts):
    """Scatter of the gradient rows into the volumes of the levels that are not projected: one call on the `keep` stream,
    or -- pipelined -- one call and one event per level, the split level on the `w` stream.  Returns d(loss)/d(points)."""
    n = len(levels)
    lo = [None if l in proj else o for l, o in enumerate(orders)]

    def scatter(want_gpoints, skip_levels):
        return ops.gather_bwd(levels, gvols, pts, gfeat, layout, ext._disp, ext._align, want_gpoints=want_gpoints,
                              level_orders=lo, level_plans=plans, skip_levels=skip_levels)

    def scatter_level(l):
        scatter(False, tuple(k for k in range(n) if k != l))
        fork.mark_level(l)

    gpts = None
    with fork.stream(fork.keep):
        if ready is not None:
            torch.cuda.current_stream().wait_event(ready)
        if fork.pipelined:
            for l in range(n - 1, -1, -1):      # (level 0, the raw grid, only when d(loss)/d(input) is wanted)
                if l != fork.split and l not in skip and l not in proj and gvols[l] is not None:
                    scatter_level(l)
        else:
            gpts = scatter(need_pts, skip if fork.split is None else tuple(skip) + (fork.split,))
        if fork.on:
            fork.keep_done = torch.cuda.Event()
            fork.keep_done.record(fork.keep)
    if fork.split is not None:
        with torch.cuda.stream(fork.w):
            fork.w.wait_event(fork.dx0_done)
            if ready is not None:
                fork.w.wait_event(ready)
            scatter_level(fork.split)
    return gpts


def _project_wide(fork, ext, levels, gvols, pts, dh0, w0p, orders, ready, proj, dPs, dw0p):
    """dP = scatter of the dh0 rows, then two GEMMs over voxels (gather_bwd_proj_kernel): gvols[l] and its slice of dW0."""
    if fork.on and ready is not None:
        fork.main.wait_event(ready)
    if dw0p is None:
        dw0p = torch.zeros_like(w0p)

    def project_level(l):
        v = levels[l]
        B_, Dl, Hl, Wl, Cl = v.shape
        c0 = ext._layout.col[l]
        dP = ops.gather_project_bwd(pts, dh0, (Dl, Hl, Wl), orders[l], ext._disp, ext._align, out=dPs.get(l))
        dP2 = dP.view(B_ * Dl * Hl * Wl, 7 * 256)
        wl = w0p[:, c0:c0 + 7 * Cl].reshape(256, 7, Cl).permute(1, 0, 2).reshape(7 * 256, Cl).contiguous()   # rows (j, n)
        gvols[l] = ops.linear_bwd_data(dP2, wl).view(v.shape)
        dwl, _ = ops.linear_bwd_weight(dP2, v.view(-1, Cl), want_bias=False)                                # (7*256, Cl)
        dw0p[:, c0:c0 + 7 * Cl] = dwl.view(7, 256, Cl).permute(1, 0, 2).reshape(256, 7 * Cl)

    own = max(proj) if (fork.pipelined and len(proj) > 1) else None     # the coarsest projected level: its own stream
    if own is not None:
        fork.p = _get_side_stream(pts.device, 2)
        fork.p.wait_stream(fork.main)
        with torch.cuda.stream(fork.p):
            if ready is not None:
                fork.p.wait_event(ready)
            project_level(own)
            gvols[own].record_stream(fork.main)       # allocated in this stream's pool, read by the stage's backward on main
            fork.mark_level(own)
    for l in proj:
        if l != own:
            project_level(l)
    return dw0p


def _stages_bwd(fork, ext, saved, gvols, training, need_x):
    """Backward of the encoder stages, last to first (BN -> ReLU -> conv per stage), from the levels' gradient volumes:
    ({parameter: gradient}, d(loss)/d(input grid) without the raw-grid level's share, or None)."""
    grads, dpooled, gx = {}, None, None
    for si in range(len(ext._stages) - 1, -1, -1):
        convs, bn = ext._stages[si]
        inp, acts, argmax, ss, mean = saved[si]
        fork.wait_level(si + 1)
        if isinstance(acts, tuple):       # ("stage1", wp): BatchNorm backward + conv_in's weight gradient in two passes
            conv = convs[0]
            grads[bn.weight], grads[bn.bias], grads[conv.weight], grads[conv.bias], dout = ops.stage1_bwd(
                inp, acts[1], conv.bias.detach(), gvols[si + 1], dpooled, argmax if dpooled is not None else None, mean, ss,
                relu_mask=True, training=training, want_dout=need_x)
            if need_x:
                gx = ops.conv3d_k3_bwd_data(dout, conv.weight.detach())
            continue
        dout, grads[bn.weight], grads[bn.bias] = ops.bn_backward(
            acts[-1], gvols[si + 1], dpooled, argmax if dpooled is not None else None, mean, ss, relu_mask=True, training=training)
        for k in range(len(convs) - 1, -1, -1):
            conv = convs[k]
            cin = acts[k - 1] if k > 0 else inp
            grads[conv.weight], grads[conv.bias] = ops.conv3d_k3_bwd_weight(cin, dout, param_layout=True)
            if k > 0:
                dout = ops.conv3d_k3_bwd_data(dout, conv.weight.detach(), mask=acts[k - 1])
            elif si > 0:
                dpooled = ops.conv3d_k3_bwd_data(dout, conv.weight.detach())
            elif need_x:
                gx = ops.conv3d_k3_bwd_data(dout, conv.weight.detach())
    return grads, gx


class _EncoderGatherFn(torch.autograd.Function):
    """x, points, encoder parameters -> feature rows (B*N, FS) in the internal column layout.

    forward  = reference model/ifnet.py:155-198 (conv/ReLU/BN/pool pyramid + 6 grid_samples + cat)
    backward = autograd of the same, hand-scheduled (gather scatter -> BN -> ReLU -> conv per stage).
    """

    @staticmethod
    def forward(ctx, ext, grad_mode, link, lease, w0p, b0, x, points, *params):
        """b0 given (with link and w0p): FUSED form -- the output is h0 = relu(fc_0(rows)) straight from the gather
        (gather_fc0.hip), the rows of the levels that are not projected are kept for the backward, and backward()
        takes the gradient wrt fc_0's PRE-activation (what _PointMLPFn's headless form returns for its input)."""
        B, _, D, H, W = x.shape
        training = ext.training
        x_cl = x.contiguous().view(B, D, H, W, 1)
        pts = points.contiguous()
        nlev = len(ext._stages) + 1
        # only when a backward can follow: grad mode of the CALLER (it is always off inside Function.forward, and
        # needs_input_grad ignores no_grad) and something that requires grad
        will_backward = bool(grad_mode) and any(ctx.needs_input_grad)
        ctx.link = link if (will_backward and link is not None) else None
        if ctx.link is not None:
            ctx.link.need_level0 = bool(ctx.needs_input_grad[6])
        proj = ctx.link.levels if ctx.link is not None else ()
        # the step arena (large cross-stream buffers, allocated once): held from here to the end of backward()
        if lease is not None and not (will_backward and x.is_cuda):
            lease.release()
            lease = None
        ctx.lease = lease
        arena = lease.arena if lease is not None else None
        ctx.fused = b0 is not None
        keep = [l for l in range(nlev) if l not in proj] if (ctx.fused and will_backward) else []
        # fused step: the backward reads the COMPACT kept-column matrix (800 columns at the 128-architecture)
        ctx.klay = ext._layout.subset(keep) if keep else None
        # The per-level visiting orders of the backward scatter depend only on the points: their radix sorts (dozens
        # of ~6 us launches) run on a side stream beside the encoder instead of in front of the scatter.
        ctx.level_orders, ctx.level_plans, ctx.orders_ready = None, None, None
        if will_backward and x.is_cuda:
            ctx.level_orders, ctx.level_plans, ctx.orders_ready = _level_orders_async(
                pts, D, H, W, nlev, ext._align, ctx.klay if ctx.klay is not None else ext._layout, ext._disp,
                proj_levels=proj, arena=arena, need_level0=bool(ctx.needs_input_grad[6]))
        levels, saved = _run_stages(ext, x_cl, training, for_backward=True)
        if training:      # one multi-tensor launch for the counters of all stages
            torch._foreach_add_([bn.num_batches_tracked for _, bn in ext._stages], 1)
        ready, ext._points_ready = getattr(ext, "_points_ready", None), None
        if ready is not None:
            torch.cuda.current_stream().wait_event(ready)      # the sorted points (IFNet.forward sorts them on the side stream)
        if ctx.fused:
            rows_out = None
            if keep and arena is not None:
                rows_out = arena.get("kept_rows", (B * pts.shape[1], ctx.klay.row_stride), torch.float32, x.device)
            out, feat = ops.gather_fc0_fwd(levels, pts, ext._layout, ext._disp, ext._align, w0p.detach(), b0.detach(), relu=True,
                                           keep_levels=keep, keep_layout=ctx.klay, rows_out=rows_out, arena=arena)
            ctx.feat = feat
        else:
            out = feat = ops.gather_fwd(levels, pts, ext._layout, ext._disp, ext._align)
        ctx.gvols, ctx.dP = None, {}
        if will_backward and x.is_cuda:
            ctx.gvols, ctx.dP, ctx.orders_ready = _zero_fill_async(levels, ctx.level_orders, ctx.level_plans, proj, arena)
        ctx.ext, ctx.saved, ctx.levels, ctx.pts = ext, saved, levels, pts
        ctx.w0p = w0p.detach() if (ctx.link is not None or ctx.fused) else None
        ctx.x_shape, ctx.training = x.shape, training
        return out

    @staticmethod
    def backward(ctx, gfeat):
        if ctx.saved is None:
            raise RuntimeError("IF-Net HIP path: second backward through the same forward pass (the saved pyramid and "
                               "activations are released by the first one; retain_graph is not supported)")
        ext, saved, levels, pts = ctx.ext, ctx.saved, ctx.levels, ctx.pts
        # plain attributes are not freed with the graph's saved tensors: a caller that keeps the loss tensor (and with it
        # this node) alive into the next step would otherwise hold ~9 GB of activations twice
        ctx.saved = ctx.levels = ctx.pts = None
        need_x, need_pts = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        gfeat = gfeat.contiguous()
        link = ctx.link
        proj = link.levels if link is not None else ()
        lease, ctx.lease = ctx.lease, None
        arena = lease.arena if lease is not None else None
        klay = ctx.klay if ctx.fused else None
        scatter_layout = klay if klay is not None else ext._layout
        skip = tuple(l for l in range(len(levels)) if klay.col[l] < 0) if ctx.fused else ()
        dPs, ctx.dP = ctx.dP, None
        gvols, ctx.gvols = ctx.gvols, None
        orders, plans, ready, gvols = _scatter_state(ctx.level_orders, ctx.level_plans, ctx.orders_ready, gvols, ext, levels,
                                                     pts, scatter_layout, proj, arena, need_x)
        main = torch.cuda.current_stream() if gfeat.is_cuda else None
        fork = _Fork(ctx.fused and link is not None and main is not None and OVERLAP_BACKWARD
                     and not torch.cuda.is_current_stream_capturing(),
                     main, gfeat.device, arena, need_pts, skip, proj, len(levels))
        dw0 = db0 = None
        if ctx.fused:
            dh0, feat, ctx.feat = gfeat, ctx.feat, None
            dw0, db0, gfeat = _fc0_kept_bwd(fork, dh0, feat, ctx.w0p, klay, arena)
            if link is not None:
                link.dh0 = dh0
        if link is not None and link.dh0 is None:
            raise RuntimeError("IF-Net HIP path: the projected backward needs dh0 from the point MLP's backward")
        gpts = _scatter_kept(fork, ext, levels, gvols, pts, gfeat, scatter_layout, orders, plans, ready, skip, proj, need_pts)
        if proj:
            dh0, link.dh0 = link.dh0, None
            dw0 = _project_wide(fork, ext, levels, gvols, pts, dh0, ctx.w0p, orders, ready, proj, dPs, dw0)
        if fork.on and not fork.pipelined:
            fork.join()
            feat = None      # (only now: see _Fork.start)
        grads, gx = _stages_bwd(fork, ext, saved, gvols, ctx.training, need_x)
        if need_x:
            fork.wait_level(0)
            gx = (gx + gvols[0]).view(ctx.x_shape)
        if fork.pipelined:
            fork.join()
        if lease is not None:
            lease.release()     # every kernel that touches the arena is enqueued; the next step orders itself behind them
            #                     (also expires the prepared weight planes: the optimizer is about to change the parameters)
        return (None, None, None, None, dw0, db0, gx, gpts) + tuple(grads.get(p) for p in ext._param_list)


class _PointMLPFn(torch.autograd.Function):
    """feature rows (B*N, FS) -> logits (B*N): fc_0, fc_1, fc_2 with ReLU, fc_out
    (reference model/ifnet.py:55-59) on the f32 matrix cores."""

    @staticmethod
    def forward(ctx, feat, row_map, w0p, b0, w1, b1, w2, b2, wo, bo, link=None):
        """row_map (int32, or None): feature row m belongs to caller point row_map[m]; the logits are
        scattered back to the caller's order by the fc_out kernel.
        w0p None: HEADLESS form -- `feat` is already h0 = relu(fc_0(rows)) (the fused gather produced it) and the
        gradient returned for it is the one wrt fc_0's pre-activation (h0's ReLU mask applied), the contract of
        _EncoderGatherFn's fused backward."""
        ctx.headless = w0p is None
        h0 = feat if ctx.headless else ops.linear_fwd(feat, w0p, b0, relu=True)
        h1, h2, logits = ops.mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, row_map)      # one kernel where it applies, else the three ops
        ctx.save_for_backward(*(() if ctx.headless else (feat, w0p)), w1, w2, wo, h0, h1, h2)
        ctx.row_map = row_map
        ctx.link = link
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        *head, w1, w2, wo, h0, h1, h2 = ctx.saved_tensors
        dh2, dwo, dbo = ops.fc_out_bwd(h2, wo, dlogits.contiguous(), ctx.row_map)   # dh2 already masked by h2 > 0
        dw2, db2 = ops.linear_bwd_weight(dh2, h1)
        dh1 = ops.linear_bwd_data(dh2, w2, mask=h1)
        dw1, db1 = ops.linear_bwd_weight(dh1, h0)
        dh0 = ops.linear_bwd_data(dh1, w1, mask=h0)      # wrt fc_0's pre-activation: what the headless form returns
        tail = (dw1, db1, dw2, db2, dwo, dbo, None)
        if ctx.headless:
            return (dh0, None, None, None) + tail
        (feat, w0p), link = head, ctx.link
        if link is None:
            dw0, db0 = ops.linear_bwd_weight(dh0, feat)
            dfeat = ops.linear_bwd_data(dh0, w0p) if ctx.needs_input_grad[0] else None
            return (dfeat, None, dw0, db0) + tail
        # projected wide levels: dX0 / dW0 only over the columns that stay (K 2592 -> 800); the encoder's backward gets dh0
        link.dh0 = dh0
        dw0 = torch.zeros_like(w0p)
        dfeat = torch.empty_like(feat)            # the projected levels' columns are never read
        db0 = None
        for a, b in link.keep:
            dws, dbs = ops.linear_bwd_weight(dh0, feat[:, a:b], want_bias=db0 is None)
            dw0[:, a:b] = dws
            db0 = dbs if db0 is None else db0
            if (a, b) in link.raw and not link.need_level0:
                continue                          # raw-grid columns: their gradient is only needed for d(loss)/d(input)
            ops.linear_bwd_data(dh0, w0p[:, a:b], out=dfeat[:, a:b])
        return (dfeat, None, dw0, db0) + tail


class _PermuteColumnsFn(torch.autograd.Function):
    """w (H, F) -> w[:, src] with zeros where mask (H, FS): a column permutation with zero padding columns.  Backward is the inverse
    permutation (one index_select) -- autograd's own backward of advanced indexing is an index_put with a sort (a dozen
    launches at the end of every step)."""

    @staticmethod
    def forward(ctx, w, src, mask, inv):
        ctx.save_for_backward(inv)
        return w.index_select(1, src).masked_fill_(mask, 0.0)

    @staticmethod
    def backward(ctx, g):
        (inv,) = ctx.saved_tensors
        return g.index_select(1, inv), None, None, None


class _ExtractorBase(nn.Module):
    """Shared host logic of the two extractor variants."""

    # Per-process scratch state that is neither parameter nor buffer: the step arena (multi-GB device buffers, allocated by
    # the first training steps and kept for the module's lifetime -- release_step_buffers() frees them) and the prepared
    # weight planes (hold a torch.cuda.Event, which can be neither pickled nor deep-copied).  copy.deepcopy(model),
    # pickle / torch.save(model) get fresh, empty ones, like the reference nn.Module that has neither.
    _SCRATCH = ("_arena", "_prepared", "_points_ready")

    def __getstate__(self):
        st = dict(self.__dict__)
        for k in self._SCRATCH:
            st.pop(k, None)
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._arena = StepArena()
        self._prepared = ops.PreparedWeights()
        self._points_ready = None

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__setstate__(copy.deepcopy(self.__getstate__(), memo))
        # (_stages / _param_list hold references to submodules / parameters: copied through the same memo, so they point at
        # the copy's own conv / bn modules)
        return new

    def release_step_buffers(self):
        """Hand the step arena's device memory (4.4 GB at configs[2]) and the prepared weight planes back: call between
        training and a memory-hungry inference phase.  The next training step allocates them again (a few hipMalloc)."""
        self._arena.release()
        self._prepared = ops.PreparedWeights()

    def _finish_init(self, net_res):
        a = _ARCH[net_res]
        self._stages = [([getattr(self, c) for c in convs], getattr(self, bn)) for convs, bn in a["stages"]]
        self._disp = float(torch.tensor(a["disp"], dtype=torch.float32))
        self._align = a["align_corners"]
        self.displacments = _displacements(a["disp"])            # plain attribute, like the reference
        chans = [1] + [convs[-1].out_channels for convs, _ in self._stages]
        self._layout = ops.FeatureLayout(chans)
        self._arena = StepArena()      # the step's large cross-stream buffers, allocated once (arena.py)
        self._prepared = ops.PreparedWeights()   # split-precision weight planes of a step, prepared on the side stream
        self._param_list = []
        for convs, bn in self._stages:
            for c in convs:
                self._param_list += [c.weight, c.bias]
            self._param_list += [bn.weight, bn.bias]

    @torch.no_grad()
    def encode_levels(self, x):
        """Inference only: the sampled pyramid [x, bn_1, ...] (channels-last), computed ONCE so dense-grid
        evaluation does not redo the encoder per chunk (the reference recomputes it for every chunk,
        model/ifnet.py:220-226).  Uses the module's current mode for BatchNorm (eval -> running stats)."""
        if not x.is_cuda:
            raise RuntimeError("IF-Net HIP path needs GPU tensors (no CPU fallback)")
        B, _, D, H, W = x.shape
        return _run_stages(self, x.float().contiguous().view(B, D, H, W, 1), self.training, for_backward=False)[0]

    @torch.no_grad()
    def feature_rows_from_levels(self, levels, points, order=None):
        return ops.gather_fwd(levels, points.float().contiguous(), self._layout, self._disp, self._align, order=order)

    def feature_rows(self, x, points, link=None, w0p=None, b0=None, lease=None):
        """(B*N, FS) rows in the internal column layout (what the point MLP consumes).  link / w0p: the backward-only
        projection of the wide levels (IFNet.forward wires it; the encoder's backward then also returns its share of
        fc_0's weight gradient)."""
        if not x.is_cuda:
            raise RuntimeError("IF-Net HIP path needs GPU tensors (no CPU fallback)")
        return _EncoderGatherFn.apply(self, torch.is_grad_enabled(), link, lease, w0p, b0, x.float(), points.float(), *self._param_list)

    def forward(self, x, points):
        """Reference layout (B, sumC, 1, 7, N) -- model/ifnet.py:197; used by API-compat callers."""
        B, N = points.shape[0], points.shape[1]
        rows = self.feature_rows(x, points)
        perm = self._layout.reference_permutation().to(rows.device)
        inv = torch.empty(self._layout.width, dtype=torch.long, device=rows.device)
        valid = perm >= 0
        inv[perm[valid]] = torch.nonzero(valid).squeeze(1)
        f = rows[:, inv].view(B, N, -1, 7).permute(0, 2, 3, 1)
        return f.unsqueeze(2)


class IFNetFeatureExtractor128(_ExtractorBase):
    def __init__(self):
        super().__init__()
        self.conv_in = nn.Conv3d(1, 16, 3, padding=1)
        self.conv_0 = nn.Conv3d(16, 32, 3, padding=1)
        self.conv_0_1 = nn.Conv3d(32, 32, 3, padding=1)
        self.conv_1 = nn.Conv3d(32, 64, 3, padding=1)
        self.conv_1_1 = nn.Conv3d(64, 64, 3, padding=1)
        self.conv_2 = nn.Conv3d(64, 128, 3, padding=1)
        self.conv_2_1 = nn.Conv3d(128, 128, 3, padding=1)
        self.conv_3 = nn.Conv3d(128, 128, 3, padding=1)
        self.conv_3_1 = nn.Conv3d(128, 128, 3, padding=1)
        self.actvn = nn.ReLU()
        self.maxpool = nn.MaxPool3d(2)
        self.conv_in_bn = nn.BatchNorm3d(16)
        self.conv0_1_bn = nn.BatchNorm3d(32)
        self.conv1_1_bn = nn.BatchNorm3d(64)
        self.conv2_1_bn = nn.BatchNorm3d(128)
        self.conv3_1_bn = nn.BatchNorm3d(128)
        self._finish_init(128)


class IFNetFeatureExtractor(_ExtractorBase):
    def __init__(self, f1, f2, f3, f4):
        super().__init__()
        self.conv_1 = nn.Conv3d(1, f1, 3, padding=1)
        self.conv_1_1 = nn.Conv3d(f1, f2, 3, padding=1)
        self.conv_2 = nn.Conv3d(f2, f3, 3, padding=1)
        self.conv_2_1 = nn.Conv3d(f3, f4, 3, padding=1)
        self.conv_3 = nn.Conv3d(f4, f4, 3, padding=1)
        self.conv_3_1 = nn.Conv3d(f4, f4, 3, padding=1)
        self.actvn = nn.ReLU()
        self.maxpool = nn.MaxPool3d(2)
        self.conv1_1_bn = nn.BatchNorm3d(f2)
        self.conv2_1_bn = nn.BatchNorm3d(f4)
        self.conv3_1_bn = nn.BatchNorm3d(f4)
        self._finish_init(32)


def _check_prepared_for(vols, levels):
    """A prepare_query() descriptor holds ITS pyramid (slab table, volume pointers): a different `levels` would be ignored."""
    if len(vols) != len(levels) or any(a.data_ptr() != b.data_ptr() or a.shape != b.shape for a, b in zip(vols, levels)):
        raise RuntimeError("IFNet.query: `prepared` was made for another pyramid than `levels` (prepare_query again)")


class IFNet(nn.Module):
    def __init__(self, hidden_dim=256, net_res=128):
        super().__init__()
        self.net_res = net_res
        if net_res == 128:
            self.ifnet_feature_extractor = IFNetFeatureExtractor128()
            feature_size = (1 + 16 + 32 + 64 + 128 + 128) * 7
            self.fc_0 = nn.Conv1d(feature_size, hidden_dim, 1)
            self.fc_1 = nn.Conv1d(hidden_dim, hidden_dim, 1)
            self.fc_2 = nn.Conv1d(hidden_dim, hidden_dim, 1)
        elif net_res == 32:
            self.ifnet_feature_extractor = IFNetFeatureExtractor(32, 64, 128, 128)
            feature_size = (1 + 64 + 128 + 128) * 7
            self.fc_0 = nn.Conv1d(feature_size, hidden_dim * 2, 1)
            self.fc_1 = nn.Conv1d(hidden_dim * 2, hidden_dim, 1)
            self.fc_2 = nn.Conv1d(hidden_dim, hidden_dim, 1)
        else:
            # the reference *returns* NotImplementedError here (model/ifnet.py:31-32); raise instead
            raise NotImplementedError(f"net_res={net_res}")
        self.fc_out = nn.Conv1d(hidden_dim, 1, 1)
        self.actvn = nn.ReLU()
        perm = self.ifnet_feature_extractor._layout.reference_permutation()
        self.register_buffer("_fc0_perm", perm, persistent=False)
        # gather index / 0-1 mask of the internal columns, and the inverse (reference feature k -> internal column)
        self.register_buffer("_fc0_src", perm.clamp(min=0), persistent=False)
        self.register_buffer("_fc0_mask", perm < 0, persistent=False)          # True on the padding columns
        inv = torch.empty(int((perm >= 0).sum()), dtype=torch.long)
        inv[perm[perm >= 0]] = torch.nonzero(perm >= 0).squeeze(1)
        self.register_buffer("_fc0_inv", inv, persistent=False)

    def _fc0_internal(self):
        """fc_0.weight (H, F, 1) with reference column order k = c*7+j -> (H, FS) in the internal
        column order (zero weight on padding columns).  The checkpoint layout never changes."""
        return _PermuteColumnsFn.apply(self.fc_0.weight.squeeze(2), self._fc0_src, self._fc0_mask, self._fc0_inv)

    @torch.no_grad()
    def _prepare_weights_async(self, lease):
        """Training step: the weight planes of every split-precision layer (encoder convolutions behind conv_in, fc_1,
        fc_2; forward and backward-data forms) are made on the side stream, in front of the Morton sort, instead of in
        2-4 launch-bound kernels in front of each layer call on the main stream (~40 launches per step).  Valid until
        the encoder's backward has been enqueued -- or the forward's graph is dropped without one (they expire with the
        arena lease) -- ops find them by the parameter's address + version (ops.PreparedWeights)."""
        if not PREPARE_WEIGHTS_AHEAD:
            return
        ext = self.ifnet_feature_extractor
        prep = ext._prepared
        main, side = torch.cuda.current_stream(), _get_side_stream(self.fc_out.weight.device)
        side.wait_stream(main)          # the optimizer step that produced these parameters
        with torch.cuda.stream(side):
            prep.begin()
            # forward planes first, with their own event: the forward pass waits for those only, the backward planes (as many
            # launches again) are made while it runs
            for which in ("fwd", "bwd"):
                for convs, _ in ext._stages:
                    for conv in convs:
                        if conv.weight.shape[1] > 1:
                            prep.add_conv(conv.weight.detach(), which)
                # fc_1 / fc_2 forward: the planes of the fused tail (ops.mlp_tail_fwd) where it runs, else one set per layer
                w1, w2 = self.fc_1.weight.detach().squeeze(2), self.fc_2.weight.detach().squeeze(2)
                if which == "bwd" or not prep.add_mlp_tail(w1, w2):
                    prep.add_linear(w1, which)
                    prep.add_linear(w2, which)
                if which == "fwd":
                    prep.mark(side)
            prep.finish(side)
        ops.set_prepared(prep)

        def expire():       # with the lease: at the end of the backward, or when the graph is dropped without one
            prep.invalidate()
            if ops._prepared is prep:
                ops.set_prepared(None)
        lease.on_release.append(expire)

    @torch.no_grad()
    def encode(self, x, storage="f32"):
        """Cache the feature pyramid of a grid for repeated queries (dense-grid inference).  storage="bf16": the
        throughput mode -- the pyramid (computed in f32) is stored in bf16 and query() runs the bf16-storage gather +
        point MLP (f32 accumulation; bf16_path.hip).  Never the default: bf16 logits are not held to the fp32 gate."""
        levels = self.ifnet_feature_extractor.encode_levels(x)
        if storage == "bf16":
            return [ops.cast_bf16(v) for v in levels]
        if storage != "f32":
            raise ValueError(f"storage={storage!r}")
        return levels

    @torch.no_grad()
    def _query_bf16(self, levels, points, row_map, prepared=None):
        B, N = points.shape[0], points.shape[1]
        ext = self.ifnet_feature_extractor
        if prepared is None and FUSE_FC0_BF16 and ops.gather_fc0_bf16_supported(levels, ext._layout, ext._disp, ext._align,
                                                                                self.fc_0.out_channels):
            prepared = ops.gather_fc0_bf16_prepare(levels, ext._layout, ext._disp, ext._align, self._fc0_internal())
        if prepared is not None:      # fused gather -> fc_0 on bf16 storage: the bf16 feature rows never reach HBM
            _check_prepared_for(prepared["vols"], levels)
            h = ops.gather_fc0_bf16_run(prepared, points, self.fc_0.bias, relu=True)
        else:
            rows = ops.gather_fwd_bf16(levels, points, ext._layout, ext._disp, ext._align)
            h = ops.linear_fwd_bf16(rows, ops.cast_bf16(self._fc0_internal()), self.fc_0.bias, relu=True)
        h = ops.linear_fwd_bf16(h, ops.cast_bf16(self.fc_1.weight.squeeze(2).contiguous()), self.fc_1.bias, relu=True)
        h = ops.linear_fwd_bf16(h, ops.cast_bf16(self.fc_2.weight.squeeze(2).contiguous()), self.fc_2.bias, relu=True)
        return ops.fc_out_fwd_bf16(h, self.fc_out.weight.reshape(-1).contiguous(), self.fc_out.bias, row_map).view(B, N)

    @torch.no_grad()
    def prepare_query(self, levels, max_points):
        """Per-pyramid preparation of the f32 query path (fc_0's weights split for the fused kernel, slab table): pass the
        result to query(..., prepared=) when one pyramid is queried chunk by chunk (dense-grid inference); None when the
        fused kernel does not cover the shapes."""
        ext = self.ifnet_feature_extractor
        if levels[0].dtype == torch.bfloat16:
            if FUSE_FC0_BF16 and ops.gather_fc0_bf16_supported(levels, ext._layout, ext._disp, ext._align, self.fc_0.out_channels):
                return ops.gather_fc0_bf16_prepare(levels, ext._layout, ext._disp, ext._align, self._fc0_internal())
            return None
        if levels[0].dtype != torch.float32 or not FUSE_FC0 or self.fc_0.out_channels != 256:
            return None
        B = levels[0].shape[0]
        probe = torch.empty(B, 1, 3, device=levels[0].device)
        if not ops.gather_fc0_supported(levels, probe, ext._layout, ext._disp, ext._align, self.fc_0.out_channels):
            return None
        return ops.gather_fc0_prepare(levels, ext._layout, ext._disp, ext._align, self._fc0_internal(), B, int(max_points))

    @torch.no_grad()
    def query(self, levels, points, spatial_sort=False, prepared=None):
        """Logits (B,N) for `points` against a pyramid from encode() (f32, or bf16 storage).  spatial_sort: visit the
        points of every sample in Morton order (pays off for scattered points: the gather's corner reads become cache
        hits; a dense lattice is ordered already); results do not depend on it.  prepared: prepare_query(levels, ...)."""
        B, N = points.shape[0], points.shape[1]
        points = points.float().contiguous()
        row_map = None
        if spatial_sort and N > 1:
            row_map, points = ops.morton_order(points, want_sorted=True)
        if levels[0].dtype == torch.bfloat16:
            return self._query_bf16(levels, points, row_map, prepared)
        ext = self.ifnet_feature_extractor
        if prepared is not None:
            _check_prepared_for(prepared.vols, levels)
            h, _ = ops.gather_fc0_run(prepared, points, self.fc_0.bias)
        elif FUSE_FC0 and ops.gather_fc0_supported(levels, points, ext._layout, ext._disp, ext._align, self.fc_0.out_channels):
            h, _ = ops.gather_fc0_fwd(levels, points, ext._layout, ext._disp, ext._align, self._fc0_internal(), self.fc_0.bias)
        else:
            rows = ext.feature_rows_from_levels(levels, points)
            h = ops.linear_fwd(rows, self._fc0_internal(), self.fc_0.bias, relu=True)
        _, _, logits = ops.mlp_tail_fwd(h, self.fc_1.weight.squeeze(2), self.fc_1.bias, self.fc_2.weight.squeeze(2), self.fc_2.bias,
                                        self.fc_out.weight.reshape(-1).contiguous(), self.fc_out.bias, row_map)
        return logits.view(B, N)

    def forward(self, x, points, spatial_sort=True):
        """logits (B,N).  With spatial_sort the points of every sample are visited in Morton order: the whole
        gather -> MLP -> scatter chain runs on the permuted point set (rows are independent), and only the
        (B,N) logits are permuted back.  That makes the gather's reads L2-local and lets the backward scatter
        combine runs of samples that share corners (gather.hip); results do not depend on the order."""
        B, N = points.shape[0], points.shape[1]
        if not x.is_cuda:
            raise RuntimeError("IF-Net HIP path needs GPU tensors (no CPU fallback)")
        row_map = None
        ext = self.ifnet_feature_extractor
        # training step: the large buffers that cross streams come from the extractor's step arena (held until the
        # encoder's backward has been enqueued; a second forward in between gets ordinary allocations)
        lease = ext._arena.lease() if (USE_ARENA and torch.is_grad_enabled() and not points.requires_grad
                                       and not torch.cuda.is_current_stream_capturing()) else None
        arena = lease.arena if lease is not None else None
        ext._points_ready = None
        if spatial_sort and N > 1:
            pts = points.detach().float().contiguous()
            if arena is not None and SORT_ON_SIDE_STREAM and not os.environ.get("SVR_NO_SIDE_STREAM"):
                self._prepare_weights_async(lease)
                # the Morton sort (a chain of ~25 launch-bound radix-sort kernels, 0.2 ms) is only needed by the gather and
                # by the scatter plans: it runs on the side stream, in front of the plans, while the encoder starts on the
                # main stream at once; the main stream waits for it in front of the gather (_EncoderGatherFn.forward).
                # (Arena buffers only: they never return to an allocator pool, so no record_stream bookkeeping.)
                main, side = torch.cuda.current_stream(), _get_side_stream(x.device)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    row_map, sorted_pts = ops.morton_order(pts, want_sorted=True, arena=arena)
                    ext._points_ready = torch.cuda.Event()
                    ext._points_ready.record(side)
            else:
                row_map, sorted_pts = ops.morton_order(pts, want_sorted=True, arena=arena)     # samples stay contiguous
            if points.requires_grad:       # rare (subsample_points > 0): keep the permutation differentiable
                points = points.reshape(B * N, 3)[row_map.long()].view(B, N, 3)
            else:
                points = sorted_pts
        w0p = self._fc0_internal()
        link = None
        if (PROJECT_WIDE_LEVELS and torch.is_grad_enabled() and w0p.requires_grad and not points.requires_grad
                and self.fc_0.out_channels == 256 and SCATTER_FORM != "atomic"
                and not (ops.GATHER_FLAGS & ops._lib.GATHER_DETERMINISTIC)):
            wide = [l for l, c in enumerate(ext._layout.channels) if c == 128 and
                    ops.project_bwd_supported(B, N, _level_dims(*x.shape[2:], l))]
            if wide and B * N * ext._layout.row_stride < 2 ** 31:
                link = _ProjLink(wide, ext._layout)
        tail = (self.fc_1.weight.squeeze(2), self.fc_1.bias, self.fc_2.weight.squeeze(2), self.fc_2.bias,
                self.fc_out.weight.reshape(-1), self.fc_out.bias)
        if (FUSE_FC0 and not points.requires_grad and B * N * ext._layout.row_stride < 2 ** 31
                and _fc0_fusable(ext._layout.channels, B, x.shape[2:], self.fc_0.out_channels)):
            h0 = ext.feature_rows(x, points, link, w0p, self.fc_0.bias, lease=lease)
            logits = _PointMLPFn.apply(h0, row_map, None, None, *tail, None)       # headless: fc_0 ran inside the gather
        else:
            rows = ext.feature_rows(x, points, link, w0p if link is not None else None, lease=lease)
            logits = _PointMLPFn.apply(rows, row_map, w0p, self.fc_0.bias, *tail, link)
        return logits.view(B, N)


def make_3d_grid(bb_min, bb_max, shape, res_increase=1):
    """Lattice of query points, C-order with the last axis fastest (model/ifnet.py:202-212)."""
    shape = [int(s) for s in shape]
    size = shape[0] * shape[1] * shape[2] * res_increase ** 3
    full = [s * res_increase for s in shape]
    pxs = torch.linspace(bb_min[0], bb_max[0], full[0]).view(-1, 1, 1).expand(*full).contiguous().view(size)
    pys = torch.linspace(bb_min[1], bb_max[1], full[1]).view(1, -1, 1).expand(*full).contiguous().view(size)
    pzs = torch.linspace(bb_min[2], bb_max[2], full[2]).view(1, 1, -1).expand(*full).contiguous().view(size)
    return torch.stack([pxs, pys, pzs], dim=1)


def evaluate_network_on_grid_device(network, x, resolution, res_increase=1, points_batch_size=2048 * 16, storage="f32"):
    """Occupancy probabilities on the dense lattice (model/ifnet.py:215-229), as a device tensor (X, Y, Z) float32.

    Same result as the reference loop, but the encoder pyramid is computed once (network.encode) instead of
    once per chunk, the lattice is built on the device, and the values stay on the device.  `network` in eval() mode
    reproduces the reference's validation call; any module without encode()/query() falls back to network(x, chunk)."""
    pointsf = make_3d_grid((-0.5,) * 3, (0.5,) * 3, resolution, res_increase).to(x.device)
    values = []
    with torch.no_grad():
        levels = (network.encode(x, storage) if storage != "f32" else network.encode(x)) if hasattr(network, "encode") else None
        prep = network.prepare_query(levels, points_batch_size) if (levels is not None and hasattr(network, "prepare_query")) else None
        for pi in torch.split(pointsf, points_batch_size):
            pi = pi.unsqueeze(0)
            z = (network.query(levels, pi, prepared=prep) if prep is not None else network.query(levels, pi)) \
                if levels is not None else network(x, pi)
            values.append(torch.sigmoid(z).squeeze(0))
    r = [int(s) * res_increase for s in resolution]
    return torch.cat(values, dim=0).view(r[0], r[1], r[2])


def evaluate_network_on_grid(network, x, resolution, res_increase=1, points_batch_size=2048 * 16, storage="f32"):
    """Occupancy probabilities on the dense lattice (model/ifnet.py:215-229) as a numpy array: the device grid of
    evaluate_network_on_grid_device with a single D2H copy at the end (the reference does one per chunk, :226)."""
    return evaluate_network_on_grid_device(network, x, resolution, res_increase, points_batch_size, storage).cpu().numpy()


def _inference_block(value):
    """0 (dense) or a block edge >= 2; anything else is refused."""
    try:
        b = int(value)
    except (TypeError, ValueError):
        b = -1
    if b != 0 and b < 2:
        raise ValueError(f"inference block must be 0 (dense) or an integer >= 2, got {value!r}")
    return b


# Block edge of the sparse lattice evaluation behind implicit_to_mesh (util/sparse_grid.py); 0 = the
# dense evaluation.  Both trainers' validation / test steps reach the sparse path through this attribute.
INFERENCE_BLOCK = _inference_block(os.environ.get("SVR_INF_BLOCK", "0"))


def evaluate_network_on_grid_sparse(network, x, resolution, threshold_p, res_increase=1, block=8, points_batch_size=2048 * 16,
                                    max_rounds=32, storage="f32", profile=False):
    """1 - occupancy probability on the lattice of evaluate_network_on_grid_device, with the network queried only in the
    blocks of `block` cells that the level set `threshold_p` passes through (util.sparse_grid.sparse_lattice_field).
    Returns its SparseLatticeField: `.field` (X, Y, Z) is what implicit_to_mesh hands to marching_cubes; an evaluated
    point holds 1 - sigmoid(query) from the same ops as the dense path, every other point a value on its block's side of
    the level.  encode / prepare_query are used as the dense path uses them."""
    from ..util.sparse_grid import sparse_lattice_field
    if not x.is_cuda:
        raise RuntimeError("IF-Net HIP path needs GPU tensors (no CPU fallback)")
    r = [int(s) * res_increase for s in resolution]
    with torch.no_grad():
        levels = network.encode(x, storage) if storage != "f32" else network.encode(x)
        prep = network.prepare_query(levels, points_batch_size)

        def fn(pts):
            pi = pts.unsqueeze(0)
            z = network.query(levels, pi, prepared=prep) if prep is not None else network.query(levels, pi)
            return 1 - torch.sigmoid(z).squeeze(0)

        return sparse_lattice_field(fn, r, threshold_p, block, points_batch_size, max_rounds, device=x.device, profile=profile)


def implicit_to_vertices(network, x, resolution, threshold_p, res_increase=1, block=None):
    """implicit_to_mesh without the file: (vertices (V,3) float32, faces (F,3) int32) as device tensors."""
    from ..util.visualize import marching_cubes
    block = INFERENCE_BLOCK if block is None else _inference_block(block)
    if block:
        sdf = evaluate_network_on_grid_sparse(network, x, resolution, threshold_p, res_increase, block).field
        return marching_cubes(sdf, threshold_p)
    value_grid = evaluate_network_on_grid_device(network, x, resolution, res_increase)
    return marching_cubes(1 - value_grid, threshold_p)


def implicit_to_mesh(network, x, resolution, threshold_p, output_path, res_increase=1, block=None):
    """The reference's implicit_to_mesh (model/ifnet.py:232-234): the mesh of the occupancy lattice at probability
    `threshold_p`, written to `output_path` as .obj.  Computes what
    ``visualize_sdf(1 - evaluate_network_on_grid(...), output_path, level=threshold_p)`` computes (1 - p in float32, as
    the reference's numpy does), but the lattice never leaves the device: only the mesh crosses to the host.
    Returns (vertices (V,3) float32, faces (F,3) int32) as device tensors.

    block: None takes INFERENCE_BLOCK; 0 is the dense evaluation above; an integer >= 2 queries the network only in the
    blocks of that many cells the surface passes through (evaluate_network_on_grid_sparse: the same mesh unless a surface
    component hides between the coarse points)."""
    from ..util.visualize import export_obj
    vertices, faces = implicit_to_vertices(network, x, resolution, threshold_p, res_increase, block)
    export_obj(vertices, faces, output_path)
    return vertices, faces
