"""Thin tensor-level wrappers over the C ABI: check device/dtype/contiguity, pass raw device
pointers and the current HIP stream.  torch is used for memory and streams only."""
import ctypes as C
import os

import torch

from . import _lib
from .arena import alloc as _alloc
from ._lib import EPI_BIAS, EPI_BIAS_RELU, EPI_MASK, EPI_NONE, GatherDesc, check  # noqa: F401
from ._lib import ptr as _p, stream as _stream


def _rp(t):
    """Address of a row-strided 2-D GPU operand whose leading dimension is passed beside it (None -> NULL); _p wants contiguity."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("svr_amd ops need GPU tensors (the HIP path has no CPU fallback)")
    return t.data_ptr()


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"expected float32, got {t.dtype}")


# ------------------------------------------------------------------------------------------
# feature-row layout
# ------------------------------------------------------------------------------------------
class FeatureLayout:
    """Column layout of a feature row: levels with C>=4 first (each 7*C wide, sample-major,
    channel contiguous, 16-float aligned), the C==1 level last; row stride padded to 32."""

    def __init__(self, channels):
        self.channels = list(channels)
        order = [l for l, c in enumerate(self.channels) if c >= 4] + [l for l, c in enumerate(self.channels) if c < 4]
        self.col = [0] * len(self.channels)
        off = 0
        for l in order:
            self.col[l] = off
            off += 7 * self.channels[l]
        self.width = off
        self.row_stride = (off + 31) // 32 * 32
        self._subsets = {}

    def subset(self, levels):
        """Compact layout of a SUBSET of the levels (same relative order, no gaps, row stride padded to 32): the
        kept-column matrix of the training step -- the levels whose backward is not projected keep their gathered
        columns in (B*N, 800) instead of a 2592-wide row (128-architecture)."""
        key = tuple(sorted(levels))
        k = self._subsets.get(key)
        if k is None:          # cached: the layout's device-side column index is uploaded once, not once per step
            k = self._subsets[key] = KeptLayout(self, levels)
        return k

    def reference_permutation(self):
        """perm[k_internal] = reference feature row k = c_global*7 + j (model/ifnet.py:43-45,197);
        -1 for padding columns."""
        perm = torch.full((self.row_stride,), -1, dtype=torch.long)
        cbase = 0
        for l, c in enumerate(self.channels):
            j = torch.arange(7).view(7, 1)
            ch = torch.arange(c).view(1, c)
            perm[self.col[l]: self.col[l] + 7 * c] = ((cbase + ch) * 7 + j).reshape(-1)
            cbase += c
        return perm


class KeptLayout:
    """Column layout of the kept-column matrix: `col[l]` for the kept levels (-1 for the others), `row_stride`, and
    `full_cols` (row_stride,) long: the column of the FULL feature row behind every kept column (a padding column of
    the full row -- zero weight, zero feature -- behind the kept matrix's own padding)."""

    def __init__(self, full, levels):
        self.full = full
        self.levels = tuple(sorted(levels, key=lambda l: full.col[l]))
        self.channels = list(full.channels)
        self.col = [-1] * len(full.channels)
        off, src = 0, []
        for l in self.levels:
            self.col[l] = off
            w = 7 * full.channels[l]
            src += list(range(full.col[l], full.col[l] + w))
            off += w
        self.width = off
        self.row_stride = (off + 31) // 32 * 32
        if self.row_stride > off and full.row_stride <= full.width:
            raise RuntimeError("KeptLayout: the full row has no padding column to stand behind the kept padding")
        src += [full.width] * (self.row_stride - off)            # a zero column of the full row
        self.full_cols = torch.tensor(src, dtype=torch.long)
        self._dev = {}

    def full_cols_on(self, device):
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = self.full_cols.to(device)
        return t


def morton_order(points, want_sorted=False, arena=None):
    """(B*N,) int32 processing order: points of one sample sorted by a 64^3 Morton code
    (and, optionally, the points gathered into that order)."""
    _f32(points)
    B, N, _ = points.shape
    l = _lib.lib()
    order = _alloc(arena, "morton_order", (B * N,), torch.int32, points.device)
    spts = _alloc(arena, "morton_points", tuple(points.shape), torch.float32, points.device) if want_sorted else None
    ws = _alloc(arena, "morton_ws", (l.svr_points_morton_order_workspace(B, N),), torch.uint8, points.device)
    check(l.svr_points_morton_order(_p(points), _p(order), _p(spts), B, N, _p(ws), _stream()), "morton_order")
    return (order, spts) if want_sorted else order


def voxel_order(points, dims, align_corners=False):
    """(B*N,) int32: points ordered by the row-major index (x fastest) of their base voxel in a volume of `dims` (D,H,W)."""
    _f32(points)
    B, N, _ = points.shape
    l = _lib.lib()
    order = torch.empty(B * N, device=points.device, dtype=torch.int32)
    ws = torch.empty(l.svr_points_morton_order_workspace(B, N), device=points.device, dtype=torch.uint8)
    check(l.svr_points_voxel_order(_p(points), _p(order), B, N, dims[0], dims[1], dims[2], int(align_corners), _p(ws),
                                   _stream()), "voxel_order")
    return order


class PullPlan:
    """Plan of the atomic-free pull-form backward scatter of one level (svr_gather_pull_plan): keeps the device
    arrays alive and hands the C struct to the gather descriptor."""

    def __init__(self, keys, recs, heads, n_items, items=None, stats=None):
        self.keys, self.recs, self.heads, self.items, self.stats = keys, recs, heads, items, stats
        self.c = _lib.PullPlan(_p(keys), _p(recs), _p(heads), n_items)

    def record_stream(self, stream):
        if self.persistent:      # arena-owned buffers never return to the allocator
            return
        for t in (self.keys, self.recs, self.heads, self.items, self.stats):
            if t is not None:
                t.record_stream(stream)

    persistent = False


def pull_plan_supported(B, N, dims, C, row_stride):
    cells = B * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    return C in (16, 32, 64) and N > 0 and cells < 2 ** 31 - 1 and 7 * B * N < 2 ** 31 and B * N * row_stride < 2 ** 31


def pull_plan(points, dims, C, col, row_stride, displacement, align_corners=False, arena=None, tag=""):
    """Sort the 7*B*N (point, displacement) items of one level by base cell and build the records / cell heads.
    arena / tag: take the plan's arrays from a StepArena (names prefixed with `tag`) instead of the allocator."""
    _f32(points)
    B, N, _ = points.shape
    l = _lib.lib()
    T = 7 * B * N
    cells = B * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    dev = points.device
    keys = _alloc(arena, tag + "keys", (max(T, 1),), torch.int32, dev)
    recs = _alloc(arena, tag + "recs", (max(T, 1), 4), torch.int32, dev)
    heads = _alloc(arena, tag + "heads", (cells + 1,), torch.int32, dev)
    items = _alloc(arena, tag + "items", (max(T, 1),), torch.int32, dev)   # sorted item ids: also this level's item order
    stats = _alloc(arena, tag + "stats", (2,), torch.int32, dev).zero_()
    # (the sort workspace is shared by all plans of a step: they are built one after the other on one stream)
    ws = _alloc(arena, "plan_ws", (l.svr_gather_pull_plan_workspace(B, N) + l.svr_gather_pull_plan_workspace_cells(B, *dims),),
                torch.uint8, dev)
    check(l.svr_gather_pull_plan(_p(points), B, N, dims[0], dims[1], dims[2], C, col, row_stride, int(align_corners),
                                 displacement, _p(keys), _p(recs), _p(heads), _p(items), _p(stats), _p(ws), _stream()),
          "gather_pull_plan")
    plan = PullPlan(keys, recs, heads, T, items, stats)
    plan.persistent = arena is not None
    return plan


def item_order(points, dims, displacement, align_corners=False, with_j=False, arena=None, tag="", x_block=None):
    """(7*B*N,) int32 item ids pn*7+j sorted by (sample, base cell of the displaced sample[, displacement j]) in a
    volume of `dims`.  x_block = K (1 .. W + 1): the x-block order of the projected scatter's atomic form, (sample, z, y,
    block of K x-adjacent cells, j, x inside the block); K = 1 is the with_j order."""
    _f32(points)
    B, N, _ = points.shape
    l = _lib.lib()
    items = _alloc(arena, tag + "items", (max(7 * B * N, 1),), torch.int32, points.device)
    ws = _alloc(arena, "plan_ws", (l.svr_gather_pull_plan_workspace(B, N),), torch.uint8, points.device)
    if x_block is not None:
        check(l.svr_gather_item_order_xblock(_p(points), B, N, dims[0], dims[1], dims[2], int(align_corners), displacement,
                                             int(x_block), _p(items), _p(ws), _stream()), "gather_item_order_xblock")
        return items
    check(l.svr_gather_item_order(_p(points), B, N, dims[0], dims[1], dims[2], int(align_corners), displacement, int(with_j),
                                  _p(items), _p(ws), _stream()), "gather_item_order")
    return items


PROJ_WAVE_CHUNK = 256      # items one wave of gather_bwd_proj_kernel walks (2 x 64 lanes x kProjReps)
PROJ_BLOCK_SHARE = 2.25    # see proj_x_block


def proj_x_block(N, dims):
    """Block length K of the x-block item order for the atomic projected scatter of one level.

    A face is handed over only between two runs that sit in the same wave's chunk of PROJ_WAVE_CHUNK items, and a block
    puts K runs of about r = N / (D*H*W) items in a row for every displacement.  Longer blocks hand more faces over, but
    move the 7 displacements of a point (which read the same dh row) further apart, so a (block, j) row of runs is
    allowed 1 / PROJ_BLOCK_SHARE of a chunk:  K = floor(PROJ_WAVE_CHUNK / (PROJ_BLOCK_SHARE * r)), at least 1 (the plain
    (cell, j) order: runs that fill a third of a chunk each leave little to hand over), at most W + 1.
    PROJ_BLOCK_SHARE was fitted on ONE workload -- the benched step, 50 000 uniform points per sample, where K = 9
    measured best among {1, 3, 4, 6, 9} at 16^3 (r = 12; tools/exp/bench_proj.py, profiles/proj_handover_bench_proj.txt)
    and K = 1 is kept at 8^3 (r = 98, where no K gains more than 5 %) -- not on a range of shapes."""
    r = N / float(dims[0] * dims[1] * dims[2])
    return max(1, min(dims[2] + 1, int(PROJ_WAVE_CHUNK / (PROJ_BLOCK_SHARE * max(r, 1e-9)))))


def project_bwd_supported(B, N, dims, lddh=256):
    cells = B * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    return N > 0 and 8 * cells < 2 ** 31 - 1 and 7 * B * N < 2 ** 31 and B * N * lddh < 2 ** 31 and max(dims) < 1022


_proj_partials = {}


class ProjPlan:
    """Plan of the two-pass (atomic-free) projected scatter of one level (svr_gather_project_plan): the items sorted by
    (sample, cell, displacement), their sorted keys, the run-start counts and the first slot of every key."""

    def __init__(self, items, keys, sidx, first_slot, slots):
        self.items, self.keys, self.sidx, self.first_slot, self.slots = items, keys, sidx, first_slot, slots

    def record_stream(self, stream):
        for t in (self.items, self.keys, self.sidx, self.first_slot):
            t.record_stream(stream)


def project_plan(points, dims, displacement, align_corners=False):
    _f32(points)
    B, N, _ = points.shape
    l = _lib.lib()
    T = 7 * B * N
    nkeys = B * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) * 8
    dev = points.device
    items = torch.empty(max(T, 1), device=dev, dtype=torch.int32)
    keys = torch.empty(max(T, 1), device=dev, dtype=torch.int32)          # uint32 bit patterns
    sidx = torch.empty(T + 1, device=dev, dtype=torch.int32)
    first_slot = torch.empty(nkeys + 1, device=dev, dtype=torch.int32)
    ws = torch.empty(l.svr_gather_project_plan_workspace(B, N), device=dev, dtype=torch.uint8)
    check(l.svr_gather_project_plan(_p(points), B, N, dims[0], dims[1], dims[2], int(align_corners), displacement, _p(items),
                                    _p(keys), _p(sidx), _p(first_slot), _p(ws), _stream()), "gather_project_plan")
    return ProjPlan(items, keys, sidx, first_slot, int(l.svr_gather_project_slots(B, N, dims[0], dims[1], dims[2])))


def gather_project_bwd(points, dh, dims, items, displacement, align_corners=False, out=None):
    """dP (B, D*H*W, 7, 256) = scatter of the 256-wide rows of dh (B*N, >= 256) with the trilinear weights of every
    (point, displacement) item; `items` = item_order(..., with_j=True) (float atomics into a zeroed dP) or a ProjPlan
    (two passes, no atomics, dP written once, bit-reproducible)."""
    _f32(points, dh)
    B, N, _ = points.shape
    assert dh.shape[0] == B * N and dh.shape[1] >= 256 and dh.stride(1) == 1
    if isinstance(items, ProjPlan):
        plan = items
        dP = torch.empty(B, dims[0] * dims[1] * dims[2], 7, 256, device=points.device, dtype=torch.float32)
        # the partial-sum buffer (2.7 GB at 16^3 x 8 samples: sized for the worst case, ~85 % used) is kept between calls:
        # as a per-step allocation it was split up by the caching allocator between two steps and re-allocated with
        # hipMalloc every time (22 instead of 18 ms/step).  One buffer per device and stream; calls on a stream serialise.
        key = (points.device.index, torch.cuda.current_stream(points.device).cuda_stream)
        partials = _proj_partials.get(key)
        if partials is None or partials.numel() < plan.slots * 8 * 256:
            partials = _proj_partials[key] = torch.empty(plan.slots * 8 * 256, device=points.device, dtype=torch.float32)
        check(_lib.lib().svr_gather_project_bwd2(_p(points), _rp(dh), dh.stride(0), B, N, dims[0], dims[1],
                                                 dims[2], int(align_corners), displacement, _p(plan.items), _p(plan.sidx),
                                                 _p(plan.first_slot), _p(partials), _p(dP), _stream()), "gather_project_bwd2")
        return dP
    # out: a ZEROED (B, D*H*W, 7, 256) buffer of the caller (the training step zero-fills it on the side stream during the forward)
    dP = out if out is not None else torch.zeros(B, dims[0] * dims[1] * dims[2], 7, 256, device=points.device, dtype=torch.float32)
    assert tuple(dP.shape) == (B, dims[0] * dims[1] * dims[2], 7, 256) and dP.is_contiguous()
    amax_forget(out)
    check(_lib.lib().svr_gather_project_bwd(_p(points), _rp(dh), dh.stride(0), B, N, dims[0], dims[1], dims[2],
                                            int(align_corners), displacement, _p(items), _p(dP), _stream()), "gather_project_bwd")
    return dP


def make_gather_desc(vols, gvols, layout, B, N, displacement, align_corners, order=None, level_orders=None, flags=0,
                     level_plans=None, skip_levels=()):
    """layout: a FeatureLayout, or a KeptLayout (compact kept-column matrix; the levels it does not hold must be in
    skip_levels).  skip_levels: these levels get NULL volume pointers (a backward skips them)."""
    d = GatherDesc()
    d.flags = int(flags)
    d.order = _p(order)
    d.n_levels = len(vols)
    d.B, d.N = B, N
    d.row_stride = layout.row_stride
    d.align_corners = int(align_corners)
    d.displacement = displacement
    for l, v in enumerate(vols):
        g = gvols[l] if gvols is not None else None
        ref = v if v is not None else g
        _f32(v, g)
        if ref.dim() != 5 or ref.shape[0] != B or ref.shape[4] != layout.channels[l]:
            raise RuntimeError(f"level {l}: expected (B,D,H,W,{layout.channels[l]}) channels-last, got {tuple(ref.shape)}")
        L = d.level[l]
        L.C, L.D, L.H, L.W = ref.shape[4], ref.shape[1], ref.shape[2], ref.shape[3]
        if l in skip_levels:
            L.vol, L.gvol, L.col = C.c_void_p(0), C.c_void_p(0), 0
            continue
        if layout.col[l] < 0:
            raise RuntimeError(f"level {l} has no columns in this layout (list it in skip_levels)")
        L.vol, L.gvol = _p(v), _p(g)
        L.col = layout.col[l]
        o = level_orders[l] if level_orders is not None else None
        # a (7*B*N) order is an ITEM order (svr_gather_item_order), a (B*N) one a point order (svr_points_voxel_order)
        if o is not None and B * N > 0 and o.numel() == 7 * B * N:
            L.item_order, L.order = _p(o), C.c_void_p(0)
        else:
            L.item_order, L.order = C.c_void_p(0), _p(o)
        if level_plans is not None and level_plans[l] is not None:
            L.plan = C.pointer(level_plans[l].c)
    return d


# Test switches (results do not change): GATHER_FLAGS is OR-ed into every gather descriptor --
# _lib.GATHER_WIDE_OFFSETS takes the 64-bit-offset forward body at any size, _lib.GATHER_DETERMINISTIC replaces the
# atomic backward scatter by the serial fixed-order one (bit-reproducible; equals ATen's CPU summation order).
GATHER_FLAGS = 0


def gather_fwd(vols, points, layout, displacement, align_corners, out=None, order=None, flags=0):
    B, N, _ = points.shape
    _f32(points)
    d = make_gather_desc(vols, None, layout, B, N, displacement, align_corners, order, flags=flags | GATHER_FLAGS)
    if out is None:   # the kernel writes every column (padding columns as zeros): no memset of the 4 GB buffer
        out = torch.empty(B * N, layout.row_stride, device=points.device, dtype=torch.float32)
    amax_forget(out)
    check(_lib.lib().svr_gather_trilinear_fwd(C.byref(d), _p(points), _p(out), _stream()), "gather_fwd")
    return out


def gather_fc0_supported(vols, points, layout, displacement, align_corners, n_out=256):
    B, N, _ = points.shape
    if n_out != 256 or not points.is_cuda:
        return False
    d = make_gather_desc(vols, None, layout, B, N, displacement, align_corners)
    return bool(_lib.lib().svr_gather_fc0_supported(C.byref(d)))


class Fc0Prepared:
    """fc_0's weights split into the fused kernel's f16 planes + the slab table of one pyramid (svr_gather_fc0_prepare):
    reusable for any number of gather_fc0_run calls on the same volumes / layout / weights."""

    def __init__(self, vols, layout, displacement, align_corners, n_out, ws, keep_levels, keep_layout, B=None, N=None):
        self.vols, self.layout, self.displacement, self.align_corners = list(vols), layout, displacement, align_corners
        # the point set the workspace was sized for (one FcBox record per 64-point tile and staged level): a larger query
        # would write past it on the device, so gather_fc0_run refuses it
        self.B, self.N = B, N
        self.n_out, self.ws, self.keep_levels, self.keep_layout = n_out, ws, tuple(keep_levels), keep_layout
        self.mask = 0
        for lv in self.keep_levels:
            self.mask |= 1 << lv
        self.kc = None
        self.stride = layout.row_stride
        if self.mask and keep_layout is not None:
            if set(keep_layout.levels) != set(self.keep_levels):
                raise RuntimeError("gather_fc0: keep_layout does not hold exactly keep_levels")
            self.stride = keep_layout.row_stride
            self.kc = (C.c_int32 * len(self.vols))(*[int(c) for c in keep_layout.col])


def gather_fc0_prepare(vols, layout, displacement, align_corners, w, B, N, keep_levels=(), keep_layout=None, arena=None):
    """Split w (n_out, >= layout.width) for the fused gather -> fc_0 kernel and store the slab table (three small
    launches); -> Fc0Prepared for gather_fc0_run.  B, N: the largest point set that will be queried."""
    _f32(w)
    d = make_gather_desc(vols, None, layout, B, N, displacement, align_corners)
    l = _lib.lib()
    n_out = w.shape[0]
    assert w.stride(1) == 1 and w.shape[1] >= layout.width
    ws_bytes = l.svr_gather_fc0_workspace(C.byref(d), n_out)
    if ws_bytes <= 0:
        raise RuntimeError("gather_fc0: unsupported level shapes (see svr_gather_fc0_supported)")
    ws = _alloc(arena, "fc0_ws", (ws_bytes,), torch.uint8, w.device)
    prep = Fc0Prepared(vols, layout, displacement, align_corners, n_out, ws, keep_levels, keep_layout, B, N)
    # (the kept matrix itself is only needed by run; prepare validates its geometry against a dummy aligned address)
    check(l.svr_gather_fc0_prepare(C.byref(d), _rp(w), w.stride(0), n_out, C.c_void_p(256) if prep.mask else None,
                                   prep.stride if prep.mask else 0, prep.kc, prep.mask, _p(ws), _stream()), "gather_fc0_prepare")
    return prep


def gather_fc0_run(prep, points, bias, relu=True, rows_out=None):
    """The fused gather -> fc_0 kernel alone, on a prepared pyramid: -> (h0 (B*N, n_out), kept rows or None)."""
    B, N, _ = points.shape
    _f32(points, bias)
    if prep.B is not None and (B != prep.B or N > prep.N):
        raise RuntimeError(f"gather_fc0: points ({B}, {N}, 3) exceed the prepared capacity (B = {prep.B}, N <= {prep.N}): "
                           "prepare again for the larger point set")
    d = make_gather_desc(prep.vols, None, prep.layout, B, N, prep.displacement, prep.align_corners)
    out = torch.empty(B * N, prep.n_out, device=points.device, dtype=torch.float32)
    rows, ldf = None, 0
    if prep.mask:
        if rows_out is not None:
            if tuple(rows_out.shape) != (B * N, prep.stride) or not rows_out.is_contiguous():
                raise RuntimeError(f"gather_fc0: rows_out must be contiguous ({B * N}, {prep.stride})")
            _f32(rows_out)
            amax_forget(rows_out)
            rows = rows_out
        else:
            rows = torch.empty(B * N, prep.stride, device=points.device, dtype=torch.float32)
        ldf = prep.stride
    epi = EPI_NONE if bias is None else (EPI_BIAS_RELU if relu else EPI_BIAS)
    check(_lib.lib().svr_gather_fc0_run(C.byref(d), _p(points), _p(bias), _p(out), out.stride(0), prep.n_out, _p(rows), ldf,
                                        prep.kc, prep.mask, epi, _p(prep.ws), _stream()), "gather_fc0_run")
    return out, rows


def gather_fc0_fwd(vols, points, layout, displacement, align_corners, w, bias, relu=True, keep_levels=(), keep_layout=None,
                   rows_out=None, arena=None):
    """h0 (B*N, 256) = [relu](feature_rows(vols, points) @ w.T + bias) without materialising the feature rows (gather_fc0.hip).
    keep_levels: levels whose gathered columns are also stored -> (h0, rows); () -> (h0, None).
      keep_layout None: rows (B*N, layout.row_stride) in the full row layout, valid ONLY in those levels' columns and the
        padding columns (the rest is uninitialised memory);
      keep_layout = layout.subset(keep_levels): rows (B*N, keep_layout.row_stride), the compact kept-column matrix (every
        column valid, padding zero).
    rows_out: write the kept rows there instead of allocating; arena: a StepArena for the per-call workspace.
    = gather_fc0_prepare + gather_fc0_run."""
    B, N, _ = points.shape
    prep = gather_fc0_prepare(vols, layout, displacement, align_corners, w, B, N, keep_levels, keep_layout, arena)
    return gather_fc0_run(prep, points, bias, relu, rows_out)


def gather_bwd(vols, gvols, points, gfeat, layout, displacement, align_corners, want_gpoints=False, order=None,
               level_orders=None, flags=0, level_plans=None, skip_levels=()):
    """level_plans[l] (PullPlan or None): that level is scattered atomic-free in pull form and its gvol OVERWRITTEN
    (it may be uninitialised); the other levels accumulate into their (zeroed) gvol with float atomics.
    layout may be a KeptLayout (gfeat = gradient of the compact kept-column matrix; skip_levels = the levels it lacks)."""
    B, N, _ = points.shape
    if gfeat.numel() != B * N * layout.row_stride:
        raise RuntimeError(f"gather_bwd: gfeat {tuple(gfeat.shape)} does not match the layout's ({B * N}, {layout.row_stride})")
    d = make_gather_desc(vols, gvols, layout, B, N, displacement, align_corners, order, level_orders,
                         flags=flags | GATHER_FLAGS, level_plans=level_plans, skip_levels=skip_levels)
    gp = torch.empty_like(points) if want_gpoints else None
    for g in gvols or ():      # accumulated into / overwritten through their raw pointers
        amax_forget(g)
    check(_lib.lib().svr_gather_trilinear_bwd(C.byref(d), _p(points), _p(gfeat), _p(gp), _stream()), "gather_bwd")
    return gp


def corner_indices(vols, points, layout, level, displacement, align_corners):
    B, N, _ = points.shape
    d = make_gather_desc(vols, None, layout, B, N, displacement, align_corners)
    out = torch.empty(B, 7, N, 3, device=points.device, dtype=torch.int32)
    check(_lib.lib().svr_gather_corner_indices(C.byref(d), level, _p(points), _p(out), _stream()), "corner_indices")
    return out


# ------------------------------------------------------------------------------------------
# bf16-storage throughput mode of the query path (bf16_path.hip): separate entry points, never the default
# ------------------------------------------------------------------------------------------
def cast_bf16(t):
    """f32 -> bf16 (round to nearest even), same shape."""
    _f32(t)
    out = torch.empty(t.shape, device=t.device, dtype=torch.bfloat16)
    check(_lib.lib().svr_cast_f32_to_bf16(_p(t), _p(out), t.numel(), _stream()), "cast_bf16")
    return out


def _bf16(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.bfloat16:
            raise RuntimeError(f"expected bfloat16, got {t.dtype}")


def gather_fwd_bf16(vols, points, layout, displacement, align_corners, order=None):
    """bf16 volumes (B,D,H,W,C) -> bf16 feature rows (B*N, row_stride); geometry and accumulation in f32."""
    B, N, _ = points.shape
    _f32(points)
    _bf16(*vols)
    d = GatherDesc()
    d.order = _p(order)
    d.n_levels, d.B, d.N, d.row_stride = len(vols), B, N, layout.row_stride
    d.align_corners, d.displacement = int(align_corners), displacement
    for l, v in enumerate(vols):
        if v.dim() != 5 or v.shape[0] != B or v.shape[4] != layout.channels[l]:
            raise RuntimeError(f"level {l}: expected (B,D,H,W,{layout.channels[l]}) channels-last, got {tuple(v.shape)}")
        L = d.level[l]
        L.vol, L.C, L.D, L.H, L.W, L.col = _p(v), v.shape[4], v.shape[1], v.shape[2], v.shape[3], layout.col[l]
    out = torch.empty(B * N, layout.row_stride, device=points.device, dtype=torch.bfloat16)
    check(_lib.lib().svr_gather_trilinear_fwd_bf16(C.byref(d), _p(points), _p(out), _stream()), "gather_fwd_bf16")
    return out


def _bf16_desc(vols, layout, B, N, displacement, align_corners):
    _bf16(*vols)
    d = GatherDesc()
    d.order = C.c_void_p(0)
    d.n_levels, d.B, d.N, d.row_stride = len(vols), B, N, layout.row_stride
    d.align_corners, d.displacement = int(align_corners), displacement
    for l, v in enumerate(vols):
        if v.dim() != 5 or v.shape[0] != B or v.shape[4] != layout.channels[l]:
            raise RuntimeError(f"level {l}: expected (B,D,H,W,{layout.channels[l]}) channels-last, got {tuple(v.shape)}")
        L = d.level[l]
        L.vol, L.C, L.D, L.H, L.W, L.col = _p(v), v.shape[4], v.shape[1], v.shape[2], v.shape[3], layout.col[l]
    return d


def gather_fc0_bf16_supported(vols, layout, displacement, align_corners, n_out):
    """The fused bf16-storage kernel covers these (bf16) volumes and fc_0's width?"""
    d = _bf16_desc(vols, layout, vols[0].shape[0], 1, displacement, align_corners)
    return n_out == 256 and bool(_lib.lib().svr_gather_fc0_supported(C.byref(d)))


def gather_fc0_bf16_prepare(vols, layout, displacement, align_corners, w):
    """w (n_out, >= layout.width) f32 -> one bf16 plane in the fused kernel's fragment order + the slab table; -> a handle
    for gather_fc0_bf16_run.  vols: the bf16 pyramid (IFNet.encode(x, storage="bf16"))."""
    _f32(w)
    B = vols[0].shape[0]
    d = _bf16_desc(vols, layout, B, 1, displacement, align_corners)
    l = _lib.lib()
    n_out = w.shape[0]
    assert w.stride(1) == 1 and w.shape[1] >= layout.width
    ws_bytes = l.svr_gather_fc0_workspace(C.byref(d), n_out)
    if ws_bytes <= 0:
        raise RuntimeError("gather_fc0_bf16: unsupported level shapes (see svr_gather_fc0_supported)")
    ws = torch.empty(ws_bytes, device=w.device, dtype=torch.uint8)
    check(l.svr_gather_fc0_bf16_prepare(C.byref(d), _rp(w), w.stride(0), n_out, _p(ws), _stream()),
          "gather_fc0_bf16_prepare")
    return {"vols": vols, "layout": layout, "disp": displacement, "ac": align_corners, "n_out": n_out, "ws": ws}


def gather_fc0_bf16_run(prep, points, bias, relu=True):
    """-> h0 (B*N, n_out) bf16 = [relu](bf16 features @ bf16(w).T + bias), the features never leave the chip."""
    B, N, _ = points.shape
    _f32(points, bias)
    d = _bf16_desc(prep["vols"], prep["layout"], B, N, prep["disp"], prep["ac"])
    out = torch.empty(B * N, prep["n_out"], device=points.device, dtype=torch.bfloat16)
    epi = EPI_NONE if bias is None else (EPI_BIAS_RELU if relu else EPI_BIAS)
    check(_lib.lib().svr_gather_fc0_bf16_run(C.byref(d), _p(points), _p(bias), _p(out), out.stride(0), prep["n_out"], epi,
                                             _p(prep["ws"]), _stream()), "gather_fc0_bf16_run")
    return out


def linear_fwd_bf16(x, w, bias, relu=True):
    """y (bf16) = [relu](x (bf16) @ w (bf16).T + bias (f32)), f32 accumulation."""
    _bf16(x, w)
    _f32(bias)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1
    out = torch.empty(M, N, device=x.device, dtype=torch.bfloat16)
    epi = EPI_NONE if bias is None else (EPI_BIAS_RELU if relu else EPI_BIAS)
    check(_lib.lib().svr_linear_fwd_bf16(_rp(x), x.stride(0), _rp(w), w.stride(0), _p(bias),
                                         _p(out), out.stride(0), M, N, K, epi, _stream()), "linear_fwd_bf16")
    return out


def fc_out_fwd_bf16(h, w, b, row_map=None):
    _bf16(h)
    _f32(w, b)
    M, K = h.shape
    out = torch.empty(M, device=h.device, dtype=torch.float32)
    check(_lib.lib().svr_fc_out_fwd_bf16(_p(h), h.stride(0), _p(w), _p(b), _p(out), _p(row_map), M, K, _stream()),
          "fc_out_fwd_bf16")
    return out


# ------------------------------------------------------------------------------------------
# point MLP
# ------------------------------------------------------------------------------------------
# Arithmetic of the forward GEMMs of the point MLP: "f16x3" (3-product f16 split with power-of-two scaling, as
# accurate as an f32 GEMM for |x| < 65504, gemm_f16x3.hip), "bf16x6" (6-product bf16 split, any f32 range,
# gemm_bf16x6.hip) or "f32" (exact-f32 MFMA).
FORWARD_GEMM = "f16x3"


class PreparedWeights:
    """Workspaces of the split-precision kernels, prepared AHEAD of the layer calls (include/svr_hip.h, PREPARE / RUN): the
    launches that only depend on the parameters (amax, split planes: 2-4 launch-bound kernels per layer and pass) run once
    per training step on a side stream instead of in front of every layer on the main stream.  Keyed by the parameter's
    storage address; valid from finish() until invalidate() -- i.e. for one forward + backward; every lookup outside that
    window, for a tensor that was not prepared, or for one that was modified in place since (its version counter moved), misses
    and the op prepares its own workspace as before."""

    def __init__(self):
        self._ws = {}
        self._valid = {}          # key -> (the parameter's version counter when its planes were made, index of their event)
        self._events = []
        self.ready = None
        self._waited = set()

    def _buf(self, key, nbytes, device):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes or t.device != device:
            t = self._ws[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
        return t

    def begin(self):
        self._valid.clear()
        self._events = []
        self._waited = set()      # (event index, stream): waits already enqueued

    def add_conv(self, w, which="both"):
        """w (Co,Ci,3,3,3): forward (f16x3) and backward-data (bf16x3 / f16x3s) planes, where those modes apply.  which: "fwd",
        "bwd" or "both" -- the caller prepares every layer's forward planes first and marks them (mark()), so that the forward
        pass waits for those only."""
        _f32(w)
        Co, Ci = w.shape[0], w.shape[1]
        l = _lib.lib()
        z = C.c_void_p(0)
        fwd, bwd = which in ("fwd", "both"), which in ("bwd", "both")
        if fwd and FORWARD_CONV == "f16x3" and Ci % 16 == 0:
            ws = self._buf(("cf", w.data_ptr()), l.svr_conv3d_fwd_f16x3_workspace(Ci, Co), w.device)
            check(l.svr_conv3d_k3_fwd_f16x3(z, _p(w), z, z, 0, 0, 0, 0, Ci, Co, EPI_NONE, _p(ws), _stream()), "conv3d_fwd_f16x3 prepare")
            self._valid[("cf", w.data_ptr())] = (w._version, len(self._events))
        if bwd and BACKWARD_CONV == "bf16x3" and Ci % 2 == 0 and Co % 16 == 0:
            ws = self._buf(("cb", w.data_ptr()), l.svr_conv3d_bwd_data_bf16x3_workspace(Ci, Co), w.device)
            check(l.svr_conv3d_k3_bwd_data_bf16x3(z, _p(w), z, 0, 0, 0, 0, Ci, Co, EPI_NONE, z, _p(ws), _stream()),
                  "conv3d_bwd_data_bf16x3 prepare")
            self._valid[("cb", w.data_ptr())] = (w._version, len(self._events))
        if bwd and BACKWARD_CONV == "f16x3s" and Ci % 2 == 0 and Co % 16 == 0:
            ws = self._buf(("cbh", w.data_ptr()), l.svr_conv3d_bwd_data_f16x3_workspace(Ci, Co), w.device)
            check(l.svr_conv3d_k3_bwd_data_f16x3(z, _p(w), z, 0, 0, 0, 0, Ci, Co, EPI_NONE, z, z, z, _p(ws), _stream()),
                  "conv3d_bwd_data_f16x3 prepare")
            self._valid[("cbh", w.data_ptr())] = (w._version, len(self._events))

    def add_linear(self, w, which="both"):
        """w (N,K) row-major: forward (f16x3) and backward-data (bf16x3 / f16x3s) planes, where those modes apply."""
        _f32(w)
        N, K = w.shape
        assert w.stride(1) == 1
        l = _lib.lib()
        z = C.c_void_p(0)
        fwd, bwd = which in ("fwd", "both"), which in ("bwd", "both")
        if fwd and FORWARD_GEMM == "f16x3" and K % 16 == 0:
            ws = self._buf(("lf", w.data_ptr()), l.svr_linear_fwd_f16x3_workspace(N, K), w.device)
            check(l.svr_linear_fwd_f16x3(z, 0, C.c_void_p(w.data_ptr()), w.stride(0), z, z, 0, 0, N, K, EPI_NONE, _p(ws), _stream()),
                  "linear_fwd_f16x3 prepare")
            self._valid[("lf", w.data_ptr())] = (w._version, len(self._events))
        if bwd and BACKWARD_GEMM == "bf16x3" and N % 32 == 0 and K % 4 == 0:
            ws = self._buf(("lb", w.data_ptr()), l.svr_linear_bwd_data_bf16x3_workspace(N, K), w.device)
            check(l.svr_linear_bwd_data_bf16x3(z, 0, C.c_void_p(w.data_ptr()), w.stride(0), z, 0, 0, N, K, EPI_NONE, z, 0, _p(ws),
                                               _stream()), "linear_bwd_data_bf16x3 prepare")
            self._valid[("lb", w.data_ptr())] = (w._version, len(self._events))
        if bwd and BACKWARD_GEMM == "f16x3s" and N % 16 == 0:
            ws = self._buf(("lbh", w.data_ptr()), l.svr_linear_bwd_data_f16x3_workspace(N, K), w.device)
            check(l.svr_linear_bwd_data_f16x3(z, 0, C.c_void_p(w.data_ptr()), w.stride(0), z, 0, 0, N, K, EPI_NONE, z, 0, z, z,
                                              _p(ws), _stream()), "linear_bwd_data_f16x3 prepare")
            self._valid[("lbh", w.data_ptr())] = (w._version, len(self._events))

    def add_mlp_tail(self, w1, w2):
        """w1, w2 (256,256): the planes of the fused fc_1 -> fc_2 -> fc_out kernel (mlp_tail_fwd), one workspace for both; False
        (nothing added) where mlp_tail_fwd would run the three ops."""
        _f32(w1, w2)
        hidden = w1.shape[1]
        if _mlp_tail_op(None, hidden, w1, w2, None, None) != "mlp_tail_f16x3":
            return False
        l = _lib.lib()
        z = C.c_void_p(0)
        ws = self._buf(("mt", w1.data_ptr()), l.svr_mlp_tail_fwd_workspace(hidden), w1.device)
        check(l.svr_mlp_tail_fwd(z, 0, C.c_void_p(w1.data_ptr()), z, C.c_void_p(w2.data_ptr()), z, z, z, z, 0, z, 0, z, z, 0, hidden,
                                 _p(ws), _stream()), "mlp_tail_fwd prepare")
        self._ws[("mt2", w2.data_ptr())] = ws      # found by either matrix; mlp_tail_fwd wants both to name this buffer
        self._valid[("mt", w1.data_ptr())] = (w1._version, len(self._events))
        self._valid[("mt2", w2.data_ptr())] = (w2._version, len(self._events))
        return True

    def mark(self, stream):
        """An event behind the planes added so far: a lookup waits for the event of ITS planes only (the forward pass does not
        wait for the backward planes -- 54 launch-bound kernels per step, 0.5 ms of side-stream time)."""
        ev = torch.cuda.Event()
        ev.record(stream)
        self._events.append(ev)

    def finish(self, stream):
        self.mark(stream)
        self.ready = self._events[-1]

    def invalidate(self):
        self._valid.clear()

    def lookup(self, kind, w):
        """The prepared workspace of `w` for `kind` ("cf" / "cb" / "lf" / "lb"; "mt" / "mt2": the fused tail's, found by fc_1's /
        fc_2's matrix), or None.  The first hit of a step makes the calling stream wait for the preparation (the step's later work
        on other streams is ordered behind it)."""
        key = (kind, w.data_ptr())
        ver, idx = self._valid.get(key, (-1, 0))
        if ver != w._version or idx >= len(self._events):      # not prepared, or modified in place since (an optimizer step)
            return None
        cur = torch.cuda.current_stream()
        if (idx, cur.cuda_stream) not in self._waited:     # once per event and stream
            cur.wait_event(self._events[idx])
            self._waited.add((idx, cur.cuda_stream))
        return self._ws[key]


_prepared = None     # the PreparedWeights of the training step in flight (model/ifnet.py), or None


def set_prepared(p):
    global _prepared
    _prepared = p


def _lookup(kind, w, mode, default):
    if _prepared is None or (mode is not None and mode != default):
        return None
    return _prepared.lookup(kind, w)


# ---- which entry point a linear op reaches, and what that entry point does with the call ---------------------------------
# The three ops below and linear_variant() take the entry point from the same _linear_*_op functions; the kernel, epilogue
# form, splits and refusal come from the library (svr_linear_variant: the function its launchers call).
LINEAR_OPS = {"fwd_f32": 0, "fwd_f16x3": 1, "fwd_bf16x6": 2, "bwd_data_f32": 3, "bwd_data_f16x3s": 4, "bwd_data_bf16x3": 5,
              "bwd_weight_f32": 6, "bwd_weight_f16x3s": 7, "bwd_weight_bf16x3": 8}      # SVR_LIN_* of svr_hip.h
LINEAR_KERNELS = ("nt", "nn", "tn", "nt128", "nt64", "nt128_bwd", "nn_x3", "tn_tr", "tn_prepass", "nt_x6")      # SVR_LIN_K_*
LINEAR_BIAS_FORMS = ("none", "kernel", "colsum_vec", "colsum_slow")      # SVR_LIN_BIAS_*


def operand_layout(t):
    """(leading dimension, low four address bits, unit column stride) of a 2-D operand; None -> None."""
    return None if t is None else (t.stride(0), t.data_ptr() & 15, t.stride(1) == 1)


def _al16(lay):
    """Rows a kernel may move as float4: unit column stride, leading dimension a multiple of 4, 16-byte aligned start."""
    return lay is None or (lay[2] and lay[0] % 4 == 0 and lay[1] == 0)


def _linear_fwd_op(mode, K):
    mode = mode or FORWARD_GEMM
    return "fwd_" + mode if mode in ("f16x3", "bf16x6") and K % 16 == 0 else "fwd_f32"


MLP_TAIL_HIDDEN = 256      # the width mlp_tail.hip is built for


def _mlp_tail_op(mode, hidden, w1, w2, wo, h0):
    """fc_1 -> fc_2 -> fc_out: "mlp_tail_f16x3" (svr_mlp_tail_fwd, one kernel) for the default arithmetic at the width the
    kernel is built for and operands it can move as float4; "three_ops" (linear_fwd twice, fc_out_fwd) for everything else.
    w1, w2, wo: the tensors (wo None: not known yet); h0: operand_layout() of the input (None: contiguous and aligned)."""
    mode = mode or FORWARD_GEMM
    if (mode == "f16x3" and hidden == MLP_TAIL_HIDDEN and tuple(w1.shape) == (hidden, hidden) and tuple(w2.shape) == (hidden, hidden)
            and w1.is_contiguous() and w2.is_contiguous() and (wo is None or (wo.is_contiguous() and wo.data_ptr() % 16 == 0))
            and _al16(h0)):
        return "mlp_tail_f16x3"
    return "three_ops"


def _linear_bwd_data_op(mode, N, dy, out, mask):
    mode = mode or BACKWARD_GEMM
    if mode == "f16x3s":      # (shapes and layouts the f16 kernels do not take: exact f32, never a narrower split)
        return "bwd_data_f16x3s" if N % 16 == 0 and _al16(dy) and _al16(out) and _al16(mask) else "bwd_data_f32"
    if mode == "bf16x3" and N % 32 == 0 and out[1] == 0 and (mask is None or mask[1] == 0):      # (its float4 epilogue; else f32)
        return "bwd_data_bf16x3"
    return "bwd_data_f32"


def _linear_bwd_weight_op(mode, M, N, K, dy, x):
    mode = mode or BACKWARD_GEMM
    if mode == "f16x3s":
        return "bwd_weight_f16x3s" if N % 4 == 0 and K % 4 == 0 and N >= 4 and K >= 4 and M > 0 and _al16(dy) and _al16(x) else "bwd_weight_f32"
    return "bwd_weight_bf16x3" if mode == "bf16x3" and N % 4 == 0 else "bwd_weight_f32"


def linear_variant(kind, mode, M, N, K, a=None, b=None, out=None, mask=None, epilogue=None, want_bias=False):
    """What linear_fwd / linear_bwd_data / linear_bwd_weight (kind "fwd" / "bwd_data" / "bwd_weight") do with a call in `mode`:
    {"op" (the entry point, a LINEAR_OPS key), "kernel" (LINEAR_KERNELS), "coalesced", "splits", "rows_per_split", "bias"
    (LINEAR_BIAS_FORMS), "status" (0 or the SVR_E_* the entry point refuses with)}.  x (M,K), w (N,K), dy (M,N); a / b / out /
    mask: operand_layout() of the first operand (x; dy backward), the second (w; x of bwd_weight), the output and the mask,
    None = contiguous and aligned (mask: none).  Host only, no GPU needed."""
    cont = {"fwd": (K, K, N), "bwd_data": (N, K, K), "bwd_weight": (N, K, K)}[kind]
    a, b, out = [(ld, 0, True) if lay is None else lay for lay, ld in zip((a, b, out), cont)]
    if kind == "fwd":
        op = _linear_fwd_op(mode, K)
    elif kind == "bwd_data":
        op = _linear_bwd_data_op(mode, N, a, out, mask)
    else:
        op = _linear_bwd_weight_op(mode, M, N, K, a, b)
    if epilogue is None:
        epilogue = EPI_MASK if mask is not None else EPI_NONE
    m = mask if mask is not None else (0, 0, True)
    i32 = [C.c_int32() for _ in range(5)]
    rows = C.c_int64()
    kernel, coalesced, splits, bias, status = i32
    check(_lib.lib().svr_linear_variant(LINEAR_OPS[op], M, N, K, a[0], b[0], out[0], m[0], a[1], b[1], out[1], m[1], epilogue,
                                        int(want_bias), C.byref(kernel), C.byref(coalesced), C.byref(splits), C.byref(rows),
                                        C.byref(bias), C.byref(status)), "linear_variant")
    return {"op": op, "kernel": LINEAR_KERNELS[kernel.value] if kernel.value >= 0 else None, "coalesced": bool(coalesced.value),
            "splits": splits.value, "rows_per_split": rows.value, "bias": LINEAR_BIAS_FORMS[bias.value], "status": status.value}


def linear_fwd(x, w, bias, relu=True, out=None, mode=None):
    """y = [relu](x @ w.T + bias); x (M,K) row stride may exceed K (padded feature rows)."""
    _f32(x, w, bias)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    _f32(out)
    amax_forget(out)
    assert out.shape == (M, N) and out.stride(1) == 1      # a column slice of a wider buffer is fine: its row stride is passed
    epi = EPI_NONE if bias is None else (EPI_BIAS_RELU if relu else EPI_BIAS)
    op = _linear_fwd_op(mode, K)
    if op == "fwd_f16x3":
        l = _lib.lib()
        ws = _lookup("lf", w, mode, "f16x3") if w.stride(0) == K else None
        wptr = C.c_void_p(0) if ws is not None else C.c_void_p(w.data_ptr())      # W NULL: the workspace is prepared
        if ws is None:
            ws = torch.empty(l.svr_linear_fwd_f16x3_workspace(N, K), device=x.device, dtype=torch.uint8)
        check(l.svr_linear_fwd_f16x3(C.c_void_p(x.data_ptr()), x.stride(0), wptr, w.stride(0), _p(bias),
                                     _rp(out), out.stride(0), M, N, K, epi, _p(ws), _stream()), "linear_fwd_f16x3")
        return out
    if op == "fwd_bf16x6":
        l = _lib.lib()
        ws = torch.empty(l.svr_linear_fwd_bf16x6_workspace(N, K), device=x.device, dtype=torch.uint8)
        check(l.svr_linear_fwd_bf16x6(C.c_void_p(x.data_ptr()), x.stride(0), C.c_void_p(w.data_ptr()), w.stride(0), _p(bias),
                                      _rp(out), out.stride(0), M, N, K, epi, _p(ws), _stream()), "linear_fwd_bf16x6")
        return out
    check(_lib.lib().svr_linear_fwd(C.c_void_p(x.data_ptr()), x.stride(0), C.c_void_p(w.data_ptr()), w.stride(0),
                                    _p(bias), _rp(out), out.stride(0), M, N, K, epi, C.c_void_p(0), 0, _stream()),
          "linear_fwd")
    return out


def mlp_tail_fwd(h0, w1, b1, w2, b2, wo, bo, row_map=None):
    """(h1, h2, logits) = relu(h0 @ w1.T + b1), relu(h1 @ w2.T + b2), fc_out(h2) scattered by row_map: the fused kernel of
    mlp_tail.hip where _mlp_tail_op says so, else the three calls -- the same bits either way."""
    _f32(h0, w1, b1, w2, b2, wo, bo)
    M, K = h0.shape
    assert w1.shape == (w1.shape[0], K) and w2.shape == (w2.shape[0], w1.shape[0]) and h0.stride(1) == 1
    if _mlp_tail_op(None, K, w1, w2, wo, operand_layout(h0)) != "mlp_tail_f16x3":
        h1 = linear_fwd(h0, w1, b1, relu=True)
        h2 = linear_fwd(h1, w2, b2, relu=True)
        return h1, h2, fc_out_fwd(h2, wo, bo, row_map)
    l = _lib.lib()
    h1 = torch.empty(M, K, device=h0.device, dtype=torch.float32)
    h2 = torch.empty(M, K, device=h0.device, dtype=torch.float32)
    logits = torch.empty(M, device=h0.device, dtype=torch.float32)
    ws = _lookup("mt", w1, None, "f16x3")
    if ws is not None and _lookup("mt2", w2, None, "f16x3") is not ws:      # (the planes of this w1 were made with another w2)
        ws = None
    z = C.c_void_p(0)
    wp1, wp2 = (z, z) if ws is not None else (C.c_void_p(w1.data_ptr()), C.c_void_p(w2.data_ptr()))      # W NULL: prepared
    if ws is None:
        ws = torch.empty(l.svr_mlp_tail_fwd_workspace(K), device=h0.device, dtype=torch.uint8)
    check(l.svr_mlp_tail_fwd(C.c_void_p(h0.data_ptr()), h0.stride(0), wp1, _p(b1), wp2, _p(b2), _p(wo), _p(bo), _p(h1), K, _p(h2), K,
                             _p(logits), _p(row_map), M, K, _p(ws), _stream()), "mlp_tail_fwd")
    return h1, h2, logits


# Arithmetic of the two backward GEMMs of the point MLP: "f16x3s" (DEFAULT since round 4: the SCALED 3-product f16 split --
# gradient operands brought into f16's range by an exact power of two taken from their |max|, 22 mantissa bits per operand =
# f32 level like the reference's fp32 backward, the same three matrix instructions per block; gemm_f16x3.hip /
# gemm_bf16x3.hip), "bf16x3" (3-term bf16 split, ~1.5e-5 relative per product: 4 % faster per step, the default of rounds
# 1-3; SVR_BACKWARD=bf16x3) or "f32" (exact-f32 MFMA).  The forward never uses them.
BACKWARD_MODES = ("bf16x3", "f16x3s", "f32")
BACKWARD_GEMM = os.environ.get("SVR_BACKWARD", "f16x3s")      # read once, here: BACKWARD_CONV / BACKWARD_CONV_WEIGHT start from it
if BACKWARD_GEMM not in BACKWARD_MODES:      # (a typo used to mean exact f32 everywhere, under whatever label it carried)
    raise ValueError(f"SVR_BACKWARD={BACKWARD_GEMM!r}: one of {BACKWARD_MODES}")


class _AmaxSlots:
    """Zero-initialised int32 words for the atomic-maximum outputs of the "f16x3s" kernels, without a memset launch and an
    allocator call per word: one ring of 512 words per (device, stream), its halves zeroed alternately by ONE fill each
    time the ring enters them -- a half is reused ~250 words (several training steps) after its words were handed out, by
    when the tensors that referred to them are gone.  A word is produced and zeroed on the stream that owns the ring; a
    consumer on another stream is ordered behind the producer by the same event that orders it behind the tensor itself."""
    N = 512

    def __init__(self):
        self._rings = {}

    def take(self, device):
        if torch.cuda.is_current_stream_capturing():      # a replayed graph must zero its words itself
            return torch.zeros(1, device=device, dtype=torch.int32)
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        r = self._rings.get(key)
        if r is None:
            r = self._rings[key] = {"buf": torch.zeros(self.N, device=device, dtype=torch.int32), "i": 0}
        i = r["i"]
        if i % (self.N // 2) == 0 and (i or r.get("lap")):    # entering a half whose words were used a lap ago
            r["buf"][i:i + self.N // 2].zero_()
        r["i"] = (i + 1) % self.N
        if r["i"] == 0:
            r["lap"] = True
        r["serial"] = r.get("serial", 0) + 1
        w = r["buf"][i:i + 1]
        w._svr_ring, w._svr_serial = r, r["serial"]       # (how old the word is: fresh() below)
        return w

    @staticmethod
    def fresh(w):
        """Is this word still the one that was handed out?  (A gradient tensor kept across many steps and fed to a later
        backward would otherwise be scaled by whatever the recycled word holds by then.)"""
        r = getattr(w, "_svr_ring", None)
        return r is None or r["serial"] - w._svr_serial < _AmaxSlots.N // 2 - 8


_amax_slots = _AmaxSlots()


def amax_slot(device):
    """A zeroed (1,) int32 word for an amax output."""
    return _amax_slots.take(device)


def _amax_stamp(t):
    """What a remembered |max| word is valid for: (version counter, storage address) of the tensor when the word was taken."""
    try:
        return (t._version, t.data_ptr())
    except RuntimeError:      # an inference tensor keeps no version counter: nothing to check a word against, never reused
        return None


def amax_remember(t, a):
    """Leave the word `a` (max |t| as t stands NOW) on the tensor object, stamped with t's version counter and address."""
    t._svr_amax = a
    t._svr_amax_stamp = _amax_stamp(t)


def amax_forget(t):
    """Drop the |max| word remembered on `t` (None: nothing to do).  For a caller that has written into t behind torch's
    back -- through `t.data`, or from a kernel of its own with the raw pointer -- and for every op here that does so."""
    if t is not None and getattr(t, "_svr_amax", None) is not None:
        t.__dict__.pop("_svr_amax", None)
        t.__dict__.pop("_svr_amax_stamp", None)


def amax_cached(t, force=False):
    """The word remembered on `t` if it may stand for t's present contents, else None.  Host only: reads attributes of the
    tensor object, never the device (tests/test_amax_cache_cpu.py runs it on CPU tensors).  A hit needs all of:
      - a word and its stamp on this tensor object (a new view or slice of the same memory is another object: miss);
      - the stamp equal to (t._version, t.data_ptr()) now: every in-place op torch knows of -- copy_, mul_, add_ (autograd's
        in-place accumulation of a second gradient contribution), t[...] = ..., _foreach_*, a write through a view of t (views
        share the counter), set_ -- moves the counter, and `t.data = other` moves the address;
      - the word not older than the ring allows (_AmaxSlots.fresh);
      - not `force`."""
    a = getattr(t, "_svr_amax", None)
    if a is None or force:
        return None
    stamp = getattr(t, "_svr_amax_stamp", None)
    if stamp is None or stamp != _amax_stamp(t) or not _AmaxSlots.fresh(a):
        return None
    return a


def amax_of(t, force=False):
    """(1,) int32 tensor = bit pattern of max |t| on the device (the power-of-two scale of a gradient operand of the
    "f16x3s" kernels).  Kernels that produce a gradient leave it on the tensor they return (attribute `_svr_amax`: no extra
    pass); otherwise one pass over t on the current stream, remembered on the tensor object -- the two products of one dy
    share one pass.  The remembered word is reused only while amax_cached() holds: it is stamped with the tensor's version
    counter and address, and recomputed after any in-place change torch has seen.
    What the stamp CANNOT see: a write through `t.data` (a detached alias with a counter of its own) and a write by a kernel
    outside this module that was handed the raw pointer.  After either, call amax_forget(t) or amax_of(t, force=True) before
    the next op that consumes t; otherwise t is scaled by its earlier contents' |max| (overflow to inf / NaN when it grew
    by more than ~4x, lost mantissa bits or zeros when it shrank)."""
    a = amax_cached(t, force)
    if a is not None:
        return a
    _f32(t)
    a = amax_slot(t.device)
    if t.dim() == 2 and t.stride(1) == 1 and t.shape[1] % 4 == 0 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        M, N, ld, src = t.shape[0], t.shape[1], t.stride(0), t
    else:
        src = t if t.is_contiguous() else t.contiguous()
        n = src.numel()
        if n % 4 or src.data_ptr() % 16:
            raise RuntimeError("amax_of: tensor must have a multiple of 4 elements and be 16-byte aligned")
        M, N, ld = n // 4, 4, 4
    check(_lib.lib().svr_amax_f32(C.c_void_p(src.data_ptr()), ld, M, N, _p(a), _stream()), "amax_f32")
    amax_remember(t, a)
    return a


def linear_bwd_data(dy, w, mask=None, out=None, mode=None):
    """dx = (dy @ w) [* (mask > 0)]; dy (M,N), w (N,K)."""
    _f32(dy, w, mask)
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, device=dy.device, dtype=torch.float32)
    epi = EPI_MASK if mask is not None else EPI_NONE
    op = _linear_bwd_data_op(mode, N, operand_layout(dy), operand_layout(out), operand_layout(mask))
    amax_forget(out)      # (a caller's `out` is overwritten through its raw pointer; the f16x3s kernel leaves the new word)
    if op == "bwd_data_f16x3s":
        l = _lib.lib()
        ws = _lookup("lbh", w, mode, "f16x3s") if (w.stride(0) == K and w.stride(1) == 1) else None
        wptr = C.c_void_p(0) if ws is not None else C.c_void_p(w.data_ptr())      # W NULL: the workspace is prepared
        if ws is None:
            assert w.stride(1) == 1
            ws = torch.empty(l.svr_linear_bwd_data_f16x3_workspace(N, K), device=dy.device, dtype=torch.uint8)
        amax_dy = amax_of(dy)
        amax_dx = amax_slot(dy.device)
        check(l.svr_linear_bwd_data_f16x3(C.c_void_p(dy.data_ptr()), dy.stride(0), wptr, w.stride(0),
                                          C.c_void_p(out.data_ptr()), out.stride(0), M, N, K, epi,
                                          _rp(mask), mask.stride(0) if mask is not None else 0, _p(amax_dy), _p(amax_dx), _p(ws), _stream()),
              "linear_bwd_data_f16x3")
        amax_remember(out, amax_dx)    # |max| of what was stored: the next layer's scale, no extra pass
        return out
    if op == "bwd_data_bf16x3":
        l = _lib.lib()
        ws = _lookup("lb", w, mode, "bf16x3") if (w.stride(0) == K and w.stride(1) == 1) else None
        wptr = C.c_void_p(0) if ws is not None else C.c_void_p(w.data_ptr())      # W NULL: the workspace is prepared
        if ws is None:
            ws = torch.empty(l.svr_linear_bwd_data_bf16x3_workspace(N, K), device=dy.device, dtype=torch.uint8)
        check(l.svr_linear_bwd_data_bf16x3(C.c_void_p(dy.data_ptr()), dy.stride(0), wptr, w.stride(0),
                                           C.c_void_p(out.data_ptr()), out.stride(0), M, N, K, epi,
                                           _rp(mask), mask.stride(0) if mask is not None else 0, _p(ws), _stream()),
              "linear_bwd_data_bf16x3")
        return out
    check(_lib.lib().svr_linear_bwd_data(C.c_void_p(dy.data_ptr()), dy.stride(0), C.c_void_p(w.data_ptr()), w.stride(0),
                                         C.c_void_p(out.data_ptr()), out.stride(0), M, N, K, epi,
                                         _rp(mask), mask.stride(0) if mask is not None else 0, _stream()), "linear_bwd_data")
    return out


def linear_bwd_weight(dy, x, want_bias=True, mode=None):
    """dW (N,K) = dy.T @ x, db (N) = dy.sum(0)."""
    _f32(dy, x)
    M, N = dy.shape
    K = x.shape[1]
    l = _lib.lib()
    dw = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = torch.empty(N, device=dy.device, dtype=torch.float32) if want_bias else None
    op = _linear_bwd_weight_op(mode, M, N, K, operand_layout(dy), operand_layout(x))
    if op == "bwd_weight_f16x3s":
        ws = torch.empty(l.svr_linear_bwd_weight_f16x3_workspace(M, N, K), device=dy.device, dtype=torch.uint8)
        check(l.svr_linear_bwd_weight_f16x3(C.c_void_p(dy.data_ptr()), dy.stride(0), C.c_void_p(x.data_ptr()), x.stride(0),
                                            _p(dw), dw.stride(0), _p(db), M, N, K, _p(amax_of(dy)), _p(ws), _stream()),
              "linear_bwd_weight_f16x3")
        return dw, db
    if op == "bwd_weight_bf16x3":
        ws = torch.empty(l.svr_linear_bwd_weight_bf16x3_workspace(M, N, K), device=dy.device, dtype=torch.uint8)
        check(l.svr_linear_bwd_weight_bf16x3(C.c_void_p(dy.data_ptr()), dy.stride(0), C.c_void_p(x.data_ptr()), x.stride(0),
                                             _p(dw), dw.stride(0), _p(db), M, N, K, _p(ws), _stream()),
              "linear_bwd_weight_bf16x3")
        return dw, db
    ws = torch.empty(l.svr_linear_bwd_weight_workspace(M, N, K), device=dy.device, dtype=torch.uint8)
    check(l.svr_linear_bwd_weight(C.c_void_p(dy.data_ptr()), dy.stride(0), C.c_void_p(x.data_ptr()), x.stride(0),
                                  _p(dw), dw.stride(0), _p(db), M, N, K, _p(ws), _stream()), "linear_bwd_weight")
    return dw, db


def fc_out_fwd(h, w, b, row_map=None):
    """logits[row_map[m]] (or [m]) = h[m] . w + b"""
    _f32(h, w, b)
    M, K = h.shape
    out = torch.empty(M, device=h.device, dtype=torch.float32)
    check(_lib.lib().svr_fc_out_fwd(_p(h), h.stride(0), _p(w), _p(b), _p(out), _p(row_map), M, K, _stream()), "fc_out_fwd")
    return out


def fc_out_bwd(h, w, dlogits, row_map=None):
    _f32(h, w, dlogits)
    M, K = h.shape
    l = _lib.lib()
    ws = torch.empty(l.svr_fc_out_bwd_workspace(M, K), device=h.device, dtype=torch.uint8)
    dh = torch.empty(M, K, device=h.device, dtype=torch.float32)
    dw = torch.empty(K, device=h.device, dtype=torch.float32)
    db = torch.empty(1, device=h.device, dtype=torch.float32)
    amax = amax_slot(h.device) if BACKWARD_GEMM == "f16x3s" else None       # |max| of dh for the next layer's scaled split
    check(l.svr_fc_out_bwd(_p(h), h.stride(0), _p(w), _p(dlogits), _p(row_map), _p(dh), dh.stride(0), _p(dw), _p(db), M, K,
                           _p(amax), _p(ws), _stream()), "fc_out_bwd")
    if amax is not None:
        amax_remember(dh, amax)
    return dh, dw, db


def bce_logits_sum_mean(logits, targets, want_grad=True, gscale=1.0, ordered=False):
    """ordered: the per-sample sums in a fixed block order (svr_bce_logits_sum_mean_ordered) instead of float64 atomics."""
    _f32(logits, targets)
    B, N = logits.shape
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    dz = torch.empty_like(logits) if want_grad else None
    if ordered:
        l = _lib.lib()
        ws = torch.empty(int(l.svr_bce_ordered_workspace(B)) // 8, device=logits.device, dtype=torch.float64)
        check(l.svr_bce_logits_sum_mean_ordered(_p(logits), _p(targets), _p(loss), _p(dz), B, N, gscale, _p(ws), _stream()),
              "bce_ordered")
        return loss, dz
    ws = torch.empty(B, device=logits.device, dtype=torch.float64)
    check(_lib.lib().svr_bce_logits_sum_mean(_p(logits), _p(targets), _p(loss), _p(dz), B, N, gscale, _p(ws), _stream()),
          "bce")
    return loss, dz


# ------------------------------------------------------------------------------------------
# encoder: conv3d / batch-norm / max-pool (channels-last volumes (B,D,H,W,C))
# ------------------------------------------------------------------------------------------
def conv3d_pack_weight(w, want_bwd=True):
    """(Co,Ci,3,3,3) -> Wp_fwd [27][Ci][Co], Wp_bwd [27][Co][Ci] (taps flipped)."""
    _f32(w)
    Co, Ci = w.shape[0], w.shape[1]
    wf = torch.empty(27, Ci, Co, device=w.device, dtype=torch.float32)
    wb = torch.empty(27, Co, Ci, device=w.device, dtype=torch.float32) if want_bwd else None
    check(_lib.lib().svr_conv3d_pack_weight(_p(w), _p(wf), _p(wb), Ci, Co, _stream()), "conv3d_pack_weight")
    return wf, wb


def conv3d_unpack_wgrad(dwp, Ci, Co):
    dw = torch.empty(Co, Ci, 3, 3, 3, device=dwp.device, dtype=torch.float32)
    check(_lib.lib().svr_conv3d_unpack_wgrad(_p(dwp), _p(dw), Ci, Co, _stream()), "conv3d_unpack_wgrad")
    return dw


def conv3d_k3(x, wp, bias=None, relu=False, mask=None):
    """x (B,D,H,W,Ci), wp [27][Ci][Co] -> (B,D,H,W,Co); epilogue: bias[+relu] or mask or none."""
    _f32(x, wp, bias, mask)
    B, D, H, W, Ci = x.shape
    Co = wp.shape[2]
    assert wp.shape[1] == Ci
    out = torch.empty(B, D, H, W, Co, device=x.device, dtype=torch.float32)
    if mask is not None:
        epi = EPI_MASK
    elif bias is not None:
        epi = EPI_BIAS_RELU if relu else EPI_BIAS
    else:
        epi = EPI_NONE
    check(_lib.lib().svr_conv3d_k3(_p(x), _p(wp), _p(bias), _p(out), B, D, H, W, Ci, Co, epi, _p(mask), _stream()), "conv3d_k3")
    return out


# Arithmetic of the encoder's backward-data convolutions: "bf16x3" (conv3d_bf16.hip) or "f32".
BACKWARD_CONV = BACKWARD_GEMM     # "bf16x3", "f16x3s" (scaled f16 split: f32 level) or "f32"
# ... and of its forward convolutions: "f16x3" (3-product f16 split, f32-level accuracy for |x| < 65504), "bf16x6"
# (6-product bf16 split, any f32 range) or "f32" (exact-f32 MFMA)
FORWARD_CONV = "f16x3"


class StatParts:
    """Per-workgroup partial sums (sum, sum of squares; float64 [blocks][2][C]) of a tensor a kernel has just written: the
    BatchNorm that follows finalizes from them (bn_forward(stats=...)) instead of reading the tensor again."""

    def __init__(self, part, blocks):
        self.part, self.blocks = part, blocks


def conv3d_k3_fwd(x, w, bias, relu=True, mode=None, want_stats=False):
    """relu(conv(x (B,D,H,W,Ci), w (Co,Ci,3,3,3)) + bias) -> (B,D,H,W,Co).  want_stats: -> (out, StatParts or None): the
    BatchNorm statistics of the output come out of the kernel's epilogue where the f16x3 kernel runs."""
    _f32(x, w, bias)
    B, D, H, W, Ci = x.shape
    Co = w.shape[0]
    if (mode or FORWARD_CONV) == "f16x3" and Ci % 16 == 0:
        l = _lib.lib()
        out = torch.empty(B, D, H, W, Co, device=x.device, dtype=torch.float32)
        ws = _lookup("cf", w, mode, "f16x3")
        wptr = C.c_void_p(0) if ws is not None else _p(w)                          # W NULL: the workspace is prepared
        if ws is None:
            ws = torch.empty(l.svr_conv3d_fwd_f16x3_workspace(Ci, Co), device=x.device, dtype=torch.uint8)
        epi = EPI_BIAS_RELU if relu else EPI_BIAS
        if want_stats:
            blocks = l.svr_conv3d_fwd_f16x3_stats_blocks(B, D, H, W, Ci, Co)
            part = torch.empty(blocks, 2, Co, device=x.device, dtype=torch.float64)
            check(l.svr_conv3d_k3_fwd_f16x3_stats(_p(x), wptr, _p(bias), _p(out), _p(part), B, D, H, W, Ci, Co, epi, _p(ws),
                                                  _stream()), "conv3d_fwd_f16x3_stats")
            return out, StatParts(part, blocks)
        check(l.svr_conv3d_k3_fwd_f16x3(_p(x), wptr, _p(bias), _p(out), B, D, H, W, Ci, Co, epi, _p(ws), _stream()),
              "conv3d_fwd_f16x3")
        return out
    if want_stats:
        return conv3d_k3_fwd(x, w, bias, relu, mode), None
    if (mode or FORWARD_CONV) == "bf16x6" and Ci % 16 == 0:
        l = _lib.lib()
        out = torch.empty(B, D, H, W, Co, device=x.device, dtype=torch.float32)
        ws = torch.empty(l.svr_conv3d_fwd_bf16x6_workspace(Ci, Co), device=x.device, dtype=torch.uint8)
        check(l.svr_conv3d_k3_fwd_bf16x6(_p(x), _p(w), _p(bias), _p(out), B, D, H, W, Ci, Co,
                                         EPI_BIAS_RELU if relu else EPI_BIAS, _p(ws), _stream()), "conv3d_fwd_bf16x6")
        return out
    wf, _ = conv3d_pack_weight(w, want_bwd=False)
    return conv3d_k3(x, wf, bias, relu=relu)


def conv3d_c1_fwd_stats(x, w, bias, relu=True):
    """conv_in (Ci == 1) forward + the BatchNorm statistics of its output: (out, stats float64 [mean | biased var])."""
    _f32(x, w, bias)
    B, D, H, W, Ci = x.shape
    Co = w.shape[0]
    assert Ci == 1 and Co in (16, 32)
    wf, _ = conv3d_pack_weight(w, want_bwd=False)
    l = _lib.lib()
    out = torch.empty(B, D, H, W, Co, device=x.device, dtype=torch.float32)
    stats = torch.empty(2 * Co, device=x.device, dtype=torch.float64)
    ws = torch.empty(l.svr_conv3d_c1_fwd_stats_workspace(B, D, H, W, Co), device=x.device, dtype=torch.uint8)
    check(l.svr_conv3d_c1_fwd_stats(_p(x), _p(wf), _p(bias), _p(out), _p(stats), B, D, H, W, Co,
                                    EPI_BIAS_RELU if relu else EPI_BIAS, _p(ws), _stream()), "conv3d_c1_fwd_stats")
    return out, stats


def conv3d_k3_bwd_data(dout, w, mask=None, mode=None):
    """din (B,D,H,W,Ci) = conv^T(dout (B,D,H,W,Co), w (Co,Ci,3,3,3)) [* (mask > 0)]."""
    _f32(dout, w, mask)
    B, D, H, W, Co = dout.shape
    Ci = w.shape[1]
    assert w.shape[0] == Co
    if (mode or BACKWARD_CONV) == "f16x3s" and Ci % 2 == 0 and Co % 16 == 0 and dout.is_contiguous() and dout.numel() % 4 == 0:
        l = _lib.lib()
        din = torch.empty(B, D, H, W, Ci, device=dout.device, dtype=torch.float32)
        ws = _lookup("cbh", w, mode, "f16x3s")
        wptr = C.c_void_p(0) if ws is not None else _p(w)                          # W NULL: the workspace is prepared
        if ws is None:
            ws = torch.empty(l.svr_conv3d_bwd_data_f16x3_workspace(Ci, Co), device=dout.device, dtype=torch.uint8)
        amax_din = amax_slot(dout.device)
        check(l.svr_conv3d_k3_bwd_data_f16x3(_p(dout), wptr, _p(din), B, D, H, W, Ci, Co,
                                             EPI_MASK if mask is not None else EPI_NONE, _p(mask), _p(amax_of(dout)), _p(amax_din),
                                             _p(ws), _stream()), "conv3d_bwd_data_f16x3")
        amax_remember(din, amax_din)
        return din
    if (mode or BACKWARD_CONV) == "f16x3s":
        mode = "f32"                   # (shapes the f16 kernel does not take: exact f32, never a narrower split)
    if (mode or BACKWARD_CONV) == "bf16x3" and Ci % 2 == 0 and Co % 16 == 0:
        l = _lib.lib()
        din = torch.empty(B, D, H, W, Ci, device=dout.device, dtype=torch.float32)
        ws = _lookup("cb", w, mode, "bf16x3")
        wptr = C.c_void_p(0) if ws is not None else _p(w)                          # W NULL: the workspace is prepared
        if ws is None:
            ws = torch.empty(l.svr_conv3d_bwd_data_bf16x3_workspace(Ci, Co), device=dout.device, dtype=torch.uint8)
        check(l.svr_conv3d_k3_bwd_data_bf16x3(_p(dout), wptr, _p(din), B, D, H, W, Ci, Co,
                                              EPI_MASK if mask is not None else EPI_NONE, _p(mask), _p(ws), _stream()),
              "conv3d_bwd_data_bf16x3")
        return din
    _, wb = conv3d_pack_weight(w, want_bwd=True)
    return conv3d_k3(dout, wb, mask=mask)


CONV_VARIANT_OPS = {"fwd_f16x3": 0, "bwd_data_f16x3s": 1, "bwd_data_bf16x3": 2, "fwd_bf16x6": 3}      # SVR_CONV_* of svr_hip.h


def conv3d_k3_variant(op, B, dims, Ci, Co):
    """The kernel instantiation the split-precision 3x3x3 entry point `op` (a key of CONV_VARIANT_OPS) takes for
    (B, *dims, Ci -> Co): {"ck", "tn", "vt", "persistent", "workgroup_rows"} (svr_conv3d_k3_variant; host only, no GPU needed)."""
    D, H, W = dims
    ck, tn, vt, pers, rows = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    check(_lib.lib().svr_conv3d_k3_variant(CONV_VARIANT_OPS[op], B, D, H, W, Ci, Co, C.byref(ck), C.byref(tn), C.byref(vt),
                                           C.byref(pers), C.byref(rows)), "conv3d_k3_variant")
    return {"ck": ck.value, "tn": tn.value, "vt": vt.value, "persistent": bool(pers.value), "workgroup_rows": rows.value}


WGRAD_VARIANT_OPS = {"bwd_weight_f32": 0, "bwd_weight_f16x3s": 1, "bwd_weight_bf16x3": 2}      # SVR_CONV_BWD_WEIGHT_* of svr_hip.h
WGRAD_KERNELS = ("C1_CO16_LDS", "C1_CO16", "C1", "BRICK", "WS_PAIR", "WS", "X3")                # SVR_WGRAD_*


def conv3d_k3_bwd_weight_variant(op, B, dims, Ci, Co):
    """The kernel the 3x3x3 weight-gradient entry point `op` (a key of WGRAD_VARIANT_OPS) runs for (B, *dims, Ci -> Co):
    {"kernel" (a name of WGRAD_KERNELS), "parts", "max_bricks_per_part"} (svr_conv3d_k3_bwd_weight_variant; host only, no GPU
    needed).  A shape the entry point refuses raises with its error code, as the entry point would."""
    D, H, W = dims
    kernel, parts, per = C.c_int32(), C.c_int32(), C.c_int64()
    check(_lib.lib().svr_conv3d_k3_bwd_weight_variant(WGRAD_VARIANT_OPS[op], B, D, H, W, Ci, Co, C.byref(kernel), C.byref(parts),
                                                      C.byref(per)), "conv3d_k3_bwd_weight_variant")
    return {"kernel": WGRAD_KERNELS[kernel.value], "parts": parts.value, "max_bricks_per_part": per.value}


# Arithmetic of the encoder's weight gradients: "bf16x3" (conv3d_bwdw_bf16.hip), "f16x3s" (its scaled f16 form: f32 level)
# or "f32" (exact-f32 MFMA)
BACKWARD_CONV_WEIGHT = BACKWARD_GEMM


def conv3d_k3_bwd_weight(x, dout, want_bias=True, mode=None, param_layout=False):
    """dWp [27][Ci][Co], db (Co).  param_layout: the weight gradient in the parameter's layout (Co,Ci,3,3,3) instead (the
    bf16x3 kernel writes it directly; the other paths unpack)."""
    _f32(x, dout)
    B, D, H, W, Ci = x.shape
    Co = dout.shape[4]
    l = _lib.lib()
    # the split-precision kernel's 32-bit offsets inside one sample (conv3d_bwdw_bf16.hip); larger volumes take the f32 kernel
    fits = D * H * W <= (1 << 24) and D * H * W * max(Ci, Co) < (1 << 30)
    if not fits and (mode or BACKWARD_CONV_WEIGHT) in ("bf16x3", "f16x3s"):
        mode = "f32"
    if (mode or BACKWARD_CONV_WEIGHT) == "f16x3s" and Ci % 4 == 0 and Co % 4 == 0 and dout.is_contiguous() and dout.numel() % 4 == 0:
        ws = torch.empty(l.svr_conv3d_k3_bwd_weight_bf16x3_workspace(B, D, H, W, Ci, Co), device=x.device, dtype=torch.uint8)
        dw = torch.empty((Co, Ci, 3, 3, 3) if param_layout else (27, Ci, Co), device=x.device, dtype=torch.float32)
        db = torch.empty(Co, device=x.device, dtype=torch.float32) if want_bias else None
        check(l.svr_conv3d_k3_bwd_weight_f16x3(_p(x), _p(dout), _p(dw), _p(db), B, D, H, W, Ci, Co, 1 if param_layout else 0,
                                               _p(amax_of(dout)), _p(ws), _stream()), "conv3d_k3_bwd_weight_f16x3")
        return dw, db
    if (mode or BACKWARD_CONV_WEIGHT) == "f16x3s":
        mode = "f32"
    if (mode or BACKWARD_CONV_WEIGHT) == "bf16x3" and Ci % 4 == 0 and Co % 4 == 0 and param_layout:
        ws = torch.empty(l.svr_conv3d_k3_bwd_weight_bf16x3_workspace(B, D, H, W, Ci, Co), device=x.device, dtype=torch.uint8)
        dw = torch.empty(Co, Ci, 3, 3, 3, device=x.device, dtype=torch.float32)
        db = torch.empty(Co, device=x.device, dtype=torch.float32) if want_bias else None
        check(l.svr_conv3d_k3_bwd_weight_bf16x3_param(_p(x), _p(dout), _p(dw), _p(db), B, D, H, W, Ci, Co, _p(ws), _stream()),
              "conv3d_k3_bwd_weight_bf16x3_param")
        return dw, db
    if param_layout:
        dwp, db = conv3d_k3_bwd_weight(x, dout, want_bias, mode)
        return conv3d_unpack_wgrad(dwp, Ci, Co), db
    if (mode or BACKWARD_CONV_WEIGHT) == "bf16x3" and Ci % 4 == 0 and Co % 4 == 0:
        ws = torch.empty(l.svr_conv3d_k3_bwd_weight_bf16x3_workspace(B, D, H, W, Ci, Co), device=x.device, dtype=torch.uint8)
        dwp = torch.empty(27, Ci, Co, device=x.device, dtype=torch.float32)
        db = torch.empty(Co, device=x.device, dtype=torch.float32) if want_bias else None
        check(l.svr_conv3d_k3_bwd_weight_bf16x3(_p(x), _p(dout), _p(dwp), _p(db), B, D, H, W, Ci, Co, _p(ws), _stream()),
              "conv3d_k3_bwd_weight_bf16x3")
        return dwp, db
    ws = torch.empty(l.svr_conv3d_k3_bwd_weight_workspace(B, D, H, W, Ci, Co), device=x.device, dtype=torch.uint8)
    dwp = torch.empty(27, Ci, Co, device=x.device, dtype=torch.float32)
    db = torch.empty(Co, device=x.device, dtype=torch.float32) if want_bias else None
    check(l.svr_conv3d_k3_bwd_weight(_p(x), _p(dout), _p(dwp), _p(db), B, D, H, W, Ci, Co, _p(ws), _stream()),
          "conv3d_k3_bwd_weight")
    return dwp, db


def bn_forward(x, gamma, beta, running_mean, running_var, training, eps=1e-5, momentum=0.1, want_pool=True, stats=None):
    """x (B,D,H,W,C) -> y, pooled, argmax, scale_shift(3C), mean.  `stats` (float64 [mean | biased var]): statistics
    of x already computed by the producer (conv3d_c1_fwd_stats); the statistics pass over x is then skipped.
    mean (for bn_backward): the f32 mean (C), and behind it, where the statistics were taken from x here, what the
    rounding to f32 left (2C in all): the backward centres x with both, so xhat stays accurate where |mean| >> std."""
    _f32(x, gamma, beta, running_mean, running_var)
    B, D, H, W, Cc = x.shape
    rows = B * D * H * W
    if training and rows <= 1:
        # same error as torch.nn.functional.batch_norm (the reference raises here too)
        raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                         f"torch.Size([{B}, {Cc}, {D}, {H}, {W}])")
    l = _lib.lib()
    dev = x.device
    amax_forget(running_mean)      # (training: the running statistics are updated through their raw pointers)
    amax_forget(running_var)
    ss = torch.empty(3 * Cc, device=dev, dtype=torch.float32)
    own_stats = training and stats is None
    mean = torch.empty(2 * Cc if own_stats else Cc, device=dev, dtype=torch.float32)
    mean_lo = C.c_void_p(mean.data_ptr() + 4 * Cc) if own_stats else C.c_void_p(0)      # (no view: host time per layer)
    if training and isinstance(stats, StatParts):      # partial sums from the producing kernel's epilogue: one launch
        check(l.svr_bn_finalize_parts(_p(stats.part), stats.blocks, C.c_void_p(0), _p(gamma), _p(beta), _p(running_mean),
                                      _p(running_var), _p(ss), _p(mean), C.c_void_p(0), rows, Cc, eps, momentum, _stream()),
              "bn_finalize_parts")
    elif own_stats:                       # statistics + finalize: two launches
        ws = torch.empty(l.svr_bn_stats_workspace(rows, Cc), device=dev, dtype=torch.uint8)
        check(l.svr_bn_stats_finalize(_p(x), C.c_void_p(0), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(ss), _p(mean),
                                      mean_lo, rows, Cc, eps, momentum, _p(ws), _stream()), "bn_stats_finalize")
    else:
        check(l.svr_bn_finalize(_p(stats if training else None), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(ss),
                                _p(mean), rows, Cc, eps, momentum, int(training), _stream()), "bn_finalize")
    y = torch.empty_like(x)
    pooled = argmax = None
    if want_pool:
        pooled = torch.empty(B, D // 2, H // 2, W // 2, Cc, device=dev, dtype=torch.float32)
        argmax = torch.empty(B, D // 2, H // 2, W // 2, Cc, device=dev, dtype=torch.uint8)
    # statistics taken from x here (any mean: the UNet's BatchNorm follows a convolution, not a ReLU): the centred apply
    check(l.svr_bn_apply_pool(_p(x), _p(ss), _p(mean if own_stats else None), mean_lo, _p(beta if own_stats else None), _p(y),
                              _p(pooled), _p(argmax), B, D, H, W, Cc, _stream()), "bn_apply_pool")
    return y, pooled, argmax, ss, mean


def bn_backward(x, dy, dpooled, argmax, mean, ss, relu_mask=True, training=True):
    """-> dx (grad wrt the conv pre-activation when relu_mask), dgamma, dbeta.  training=False: the forward normalised
    with the running statistics (eval mode), so dx has no batch-mean terms."""
    _f32(x, dy, dpooled, mean, ss)
    B, D, H, W, Cc = x.shape
    l = _lib.lib()
    dev = x.device
    sums = torch.empty(2 * Cc, device=dev, dtype=torch.float64)
    ws = torch.empty(l.svr_bn_stats_workspace(B * D * H * W, Cc), device=dev, dtype=torch.uint8)
    if mean.numel() not in (Cc, 2 * Cc):
        raise ValueError(f"bn_backward: mean has {mean.numel()} elements for {Cc} channels")
    mean_lo = C.c_void_p(mean.data_ptr() + 4 * Cc if mean.numel() == 2 * Cc else 0)
    check(l.svr_bn_bwd_reduce(_p(x), _p(dy), _p(dpooled), _p(argmax), _p(mean), mean_lo, _p(ss), _p(sums), B, D, H, W, Cc, _p(ws),
                              _stream()), "bn_bwd_reduce")
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, device=dev, dtype=torch.float32)
    dbeta = torch.empty(Cc, device=dev, dtype=torch.float32)
    amax = amax_slot(dev) if "f16x3s" in (BACKWARD_CONV, BACKWARD_CONV_WEIGHT, BACKWARD_GEMM) else None
    check(l.svr_bn_bwd_apply(_p(x), _p(dy), _p(dpooled), _p(argmax), _p(mean), mean_lo, _p(ss), C.c_void_p(0), _p(sums), _p(dx),
                             _p(dgamma), _p(dbeta), B, D, H, W, Cc, int(relu_mask) | (0 if training else 2), _p(amax), _stream()),
          "bn_bwd_apply")
    if amax is not None:
        amax_remember(dx, amax)     # |max| of dx: the scale of the convolution gradients' scaled f16 split, no extra pass
    return dx, dgamma, dbeta


def stage1_supported(x, Co):
    """The recomputed first stage (stage1.hip) covers this input grid?  x (B,D,H,W,1)."""
    B, D, H, W, Ci = x.shape
    return Ci == 1 and bool(_lib.lib().svr_stage1_supported(B, D, H, W, Co))


def stage1_arith(mode=None):
    """1 if the first stage's recomputed convolution runs as the f16 split (FORWARD_CONV == "f16x3", the default), 0 = exact
    f32.  The backward recomputes the forward's activation, so it must get the forward's value (stage1_fwd stores it on wp)."""
    return 1 if (mode or FORWARD_CONV) == "f16x3" else 0


def stage1_fwd(x, w, bias, gamma, beta, running_mean, running_var, training, eps=1e-5, momentum=0.1, want_pool=True, mode=None):
    """x (B,D,H,W,1) -> y = BN(relu(conv_in(x))), pooled, argmax, scale_shift (3*16), mean (16), wp: conv_in's activation
    is recomputed wherever it is needed and never stored (stage1.hip).  mode: "f16x3" / "f32" (default: FORWARD_CONV)."""
    _f32(x, w, bias, gamma, beta, running_mean, running_var)
    B, D, H, W, _ = x.shape
    Co = w.shape[0]
    if training and B * D * H * W <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([{B}, {Co}, {D}, {H}, {W}])")
    l = _lib.lib()
    dev = x.device
    amax_forget(running_mean)      # (training: the running statistics are updated through their raw pointers)
    amax_forget(running_var)
    wp, _ = conv3d_pack_weight(w, want_bwd=False)
    y = torch.empty(B, D, H, W, Co, device=dev, dtype=torch.float32)
    pooled = argmax = None
    if want_pool:
        pooled = torch.empty(B, D // 2, H // 2, W // 2, Co, device=dev, dtype=torch.float32)
        argmax = torch.empty(B, D // 2, H // 2, W // 2, Co, device=dev, dtype=torch.uint8)
    ss = torch.empty(3 * Co, device=dev, dtype=torch.float32)
    mean = torch.empty(Co, device=dev, dtype=torch.float32)
    stats = torch.empty(2 * Co, device=dev, dtype=torch.float64) if training else None
    ws = torch.empty(l.svr_stage1_workspace(B, D, H, W), device=dev, dtype=torch.uint8)
    check(l.svr_stage1_fwd(_p(x), _p(wp), _p(bias), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y), _p(pooled),
                           _p(argmax), _p(ss), _p(mean), _p(stats), B, D, H, W, Co, eps, momentum, int(training),
                           stage1_arith(mode), _p(ws), _stream()), "stage1_fwd")
    wp.svr_stage1_arith = stage1_arith(mode)     # the arithmetic the backward has to recompute with
    return y, pooled, argmax, ss, mean, wp


def stage1_bwd(x, wp, bias, dy, dpooled, argmax, mean, ss, relu_mask=True, training=True, want_dout=False):
    """Backward of stage1_fwd -> dgamma, dbeta, dW (16,1,3,3,3), db, dout (None unless want_dout).  wp: the tensor
    stage1_fwd returned (it carries the forward's arithmetic)."""
    _f32(x, wp, bias, dy, dpooled, mean, ss)
    B, D, H, W, _ = x.shape
    Co = wp.shape[2]
    l = _lib.lib()
    dev = x.device
    sums = torch.empty(2 * Co, device=dev, dtype=torch.float64)
    dgamma = torch.empty(Co, device=dev, dtype=torch.float32)
    dbeta = torch.empty(Co, device=dev, dtype=torch.float32)
    dwp = torch.empty(Co, 1, 3, 3, 3, device=dev, dtype=torch.float32)      # the parameter's layout
    db = torch.empty(Co, device=dev, dtype=torch.float32)
    dout = torch.empty(B, D, H, W, Co, device=dev, dtype=torch.float32) if want_dout else None
    ws = torch.empty(l.svr_stage1_workspace(B, D, H, W), device=dev, dtype=torch.uint8)
    check(l.svr_stage1_bwd(_p(x), _p(wp), _p(bias), _p(dy), _p(dpooled), _p(argmax), _p(mean), _p(ss), _p(sums), _p(dgamma),
                           _p(dbeta), _p(dwp), _p(db), _p(dout), B, D, H, W, Co, int(relu_mask) | (0 if training else 2),
                           int(getattr(wp, "svr_stage1_arith", stage1_arith())), _p(ws), _stream()), "stage1_bwd")
    return dgamma, dbeta, dwp, db, dout


# ------------------------------------------------------------------------------------------
# projection: unproject / splat / clamp / blur
# ------------------------------------------------------------------------------------------
def _consts(c):
    arr = (C.c_float * 12)(*[float(v) for v in c])
    return arr


def unproject(depth, consts, normalize):
    _f32(depth)
    B, Hi, Wi = depth.shape
    pc = torch.empty(B, Hi * Wi, 3, device=depth.device, dtype=torch.float32)
    check(_lib.lib().svr_unproject_fwd(_p(depth), _p(pc), B, Hi, Wi, _consts(consts), int(normalize), _stream()), "unproject_fwd")
    return pc


def unproject_bwd(depth, gpc, consts, normalize):
    B, Hi, Wi = depth.shape
    gd = torch.empty_like(depth)
    check(_lib.lib().svr_unproject_bwd(_p(depth), _p(gpc), _p(gd), B, Hi, Wi, _consts(consts), int(normalize), _stream()),
          "unproject_bwd")
    return gd


def splat_ordered_supported(B, N, dims):
    """32-bit keys of the ordered splat: cells of the (D0+1)(D1+1)(D2+1) lattice below 2^31 - 1, points below 2^31."""
    return B * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) < 2 ** 31 - 1 and B * N < 2 ** 31


def splat_fwd(pts, dims, want_indices=False, ordered=False, want_vox=False):
    """-> acc (B, *dims), base, valid.  ordered: the atomic-free splat in the fixed summation order of include/svr_hip.h
    (svr_voxelize_splat_fwd_ordered; bit-reproducible, raises beyond its 32-bit limits); with want_vox a fourth result,
    clamp(8 * acc, 0, 1) from the same kernel."""
    _f32(pts)
    B, N, _ = pts.shape
    base = torch.empty(B, N, 3, device=pts.device, dtype=torch.int32) if want_indices else None
    valid = torch.empty(B, N, device=pts.device, dtype=torch.uint8) if want_indices else None
    if ordered:
        dims = tuple(int(d) for d in dims)
        if not splat_ordered_supported(B, N, dims):
            raise RuntimeError(f"splat_fwd(ordered=True): B={B}, N={N}, dims={dims} exceed the ordered splat's 32-bit limits "
                               "(B*(D0+1)(D1+1)(D2+1) < 2^31 - 1 and B*N < 2^31); there is no silent fall-back to atomics")
        if not pts.is_cuda:
            raise RuntimeError("svr_amd ops need GPU tensors (the HIP path has no CPU fallback)")
        l = _lib.lib()
        nbytes = int(l.svr_voxelize_splat_ordered_workspace(B, N, *dims))
        if nbytes < 0:
            raise RuntimeError(f"splat_fwd(ordered=True): unsupported shape B={B}, N={N}, dims={dims}")
        acc = torch.empty(B, *dims, device=pts.device, dtype=torch.float32)      # every voxel is written
        vox = torch.empty_like(acc) if want_vox else None
        ws = torch.empty(nbytes, device=pts.device, dtype=torch.uint8)
        check(l.svr_voxelize_splat_fwd_ordered(_p(pts), _p(acc), _p(vox), _p(base), _p(valid), B, N, dims[0], dims[1], dims[2],
                                               _p(ws), _stream()), "splat_fwd_ordered")
        return (acc, base, valid, vox) if want_vox else (acc, base, valid)
    if want_vox:
        raise RuntimeError("splat_fwd: want_vox is an output of the ordered kernel only")
    acc = torch.zeros(B, *dims, device=pts.device, dtype=torch.float32)
    check(_lib.lib().svr_voxelize_splat_fwd(_p(pts), _p(acc), _p(base), _p(valid), B, N, dims[0], dims[1], dims[2], _stream()),
          "splat_fwd")
    return acc, base, valid


def splat_bwd(pts, gacc, dims):
    B, N, _ = pts.shape
    gp = torch.empty_like(pts)
    check(_lib.lib().svr_voxelize_splat_bwd(_p(pts), _p(gacc), _p(gp), B, N, dims[0], dims[1], dims[2], _stream()), "splat_bwd")
    return gp


def scale_clamp01(x, scale):
    out = torch.empty_like(x)
    check(_lib.lib().svr_scale_clamp01_fwd(_p(x), _p(out), x.numel(), scale, _stream()), "scale_clamp01_fwd")
    return out


def scale_clamp01_bwd(x, gout, scale):
    gin = torch.empty_like(x)
    check(_lib.lib().svr_scale_clamp01_bwd(_p(x), _p(gout), _p(gin), x.numel(), scale, _stream()), "scale_clamp01_bwd")
    return gin


def blur_axis(x, taps, axis):
    _f32(x, taps)
    B, D0, D1, D2 = x.shape
    out = torch.empty_like(x)
    check(_lib.lib().svr_blur_axis_fwd(_p(x), _p(taps), _p(out), B, D0, D1, D2, axis, taps.numel(), _stream()), "blur_fwd")
    return out


def blur_axis_bwd(x, taps, gout, axis, want_gin=True, want_gtaps=True, ordered=False):
    """ordered: the tap gradient's block sums are added in block order (svr_blur_axis_bwd_ordered) instead of atomically."""
    B, D0, D1, D2 = x.shape
    gin = torch.empty_like(x) if want_gin else None
    if ordered:
        l = _lib.lib()
        K = taps.numel()
        gt = torch.empty(K, device=x.device, dtype=torch.float64) if want_gtaps else None
        ws = (torch.empty(int(l.svr_blur_axis_bwd_ordered_workspace(B, D0, D1, D2, K)) // 8, device=x.device, dtype=torch.float64)
              if want_gtaps else None)
        check(l.svr_blur_axis_bwd_ordered(_p(x), _p(taps), _p(gout), _p(gin), _p(gt), B, D0, D1, D2, axis, K, _p(ws), _stream()),
              "blur_bwd_ordered")
        return gin, gt
    gt = torch.zeros(taps.numel(), device=x.device, dtype=torch.float64) if want_gtaps else None
    check(_lib.lib().svr_blur_axis_bwd(_p(x), _p(taps), _p(gout), _p(gin), _p(gt), B, D0, D1, D2, axis, taps.numel(),
                                       _stream()), "blur_bwd")
    return gin, gt


# ------------------------------------------------------------------------------------------
# UNet 2-D convolution blocks (conv2d.hip): act -> [x2 upsample] -> conv on cat(src0, src1), channels-last
# ------------------------------------------------------------------------------------------
ACT_NONE, ACT_LEAKY, ACT_RELU = 0, 1, 2


def _conv2d_desc(src0, src1, k, stride, act, up):
    _f32(src0, src1)
    B, H, W, C0 = src0.shape
    if (2 if up else 1) * min(H, W) + 2 * (0 if k == 1 else 1) < k:      # (the library refuses it too: SVR_E_BADSHAPE)
        raise ValueError(f"conv2d: input {H} x {W}{' upsampled x2' if up else ''} with padding {0 if k == 1 else 1} is smaller than "
                         f"the {k} x {k} window: no output")
    d = _lib.Conv2dDesc(_p(src0), _p(src1), B, H, W, C0, src1.shape[3] if src1 is not None else 0, k, stride, act, int(up))
    Hv, Wv = (2 * H, 2 * W) if up else (H, W)
    pad = 0 if k == 1 else 1
    Ho, Wo = (Hv + 2 * pad - k) // stride + 1, (Wv + 2 * pad - k) // stride + 1
    return d, (Hv, Wv, Ho, Wo)


def conv2d_im2col(src0, src1, k, stride, act, up):
    """-> col (B*Ho*Wo, k*k*C) float32 and (Ho, Wo)."""
    d, (Hv, Wv, Ho, Wo) = _conv2d_desc(src0, src1, k, stride, act, up)
    C_ = d.C0 + d.C1
    col = torch.empty(d.B * Ho * Wo, k * k * C_, device=src0.device, dtype=torch.float32)
    check(_lib.lib().svr_conv2d_im2col(C.byref(d), _p(col), _stream()), "conv2d_im2col")
    return col, (Ho, Wo)


def conv2d_col2im(src0, src1, k, stride, act, up, dcol, need0=True, need1=True):
    """dcol (B*Ho*Wo, k*k*C) -> gradients wrt src0 / src1 (None where not needed)."""
    d, (Hv, Wv, Ho, Wo) = _conv2d_desc(src0, src1, k, stride, act, up)
    C_ = d.C0 + d.C1
    dvirt = torch.empty(d.B, Hv, Wv, C_, device=src0.device, dtype=torch.float32)
    d0 = torch.empty_like(src0) if need0 else None
    d1 = torch.empty_like(src1) if (src1 is not None and need1) else None
    if d0 is None and d1 is None:
        return None, None
    check(_lib.lib().svr_conv2d_col2im(C.byref(d), _p(dcol), _p(dvirt), _p(d0), _p(d1), _stream()), "conv2d_col2im")
    return d0, d1


# ---- the same blocks as implicit GEMMs (conv2d_igemm.hip; the default of model/unet.py) -------------------------------------
UNET_IGEMM = os.environ.get("SVR_UNET_IGEMM", "1") != "0"      # "0": the explicit patch-matrix path above (A/B)


class Conv2dPlanes:
    """Split f16 planes of one nn.Conv2d weight (forward and backward-data products) + the word holding max|W|.  Layers with
    1..4 output channels keep the f32 weight itself (`small`: plain-FMA kernels, conv2d.hip)."""

    def __init__(self, weight, stride, want_bwd=True, prepare=True):
        """prepare=False (conv2d_prepare_many): classify the layer only; a layer that is not `small` then gets its buffer
        and its planes from the batched launch."""
        _f32(weight)
        w = weight.detach().contiguous()
        self.Cout, self.C, self.k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        self.stride, self.has_bwd = stride, bool(want_bwd)
        self.small = bool(_lib.lib().svr_conv2d_small_supported(self.Cout, self.C, self.k))
        if self.small:
            self.w, self.has_bwd = w, True
        elif prepare:
            nbytes = 256 + _lib.lib().svr_conv2d_planes_bytes(self.Cout, self.C, self.k)
            self.buf = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
            self._amax, self._planes = self.buf.data_ptr(), self.buf.data_ptr() + 256
            check(_lib.lib().svr_conv2d_prepare(_p(w), self.Cout, self.C, self.k, stride, int(self.has_bwd), self.amax_ptr(),
                                                self.planes_ptr(), _stream()), "conv2d_prepare")

    def amax_ptr(self):
        return self._amax

    def planes_ptr(self):
        return self._planes


def conv2d_prepare_many(items):
    """[(weight, stride, want_bwd), ...] -> [Conv2dPlanes, ...]: the planes of all layers of a network in three launches per
    16 layers (svr_conv2d_prepare_many) instead of four per layer; bit-identical to preparing them one by one."""
    l = _lib.lib()
    out, todo = [None] * len(items), []
    for i, (weight, stride, want_bwd) in enumerate(items):
        w = weight.detach().contiguous()               # (kept here: the batched launch below reads it)
        pl = out[i] = Conv2dPlanes(w, stride, want_bwd, prepare=False)
        if not pl.small:
            todo.append((pl, w))
    for g0 in range(0, len(todo), 16):
        grp = todo[g0:g0 + 16]
        n = len(grp)
        sizes = [(int(l.svr_conv2d_planes_bytes(pl.Cout, pl.C, pl.k)) + 255) // 256 * 256 for pl, _ in grp]
        buf = torch.empty(256 * n + sum(sizes), device=grp[0][1].device, dtype=torch.uint8)
        base, off = buf.data_ptr(), 256 * n
        ptrs = []
        for i, (pl, _) in enumerate(grp):
            pl.buf, pl._amax, pl._planes = buf, base + 256 * i, base + off
            ptrs.append(base + off)
            off += sizes[i]
        I32A, PA = C.c_int32 * n, C.c_void_p * n
        check(l.svr_conv2d_prepare_many(n, PA(*[w.data_ptr() for _, w in grp]), I32A(*[pl.Cout for pl, _ in grp]),
                                        I32A(*[pl.C for pl, _ in grp]), I32A(*[pl.k for pl, _ in grp]),
                                        I32A(*[pl.stride for pl, _ in grp]), I32A(*[int(pl.has_bwd) for pl, _ in grp]),
                                        C.c_void_p(base), PA(*ptrs), _stream()), "conv2d_prepare_many")
    return out


def _amax_any(t):
    """amax word of a gradient tensor of any element count (amax_of wants multiples of 4 and 16-byte alignment)."""
    if t.numel() % 4 == 0 and t.data_ptr() % 16 == 0:
        return amax_of(t)
    a = t.detach().abs()      # (a NaN does not move the scale, as in the kernel's fmaxf: it must poison its own window only)
    return torch.where(torch.isnan(a), torch.zeros_like(a), a).max().reshape(1).view(torch.int32)


def _conv2d_ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), device=device, dtype=torch.uint8)


def conv2d_virtual(src0, src1, act, up):
    """V (B,Hv,Wv,C0+C1) = [x2 upsample](act(cat(src0, src1))): a decoder block's input, written once."""
    d, (Hv, Wv, _, _) = _conv2d_desc(src0, src1, 3, 1, act, up)
    V = torch.empty(d.B, Hv, Wv, d.C0 + d.C1, device=src0.device, dtype=torch.float32)
    check(_lib.lib().svr_conv2d_virtual(C.byref(d), _p(V), _stream()), "conv2d_virtual")
    return V


def conv2d_fwd(src0, src1, k, stride, act, planes, bias, amax_x=None, want_amax=False):
    """y (B,Ho,Wo,Cout) = conv_k(act(cat(src0, src1))) + bias as one implicit GEMM (no upsample here: conv2d_virtual first).
    amax_x: the input is a gradient operand (scaled f16 split); want_amax: leave max|y| on the result (`_svr_amax`)."""
    d, (_, _, Ho, Wo) = _conv2d_desc(src0, src1, k, stride, act, False)
    if planes.C != d.C0 + d.C1 or planes.k != k or planes.stride != stride:
        raise ValueError("conv2d_fwd: the planes were prepared for another layer")
    _f32(bias)
    y = torch.empty(d.B, Ho, Wo, planes.Cout, device=src0.device, dtype=torch.float32)
    if planes.small:
        check(_lib.lib().svr_conv2d_small_fwd(C.byref(d), _p(planes.w), _p(bias), _p(y), planes.Cout, _stream()), "conv2d_small_fwd")
        return y
    ws = _conv2d_ws(_lib.lib().svr_conv2d_workspace_bytes(C.byref(d), planes.Cout), src0.device)
    amax_y = amax_slot(src0.device) if want_amax else None
    check(_lib.lib().svr_conv2d_fwd(C.byref(d), planes.planes_ptr(), planes.amax_ptr(), _p(bias), _p(y), planes.Cout, _p(amax_x),
                                    _p(amax_y), _p(ws), _stream()), "conv2d_fwd")
    if want_amax:
        amax_remember(y, amax_y)
    return y


def linear_bwd_data_splitk(dy, wt):
    """dx (M,K) = dy (M,N) @ wt.T for wt (K,N) contiguous, through the implicit-GEMM kernel's k = 1 mode: the reduction over N is
    split over workgroups and the partial tiles are summed in a fixed order (few output tiles, long reduction).  f16x3s
    arithmetic.  Measured on IF-Net's projected levels' voxel GEMMs (reduction 1 792, 128 outputs): 22 + 26 us against 96 at
    4 096 rows, 77 + 41 against 104 at 32 768 rows -- and no change of the step's median (the GEMMs sit in the shadow of the
    projected scatter), so the step keeps linear_bwd_data; kept as an op for callers with that shape (tools/exp/dbg_splitk.py).
    K in 1..4 with K * N <= 8192 is refused (ValueError): that weight is the 2-D convolution's plain-FMA class, which has no k = 1 form."""
    _f32(dy, wt)
    M, N = dy.shape
    K = wt.shape[0]
    planes = Conv2dPlanes(wt.view(K, N, 1, 1), 1, want_bwd=False)
    if planes.small:      # 1..4 outputs with K * N <= 8192 weights: the plain-FMA class, which has no k = 1 form and leaves no word
        raise ValueError(f"linear_bwd_data_splitk: K = {K} output columns over a reduction of N = {N}: the split-reduction kernel "
                         f"takes K >= 5, or K * N > 8192 (K <= 4 with K * N <= 8192 is the plain-FMA class of conv2d.hip, which has "
                         f"no 1x1 form); use linear_bwd_data")
    y = conv2d_fwd(dy.view(1, 1, M, N), None, 1, 1, ACT_NONE, planes, None, amax_x=amax_of(dy), want_amax=True)
    out = y.view(M, K)
    amax_remember(out, y._svr_amax)
    return out


def conv2d_bwd_data(src0, src1, k, stride, planes, dy):
    """dIn (B,H,W,C0+C1): gradient of the convolution's activated, concatenated input (scaled f16 split on dy)."""
    d, _ = _conv2d_desc(src0, src1, k, stride, 0, False)
    if not planes.has_bwd:
        raise ValueError("conv2d_bwd_data: the planes were prepared without the backward product")
    _f32(dy)
    dy = dy.contiguous()
    din = torch.empty(d.B, d.H, d.W, d.C0 + d.C1, device=dy.device, dtype=torch.float32)
    if planes.small:
        check(_lib.lib().svr_conv2d_small_bwd_data(C.byref(d), _p(planes.w), _p(dy), planes.Cout, _p(din), _stream()), "conv2d_small_bwd_data")
        return din
    ws = _conv2d_ws(_lib.lib().svr_conv2d_workspace_bytes(C.byref(d), planes.Cout), dy.device)
    check(_lib.lib().svr_conv2d_bwd_data(C.byref(d), planes.planes_ptr(), planes.amax_ptr(), _p(dy), _amax_any(dy).data_ptr(),
                                         planes.Cout, _p(din), _p(ws), _stream()), "conv2d_bwd_data")
    return din


def conv2d_finish_bwd(src0, src1, act, up, dvirt, need0=True, need1=True):
    """dvirt (B,Hv,Wv,C) -> gradients of src0 / src1 (upsample adjoint, activation derivative, channel split)."""
    d, _ = _conv2d_desc(src0, src1, 3, 1, act, up)
    d0 = torch.empty_like(src0) if need0 else None
    d1 = torch.empty_like(src1) if (src1 is not None and need1) else None
    if d0 is None and d1 is None:
        return None, None
    check(_lib.lib().svr_conv2d_finish_bwd(C.byref(d), _p(dvirt), _p(d0), _p(d1), _stream()), "conv2d_finish_bwd")
    return d0, d1


def conv2d_bwd_weight(src0, src1, k, stride, act, dy, Cout, want_bias=True):
    """dW (Cout, C0+C1, k, k) in nn.Conv2d's layout and db from dy (B,Ho,Wo,Cout) and the gathered input."""
    d, _ = _conv2d_desc(src0, src1, k, stride, act, False)
    _f32(dy)
    dy = dy.contiguous()
    dw = torch.empty(Cout, d.C0 + d.C1, k, k, device=dy.device, dtype=torch.float32)
    db = torch.empty(Cout, device=dy.device, dtype=torch.float32) if want_bias else None
    if _lib.lib().svr_conv2d_small_supported(Cout, d.C0 + d.C1, k):
        ws = _conv2d_ws(_lib.lib().svr_conv2d_small_bwd_weight_workspace(C.byref(d), Cout), dy.device)
        check(_lib.lib().svr_conv2d_small_bwd_weight(C.byref(d), _p(dy), Cout, _p(dw), _p(db), _p(ws), _stream()), "conv2d_small_bwd_weight")
        return dw, db
    ws = _conv2d_ws(_lib.lib().svr_conv2d_bwd_weight_workspace(C.byref(d), Cout), dy.device)
    check(_lib.lib().svr_conv2d_bwd_weight(C.byref(d), _p(dy), _amax_any(dy).data_ptr(), Cout, _p(dw), _p(db), _p(ws), _stream()),
          "conv2d_bwd_weight")
    return dw, db


CONV2D_VARIANT_OPS = {"fwd": 0, "bwd_data": 1, "bwd_weight": 2}      # SVR_CV2_* of svr_hip.h
CONV2D_FAMILIES = ("small", "igemm64", "igemm128", "wgrad_tr")
CONV2D_EPILOGUES = ("coal", "lane", "reduce_v4", "reduce_scalar")


def conv2d_variant(op, B, H, W, C0, C1, Cout, k, stride, lo_src0=0, lo_src1=0, lo_dy=0, lo_out=0):
    """What the conv2d op `op` (a key of CONV2D_VARIANT_OPS) does with a layer: the plan its launcher runs on, as a dict
    (svr_conv2d_variant; host only, no GPU needed).  lo_*: the low four address bits of the sources, dY and the output.
    "family" is a name of CONV2D_FAMILIES, "epilogue" (the GEMM forward / backward-data) one of CONV2D_EPILOGUES, else None.
    A layer the entry point refuses raises with its error code and message, as the entry point would."""
    p = _lib.Conv2dPlan()
    check(_lib.lib().svr_conv2d_variant(CONV2D_VARIANT_OPS[op], B, H, W, C0, C1, Cout, k, stride, lo_src0, lo_src1, lo_dy, lo_out,
                                        C.byref(p)), "conv2d_variant")
    v = {n: int(getattr(p, n)) for n, _ in p._fields_}
    v["op"], v["family"] = op, CONV2D_FAMILIES[p.family]
    v["epilogue"] = CONV2D_EPILOGUES[p.epilogue] if v["family"] in ("igemm64", "igemm128") else None
    for n in ("vec4", "dy_vec4", "capped"):
        v[n] = bool(v[n])
    return v


# ------------------------------------------------------------------------------------------
# depth head of the UNet regressor (depth_head.hip)
# ------------------------------------------------------------------------------------------
def _depth_head_shape(raw, size, rows):
    if raw.dim() != 4 or raw.shape[1] != 1:
        raise ValueError(f"depth_head: raw is (B, 1, Hs, Ws), got {tuple(raw.shape)}")
    B, _, Hs, Ws = raw.shape
    S = int(size or 0)
    r0, r1 = (int(rows[0]), int(rows[1])) if S else (0, 0)
    return B, Hs, Ws, S, r0, r1, ((B, 1, r1 - r0, S) if S else (B, 1, Hs, Ws))


def depth_head_fwd(raw, target, size, rows, min_z, max_z, want_grad):
    """-> depth, loss (1,) or None, gdst (d loss / d y on the output's pixels) or None: one or two launches."""
    _f32(raw, target)
    B, Hs, Ws, S, r0, r1, shape = _depth_head_shape(raw, size, rows)
    if target is not None and tuple(target.shape) != shape:
        raise ValueError(f"depth_head: target {tuple(target.shape)} for a depth map {shape}")
    l = _lib.lib()
    depth = torch.empty(shape, device=raw.device, dtype=torch.float32)
    loss = gdst = ws = None
    if target is not None:
        loss = torch.empty(1, device=raw.device, dtype=torch.float32)
        ws = torch.empty(int(l.svr_depth_head_workspace(B, shape[2], shape[3])) // 8, device=raw.device, dtype=torch.float64)
        gdst = torch.empty(shape, device=raw.device, dtype=torch.float32) if want_grad else None
    check(l.svr_depth_head_fwd(_p(raw), _p(target), _p(depth), _p(loss), _p(gdst), B, Hs, Ws, S, r0, r1, float(min_z),
                               float(max_z), _p(ws), _stream()), "depth_head_fwd")
    return depth, loss, gdst


def depth_head_bwd(gdst, raw_shape, size, rows):
    """d loss / d raw from d loss / d y: the transposed interpolation (identity mode: gdst itself)."""
    B, _, Hs, Ws = raw_shape
    S = int(size or 0)
    if not S:
        return gdst
    draw = torch.empty(tuple(raw_shape), device=gdst.device, dtype=torch.float32)
    check(_lib.lib().svr_depth_head_bwd(_p(gdst), _p(draw), B, Hs, Ws, S, int(rows[0]), int(rows[1]), _stream()), "depth_head_bwd")
    return draw


class _DepthHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, target, size, rows, min_z, max_z):
        raw = raw.contiguous()
        want = ctx.needs_input_grad[0]
        depth, loss, gdst = depth_head_fwd(raw, target.contiguous(), size, rows, min_z, max_z, want)
        if want:                     # d raw for unit upstream gradient, left by the forward
            ctx.save_for_backward(depth_head_bwd(gdst, raw.shape, size, rows))
        ctx.mark_non_differentiable(depth)
        return depth, loss.squeeze(0)

    @staticmethod
    def backward(ctx, _gdepth, gloss):
        (draw,) = ctx.saved_tensors
        return draw * gloss, None, None, None, None, None


def depth_head(raw, target=None, size=320, rows=(40, 280), min_z=0.1953997164964676, max_z=7.0):
    """The UNet regressor's head (trainer/trainer_unet.py:43-61) in the kernels of depth_head.hip:

        depth = sigmoid(F.interpolate(raw, size=size, mode='bilinear')[:, :, rows[0]:rows[1], :]) * (max_z - min_z) + min_z
        loss  = F.mse_loss(depth, target)                                         (None without a target)

    raw: (B, 1, Hs, Ws) float32 (a permuted view is copied); size=0 / None: no resize (UNetMini on un-resized input).
    Returns (depth, loss).  The loss is differentiable in `raw`; `depth` is not (marked non-differentiable)."""
    if target is None:
        depth, _, _ = depth_head_fwd(raw.detach().contiguous(), None, size, rows, min_z, max_z, False)
        return depth, None
    return _DepthHeadFn.apply(raw, target, size, rows, min_z, max_z)


class _DepthHeadSceneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, size, rows, min_z, max_z):
        raw = raw.contiguous()
        depth, _, _ = depth_head_fwd(raw, None, size, rows, min_z, max_z, False)
        ctx.save_for_backward(depth)
        ctx.raw_shape, ctx.size, ctx.rows, ctx.min_z, ctx.max_z = tuple(raw.shape), size, rows, float(min_z), float(max_z)
        return depth

    @staticmethod
    def backward(ctx, gdepth):
        (depth,) = ctx.saved_tensors
        lo, hi = ctx.min_z, ctx.max_z
        # d depth / d y of depth = sigmoid(y) * (hi - lo) + lo, from the depth map itself (elementwise: no order to fix)
        gy = (gdepth * ((depth - lo) * (hi - depth) / (hi - lo))).contiguous()
        return depth_head_bwd(gy, ctx.raw_shape, ctx.size, ctx.rows), None, None, None, None


def depth_head_scene(raw, size=320, rows=(40, 280), min_z=0.1953997164964676, max_z=7.0):
    """depth_head's depth map WITH a gradient, for the scene step (the depth map feeds the unprojection there):
    forward = svr_depth_head_fwd without a target, backward = gy = g_depth * (depth - min_z)(max_z - depth)/(max_z - min_z)
    and the gather-form transposed interpolation svr_depth_head_bwd -- no atomics, unlike ATen's backward of
    F.interpolate(mode='bilinear').  size=0 / None: no resize.  Returns depth (B, 1, Ho, Wo)."""
    if not raw.is_cuda:
        raise RuntimeError("depth_head_scene HIP path needs GPU tensors (no CPU fallback)")
    return _DepthHeadSceneFn.apply(raw, size, rows, min_z, max_z)


# ------------------------------------------------------------------------------------------
# RGB preprocessing (rgb_preprocess.hip): SquarePad -> Pillow's 8-bit bilinear resize -> ToTensor -> Normalize(0.5, 0.5)
# ------------------------------------------------------------------------------------------
_rgb_tables = {}      # (in, out, device) -> (device int32 (out, K + 2), K); like project._consts: built once per size
_rgb_norm = {}        # device -> (256,) float32


def rgb_resize_table(n_in, n_out):
    """Pillow's coefficient table of one axis, from the library's host code (double): int32 (n_out, K + 2) numpy array, row
    xx = [xmin, tap count, K taps in 22-bit fixed point]."""
    import numpy as np
    l = _lib.lib()
    K = int(l.svr_rgb_resize_taps(int(n_in), int(n_out)))
    if K < 0:
        check(K, "rgb_resize_taps")
    table = np.empty((int(n_out), K + 2), dtype=np.int32)
    check(l.svr_rgb_resize_table(int(n_in), int(n_out), K, table.ctypes.data_as(C.c_void_p)), "rgb_resize_table")
    return table


def _rgb_table(n_in, n_out, device):
    key = (int(n_in), int(n_out), device)
    hit = _rgb_tables.get(key)
    if hit is None:
        t = rgb_resize_table(n_in, n_out)
        hit = _rgb_tables[key] = (torch.from_numpy(t).to(device), t.shape[1] - 2)
    return hit


def _rgb_norm_table(device):
    t = _rgb_norm.get(device)
    if t is None:
        # ToTensor's and Normalize's own float32 operations, on the host like rgb_transform, once per byte value
        x = torch.arange(256, dtype=torch.uint8).float().div(255)
        t = _rgb_norm[device] = ((x - 0.5) / 0.5).to(device)
    return t


def rgb_preprocess(images_u8, W=256, resize_input=True, flip=False, return_u8=False):
    """dataset.scene_net_data.rgb_transform on the device, for a batch of equal-sized images.

    images_u8: (B, H, W, C) uint8 GPU tensor, C 1 or 3 (raw pixels, rows of interleaved bands as PIL stores them).
    resize_input: SquarePad with zeros, then Pillow's ``Image.resize((W, W), Image.BILINEAR)`` (antialiased, two 8-bit
    passes) bit for bit; otherwise only the layout change.  flip: ``Image.FLIP_LEFT_RIGHT`` in front of the pad.
    -> (B, C, Ho, Wo) float32, ``(x / 255 - 0.5) / 0.5`` as torch rounds it; with return_u8 also the resized bytes
    (B, Ho, Wo, C) uint8.  The per-axis tables and the byte -> float table are cached on the device."""
    if not torch.is_tensor(images_u8) or not images_u8.is_cuda:
        raise RuntimeError("rgb_preprocess HIP path needs GPU tensors (no CPU fallback)")
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise ValueError(f"rgb_preprocess: expected (B, H, W, C) uint8, got {tuple(images_u8.shape)} {images_u8.dtype}")
    src = images_u8.contiguous()
    B, H, Wi, Cn = (int(s) for s in src.shape)
    if Cn not in (1, 3):
        raise ValueError(f"rgb_preprocess: {Cn} bands (1 or 3)")
    if min(B, H, Wi) < 1:
        raise ValueError(f"rgb_preprocess: empty batch {tuple(src.shape)}")
    dev = src.device
    tx = ty = tmp = None
    Kx = Ky = 0
    if resize_input:
        Wout = int(W)
        if Wout < 1:
            raise ValueError(f"rgb_preprocess: W={W}")
        m = max(H, Wi)
        Hp, Wp = H + 2 * ((m - H) // 2), Wi + 2 * ((m - Wi) // 2)
        if Wp != Wout:
            tx, Kx = _rgb_table(Wp, Wout, dev)
        if Hp != Wout:
            ty, Ky = _rgb_table(Hp, Wout, dev)
        if tx is not None and ty is not None:
            tmp = torch.empty((B, Hp, Wout, Cn), device=dev, dtype=torch.uint8)
        Ho = Wo = Wout
    else:
        Wout, Ho, Wo = 0, H, Wi
    out = torch.empty((B, Cn, Ho, Wo), device=dev, dtype=torch.float32)
    u8 = torch.empty((B, Ho, Wo, Cn), device=dev, dtype=torch.uint8) if return_u8 else None
    check(_lib.lib().svr_rgb_preprocess(_p(src), B, H, Wi, Cn, Wout, int(bool(flip)), _p(tx), Kx, _p(ty), Ky,
                                        _p(_rgb_norm_table(dev)), _p(tmp), _p(u8), _p(out), _stream()), "rgb_preprocess")
    return (out, u8) if return_u8 else out


def grid_to_camera(points, scale_shift):
    """(n, 3) float32 grid-space points -> camera space: (p - t) / s per axis, scale_shift = (s0, t0, s1, t1, s2, t2): the
    inverse of the affine behind `unproject` (consts[3:9])."""
    _f32(points)
    pts = points.contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"grid_to_camera: expected (n, 3), got {tuple(pts.shape)}")
    out = torch.empty_like(pts)
    k = (C.c_float * 6)(*[float(v) for v in scale_shift])
    check(_lib.lib().svr_grid_to_camera(_p(pts), _p(out), pts.shape[0], k, _stream()), "grid_to_camera")
    return out
