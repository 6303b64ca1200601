"""Block-sparse evaluation of a scalar function on the query lattice (not a reference module: the reference evaluates
every lattice point).  A coarse-to-fine extractor in the manner of Occupancy Networks' MISE, on the library's svr_sl_*
kernels (csrc/sparse_lattice.hip; the rule is pinned in include/svr_hip.h and DESIGN.md section 15):

``sparse_lattice_field(fn, shape, level, block, points_batch_size=2048*16, max_rounds=32) -> SparseLatticeField``

`fn` maps (n, 3) float32 device points to (n,) float32 values; it is called on the corners of blocks of `block` cells,
then only on the points of blocks the level set passes through, following the surface from block to block until no
lattice edge with differing sides has an unevaluated endpoint.  Every other point keeps the value of its block's minimum
corner, which lies on the same side of `level` unless a surface component hides between the coarse points (the limit
of every such extractor).  The result's `field` goes to `marching_cubes` like a dense one.

The point coordinates are rows of ``make_3d_grid((-0.5,)*3, (0.5,)*3, shape)``, bit for bit: the kernels copy entries
of the same three linspace tables.  One host read per round (the totals that size the point list)."""
import contextlib
from dataclasses import dataclass, field as _dc_field

import torch

from .. import _lib
from .._lib import check, ptr as _p, stream as _stream

_MAX_ROUNDS = 254          # the block state is a uint8 and the fall-back round comes on top


@dataclass
class SparseLatticeField:
    field: torch.Tensor            # (X, Y, Z) float32, device
    state: torch.Tensor            # (nbx, nby, nbz) uint8, device: 0 = filled from the coarse value, r = evaluated in round r
    n_points: int                  # points fn was called on: the coarse points and the points of every round
    rounds: int                    # rounds that evaluated at least one block
    leaks: list = _dc_field(default_factory=list)     # per round: edges that led into a block never evaluated
    fell_back: bool = False        # max_rounds did not end leak-free: the last round evaluated every remaining block
    timings: dict = None           # profile=True: {"bookkeeping_ms", "query_ms", "host_reads"}

    @property
    def evaluated_fraction(self):
        return self.n_points / self.field.numel()


class _Clock:
    """HIP-event brackets summed per label; read once at the end (profile=True only)."""

    def __init__(self, on):
        self.on, self.spans = on, []

    @contextlib.contextmanager
    def span(self, label):
        if not self.on:
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.spans.append((label, a, b))

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for label, a, b in self.spans:
            out[label] = out.get(label, 0.0) + a.elapsed_time(b)
        return out


def _evaluate(fn, pts, points_batch_size):
    vals = [fn(pi).reshape(-1) for pi in torch.split(pts, points_batch_size)]
    if any(v.device != pts.device for v in vals):
        raise RuntimeError("sparse_lattice_field HIP path needs GPU tensors from fn (no CPU fallback)")
    out = (vals[0] if len(vals) == 1 else torch.cat(vals)).to(torch.float32).contiguous()
    if out.numel() != pts.shape[0]:
        raise ValueError(f"sparse_lattice_field: fn returned {out.numel()} values for {pts.shape[0]} points")
    return out


def sparse_lattice_field(fn, shape, level, block, points_batch_size=2048 * 16, max_rounds=32, device=None, profile=False):
    shape = tuple(int(v) for v in shape)
    block, max_rounds, points_batch_size = int(block), int(max_rounds), int(points_batch_size)
    if len(shape) != 3:
        raise ValueError(f"sparse_lattice_field: shape must be (X, Y, Z), got {shape}")
    if not 1 <= max_rounds <= _MAX_ROUNDS:
        raise ValueError(f"sparse_lattice_field: max_rounds must be in [1, {_MAX_ROUNDS}], got {max_rounds}")
    if points_batch_size < 1:
        raise ValueError("sparse_lattice_field: points_batch_size must be positive")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("sparse_lattice_field HIP path needs a GPU device (no CPU fallback)")
    X, Y, Z = shape
    l = _lib.lib()
    ws_bytes = int(l.svr_sl_workspace_bytes(X, Y, Z, block))
    if ws_bytes < 0:
        check(ws_bytes, "sl_workspace_bytes")
    level = float(level)
    clock = _Clock(profile)
    with torch.cuda.device(device), torch.no_grad():
        # the tables make_3d_grid expands: built on the host like there, so the coordinates carry the same bits
        tx, ty, tz = (torch.linspace(-0.5, 0.5, n).to(device) for n in shape)
        nb = [-(-(n - 1) // block) for n in shape]
        n_coarse = (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1)
        ws = torch.empty(ws_bytes, device=device, dtype=torch.uint8)
        totals = torch.zeros(3, device=device, dtype=torch.int64)
        field = torch.empty(shape, device=device, dtype=torch.float32)
        state = torch.empty(nb, device=device, dtype=torch.uint8)
        pts = torch.empty((n_coarse, 3), device=device, dtype=torch.float32)
        dims = (X, Y, Z, block)
        with clock.span("bookkeeping_ms"):
            check(l.svr_sl_coarse_points(_p(tx), _p(ty), _p(tz), *dims, _p(pts), _stream()), "sl_coarse_points")
        with clock.span("query_ms"):
            coarse = _evaluate(fn, pts, points_batch_size)
        with clock.span("bookkeeping_ms"):
            check(l.svr_sl_fill_seed(_p(coarse), *dims, level, _p(field), _p(state), _p(ws), ws_bytes, _stream()), "sl_fill_seed")
        res = SparseLatticeField(field=field, state=state, n_points=n_coarse, rounds=0)
        host_reads = 0
        while True:
            r = res.rounds + 1
            with clock.span("bookkeeping_ms"):
                check(l.svr_sl_select(*dims, 0, _p(state), _p(ws), _p(totals), _stream()), "sl_select")
            n_blocks, n_pts, leaked = totals.tolist()          # the round's host synchronisation: sizes the point list
            host_reads += 1
            if res.leaks:
                res.leaks[-1] = leaked
            if n_blocks == 0:
                break
            if r > max_rounds:                                 # still leaking: one last round over every block left
                with clock.span("bookkeeping_ms"):
                    check(l.svr_sl_select(*dims, 1, _p(state), _p(ws), _p(totals), _stream()), "sl_select")
                n_blocks, n_pts, _ = totals.tolist()
                host_reads += 1
                res.fell_back = True
            pts = torch.empty((n_pts, 3), device=device, dtype=torch.float32)
            with clock.span("bookkeeping_ms"):
                check(l.svr_sl_block_points(_p(tx), _p(ty), _p(tz), *dims, _p(ws), n_blocks, _p(pts), _stream()), "sl_block_points")
            with clock.span("query_ms"):
                vals = _evaluate(fn, pts, points_batch_size)
            with clock.span("bookkeeping_ms"):
                check(l.svr_sl_scatter(_p(vals), *dims, _p(ws), n_blocks, r, _p(field), _p(state), _stream()), "sl_scatter")
                check(l.svr_sl_leak_check(_p(field), *dims, level, _p(state), _p(ws), n_blocks, _p(totals), _stream()),
                      "sl_leak_check")
            res.n_points += n_pts
            res.rounds = r
            res.leaks.append(0)
            if res.fell_back:                                  # every block is evaluated: nothing can leak
                break
        if profile:
            res.timings = dict(clock.totals(), host_reads=host_reads)
    return res
