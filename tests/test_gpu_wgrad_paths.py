"""Every kernel the 3x3x3 weight-gradient launchers can select (csrc/conv3d.hip: the three Ci == 1 kernels and the f32 brick
kernel; csrc/conv3d_bwdw_bf16.hip: the wave-specialised kernel on paired-row and on full tiles, the 8-wave kernel with one and
with several bricks per workgroup) against a float64 reference, one case per row of tests/_wgrad_cases.py.  A case first
ASSERTS, through svr_conv3d_k3_bwd_weight_variant (the function the launchers call), that it runs the kernel it is named for;
the CPU test test_wgrad_variant_table_and_every_kernel_is_reached checks that the rows reach all of them.

The C entry points are called directly, so the test owns every buffer:
  a. integer operands (x in {0..3}, about half zeros; dout in {-3..3}): every product and every partial sum is an integer below
     2^24 (9 x voxels <= 2.2 M), the bf16 and f16 `hi` terms hold the operands exactly and the low terms are 0, the f16x3s scale is
     a power of two, the slab sums are f64 -- so all three arithmetics must return the int64 result BIT FOR BIT, dW and db, in
     the packed layout [tap][ci][co] and in the parameter's (Co,Ci,3,3,3), with db and with db == NULL.  One halo row, tap or
     partial brick off by a voxel changes an integer;
  b. gradient-like float operands (tests/test_gpu_conv_wgrad.py::_inputs, one gscale per row from 1e-6 to 30), the project's
     gates applied to each of the 27 taps ON ITS OWN (max |err| over the tap / max |ref| over the tap): f32 3e-6, f16x3s 3e-6 and
     <= 3 x the f32 kernel's error on the same tap + 1e-7, bf16x3 3e-5; db 3e-6;
  c. dW and db start as NaN and come back finite everywhere; the workspace is the queried size, NaN-filled, and 4096 guard bytes
     behind it, behind dW and behind db are unchanged after every launch;
  d. two runs of a split entry point give identical bytes.
The reference is 27 shifted dout^T @ x products in f64 with stock torch ops on the device; it is computed once per operand set
and shared by the entry points.

Wall time of the file on one MI355X: 6 s for its 14 rows (the largest, 61 x 62 x 63 voxels x 32 channels = 30 MB per operand,
takes 1.6 s with its references).  Measured worst taps: DESIGN.md, "3x3x3 weight gradient"."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _wgrad_cases as WC  # noqa: E402
from tests.test_gpu_conv_wgrad import _inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN, NAN_BYTE = 4096, 0xA5, 0xFF       # four 0xFF bytes are a float32 NaN
GATE = {"bwd_weight_f32": 3e-6, "bwd_weight_f16x3s": 3e-6, "bwd_weight_bf16x3": 3e-5}
DB_GATE = 3e-6


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def _ref_f64(x, dy):
    """dW (Co,Ci,3,3,3) and db (Co) in f64 on the device: dW[:, :, kz, ky, kx] = sum over voxels of dout[v] x[v + tap - 1]"""
    B, D, H, W, Ci = x.shape
    Co = dy.shape[-1]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    d = dy.double().reshape(-1, Co)
    dw = torch.empty(Co, Ci, 3, 3, 3, dtype=torch.float64, device=x.device)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                dw[:, :, kz, ky, kx] = d.t() @ xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Ci)
    return dw, d.sum(0)


def _packed(dw):
    """(Co,Ci,3,3,3) -> the packed layout [tap][ci][co]"""
    Co, Ci = dw.shape[:2]
    return dw.reshape(Co, Ci, 27).permute(2, 1, 0).contiguous()


def _guarded(nbytes):
    """nbytes of NaN with GUARD pattern bytes behind them"""
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf[:nbytes] = NAN_BYTE
    buf[nbytes:] = PATTERN
    return buf


def _tail_intact(buf):
    return bool((buf[-GUARD:] == PATTERN).all())


def _run(op, x, dy, param_layout, want_db):
    """One launch of entry point `op` on buffers of this test: -> dW ((Co,Ci,3,3,3) or [27][Ci][Co]), db or None.  Asserts (c)."""
    from svr_amd import _lib
    l = _lib.lib()
    B, D, H, W, Ci = x.shape
    Co = dy.shape[-1]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    query = l.svr_conv3d_k3_bwd_weight_workspace if op == WC.F32_OP else l.svr_conv3d_k3_bwd_weight_bf16x3_workspace
    ws = _guarded(query(B, D, H, W, Ci, Co))
    wbuf, bbuf = _guarded(27 * Ci * Co * 4), _guarded(Co * 4) if want_db else None
    dw = wbuf[:-GUARD].view(torch.float32).view((Co, Ci, 3, 3, 3) if param_layout else (27, Ci, Co))
    db = bbuf[:-GUARD].view(torch.float32) if want_db else None
    if op == WC.F32_OP:
        assert not param_layout
        rc = l.svr_conv3d_k3_bwd_weight(p(x), p(dy), p(dw), p(db), B, D, H, W, Ci, Co, p(ws), s)
    elif op == "bwd_weight_f16x3s":
        amax = dy.abs().max().reshape(1).view(torch.int32)      # the bit pattern of max |dout|, what svr_amax_f32 leaves
        rc = l.svr_conv3d_k3_bwd_weight_f16x3(p(x), p(dy), p(dw), p(db), B, D, H, W, Ci, Co, 1 if param_layout else 0, p(amax), p(ws), s)
    else:
        f = l.svr_conv3d_k3_bwd_weight_bf16x3_param if param_layout else l.svr_conv3d_k3_bwd_weight_bf16x3
        rc = f(p(x), p(dy), p(dw), p(db), B, D, H, W, Ci, Co, p(ws), s)
    what = (op, param_layout, want_db)
    assert rc == 0, what
    assert bool(torch.isfinite(dw).all()), ("dW: an element not written, or made from an unwritten slab", what)
    assert _tail_intact(wbuf), ("written past dW", what)
    if want_db:
        assert bool(torch.isfinite(db).all()), ("db: an element not written", what)
        assert _tail_intact(bbuf), ("written past db", what)
    assert _tail_intact(ws), ("written past the queried workspace", what)
    return dw, db


def _layouts(op):
    return (False,) if op == WC.F32_OP else (False, True)      # the f32 entry point writes the packed layout only


def _tap_err(dw, ref, param_layout):
    """per tap: max |dw - ref| / max |ref|, both over the tap's (ci, co) -> (27,) f64"""
    e = (dw.double() - ref).abs()
    if param_layout:
        Co, Ci = dw.shape[:2]
        return e.reshape(Co, Ci, 27).amax((0, 1)) / ref.abs().reshape(Co, Ci, 27).amax((0, 1)).clamp_min(1e-300)
    return e.amax((1, 2)) / ref.abs().amax((1, 2)).clamp_min(1e-300)


@pytest.mark.parametrize("name,B,dims,Ci,Co,gscale,ftag,stag,fper,sper", WC.CASES, ids=[c[0] for c in WC.CASES])
def test_wgrad_row(name, B, dims, Ci, Co, gscale, ftag, stag, fper, sper):
    ops = _ops()
    # ---- the kernel this row is there for is the kernel it runs
    run_ops = []
    for op, tag, per in [(WC.F32_OP, ftag, fper)] + [(o, stag, sper) for o in WC.SPLIT_OPS]:
        if tag is None:
            continue
        v = ops.conv3d_k3_bwd_weight_variant(op, B, dims, Ci, Co)
        assert v["kernel"] == tag, (name, op, v)
        if per is not None and tag in ("X3", "BRICK"):
            assert (v["max_bricks_per_part"] == 1) == (per == "1"), (name, op, v)
        run_ops.append(op)
    g = torch.Generator(device="cuda").manual_seed(_seed(name))

    # ---- a. exact on integers (+ c. in every launch)
    voxels = B * dims[0] * dims[1] * dims[2]
    assert 9 * voxels < 2 ** 24      # the bound of every partial sum, whatever the order
    x = torch.randint(-3, 4, (B, *dims, Ci), generator=g, device="cuda").clamp_min_(0).float()      # ReLU-like: 4 of 7 are zero
    dy = torch.randint(-3, 4, (B, *dims, Co), generator=g, device="cuda").float()
    rw, rb = _ref_f64(x, dy)
    assert float(rw.abs().max()) < 2 ** 24 and bool((rw == rw.round()).all())
    ref = {True: rw.float(), False: _packed(rw).float()}
    rb = rb.float()
    for op in run_ops:
        for param_layout in _layouts(op):
            for want_db in (True, False):
                dw, db = _run(op, x, dy, param_layout, want_db)
                bad = int((dw != ref[param_layout]).sum())
                assert bad == 0, (name, op, "param" if param_layout else "packed", want_db, f"{bad} of {dw.numel()} integers differ",
                                  float((dw - ref[param_layout]).abs().max()))
                assert db is None or torch.equal(db, rb), (name, op, param_layout, "db", float((db - rb).abs().max()))

    # ---- b. float operands, each tap on its own (+ c.), d. run-to-run bytes
    x, dy = _inputs(B, dims, Ci, Co, gscale, seed=_seed(name))
    rw, rb = _ref_f64(x, dy)
    ref = {True: rw, False: _packed(rw)}
    worst, dberr, taps = {}, {}, {}
    for op in run_ops:
        for param_layout in _layouts(op):
            dw, db = _run(op, x, dy, param_layout, True)
            te = _tap_err(dw, ref[param_layout], param_layout)
            taps[op] = te if op not in taps else torch.maximum(taps[op], te)
            dberr[op] = max(dberr.get(op, 0.0), float((db.double() - rb).abs().max() / rb.abs().max()))
            if op != WC.F32_OP:
                dw2, db2 = _run(op, x, dy, param_layout, True)
                assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32)), \
                    (name, op, param_layout, "two runs, different bytes")
        worst[op] = float(taps[op].max())
    print(f"WGRAD {name} worst tap " + " ".join(f"{op[11:]}={worst[op]:.2e}(tap {int(taps[op].argmax())})" for op in run_ops) +
          " db " + " ".join(f"{op[11:]}={dberr[op]:.2e}" for op in run_ops))
    for op in run_ops:
        assert worst[op] < GATE[op], (name, op, taps[op].tolist())
        assert dberr[op] < DB_GATE, (name, op, dberr[op])
    if "bwd_weight_f16x3s" in run_ops:
        over = taps["bwd_weight_f16x3s"] - (3 * taps[WC.F32_OP] + 1e-7)
        assert float(over.max()) <= 0, (name, "f16x3s over 3 x f32 + 1e-7 at tap", int(over.argmax()), taps["bwd_weight_f16x3s"].tolist(),
                                        taps[WC.F32_OP].tolist())
