"""Every kernel and launcher branch of the UNet's 2-D convolutions (csrc/conv2d_igemm.hip, csrc/conv2d.hip, the CONV form of
linear_tn_x3_tr_kernel and conv_wgrad_reduce_kernel in csrc/gemm_bf16x3.hip, the loaders of csrc/conv2d_virt.h) against float64,
one op at a time -- ops.Conv2dPlanes, conv2d_fwd, conv2d_bwd_data, conv2d_bwd_weight, conv2d_virtual, conv2d_finish_bwd,
conv2d_im2col / conv2d_col2im -- never through the autograd block.  Each case first ASSERTS, through ops.conv2d_variant, that
it runs the branch it is named for (tests/_conv2d_cases.py; test_conv2d_variant_table_and_every_branch_is_reached in
tests/test_capi_cpu.py checks that the rows reach all of them).

Inputs are made on the device: activations with exact 0.0 and -0.0, gradients at magnitudes 1e-6 / 1 / 1e+4 with a per-pixel
e^(2 sigma) spread, weights at 1e-6 / 1/sqrt(fan_in) / 1e+3 and a family with per-output-channel scales 2^-8 .. 1 (judged per
channel too).  The reference is tests/conv2d_f64.py (k*k shifted float64 addmm, differentiable; pinned on the CPU by
tests/test_conv2d_f64_cpu.py).  Errors are tests._golden.rel_err (max |a - b| / max |b|) on the device.  Gates: 3e-6 forward,
conv2d_virtual, finish and the explicit path's elementwise kernels; 5e-6 backward-data and weight gradient; 1e-6 db.  The
long-reduction cases (LONG: 4 608- and 9 360-term sums) meet the plain gates; the error of an exact-f32 matmul of the same patch
matrix is printed next to theirs (DESIGN.md section 4 has both).

Wall time of the file on one MI355X: 6 s for its 127 tests, float64 references included.  Measured errors: DESIGN.md section 4."""
import pytest
import torch

from tests import _conv2d_cases as K
from tests import conv2d_f64 as R

pytestmark = pytest.mark.gpu

G_FWD, G_BWD, G_DB = 3e-6, 5e-6, 1e-6
LONG = ("ig_n1_k585", "ig_n3")                              # 9 360- and 4 608-term sums
BIG = ("tiles547", "reduce_stride", "small_cap_c4", "small_cap_c68")      # one data family: the branch is what they are there for
# (name, dY magnitude, weight scale, activations the forward and the weight gradient run with)
FAMILIES = (("unit", 1.0, None, (0, 1, 2)), ("tiny_dy_big_w", 1e-6, 1e3, (1,)), ("big_dy_tiny_w", 1e4, 1e-6, (2,)), ("per_channel", 1.0, "chan", (0,)))


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _rel_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _chan_err(a, ref):
    """the same figure per output channel (last dimension): a fault confined to one n-tile edge or to the small channels"""
    d = (a.double() - ref).abs().reshape(-1, ref.shape[-1]).max(0).values
    return float((d / ref.abs().reshape(-1, ref.shape[-1]).max(0).values.clamp_min(1e-300)).max())


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def _mis(t, on):
    """the same values in a tensor that starts 4 bytes into its buffer (16-byte loaders off)"""
    if not on:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _inputs(shape, mis, gscale, wscale, seed):
    B, H, W, C0, C1, Cout, k, stride = shape
    g = torch.Generator(device="cuda").manual_seed(seed)

    def src(C):
        t = torch.randn(B, H, W, C, generator=g, device="cuda")
        t.view(-1)[::5] = 0.0
        t.view(-1)[2::7] = -0.0
        return t
    s0, s1 = _mis(src(C0), "src0" in mis), (_mis(src(C1), "src1" in mis) if C1 else None)
    fan = (C0 + C1) * k * k
    w = torch.randn(Cout, C0 + C1, k, k, generator=g, device="cuda")
    b = torch.randn(Cout, generator=g, device="cuda")
    if wscale == "chan":
        sc = torch.exp2(-8 * torch.arange(Cout, device="cuda") / max(Cout - 1, 1))
        w, b = w * sc.view(-1, 1, 1, 1) / fan ** 0.5, b * sc
    else:
        w, b = w * (wscale if wscale is not None else 1 / fan ** 0.5), b * (wscale if wscale is not None else 1.0)
    pad = 0 if k == 1 else 1
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn(B, Ho, Wo, Cout, generator=g, device="cuda") * gscale
    dy *= torch.exp(2 * torch.randn(B, Ho, Wo, 1, generator=g, device="cuda"))
    return s0, s1, w.contiguous(), b, _mis(dy.contiguous(), "dy" in mis)


def _reference(s0, s1, w, b, dy, k, stride, act):
    xa = R.virtual_f64(s0, s1, act, False).requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = R.conv_f64(xa, wd, bd, k, stride)
    din, dw, db = torch.autograd.grad(y, (xa, wd, bd), dy.double())
    return xa.detach(), y.detach(), din, dw, db


def _f32_yardstick(xa, w, b, y):
    """error of an exact-f32 evaluation of the same sums (stock f32 matmul of the float64 reference's patch matrix)"""
    k = w.shape[2]
    pm = R.patches(xa, k, 1 if k != 4 else 2).float()
    y32 = pm @ R.weight_matrix(w).t().float() + b
    return _rel_err(y32.view(y.shape), y)


def _assert_tags(ops, name, shape, mis, tags):
    for op, tag in tags.items():
        v = K.query(ops, op, shape, mis)
        assert K.tag(v) == tag, (name, op, K.tag(v), tag)


def _amax_is_exact(y):
    return float(y._svr_amax.view(torch.float32)) == float(y.abs().max())


def _check_layer(ops, name, shape, mis, fam, gscale, wscale, acts):
    """one layer, one data family: forward (bias, fused |max|) and weight gradient / db with EVERY activation of `acts`,
    backward-data (which sees no activation) once; bit identity of a second run; -> [(label, errors, gates)]"""
    B, H, W, C0, C1, Cout, k, stride = shape
    s0, s1, w, b, dy = _inputs(shape, mis, gscale, wscale, _seed(name))
    planes = ops.Conv2dPlanes(w, stride, want_bwd=k != 1)
    out = []
    for i, act in enumerate(acts):
        xa, y_ref, din_ref, dw_ref, db_ref = _reference(s0, s1, w, b, dy, k, stride, act)
        y = ops.conv2d_fwd(s0, s1, k, stride, act, planes, b, want_amax=not planes.small)
        y2 = ops.conv2d_fwd(s0, s1, k, stride, act, planes, b)
        assert y.shape == y_ref.shape and torch.equal(y, y2), (name, fam, act, "forward: other bits on the second run / without amax")
        if not planes.small:
            assert _amax_is_exact(y), (name, fam, act, "fused |max| of y")
        e = {"fwd": _rel_err(y, y_ref)}
        gate = {"fwd": G_FWD, "din": G_BWD, "dw": G_BWD, "db": G_DB}
        if name in LONG:
            e["f32"] = _f32_yardstick(xa, w.double(), b.double(), y_ref)      # (printed for DESIGN.md; the plain gate holds)
        if fam == "per_channel":
            e["fwd_chan"] = _chan_err(y, y_ref)
            gate["fwd_chan"] = G_FWD
        if k != 1:
            if i == 0:
                din = ops.conv2d_bwd_data(s0, s1, k, stride, planes, dy)
                assert din.shape == din_ref.shape and torch.equal(din, ops.conv2d_bwd_data(s0, s1, k, stride, planes, dy)), (name, fam, "din bits")
                e["din"] = _rel_err(din, din_ref)
            dw, db = ops.conv2d_bwd_weight(s0, s1, k, stride, act, dy, Cout)
            dw2, db2 = ops.conv2d_bwd_weight(s0, s1, k, stride, act, dy, Cout)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), (name, fam, act, "dw / db bits")
            assert ops.conv2d_bwd_weight(s0, s1, k, stride, act, dy, Cout, want_bias=False)[1] is None
            e.update(dw=_rel_err(dw, dw_ref), db=_rel_err(db, db_ref))
            if fam == "per_channel":
                e["dw_chan"] = _chan_err(dw.reshape(Cout, -1).t(), dw_ref.reshape(Cout, -1).t())
                gate["dw_chan"] = G_BWD
        out.append((f"{fam}/act{act}", e, gate))
        print(f"conv2d_paths {name} {fam} act={act} " + " ".join(f"{k_}={v:.2e}" for k_, v in e.items()))
    return out


def _assert_gates(name, out):
    for label, e, gate in out:
        for key, g_ in gate.items():
            if key in e:
                assert e[key] < g_, (name, label, key, e)


@pytest.mark.parametrize("name,shape,mis,tags,ext", K.CASES, ids=[c[0] for c in K.CASES])
def test_ops_against_f64(name, shape, mis, tags, ext):
    """forward (bias, fused |max|), backward-data, weight gradient and db of one layer against float64: every activation
    (none, LeakyReLU, ReLU) at unit scales, then the other data families with the activation FAMILIES names; two runs give the
    same bits; want_amax leaves exactly max |y|."""
    ops = _ops()
    _assert_tags(ops, name, shape, mis, tags)
    out = []
    for fam, gscale, wscale, acts in FAMILIES[:1] if name in BIG else FAMILIES:
        out += _check_layer(ops, name, shape, mis, fam, gscale, wscale, acts)
    _assert_gates(name, out)


def _real_layers():
    from svr_amd.model import UNetMini, Unet
    return [(f"{nm}_{lname}", shape) for nm, cls, (H, W) in (("full", Unet, (256, 256)), ("mini", UNetMini, (240, 320)))
            for lname, shape in K.unet_layers(cls, 1, H, W)]


@pytest.mark.parametrize("idx", range(16 + 8))
def test_real_unet_layers_at_batch_1_against_f64(idx):
    """Every convolution of Unet (256 x 256) and UNetMini (240 x 320) at num_filters = 32, batch 1, as its ops see it: the
    variant is the one tests/golden/conv2d_unet_layers.json holds for it (the table the CPU test asserts through the query),
    forward / backward-data / weight gradient / db against float64 at the gates of the other cases.
    Encoder layers run LeakyReLU (conv1: none), decoder layers read conv2d_virtual's tensor (no activation), as the network does."""
    import json
    import os
    ops = _ops()
    lname, shape = _real_layers()[idx]
    rows = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv2d_unet_layers.json")))
    key = "full_256x256_b1" if lname.startswith("full_") else "mini_240x320_b1"
    row = [r for r in rows[key] if r[0] == lname.split("_", 1)[1]][0]
    assert row[1] == list(shape), (lname, row[1], shape)
    _assert_tags(ops, lname, shape, (), dict(zip(K.OPS, row[2:5])))
    act = 0 if (lname.endswith("_conv1") or "dconv" in lname) else 1
    _assert_gates(lname, _check_layer(ops, lname, shape, (), "unit", 1.0, None, (act,)))


NAN_CASES = [("f128_coal_2src", ()), ("mis_src1", ("src1",)), ("sm_nan", ()), ("s2_even", ()), ("s2_even", ("src0",)), ("sm_s2_even", ())]
NAN_SHAPES = {"sm_nan": (2, 9, 7, 8, 4, 2, 3, 1), "s2_even": (2, 6, 8, 8, 4, 40, 4, 2), "sm_s2_even": (2, 6, 8, 8, 4, 3, 4, 2)}


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("which", range(6))
def test_nan_in_the_input_reaches_exactly_its_window(which, act):
    """One NaN at pixel (0, 0) and one at (H-1, W-1), channel 0, of a two-source layer whose channel count is no multiple of 16,
    through both loaders (16-byte: loads from clamped coordinates, then selects; per element) and the small kernels, at k3 s1
    and at k4 s2 on even sides (where the clamped loads land on the NaN for taps that never own it): the
    non-finite outputs of the forward and of the weight gradient are exactly the float64 reference's, the rest meets the gate.
    ReLU keeps the NaN (cv_act; fmaxf alone would return 0)."""
    ops = _ops()
    name, mis = NAN_CASES[which]
    shape = NAN_SHAPES[name] if name in NAN_SHAPES else K.by_name(name)[1]
    B, H, W, C0, C1, Cout, k, stride = shape
    assert (C0 + C1) % 16 and C1
    want_vec = not mis
    assert K.query(ops, "fwd", shape, mis)["vec4"] == want_vec and K.query(ops, "bwd_weight", shape, mis)["vec4"] == want_vec
    s0, s1, w, b, dy = _inputs(shape, mis, 1.0, None, 77 + which)
    s0[0, 0, 0, 0] = float("nan")
    s0[B - 1, H - 1, W - 1, 0] = float("nan")
    _, y_ref, _, dw_ref, db_ref = _reference(s0, s1, w, b, dy, k, stride, act)
    planes = ops.Conv2dPlanes(w, stride)
    y = ops.conv2d_fwd(s0, s1, k, stride, act, planes, b)
    dw, db = ops.conv2d_bwd_weight(s0, s1, k, stride, act, dy, Cout)
    for got, ref, gate, what in ((y, y_ref, G_FWD, "y"), (dw, dw_ref, G_BWD, "dw"), (db, db_ref, G_DB, "db")):
        bad, rbad = ~torch.isfinite(got), ~torch.isfinite(ref)
        assert torch.equal(bad, rbad), (name, act, what, int(bad.sum()), int(rbad.sum()))
        assert _rel_err(torch.where(bad, 0, got), torch.where(rbad, 0, ref)) < gate, (name, act, what)
    rbad = ~torch.isfinite(dw_ref)
    if k == 3:
        # 2 x 2 output pixels per corner; taps (0..1, 0..1) reach pixel (0, 0) and (1..2, 1..2) the last one: 7 taps of channel 0
        assert int((~torch.isfinite(y_ref)).sum()) == 2 * 4 * Cout and int(rbad.sum()) == Cout * 7
    else:
        # k4 s2 on even sides: row 0 is read by the odd taps only (2 oy - 1 + ky = 0) and row H-1 by the even ones, but the loads
        # of row -1 (tap 0 at oy = 0) and of row H (tap 3 at the last oy) are CLAMPED onto them -- a loader that let a clamped
        # load through (a mask-multiply where the select belongs) would put NaN into taps (0, 0) and (3, 3), which stay finite here
        assert H % 2 == 0 and W % 2 == 0 and int((~torch.isfinite(y_ref)).sum()) == 2 * Cout
        assert rbad[:, 0].reshape(Cout, 16).any(0).tolist() == [i in (5, 10) for i in range(16)], rbad[0, 0]


@pytest.mark.parametrize("name,mis", [("f64_unsplit", ()), ("mis_dy", ("dy",)), ("m2_128_coal_split", ()), ("odd_s2", ()), ("sm_co2_k4_s", ())])
def test_nan_in_dy_reaches_exactly_its_window(name, mis):
    """the same for dY in backward-data: stride-1 and the four parity classes of stride 2, both loaders, split and unsplit"""
    ops = _ops()
    _, shape, cmis, tags, _ = K.by_name(name)
    assert tuple(cmis) == tuple(mis)
    B, H, W, C0, C1, Cout, k, stride = shape
    s0, s1, w, b, dy = _inputs(shape, mis, 1.0, None, _seed(name))
    dy[0, 0, 0, 0] = float("nan")
    dy[B - 1, dy.shape[1] - 1, dy.shape[2] - 1, 0] = float("nan")
    _, _, din_ref, _, _ = _reference(s0, s1, w, b, dy, k, stride, 0)
    din = ops.conv2d_bwd_data(s0, s1, k, stride, ops.Conv2dPlanes(w, stride), dy)
    bad, rbad = ~torch.isfinite(din), ~torch.isfinite(din_ref)
    assert 0 < int(rbad.sum()) < rbad.numel() and torch.equal(bad, rbad), (name, int(bad.sum()), int(rbad.sum()))
    assert _rel_err(torch.where(bad, 0, din), torch.where(rbad, 0, din_ref)) < G_BWD, name


@pytest.mark.parametrize("B,H,W,C0,C1,mis", [(2, 5, 7, 8, 4, ()), (1, 6, 5, 5, 3, ()), (2, 3, 4, 16, 0, ()), (2, 5, 7, 8, 4, ("src0",)), (1, 1, 1, 4, 0, ())])
@pytest.mark.parametrize("act,up", [(0, False), (1, False), (2, True), (1, True)])
def test_virtual_and_finish_bwd_against_f64(B, H, W, C0, C1, mis, act, up):
    """conv2d_virtual (activation, concatenation, x2 bilinear upsample) and conv2d_finish_bwd (upsample adjoint, derivative of
    the activation -- 0.2 / 0 at +-0, as torch --, channel split), float4 and per-element kernels; need0 / need1 give None where
    not asked and the same bits where asked."""
    ops = _ops()
    s0, s1, _, _, _ = _inputs((B, H, W, C0, C1, 8, 3, 1), mis, 1.0, None, B * 100 + H * 10 + C0 + act)
    l0 = s0.double().requires_grad_(True)
    l1 = s1.double().requires_grad_(True) if C1 else None
    v_ref = R.virtual_f64(l0, l1, act, up)
    V = ops.conv2d_virtual(s0, s1, act, up)
    assert V.shape == v_ref.shape and _rel_err(V, v_ref.detach()) < G_FWD
    assert torch.equal(V, ops.conv2d_virtual(s0, s1, act, up))
    g = torch.Generator(device="cuda").manual_seed(3)
    dv = torch.randn(V.shape, generator=g, device="cuda")
    refs = torch.autograd.grad(v_ref, [t for t in (l0, l1) if t is not None], dv.double())
    d0, d1 = ops.conv2d_finish_bwd(s0, s1, act, up, dv)
    assert _rel_err(d0, refs[0]) < G_FWD and (d1 is None) == (C1 == 0)
    if C1:
        assert _rel_err(d1, refs[1]) < G_FWD
        a0, a1 = ops.conv2d_finish_bwd(s0, s1, act, up, dv, need0=True, need1=False)
        assert a1 is None and torch.equal(a0, d0)
        a0, a1 = ops.conv2d_finish_bwd(s0, s1, act, up, dv, need0=False, need1=True)
        assert a0 is None and torch.equal(a1, d1)
    assert ops.conv2d_finish_bwd(s0, s1, act, up, dv, need0=False, need1=False) == (None, None)


@pytest.mark.parametrize("B,H,W,C0,C1,k,stride,act,up", [(2, 5, 7, 8, 4, 3, 1, 2, True), (1, 6, 5, 5, 3, 4, 2, 1, False), (2, 3, 3, 16, 0, 4, 2, 0, True)])
def test_explicit_path_im2col_col2im_against_f64(B, H, W, C0, C1, k, stride, act, up):
    """the explicit path's four kernels: the patch matrix and, from a gradient of it, the gradients of the two sources"""
    ops = _ops()
    s0, s1, _, _, _ = _inputs((B, H, W, C0, C1, 8, 3, 1), (), 1.0, None, H * 10 + C0)
    l0 = s0.double().requires_grad_(True)
    l1 = s1.double().requires_grad_(True) if C1 else None
    pm_ref = R.patches(R.virtual_f64(l0, l1, act, up), k, stride)
    col, _ = ops.conv2d_im2col(s0, s1, k, stride, act, up)
    assert col.shape == pm_ref.shape and _rel_err(col, pm_ref.detach()) < G_FWD
    g = torch.Generator(device="cuda").manual_seed(4)
    dcol = torch.randn(col.shape, generator=g, device="cuda")
    refs = torch.autograd.grad(pm_ref, [t for t in (l0, l1) if t is not None], dcol.double())
    d0, d1 = ops.conv2d_col2im(s0, s1, k, stride, act, up, dcol)
    assert _rel_err(d0, refs[0]) < G_FWD and (C1 == 0 or _rel_err(d1, refs[1]) < G_FWD)


@pytest.mark.parametrize("Cout,C,k,stride,wscale", [(72, 12, 3, 1, 1e3), (7, 5, 3, 1, 1e-6), (40, 16, 4, 2, 1.0)])
def test_planes_from_every_preparation_give_the_same_forward_bits(Cout, C, k, stride, wscale):
    """Planes from conv2d_prepare_many, from Conv2dPlanes and from a weight that starts 4 bytes into its buffer (the
    w_amax_launch branch of svr_conv2d_prepare; 7 x 5 x 3 x 3 = 315 weights: the tail of ig_amax_kernel) give the same forward
    and backward-data bits, and that forward meets the float64 gate at the moved weight scale."""
    ops = _ops()
    shape = (2, 9, 7, C, 0, Cout, k, stride)
    s0, _, w, b, dy = _inputs(shape, (), 1.0, wscale, Cout + C)
    one = ops.Conv2dPlanes(w, stride)
    many = ops.conv2d_prepare_many([(w, stride, True), (w * 2, stride, True)])[0]
    off = ops.Conv2dPlanes(_mis(w, True), stride)
    assert not one.small
    ys = [ops.conv2d_fwd(s0, None, k, stride, 1, p, b) for p in (one, many, off)]
    ds = [ops.conv2d_bwd_data(s0, None, k, stride, p, dy) for p in (one, many, off)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]) and torch.equal(ds[0], ds[1]) and torch.equal(ds[0], ds[2])
    _, y_ref, din_ref, _, _ = _reference(s0, None, w, b, dy, k, stride, 1)
    assert _rel_err(ys[0], y_ref) < G_FWD and _rel_err(ds[0], din_ref) < G_BWD
