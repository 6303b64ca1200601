"""Every instantiation of the 3x3x3 forward / backward-data kernels of csrc/conv3d_bf16.hip that the launchers can select
(persistent 8x4x8 bricks, their one-brick VT2 form, {CK16, CK32} x {TN1, TN2, TN4}) against an f64 reference: the encoder's
real layers at batch 8, partial bricks, dead column tiles, prepared weight planes, run-to-run bit identity, the
SVR_CONV_PERSISTENT=0 switch (child process) and the index limit of persistent_bricks().  Each case first ASSERTS, through
svr_conv3d_k3_variant, that it runs the kernel it is named for (tests/_conv_cases.py; the CPU test
test_conv3d_variant_table_and_every_instantiation_is_reached checks that the cases reach all of them).

Inputs are made on the device; the reference is 27 shifted f64 matmuls with stock torch ops on the device and never calls a
project kernel; it is computed once per case and shared by the modes.  Errors are tests._golden.rel_err (max |a - b| / max |b|),
evaluated on the device.  Gates (those of test_conv3d_fwd_bwd, test_conv3d_backward_at_f32_level_f16x3s and
test_conv_epilogue_batchnorm_statistics in tests/test_gpu_kernels.py): 3e-6 for f32 / f16x3 / f16x3s / bf16x6, f16x3s also
<= 3 x the exact-f32 kernel's error + 1e-7, 5e-5 for bf16x3 backward-data, 1e-6 for the statistics.

Wall time of the file on one MI355X: 7 s for its 58 tests (a 64^3 batch-8 case, f64 reference included, stays under a second;
the child process of the SVR_CONV_PERSISTENT=0 test, 3 s, is the longest item).  Measured errors per variant: DESIGN.md section 4."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import _conv_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

FWD_MODES = ("f32", "f16x3", "bf16x6")
BWD_MODES = ("f32", "f16x3s", "bf16x3")
GATE = {"f32": 3e-6, "f16x3": 3e-6, "bf16x6": 3e-6, "f16x3s": 3e-6, "bf16x3": 5e-5}


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _rel_err(a, ref):
    """tests._golden.rel_err on the device: max |a - ref| / max |ref|, in f64"""
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def _inputs(B, dims, Ci, Co, gscale, seed, device="cuda"):
    """channels-last x (a ReLU output: exact zeros for the mask), w scaled 1 / sqrt(27 Ci), a bias and a gradient-like dout
    (magnitude gscale, per-voxel spread e^(+-2 sigma): f16 would overflow or flush without the kernels' scale)"""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, *dims, Ci, generator=g, device=device).relu_()
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g, device=device) / (27 * Ci) ** 0.5
    b = torch.randn(Co, generator=g, device=device)
    dy = torch.randn(B, *dims, Co, generator=g, device=device) * gscale
    dy *= torch.exp(2 * torch.randn(B, *dims, 1, generator=g, device=device))
    return x, w, b, dy


def _ref_fwd(x, w, b):
    """conv(x, w) + b before the ReLU, f64 (B,D,H,W,Co): out[v] = b + sum over taps of x[v + tap - 1] w[:, :, tap]^T"""
    B, D, H, W, Ci = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    wd = w.double()
    out = b.double().repeat(B * D * H * W, 1)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out.addmm_(xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Ci), wd[:, :, kz, ky, kx].t())
    return out.view(B, D, H, W, -1)


def _ref_bwd(dy, w):
    """d conv / d x applied to dy, f64 (B,D,H,W,Ci), unmasked: din[v] = sum over taps of dy[v - (tap - 1)] w[:, :, tap]"""
    B, D, H, W, Co = dy.shape
    dp = F.pad(dy.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    wd = w.double()
    out = torch.zeros(B * D * H * W, w.shape[1], dtype=torch.float64, device=dy.device)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out.addmm_(dp[:, 2 - kz:2 - kz + D, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, :].reshape(-1, Co), wd[:, :, kz, ky, kx])
    return out.view(B, D, H, W, -1)


def _assert_variant(ops, name, B, dims, Ci, Co, ftag, btag):
    """the kernel this case is there for is the kernel it runs; -> workgroup rows of the forward"""
    rows = None
    for op in K.FWD_OPS if ftag else ():
        v = ops.conv3d_k3_variant(op, B, dims, Ci, Co)
        assert K.tag(v) == ftag, (name, op, v)
        rows = v["workgroup_rows"]
    for op in K.BWD_OPS if btag else ():
        v = ops.conv3d_k3_variant(op, B, dims, Ci, Co)
        assert K.tag(v) == btag, (name, op, v)
    return rows


def _amax_is_exact(din):
    return float(din._svr_amax.view(torch.float32)) == float(din.abs().max())


FWD_CASES = [c for c in K.CASES if c[6]]
BWD_CASES = [c for c in K.CASES if c[7]]


@pytest.mark.parametrize("name,B,dims,Ci,Co,gscale,ftag,btag", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_against_f64(name, B, dims, Ci, Co, gscale, ftag, btag):
    """Forward in every mode, with and without the ReLU, against f64; the statistics epilogue returns the plain call's bits,
    one partial-sum row per workgroup row of the variant, and the sums of the F64 REFERENCE's output."""
    ops = _ops()
    rows = _assert_variant(ops, name, B, dims, Ci, Co, ftag, None)
    x, w, b, _ = _inputs(B, dims, Ci, Co, gscale, _seed(name))
    pre = _ref_fwd(x, w, b)
    err, serr = {}, {}
    for relu in (True, False):
        ref = pre.clamp_min(0) if relu else pre
        for mode in FWD_MODES:
            y = ops.conv3d_k3_fwd(x, w, b, relu=relu, mode=mode)
            assert y.shape == ref.shape and bool(torch.isfinite(y).all()), (mode, relu)
            err[mode, relu] = _rel_err(y, ref)
            if mode == "f16x3":
                y1, st = ops.conv3d_k3_fwd(x, w, b, relu=relu, mode=mode, want_stats=True)
                assert st is not None and torch.equal(y, y1), ("stats call: other bits", relu)
                assert st.blocks == rows and tuple(st.part.shape) == (rows, 2, Co), (st.blocks, rows)
                sums = st.part.sum(0)
                r2 = ref.reshape(-1, Co)
                serr[relu] = (_rel_err(sums[0], r2.sum(0)), _rel_err(sums[1], (r2 * r2).sum(0)))
    print(f"conv_paths fwd {name} [{ftag}] err={ {f'{m}/{int(r)}': f'{e:.2e}' for (m, r), e in err.items()} } "
          f"stats={ {int(r): (f'{a:.2e}', f'{q:.2e}') for r, (a, q) in serr.items()} }")
    for (mode, relu), e in err.items():
        assert e < GATE[mode], (name, mode, relu, err)
    for relu, (es, eq) in serr.items():
        assert es < 1e-6 and eq < 1e-6, (name, relu, serr)


@pytest.mark.parametrize("name,B,dims,Ci,Co,gscale,ftag,btag", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward_data_against_f64(name, B, dims, Ci, Co, gscale, ftag, btag):
    """Backward-data in every mode, unmasked and with the ReLU mask of x, against f64; f16x3s within 3x the exact-f32 kernel's
    error; the fused |max| of din (f16x3s) equals din.abs().max() bit for bit."""
    ops = _ops()
    _assert_variant(ops, name, B, dims, Ci, Co, None, btag)
    x, w, _, dy = _inputs(B, dims, Ci, Co, gscale, _seed(name))
    assert dy.numel() % 4 == 0
    ref = _ref_bwd(dy, w)
    refm = ref * (x > 0)
    err, amax_ok = {}, {}
    for mode in BWD_MODES:
        for masked in (False, True):
            din = ops.conv3d_k3_bwd_data(dy, w, mask=x if masked else None, mode=mode)
            assert din.shape == ref.shape and bool(torch.isfinite(din).all()), (mode, masked)
            err[mode, masked] = _rel_err(din, refm if masked else ref)
            if mode == "f16x3s":
                assert hasattr(din, "_svr_amax"), "the f16x3s kernel did not run"
                amax_ok[masked] = _amax_is_exact(din)
    print(f"conv_paths bwd {name} [{btag}] err={ {f'{m}/{int(k)}': f'{e:.2e}' for (m, k), e in err.items()} } amax={amax_ok}")
    for (mode, masked), e in err.items():
        assert e < GATE[mode], (name, mode, masked, err)
    for masked in (False, True):
        assert err["f16x3s", masked] < 3 * err["f32", masked] + 1e-7, (name, masked, err)
        assert amax_ok[masked], (name, masked, "fused |max| of din")


@pytest.mark.parametrize("name", ["real64_32_32", "part37_16_32", "real32_64_64", "tn4_128_128"])
def test_prepared_planes_give_the_same_bits(name):
    """include/svr_hip.h PREPARE / RUN on the persistent kernel (both directions), on TN2 and on TN4: a layer run with W == NULL
    on planes prepared ahead (ops.PreparedWeights) returns the bits of the one-call form."""
    ops = _ops()
    _, B, dims, Ci, Co, gscale, ftag, btag = K.by_name(name)
    _assert_variant(ops, name, B, dims, Ci, Co, ftag, btag)
    x, w, b, dy = _inputs(B, dims, Ci, Co, gscale, _seed(name))
    saved = ops.BACKWARD_CONV
    assert ops.FORWARD_CONV == "f16x3"
    try:
        for bwd, kind in (("f16x3s", "cbh"), ("bf16x3", "cb")):
            ops.BACKWARD_CONV = bwd
            ops.set_prepared(None)
            base = (ops.conv3d_k3_fwd(x, w, b), ops.conv3d_k3_bwd_data(dy, w, mask=x))
            prep = ops.PreparedWeights()
            prep.begin()
            prep.add_conv(w)
            prep.finish(torch.cuda.current_stream())
            ops.set_prepared(prep)
            assert prep.lookup("cf", w) is not None and prep.lookup(kind, w) is not None
            got = (ops.conv3d_k3_fwd(x, w, b), ops.conv3d_k3_bwd_data(dy, w, mask=x))
            assert torch.equal(base[0], got[0]), (name, "forward")
            assert torch.equal(base[1], got[1]), (name, bwd)
            if bwd == "f16x3s":
                assert _amax_is_exact(got[1])
    finally:
        ops.set_prepared(None)
        ops.BACKWARD_CONV = saved


@pytest.mark.parametrize("name", ["real64_32_32", "part37_16_32", "real32_64_64", "tn4_128_128"])
def test_runs_are_bit_identical(name):
    """The persistent kernel hands bricks to workgroups: the result must not depend on which one got which (nor may any other
    variant's): every mode twice, same bits, statistics partial sums included."""
    ops = _ops()
    _, B, dims, Ci, Co, gscale, ftag, btag = K.by_name(name)
    _assert_variant(ops, name, B, dims, Ci, Co, ftag, btag)
    x, w, b, dy = _inputs(B, dims, Ci, Co, gscale, _seed(name))

    def run():
        out = {("fwd", m): ops.conv3d_k3_fwd(x, w, b, mode=m) for m in FWD_MODES}
        out.update({("bwd", m, k): ops.conv3d_k3_bwd_data(dy, w, mask=x if k else None, mode=m) for m in BWD_MODES for k in (0, 1)})
        out["stats"] = ops.conv3d_k3_fwd(x, w, b, mode="f16x3", want_stats=True)[1].part
        return out

    first = run()
    filler = torch.randn(1 << 24, device="cuda").sum()       # other work in between
    second = run()
    assert bool(torch.isfinite(filler))
    for key in first:
        assert torch.equal(first[key], second[key]), (name, key)


# ---- SVR_CONV_PERSISTENT=0: the one-brick form of the 8x4x8 tile (conv3d_brick_x3_kernel<16, 1, 2, ., 2>) -----------------------
def _no_persistent_results(ops, name):
    """what parent and child both compute for a case: forward f16x3 (ReLU) where the shape allows, backward-data f16x3s and bf16x3
    (masked); + the variant tags the process saw"""
    _, B, dims, Ci, Co, gscale, ftag, btag = K.by_name(name)
    x, w, b, dy = _inputs(B, dims, Ci, Co, gscale, _seed(name))
    out, tags = {}, {}
    if ftag:
        tags["fwd_f16x3"] = K.tag(ops.conv3d_k3_variant("fwd_f16x3", B, dims, Ci, Co))
        out["fwd_f16x3"], st = ops.conv3d_k3_fwd(x, w, b, relu=True, mode="f16x3", want_stats=True)
        out["stats"] = st.part.sum(0)
    for mode in ("f16x3s", "bf16x3"):
        tags["bwd_data_" + mode] = K.tag(ops.conv3d_k3_variant("bwd_data_" + mode, B, dims, Ci, Co))
        out["bwd_" + mode] = ops.conv3d_k3_bwd_data(dy, w, mask=x, mode=mode)
    out["amax_ok"] = torch.tensor(_amax_is_exact(out["bwd_f16x3s"]))
    return (x, w, b, dy), out, tags


def _child(path):
    ops = _ops()
    res = {}
    for name in K.NO_PERSISTENT:
        _, out, tags = _no_persistent_results(ops, name)
        assert set(tags.values()) == {"VT2"}, (name, tags)
        res[name] = {k: v.cpu() for k, v in out.items()}
    torch.cuda.synchronize()
    torch.save(res, path)


def test_persistent_switch_off_in_a_child_process(tmp_path):
    """persistent_bricks() reads SVR_CONV_PERSISTENT once per process: ONE fresh child with SVR_CONV_PERSISTENT=0 runs the cases
    of K.NO_PERSISTENT on the VT2 kernels (it asserts so through the query) and saves its outputs; this process runs them on the
    persistent kernel.  Both are held to the f64 gates; whether the two kernels also agree bit for bit is reported."""
    ops = _ops()
    path = str(tmp_path / "no_persistent.pt")
    env = dict(os.environ, SVR_CONV_PERSISTENT="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--no-persistent-child", path], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    child = torch.load(path, map_location="cuda", weights_only=True)
    for name in K.NO_PERSISTENT:
        (x, w, b, dy), mine, tags = _no_persistent_results(ops, name)
        assert set(tags.values()) == {"P"}, (name, tags)
        refs = {}
        if "fwd_f16x3" in mine:
            refs["fwd_f16x3"] = _ref_fwd(x, w, b).clamp_min(0)
            r2 = refs["fwd_f16x3"].reshape(-1, refs["fwd_f16x3"].shape[-1])
            refs["stats"] = torch.stack((r2.sum(0), (r2 * r2).sum(0)))
        refs["bwd_f16x3s"] = refs["bwd_bf16x3"] = _ref_bwd(dy, w) * (x > 0)
        assert set(child[name]) == set(mine)
        for key, ref in refs.items():
            if key == "stats":
                em, ec = (max(_rel_err(o[key][i], ref[i]) for i in (0, 1)) for o in (mine, child[name]))
                gate = 1e-6
            else:
                em, ec = _rel_err(mine[key], ref), _rel_err(child[name][key], ref)
                gate = 5e-5 if key == "bwd_bf16x3" else 3e-6
            print(f"conv_paths no-persistent {name} {key}: persistent err={em:.2e} VT2 err={ec:.2e} "
                  f"same bits={torch.equal(mine[key], child[name][key])}")
            assert em < gate and ec < gate, (name, key, em, ec)
        assert bool(mine["amax_ok"]) and bool(child[name]["amax_ok"]), (name, "fused |max| of din")


# ---- the index limit of persistent_bricks() --------------------------------------------------------------------------------------
def _sample_voxels(B, dims, n_random, seed):
    """(N, 4) int64 [b, z, y, x]: the corners, a line across every face, the last voxels in memory order and n_random random ones"""
    D, H, W = dims
    g = torch.Generator().manual_seed(seed)
    v = [(B - 1 if i & 8 else 0, (D - 1) * (i & 1), (H - 1) * ((i >> 1) & 1), (W - 1) * ((i >> 2) & 1)) for i in range(16)]
    for z in (0, D - 1):
        v += [(B - 1, z, H // 2, xx) for xx in range(W)]
    for y in (0, H - 1):
        v += [(B - 1, zz, y, W // 2) for zz in range(D)]
    for xx in (0, W - 1):
        v += [(B - 1, D // 2, yy, xx) for yy in range(H)]
    v += [(B - 1, D - 1, H - 1, xx) for xx in range(max(0, W - 64), W)]
    t = torch.tensor(v, dtype=torch.int64)
    r = torch.stack([torch.randint(0, n, (n_random,), generator=g) for n in (B, D, H, W)], 1)
    return torch.cat((t, r))


def _gather_taps(t, vox, shift):
    """rows t[b, z + shift[0], y + shift[1], x + shift[2], :] of the sample voxels in f64, zero outside the volume"""
    _, D, H, W, _ = t.shape
    z, y, x = vox[:, 1] + shift[0], vox[:, 2] + shift[1], vox[:, 3] + shift[2]
    ok = (z >= 0) & (z < D) & (y >= 0) & (y < H) & (x >= 0) & (x < W)
    rows = t[vox[:, 0], z.clamp(0, D - 1), y.clamp(0, H - 1), x.clamp(0, W - 1)].double()
    return rows * ok[:, None]


@pytest.mark.parametrize("name,B,dims,Ci,Co,ftag,btag", K.LIMIT, ids=[c[0] for c in K.LIMIT])
def test_index_limit_of_the_persistent_kernel(name, B, dims, Ci, Co, ftag, btag):
    """persistent_bricks() keeps the persistent kernel's 32-bit offsets inside D H W max(Ci, Co) < 2^30: a shape just over must
    take the VT2 form in this process, one just under stays persistent (the query says which).  The 4.4 GB operand is where a
    32-bit byte offset would wrap: a SAMPLE of output voxels (corners, a line across every face, the last voxels in memory,
    4096 random ones) against f64 computed for those voxels only.  Skipped only if the device cannot hold the tensors."""
    ops = _ops()
    _assert_variant(ops, name, B, dims, Ci, Co, ftag, btag)
    n = B * dims[0] * dims[1] * dims[2]
    need = 4 * n * (Ci + Co) * 3 + (2 << 30)          # the operands, the output and the generators' temporaries
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip(f"{need / 2 ** 30:.0f} GiB of device memory needed for {name}")
    x, w, b, dy = _inputs(B, dims, Ci, Co, 1e-3, _seed(name))
    vox = _sample_voxels(B, dims, 4096, _seed(name)).cuda()
    bi, zi, yi, xi = vox.unbind(1)
    wd = w.double()
    taps = [(kz, ky, kx) for kz in range(3) for ky in range(3) for kx in range(3)]
    if ftag:
        del dy
        ref = b.double().repeat(vox.shape[0], 1)
        for kz, ky, kx in taps:
            ref.addmm_(_gather_taps(x, vox, (kz - 1, ky - 1, kx - 1)), wd[:, :, kz, ky, kx].t())
        ref.clamp_min_(0)
        y = ops.conv3d_k3_fwd(x, w, b, relu=True, mode="f16x3")
        e = _rel_err(y[bi, zi, yi, xi], ref)
        print(f"conv_paths limit {name} [{ftag}] f16x3 err={e:.2e} over {vox.shape[0]} voxels")
        assert e < GATE["f16x3"], (name, e)
    else:
        ref = torch.zeros(vox.shape[0], Ci, dtype=torch.float64, device="cuda")
        for kz, ky, kx in taps:
            ref.addmm_(_gather_taps(dy, vox, (1 - kz, 1 - ky, 1 - kx)), wd[:, :, kz, ky, kx])
        ref *= x[bi, zi, yi, xi] > 0
        for mode in ("f16x3s", "bf16x3"):
            din = ops.conv3d_k3_bwd_data(dy, w, mask=x, mode=mode)
            e = _rel_err(din[bi, zi, yi, xi], ref)
            print(f"conv_paths limit {name} [{btag}] {mode} err={e:.2e} over {vox.shape[0]} voxels")
            assert e < GATE[mode], (name, mode, e)
            if mode == "f16x3s":
                assert _amax_is_exact(din), (name, "fused |max| of din")
            del din


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--no-persistent-child", sys.argv
    _child(sys.argv[2])
