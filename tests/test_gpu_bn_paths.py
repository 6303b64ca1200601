"""The BatchNorm kernels (csrc/bn_pool.hip) against float64 at the shapes and statistics the UNet gives them.

tests/test_gpu_kernels.py::test_bn_pool_fwd_bwd pins the IF-Net encoder's use: post-ReLU input, relu_mask=True,
C in {16..128}, a few workgroups.  The UNet (model/unet.py _BN2dFn) calls the same kernels with D = 1, no pool,
relu_mask=False, C from 4 to 256, on raw convolution outputs (any mean) with as few as 4 values per channel.  Every
case here draws its input in float64 from a seeded generator, rounds it to float32, and computes the float64
reference (F.batch_norm, F.max_pool3d, torch.autograd.grad on the CPU) from the rounded values.

Not reachable at a test's size: the 65535*16 grid clamp of svr_bn_bwd_apply (it needs more than 2^20 * CL pool cells
with CL >= 4, i.e. > 33M voxels even at C = 256).  The apply kernel's loop is the reduce kernel's loop, which
test_reduce_grid_clamps runs more than once per thread.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import _golden as G
from tests.test_bn_stats_cpu import CONST_CH, ILL_SHAPES, gate, ill_conditioned_input     # section 4: same inputs, same gate

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _cl(v):  # NCDHW -> channels-last (B,D,H,W,C) on the GPU
    return v.permute(0, 2, 3, 4, 1).contiguous().cuda()


def _ncdhw(v):  # channels-last GPU -> NCDHW CPU
    return v.cpu().permute(0, 4, 1, 2, 3).contiguous()


def _r32(t64):  # float64 draw -> the float32 value the kernel sees (kept as float32)
    return t64.float()


def _well_conditioned(B, dims, C, seed):
    """randn with per-channel scales in [0.5, 2] and offsets in [-1, 1]; gamma in [0.5, 1.5], beta in [-0.5, 0.5]."""
    g = torch.Generator().manual_seed(seed)
    scale = 0.5 * 4.0 ** torch.rand(C, generator=g, dtype=torch.float64)
    offs = torch.rand(C, generator=g, dtype=torch.float64) * 2 - 1
    x = torch.randn(B, C, *dims, generator=g, dtype=torch.float64) * scale.view(1, C, 1, 1, 1) + offs.view(1, C, 1, 1, 1)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    rm = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn(B, C, *dims, generator=g, dtype=torch.float64)
    dp = torch.randn(B, C, *(d // 2 for d in dims), generator=g, dtype=torch.float64)
    return tuple(_r32(t) for t in (x, gamma, beta, rm, rv, dy, dp))


def _reference(x, gamma, beta, rm, rv, dy, dp, training, pool, relu_mask, momentum=0.1):
    """float64 forward and backward of F.batch_norm (+ F.max_pool3d(2)) from the float32 inputs."""
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xd, rm64, rv64, gd, bd, training, momentum, EPS)
    obj = (y * dy.double()).sum()
    p = None
    if pool:
        p = F.max_pool3d(y, 2)
        obj = obj + (p * dp.double()).sum()
    gx, gg, gb = torch.autograd.grad(obj, (xd, gd, bd))
    if relu_mask:
        gx = gx * (x > 0)
    return y.detach(), None if p is None else p.detach(), rm64, rv64, gx, gg, gb


def _check(x, gamma, beta, rm, rv, dy, dp, training, pool, relu_mask):
    """forward, running statistics, dx, dgamma, dbeta of ops.bn_forward / ops.bn_backward at test_bn_pool_fwd_bwd's gates"""
    ops = _ops()
    y_ref, p_ref, rm_ref, rv_ref, gx, gg, gb = _reference(x, gamma, beta, rm, rv, dy, dp, training, pool, relu_mask)
    rm_g, rv_g = rm.clone().cuda(), rv.clone().cuda()
    xc = _cl(x)
    y, pooled, argmax, ss, mean = ops.bn_forward(xc, gamma.cuda(), beta.cuda(), rm_g, rv_g, training, eps=EPS, want_pool=pool)
    e = {"y": G.rel_err(_ncdhw(y).numpy(), y_ref.numpy()),
         "running_mean": G.rel_err(rm_g.cpu().numpy(), rm_ref.numpy()),
         "running_var": G.rel_err(rv_g.cpu().numpy(), rv_ref.numpy())}
    if pool:
        e["pooled"] = G.rel_err(_ncdhw(pooled).numpy(), p_ref.numpy())
    else:
        assert pooled is None and argmax is None
    dx, dgamma, dbeta = ops.bn_backward(xc, _cl(dy), _cl(dp) if pool else None, argmax, mean, ss, relu_mask=relu_mask,
                                        training=training)
    e["dx"] = G.rel_err(_ncdhw(dx).numpy(), gx.numpy())
    e["dgamma"] = G.rel_err(dgamma.cpu().numpy(), gg.numpy())
    e["dbeta"] = G.rel_err(dbeta.cpu().numpy(), gb.numpy())
    print({k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] < 2e-6 and e.get("pooled", 0.0) < 2e-6, e
    assert e["running_mean"] < 1e-6 and e["running_var"] < 1e-6, e
    assert e["dx"] < 1e-5 and e["dgamma"] < 1e-5 and e["dbeta"] < 1e-5, e
    if not training:
        assert torch.equal(rm_g.cpu(), rm) and torch.equal(rv_g.cpu(), rv), "eval mode must not touch the running statistics"


# ---------------------------------------------------------------------------------------- 1. the UNet form
# (B, H, W, C): the Unet bottleneck at B = 2 and B = 1, two rows, odd extents (every cell cut in z, some in y and x),
# and the extreme thread mappings C = 4 (Q = 1, RL = 256) and C = 8 (Q = 2)
UNET_SHAPES = [(2, 2, 2, 256), (1, 2, 2, 256), (2, 1, 1, 128), (2, 3, 5, 64), (1, 7, 1, 32), (3, 4, 4, 8), (2, 5, 3, 4)]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,H,W,C", UNET_SHAPES)
def test_unet_form(B, H, W, C, training):
    """D = 1, want_pool=False, relu_mask=False; eval = training=False in the forward and bit 1 of relu_mask in the
    backward (dx = scale * dy)."""
    _check(*_well_conditioned(B, (1, H, W), C, 1000 + B * 100 + H * 10 + W + C), training=training, pool=False, relu_mask=False)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B,H,W,C", UNET_SHAPES)
def test_unet_wrapper(B, H, W, C, training):
    """model.unet._BN2dFn.apply on a (B,H,W,C) tensor with a non-contiguous dy: the wrapper's views, .contiguous() and
    num_batches_tracked."""
    _ops()
    from svr_amd.model.unet import _BN2dFn
    x, gamma, beta, rm, rv, dy, dp = _well_conditioned(B, (1, H, W), C, 2000 + B * 100 + H * 10 + W + C)
    y_ref, _, rm_ref, rv_ref, gx, gg, gb = _reference(x, gamma, beta, rm, rv, dy, dp, training, False, False)
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=0.1).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    bn.train(training)
    xg = x[:, :, 0].permute(0, 2, 3, 1).contiguous().cuda().requires_grad_(True)          # (B,H,W,C)
    y = _BN2dFn.apply(xg, bn.weight, bn.bias, bn)
    assert y.shape == (B, H, W, C)
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    dy_nc = dy[:, :, 0].permute(0, 3, 2, 1).contiguous().cuda().permute(0, 2, 1, 3)     # (B,H,W,C) view of a (B,W,H,C) buffer
    assert dy_nc.shape == y.shape and (not dy_nc.is_contiguous() or H == 1 or W == 1)
    dx, dgamma, dbeta = torch.autograd.grad(y, (xg, bn.weight, bn.bias), dy_nc)
    nchw = lambda t: t.detach().cpu().permute(0, 3, 1, 2).unsqueeze(2)
    e = {"y": G.rel_err(nchw(y).numpy(), y_ref.numpy()),
         "running_mean": G.rel_err(bn.running_mean.cpu().numpy(), rm_ref.numpy()),
         "running_var": G.rel_err(bn.running_var.cpu().numpy(), rv_ref.numpy()),
         "dx": G.rel_err(nchw(dx).numpy(), gx.numpy()),
         "dgamma": G.rel_err(dgamma.cpu().numpy(), gg.numpy()), "dbeta": G.rel_err(dbeta.cpu().numpy(), gb.numpy())}
    print({k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] < 2e-6 and e["running_mean"] < 1e-6 and e["running_var"] < 1e-6, e
    assert e["dx"] < 1e-5 and e["dgamma"] < 1e-5 and e["dbeta"] < 1e-5, e


@pytest.mark.parametrize("C", [4, 32, 256])
def test_statistics_alone_then_finalize(C):
    """svr_bn_stats (bn_stats_final_kernel without its finalize part), then ops.bn_forward(stats=...) -> bn_finalize_kernel
    in training mode, the scale / shift apply and a backward with the f32 mean alone."""
    ops = _ops()
    from svr_amd import _lib
    B, dims = 2, (1, 3, 5)
    x, gamma, beta, rm, rv, dy, dp = _well_conditioned(B, dims, C, 2500 + C)
    xc = _cl(x)
    rows = B * 15
    l = _lib.lib()
    stats = torch.empty(2 * C, device="cuda", dtype=torch.float64)
    ws = torch.empty(l.svr_bn_stats_workspace(rows, C), device="cuda", dtype=torch.uint8)
    _lib.check(l.svr_bn_stats(_lib.ptr(xc), _lib.ptr(stats), rows, C, _lib.ptr(ws), _lib.stream()), "bn_stats")
    x64 = x.double()
    e_mean = G.rel_err(stats[:C].cpu().numpy(), x64.mean((0, 2, 3, 4)).numpy())
    e_var = G.rel_err(stats[C:].cpu().numpy(), x64.var((0, 2, 3, 4), unbiased=False).numpy())
    print(f"mean {e_mean:.2e} var {e_var:.2e}")
    assert e_mean < 1e-6 and e_var < 1e-6
    y_ref, _, rm_ref, rv_ref, gx, gg, gb = _reference(x, gamma, beta, rm, rv, dy, dp, True, False, False)
    rm_g, rv_g = rm.clone().cuda(), rv.clone().cuda()
    y, _, _, ss, mean = ops.bn_forward(xc, gamma.cuda(), beta.cuda(), rm_g, rv_g, True, eps=EPS, want_pool=False, stats=stats)
    assert mean.numel() == C
    assert G.rel_err(_ncdhw(y).numpy(), y_ref.numpy()) < 2e-6
    assert G.rel_err(rm_g.cpu().numpy(), rm_ref.numpy()) < 1e-6 and G.rel_err(rv_g.cpu().numpy(), rv_ref.numpy()) < 1e-6
    dx, dgamma, dbeta = ops.bn_backward(xc, _cl(dy), None, None, mean, ss, relu_mask=False)
    assert G.rel_err(_ncdhw(dx).numpy(), gx.numpy()) < 1e-5
    assert G.rel_err(dgamma.cpu().numpy(), gg.numpy()) < 1e-5 and G.rel_err(dbeta.cpu().numpy(), gb.numpy()) < 1e-5


# ---------------------------------------------------------------------------------------- 2. launch geometry
@pytest.mark.parametrize("B,dims,C,training", [
    (1, (1, 1, 257), 32, True),        # rows = 257: two statistics blocks, the second one row short of the first
    (1, (1, 1, 257), 32, False),
    (1, (1, 12, 25), 32, True),        # rows = 300: two blocks of 150, no full 256-row block
    (1, (1, 1, 2048 * 256 + 5), 4, True),   # stats_blocks clamps at STAT_BLOCKS_MAX; rows_per_block = 257 does not divide the rows
    (1, (1, 184, 184), 256, True),     # 8464 cells > 2048 * CL (CL = 4): bwd_blocks clamps, bn_bwd_kernel<false> loops
])
def test_reduce_grid_clamps(B, dims, C, training):
    _check(*_well_conditioned(B, dims, C, 3000 + dims[2] + C), training=training, pool=False, relu_mask=False)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu_mask", [True, False], ids=["mask", "nomask"])
def test_pooled_widest_channel_count(relu_mask, training):
    """the pooled form (argmax routing, cut cells in z and y) at C = 256"""
    _check(*_well_conditioned(2, (9, 7, 10), 256, 4000), training=training, pool=True, relu_mask=relu_mask)


# ---------------------------------------------------------------------------------------- 3. pool semantics
def _decode_argmax(idx, dims):
    """F.max_pool3d's flat input index (B,C,Dp,Hp,Wp) -> the kernel's byte: (z & 1) << 2 | (y & 1) << 1 | (x & 1)"""
    D, H, W = dims
    z, y, x = idx // (H * W), (idx // W) % H, idx % W
    return ((z & 1) << 2 | (y & 1) << 1 | (x & 1)).to(torch.uint8)


def _tie_volume(seed):
    B, C, dims = 1, 16, (4, 6, 5)
    x, gamma, beta, rm, rv, dy, dp = _well_conditioned(B, dims, C, seed)
    g = torch.Generator().manual_seed(seed + 1)
    D, H, W = dims
    # channel 0: constant over whole cells (all eight voxels tie; W = 5 leaves a cut, unpooled column)
    cellv = _r32(torch.randn(D // 2, H // 2, (W + 1) // 2, generator=g, dtype=torch.float64))
    x[0, 0] = cellv.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :, :W]
    # channel 1: two equal maxima per cell, at two random corners
    for cz in range(D // 2):
        for cy in range(H // 2):
            for cx in range(W // 2):
                cell = x[0, 1, 2 * cz:2 * cz + 2, 2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2]
                k = torch.randperm(8, generator=g)[:2]
                top = cell.max() + 1.0
                for kk in k.tolist():
                    cell[kk >> 2, (kk >> 1) & 1, kk & 1] = top
    return x, gamma, beta, rm, rv, dy, dp, dims


def test_pool_exact_ties_route_like_max_pool3d():
    """Equal maxima: dpooled must land on the voxel F.max_pool3d(return_indices=True) picks (the first in z,y,x order)."""
    ops = _ops()
    x, gamma, beta, rm, rv, dy, dp, dims = _tie_volume(5000)
    y_ref, p_ref, _, _, gx, gg, gb = _reference(x, gamma, beta, rm, rv, dy, dp, True, True, False)
    _, idx = F.max_pool3d(y_ref, 2, return_indices=True)
    # the float64 reference really has the ties: whole cells of channel 0 and two voxels of channel 1 equal the maximum
    win = y_ref[..., :4] == p_ref.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    cells = win.view(1, 16, 2, 2, 3, 2, 2, 2).sum((3, 5, 7))
    assert torch.all(cells[0, 0] == 8) and torch.all(cells[0, 1] == 2) and torch.all(cells[0, 2:] == 1)
    xc = _cl(x)
    rm_g, rv_g = rm.clone().cuda(), rv.clone().cuda()
    y, pooled, argmax, ss, mean = ops.bn_forward(xc, gamma.cuda(), beta.cuda(), rm_g, rv_g, True, eps=EPS, want_pool=True)
    assert G.rel_err(_ncdhw(pooled).numpy(), p_ref.numpy()) < 2e-6
    assert torch.equal(_ncdhw(argmax), _decode_argmax(idx, dims))
    dx, dgamma, dbeta = ops.bn_backward(xc, _cl(dy), _cl(dp), argmax, mean, ss, relu_mask=False)
    d = (_ncdhw(dx).double() - gx).abs()
    assert float(d.max()) < 1e-5 * float(gx.abs().max()), "dx, voxel by voxel"
    assert G.rel_err(dgamma.cpu().numpy(), gg.numpy()) < 1e-5 and G.rel_err(dbeta.cpu().numpy(), gb.numpy()) < 1e-5
    # the routing alone: frozen statistics and no dy, so dx = scale * dpooled on the chosen voxel and exactly 0 elsewhere
    ye_ref, pe_ref, _, _, gxe, _, _ = _reference(x, gamma, beta, rm, rv, torch.zeros_like(dy), dp, False, True, False)
    _, idx_e = F.max_pool3d(ye_ref, 2, return_indices=True)
    _, _, am_e, ss_e, mean_e = ops.bn_forward(xc, gamma.cuda(), beta.cuda(), rm.clone().cuda(), rv.clone().cuda(), False, eps=EPS,
                                              want_pool=True)
    assert torch.equal(_ncdhw(am_e), _decode_argmax(idx_e, dims))
    dxe = _ncdhw(ops.bn_backward(xc, None, _cl(dp), am_e, mean_e, ss_e, relu_mask=False, training=False)[0])
    assert torch.equal(dxe != 0, gxe != 0), "dpooled landed on another voxel than max_pool3d's"
    assert G.rel_err(dxe.numpy(), gxe.numpy()) < 1e-5


def test_pool_nan_propagates_with_aten_argmax():
    """One NaN voxel (not the cell's first) in an otherwise finite cell: pooled is NaN there and the argmax is that voxel
    (ATen max_pool3d: val > max || isnan(val)).  Eval mode, so scale and shift stay finite."""
    ops = _ops()
    B, C, dims = 1, 16, (4, 6, 5)
    x, gamma, beta, rm, rv, dy, dp = _well_conditioned(B, dims, C, 6000)
    # (channel, cell z, y, x, corner k != 0): every corner but the first, in several lanes of the float4 and several cells
    spots = [(0, 0, 0, 0, 1), (1, 0, 1, 1, 2), (2, 1, 2, 0, 3), (3, 1, 0, 1, 4), (5, 0, 2, 1, 5), (10, 1, 1, 0, 6), (15, 0, 0, 1, 7)]
    for c, cz, cy, cx, k in spots:
        x[0, c, 2 * cz + (k >> 2), 2 * cy + ((k >> 1) & 1), 2 * cx + (k & 1)] = float("nan")
    y_ref = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, EPS)
    p_ref, idx = F.max_pool3d(y_ref, 2, return_indices=True)
    assert int(torch.isnan(p_ref).sum()) == len(spots)
    rm_g, rv_g = rm.clone().cuda(), rv.clone().cuda()
    y, pooled, argmax, ss, mean = ops.bn_forward(_cl(x), gamma.cuda(), beta.cuda(), rm_g, rv_g, False, eps=EPS, want_pool=True)
    assert bool(torch.isfinite(ss).all()) and bool(torch.isfinite(mean).all())
    pooled, argmax, y = _ncdhw(pooled), _ncdhw(argmax), _ncdhw(y)
    for c, cz, cy, cx, k in spots:
        assert torch.isnan(pooled[0, c, cz, cy, cx]) and int(argmax[0, c, cz, cy, cx]) == k, (c, cz, cy, cx, k)
    assert torch.equal(torch.isnan(pooled), torch.isnan(p_ref)) and torch.equal(torch.isnan(y), torch.isnan(y_ref))
    assert torch.equal(argmax, _decode_argmax(idx, dims))
    assert G.rel_err(torch.nan_to_num(pooled).numpy(), torch.nan_to_num(p_ref).numpy()) < 2e-6
    assert G.rel_err(torch.nan_to_num(y).numpy(), torch.nan_to_num(y_ref).numpy()) < 2e-6


# ---------------------------------------------------------------------------------------- 4. ill-conditioned statistics
# Worst per-channel relative error over the channels of one mean/std group, measured on an MI355X: kernel / stock /
# before.  "stock" is float32 torch.native_batch_norm on the CPU on the same tensor; "before" is the kernel this file was
# written against (sums of x and x^2, var = E[x^2] - mean^2 of float32 squares, f32 mean in the backward, y = x * scale +
# shift).  "alt" is the channel that alternates between 3.0 and 3.01 (mean/std = 601).
#
# unbiased variance
#  mean/std   rows = 2                   rows = 8                   rows = 64                  rows = 4096
#      0      6.3e-8 / 6.9e-8 / 1.6e-5   1.3e-7 / 3.3e-8 / 5.5e-8   5.9e-8 / 3.1e-8 / 4.5e-8   5.5e-8 / 5.5e-8 / 3.7e-8
#      1      8.3e-8 / 5.0e-8 / 6.2e-3   8.8e-8 / 5.3e-8 / 1.5e-7   5.7e-8 / 5.7e-8 / 6.2e-8   7.8e-8 / 4.8e-8 / 5.1e-8
#    -10      4.0e-8 / 6.5e-8 / 1.6e-3   5.8e-8 / 7.5e-8 / 3.0e-6   3.7e-8 / 7.5e-8 / 1.6e-6   3.8e-8 / 8.7e-8 / 6.4e-7
#     10      4.2e-8 / 4.2e-8 / 1.4e-1   5.4e-8 / 1.0e-7 / 7.3e-7   2.8e-8 / 5.7e-8 / 1.1e-6   1.2e-8 / 1.2e-8 / 7.9e-7
#    100      4.8e-8 / 6.4e-8 / 7.9e-3   3.9e-8 / 8.7e-8 / 3.0e-4   5.5e-8 / 5.5e-8 / 2.5e-4   1.2e-8 / 1.2e-8 / 2.9e-5
#   -100      4.4e-8 / 4.4e-8 / 2.5e-1   5.5e-8 / 9.1e-8 / 2.5e-4   3.7e-8 / 3.7e-8 / 2.4e-4   3.0e-8 / 3.0e-8 / 9.5e-5
#   1000      5.7e-8 / 5.7e-8 / 2.8e-2   5.9e-8 / 5.9e-8 / 3.5e-2   4.3e-8 / 6.0e-8 / 3.7e-2   5.9e-8 / 4.0e-8 / 3.7e-3
#    alt      9.7e-9 / 9.7e-9 / 6.8e-3   5.7e-10/ 5.7e-10/ 6.8e-3   1.5e-8 / 1.5e-8 / 6.8e-3   1.2e-7 / 2.8e-8 / 6.8e-3
# invstd against 1 / sqrt(var64 + eps)
#      0      7.3e-8 / 3.9e-8 / 7.8e-6   8.0e-8 / 4.8e-8 / 5.0e-8   7.1e-8 / 5.9e-8 / 5.1e-8   4.0e-8 / 4.0e-8 / 4.0e-8
#      1      7.0e-8 / 2.8e-8 / 2.1e-3   3.6e-8 / 3.6e-8 / 1.1e-7   5.3e-8 / 5.3e-8 / 3.7e-8   3.7e-8 / 3.7e-8 / 3.5e-8
#    -10      6.2e-8 / 4.2e-8 / 8.0e-4   3.1e-8 / 3.1e-8 / 1.5e-6   3.9e-8 / 4.2e-8 / 8.6e-7   3.8e-8 / 5.2e-8 / 3.5e-7
#     10      5.6e-8 / 1.6e-8 / 2.9e-2   4.5e-8 / 6.5e-8 / 3.3e-7   3.1e-8 / 4.1e-8 / 5.8e-7   3.8e-8 / 3.8e-8 / 4.2e-7
#    100      7.9e-8 / 4.5e-8 / 3.9e-3   4.3e-8 / 4.3e-8 / 1.5e-4   3.4e-8 / 3.4e-8 / 1.3e-4   2.4e-8 / 2.4e-8 / 1.5e-5
#   -100      6.8e-8 / 5.7e-8 / 1.5e-1   6.9e-8 / 1.9e-8 / 1.2e-4   3.2e-8 / 3.2e-8 / 1.2e-4   3.2e-8 / 3.8e-8 / 4.7e-5
#   1000      4.4e-8 / 4.4e-8 / 1.4e-2   4.4e-8 / 4.4e-8 / 1.7e-2   4.1e-8 / 4.1e-8 / 1.9e-2   5.9e-8 / 4.8e-8 / 1.8e-3
#    alt      5.5e-8 / 3.6e-8 / 2.4e-3   5.5e-8 / 3.6e-8 / 2.4e-3   5.5e-8 / 3.6e-8 / 2.4e-3   3.6e-8 / 3.6e-8 / 2.4e-3
# worst over all of the above channels and row counts (measures as in the test's docstring):
#   y 1.3e-7 / 2.0e-4 / 1.3e-1    dx 1.8e-7 / 1.4e-4 / 2.6e-1    dgamma 1.3e-7 / 5.6e-5 / 1.5e-1    dbeta 4.7e-8 / 5.0e-8 / 5.0e-8
#   the mean the backward centres with, in units of std: 5.5e-8 / 1.4e-4 / 1.4e-4
# The constant channel: var = 0 and y = beta exactly at every row count; before: y off by up to 7e-2 |beta|, and at 4096
# rows a mean 2e-2 std off the (constant) value.


def _per_channel(a, b, scale=None):
    """max over a channel of |a - b| divided by `scale` (default: the channel's max |b|); a, b (B,C,...) or (C,)"""
    a, b = a.double(), b.double()
    if a.dim() == 1:
        d, m = (a - b).abs(), b.abs()
    else:
        red = [i for i in range(a.dim()) if i != 1]
        d, m = (a - b).abs().amax(red), b.abs().amax(red)
    return d / (m if scale is None else scale).clamp_min(1e-300)


@pytest.mark.parametrize("shape", ILL_SHAPES, ids=[f"rows{np.prod(s)}" for s in ILL_SHAPES])
def test_ill_conditioned_statistics(shape):
    """ops.bn_forward(training=True, stats=None) -> svr_bn_stats_finalize on channels whose mean/std runs up to 1000, a
    constant channel and a two-valued one, per channel against float64.  The gate is not chosen from the kernel: stock
    float32 batch norm on the CPU runs on the same tensor, and the kernel may be 4x worse than it (another, equally
    sound summation order) or 1e-6 (the bar test_bn_pool_fwd_bwd sets for the running statistics), whichever is larger.

    momentum = 1 makes running_mean / running_var the batch mean / unbiased variance; ss[2C:3C] is invstd.

    Error measures.  var, invstd: |a - ref| / |ref| per channel; the running mean: |a - ref| / max(|ref|, std) (the mean
    of a centred channel is a sum of values of the size of std, not of its own size).  The mean handed to the backward is
    measured in units of the channel's standard deviation (that is what xh = (a - mu) * invstd turns its error into).  y: max |y -
    ref| over the channel / max |ref|.  dx, dgamma, dbeta: the error over the magnitude of the terms that are summed, not
    of the sum -- scale * max|dy| for dx, sum |dy| for dbeta and for dgamma (xhat has unit rms).  With two rows dx is (dy0 -
    dy1) / 2 * eps / (var + eps), 1e-5 of its terms, so an error relative to dx itself would measure the cancellation
    (which stock float32 has too, by luck more or less than the kernel), not the kernel.

    The constant channel: var = 0 exactly, invstd = 1/sqrt(eps) to 1e-6, and y = beta bit for bit (x - mean is 0 before
    anything is scaled; a scale / shift form would leave the rounding of shift = beta - 1000.1 * 316 * gamma, ~1e-2).
    """
    ops = _ops()
    x, gamma, beta, groups = ill_conditioned_input(shape)
    C = x.shape[1]
    rows = x.numel() // C
    g = torch.Generator().manual_seed(7000 + rows)
    dy = _r32(torch.randn(x.shape, generator=g, dtype=torch.float64))
    # float64
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y64 = F.batch_norm(xd, rm64, rv64, gd, bd, True, 1.0, EPS)
    gx64, gg64, gb64 = torch.autograd.grad((y64 * dy.double()).sum(), (xd, gd, bd))
    var_b = x.double().var((0, 2, 3, 4), unbiased=False)
    inv64 = 1.0 / torch.sqrt(var_b + EPS)
    std64 = torch.sqrt(var_b + EPS)
    t_dx = (gamma.double() * inv64) * dy.double().abs().amax((0, 2, 3, 4))
    t_db = dy.double().abs().sum((0, 2, 3, 4))
    t_dg = t_db

    def errors(y, rmean, rvar, invstd, mean_bwd, dx, dg, db):
        return {"var": _per_channel(rvar, rv64), "inv": _per_channel(invstd, inv64),
                "mean": _per_channel(rmean, rm64, torch.maximum(rm64.abs(), std64)),
                "mean_bwd": _per_channel(mean_bwd, rm64, std64), "y": _per_channel(y, y64.detach()),
                "dx": _per_channel(dx, gx64, t_dx), "dgamma": _per_channel(dg, gg64, t_dg), "dbeta": _per_channel(db, gb64, t_db)}

    # stock float32 on the CPU
    xs, gs, bs = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_s, rv_s = torch.zeros(C), torch.ones(C)
    y_s, mean_s, inv_s = torch.native_batch_norm(xs, gs, bs, rm_s, rv_s, True, 1.0, EPS)
    gx_s, gg_s, gb_s = torch.autograd.grad(y_s, (xs, gs, bs), dy)
    stock = errors(y_s.detach(), rm_s, rv_s, inv_s.detach(), mean_s.detach(), gx_s, gg_s, gb_s)
    # the kernels
    rm_g, rv_g = torch.zeros(C).cuda(), torch.ones(C).cuda()
    xc = _cl(x)
    y, _, _, ss, mean = ops.bn_forward(xc, gamma.cuda(), beta.cuda(), rm_g, rv_g, True, eps=EPS, momentum=1.0, want_pool=False)
    dx, dgamma, dbeta = ops.bn_backward(xc, _cl(dy), None, None, mean, ss, relu_mask=False)
    mean_bwd = mean.cpu().double().view(-1, C).sum(0)          # what the backward centres x with: f32 mean (+ its remainder)
    kern = errors(_ncdhw(y), rm_g.cpu(), rv_g.cpu(), ss[2 * C:].cpu(), mean_bwd, _ncdhw(dx), dgamma.cpu(), dbeta.cpu())

    for name, chans in groups.items():
        print(f"rows={rows} {name:>9}: " + "  ".join(
            f"{q} {float(kern[q][chans].max()):.1e}/{float(stock[q][chans].max()):.1e}" for q in kern))
    # the constant channel (its float64 variance is 0: no relative variance error)
    c = CONST_CH
    assert abs(float(ss[2 * C + c]) * EPS ** 0.5 - 1.0) < 1e-6, float(ss[2 * C + c])
    assert float(rv_g[c]) == 0.0
    yc = _ncdhw(y)[:, c]
    assert torch.equal(yc, beta[c].expand_as(yc)), float((yc - beta[c]).abs().max())
    bad = []
    for q in kern:
        for ch in range(C):
            if ch == c and q in ("var", "y"):
                continue
            k, s = float(kern[q][ch]), float(stock[q][ch])
            if not k <= gate(s):
                bad.append((q, ch, f"kernel {k:.2e}", f"stock {s:.2e}"))
    assert not bad, bad
