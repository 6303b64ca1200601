"""The 3x3x3 weight gradient's wave-specialised kernel (conv3d_bwdw_bf16.hip, conv3d_bwd_weight_ws_kernel): the encoder's real
layer shapes against an f64 reference and the exact-f32 kernel, run-to-run bit identity, and odd volumes with partial bricks
that still take the new kernel (>= 8 bricks per workgroup)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _golden as G


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


def _inputs(B, dims, Ci, Co, gscale, seed):
    """channels-last x (a ReLU output) and a gradient-like dout (magnitude gscale, per-voxel spread e^(+-2 sigma)), on the GPU"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = F.relu(torch.randn(B, *dims, Ci, generator=g, device="cuda"))
    dy = torch.randn(B, *dims, Co, generator=g, device="cuda") * gscale
    dy *= torch.exp(2 * torch.randn(B, *dims, 1, generator=g, device="cuda"))
    return x.contiguous(), dy.contiguous()


def _ref_f64(x, dy):
    """dW (Co, Ci, 3, 3, 3) and db in f64: dW[:, :, dz, dy, dx] = sum over voxels of dout[v] x[v + tap - 1]"""
    B, D, H, W, Ci = x.shape
    Co = dy.shape[-1]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))
    d = dy.double().reshape(-1, Co)
    dw = torch.empty(Co, Ci, 3, 3, 3, dtype=torch.float64, device=x.device)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                xs = xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Ci)
                dw[:, :, kz, ky, kx] = d.t() @ xs
    return dw.cpu().numpy(), d.sum(0).cpu().numpy()


# the encoder's weight-gradient layers at batch 8 (64^3: conv_0 16 -> 32 and 32 -> 32, then 32^3, 16^3, 8^3)
REAL = [(8, 64, 16, 32, 1e-6), (8, 64, 32, 32, 1e-5), (8, 32, 32, 64, 1e-4), (8, 32, 64, 64, 1e-3), (8, 16, 64, 128, 1e-2),
        (8, 16, 128, 128, 1.0), (8, 8, 128, 128, 30.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,Ci,Co,gscale", REAL)
def test_wgrad_real_layer_shapes(B, n, Ci, Co, gscale):
    ops = _ops()
    x, dy = _inputs(B, (n, n, n), Ci, Co, gscale, seed=Ci * 1000 + Co + n)
    gw, gb = _ref_f64(x, dy)
    err = {}
    for mode in ("f32", "f16x3s", "bf16x3"):
        dw, db = ops.conv3d_k3_bwd_weight(x, dy, mode=mode, param_layout=True)
        dwp, db2 = ops.conv3d_k3_bwd_weight(x, dy, mode=mode)
        assert torch.equal(ops.conv3d_unpack_wgrad(dwp, Ci, Co), dw) and torch.equal(db, db2), mode
        err[mode] = G.rel_err(dw.cpu().numpy(), gw)
        assert G.rel_err(db.cpu().numpy(), gb) < 3e-6, mode
    assert err["f32"] < 3e-6 and err["f16x3s"] < 3e-6, err
    assert err["f16x3s"] < 3 * err["f32"] + 1e-7, err
    assert err["bf16x3"] < 3e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("B,dims,Ci,Co", [(8, (64, 64, 64), 16, 32), (8, (64, 64, 64), 32, 32), (8, (32, 32, 32), 64, 64),
                                          (4, (37, 30, 61), 16, 32)])
def test_wgrad_bit_identical_runs(B, dims, Ci, Co):
    ops = _ops()
    x, dy = _inputs(B, dims, Ci, Co, 1e-4, seed=Ci + Co + B)
    for mode in ("f16x3s", "bf16x3"):
        for param_layout in (True, False):
            w1, b1 = ops.conv3d_k3_bwd_weight(x, dy, mode=mode, param_layout=param_layout)
            w2, b2 = ops.conv3d_k3_bwd_weight(x, dy, mode=mode, param_layout=param_layout)
            assert torch.equal(w1, w2) and torch.equal(b1, b2), (mode, param_layout)


# volumes that leave partial bricks (4 x 4 x 8 voxels) on every face, with enough bricks per workgroup for the new kernel;
# Ci = 8 and 16 take the paired-row tiles, Ci = 48 / Co = 40 padded channel tiles
@pytest.mark.gpu
@pytest.mark.parametrize("B,dims,Ci,Co", [(4, (37, 30, 61), 16, 32), (4, (37, 30, 61), 8, 16), (4, (29, 19, 27), 64, 64),
                                          (4, (29, 19, 27), 48, 40), (4, (37, 30, 61), 32, 32)])
def test_wgrad_partial_bricks(B, dims, Ci, Co):
    ops = _ops()
    x, dy = _inputs(B, dims, Ci, Co, 1e-3, seed=Ci * 7 + Co)
    gw, gb = _ref_f64(x, dy)
    err = {}
    for mode in ("f32", "f16x3s", "bf16x3"):
        dw, db = ops.conv3d_k3_bwd_weight(x, dy, mode=mode, param_layout=True)
        err[mode] = G.rel_err(dw.cpu().numpy(), gw)
        assert G.rel_err(db.cpu().numpy(), gb) < 3e-6, mode
        assert np.isfinite(dw.cpu().numpy()).all(), mode
    assert err["f32"] < 3e-6 and err["f16x3s"] < 3e-6, err
    assert err["f16x3s"] < 3 * err["f32"] + 1e-7, err
    assert err["bf16x3"] < 3e-5, err
