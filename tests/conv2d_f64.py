"""float64 reference of a UNet convolution block on channels-last tensors, from stock torch ops that exist in float64 on every
device (pad, slices, index_select, addmm): no F.conv2d (MIOpen has no float64 convolution), no project kernel.  Differentiable,
so torch.autograd.grad gives the gradients of the input, the weight and the bias in float64.
tests/test_conv2d_f64_cpu.py pins it on the CPU against F.conv2d / F.interpolate in float64."""
import torch
import torch.nn.functional as F


def act_f64(x, act):
    """0 none, 1 LeakyReLU(0.2), 2 ReLU; NaN stays NaN, the derivative at +-0 is torch's (0.2 / 0)"""
    return F.leaky_relu(x, 0.2) if act == 1 else (torch.relu(x) if act == 2 else x)


def _up_axis(x, dim):
    n = x.shape[dim]
    dst = torch.arange(2 * n, device=x.device, dtype=torch.float64)
    src = (0.5 * (dst + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp_max(n - 1)
    l1 = (src - i0).view([-1 if d == dim else 1 for d in range(x.dim())])
    return x.index_select(dim, i0) * (1 - l1) + x.index_select(dim, i1) * l1


def virtual_f64(s0, s1, act, up):
    """[x2 bilinear upsample, align_corners False]( act( cat(s0, s1) ) ), (B,H,W,C) float64"""
    x = s0.double() if s1 is None else torch.cat((s0.double(), s1.double()), 3)
    x = act_f64(x, act)
    return _up_axis(_up_axis(x, 1), 2) if up else x


def conv_f64(x, w, b, k, stride):
    """x (B,H,W,C), w (Cout,C,k,k), b (Cout) or None, all float64 -> (B,Ho,Wo,Cout): k*k shifted addmm, padding 1 (0 for k = 1)"""
    pad = 0 if k == 1 else 1
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    out = (b if b is not None else torch.zeros(w.shape[0], dtype=x.dtype, device=x.device)).repeat(B * Ho * Wo, 1)
    for ky in range(k):
        for kx in range(k):
            sl = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
            out = torch.addmm(out, sl.reshape(-1, C), w[:, :, ky, kx].t())
    return out.view(B, Ho, Wo, -1)


def patches(x, k, stride):
    """the patch matrix of conv_f64, (B*Ho*Wo, k*k*C) in tap-major order, and w's matching (Cout, k*k*C) view maker"""
    pad = 0 if k == 1 else 1
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    cols = [xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :].reshape(-1, C)
            for ky in range(k) for kx in range(k)]
    return torch.cat(cols, 1)


def weight_matrix(w):
    """(Cout, C, k, k) -> (Cout, k*k*C) in the order of patches()"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
