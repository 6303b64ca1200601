"""CPU: the float64 reference of tests/test_gpu_conv2d_paths.py (tests/conv2d_f64.py: shifted addmm, index_select lerp) against
F.conv2d / F.interpolate / F.leaky_relu in float64 -- output and all gradients, both kernel sizes, odd sides, two sources, the
activations' derivative at +-0 and NaN passing through ReLU -- so the reference needs no GPU to be trusted."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv2d_f64 as R


@pytest.mark.parametrize("B,H,W,C0,C1,Cout,k,stride,act,up", [
    (2, 5, 7, 3, 2, 4, 4, 2, 1, False), (1, 6, 5, 5, 0, 7, 3, 1, 2, True), (2, 3, 3, 4, 4, 2, 4, 2, 0, True), (1, 1, 1, 2, 0, 3, 3, 1, 2, True),
    (1, 4, 9, 6, 0, 5, 1, 1, 1, False), (1, 2, 2, 3, 1, 2, 4, 2, 2, False)])
def test_reference_matches_stock_float64(B, H, W, C0, C1, Cout, k, stride, act, up):
    g = torch.Generator().manual_seed(H * 10 + W)
    s0 = torch.randn(B, H, W, C0, generator=g, dtype=torch.float64)
    s0.view(-1)[::5] = 0.0
    s0.view(-1)[1::7] = -0.0
    s0.requires_grad_(True)
    s1 = torch.randn(B, H, W, C1, generator=g, dtype=torch.float64).requires_grad_(True) if C1 else None
    w = torch.randn(Cout, C0 + C1, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=g, dtype=torch.float64, requires_grad=True)
    y = R.conv_f64(R.virtual_f64(s0, s1, act, up), w, b, k, stride)
    x = torch.cat((s0, s1), 3) if C1 else s0
    x = R.act_f64(x, act).permute(0, 3, 1, 2)
    if up:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    ref = F.conv2d(x, w, b, stride=stride, padding=0 if k == 1 else 1).permute(0, 2, 3, 1)
    assert y.shape == ref.shape and float((y - ref).detach().abs().max()) < 1e-12
    dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    leaves = [t for t in (s0, s1, w, b) if t is not None]
    for a, r in zip(torch.autograd.grad(y, leaves, dy), torch.autograd.grad(ref, leaves, dy)):
        assert float((a - r).abs().max()) < 1e-11 * max(1.0, float(r.abs().max()))
    # the patch matrix the exact-f32 yardstick multiplies
    pm = R.patches(R.virtual_f64(s0, s1, act, up).detach(), k, stride)
    assert float((pm @ R.weight_matrix(w.detach()).t() + b.detach() - ref.detach().reshape(-1, Cout)).abs().max()) < 1e-12


def test_reference_conventions_at_zero_and_nan():
    x = torch.tensor([0.0, -0.0, 2.0, -2.0], dtype=torch.float64).view(1, 1, 4, 1).requires_grad_(True)
    nan = torch.full((1, 1, 1, 1), float("nan"), dtype=torch.float64)
    for act, want, dwant in ((1, [0, 0, 2, -0.4], [0.2, 0.2, 1, 0.2]), (2, [0, 0, 2, 0], [0, 0, 1, 0])):
        y = R.virtual_f64(x, None, act, False)
        (gx,) = torch.autograd.grad(y.sum(), x)
        assert y.view(-1).tolist() == want and gx.view(-1).tolist() == dwant, act
        assert bool(torch.isnan(R.virtual_f64(nan, None, act, False)).all())      # ReLU and LeakyReLU keep a NaN (torch.relu does)
