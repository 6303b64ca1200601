"""Float64 CPU restatement of the UNet regressor's head (the reference's trainer/trainer_unet.py:43-61): bilinear resize to
a square of side `size`, crop of rows r0:r1, sigmoid, renormalisation into [min_z, max_z], mean squared error -- stock torch
ops, autograd for the gradient.  `dtype` = torch.float32 gives torch's own single-precision arithmetic on the same inputs:
its distance from the float64 result is the yardstick the kernel tests measure against."""
import torch
import torch.nn.functional as F

MIN_Z, MAX_Z = 0.1953997164964676, 7.0


def head(raw, size, rows, min_z=MIN_Z, max_z=MAX_Z):
    """raw (B, 1, Hs, Ws) -> renormalised depth: (B, 1, r1 - r0, size), or raw's shape with size == 0 (no resize)."""
    y = F.interpolate(raw, size=size, mode="bilinear")[:, :, rows[0]:rows[1], :] if size else raw
    return torch.sigmoid(y) * (max_z - min_z) + min_z


def head_loss_grad(raw, target, size, rows, min_z=MIN_Z, max_z=MAX_Z, dtype=torch.float64):
    """-> depth, loss, d loss / d raw, all of `dtype`, on the CPU."""
    r = raw.detach().cpu().to(dtype).requires_grad_(True)
    depth = head(r, size, rows, min_z, max_z)
    loss = F.mse_loss(depth, target.detach().cpu().to(dtype), reduction="mean")
    (g,) = torch.autograd.grad(loss, r)
    return depth.detach(), loss.detach(), g
