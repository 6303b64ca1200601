"""The x-block item order (svr_gather_item_order_xblock) and the face hand-over of the atomic projected scatter
(gather.hip, gather_bwd_proj_kernel): values against CPU autograd of grid_sample at the project's own gate for this
quantity (1e-5, as tests/test_gpu_kernels.py::test_projected_scatter_of_dh_rows), the order itself, and the property the
design rests on: ANY item order gives the same dP, because the kernel finds its runs from the points.

Points are (rand - 0.5) * 1.2: some items fall outside the volume and some land in the half-empty edge cells x0 = -1 and
x0 = W - 1, where a handed face lies partly outside the volume."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ifnet_oracle as O
from tests import _golden as G

pytestmark = pytest.mark.gpu

# (dims, align_corners, N, B, block lengths)
CASES = [
    ((4, 4, 4), False, 2000, 2, (2, 5)),      # runs of ~16 items: 256-item chunks cut through runs and blocks; K = 5: whole row
    ((5, 6, 4), True, 500, 3, (2, 3)),        # W + 1 = 5 is no multiple of K; 3 samples: the adjacent key of ANOTHER sample
    ((16, 16, 16), False, 700, 1, (4,)),      # sparse: consecutive runs are usually not adjacent
    ((8, 8, 8), False, 3000, 2, (3,)),
]
CASE_K = [(c, K) for c in range(len(CASES)) for K in CASES[c][4]]


def _ops():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _case(c):
    """Inputs and the CPU reference of one case, computed once and shared (read-only) by all tests."""
    dims, align, N, B, _ = CASES[c]
    net_res = 32 if align else 128
    disp = float(np.float32(O.ARCH[net_res]["disp"]))
    g = torch.Generator().manual_seed(71 + N)
    pts = (torch.rand(B, N, 3, generator=g) - 0.5) * 1.2
    dh = torch.randn(B * N, 256, generator=g)
    grid = O.sample_grid(pts, net_res)                                                          # (B,1,7,N,3)
    ref = []
    for j in range(7):
        vol = torch.zeros(B, 256, *dims, requires_grad=True)
        out = F.grid_sample(vol, grid[:, :, j:j + 1], mode="bilinear", padding_mode="zeros", align_corners=align)
        (out[:, :, 0, 0].permute(0, 2, 1) * dh.view(B, N, 256)).sum().backward()
        ref.append(vol.grad.permute(0, 2, 3, 4, 1).reshape(B, -1, 256).numpy())
    ref = np.stack(ref, 2)                                                                      # (B, V, 7, 256)
    ref.setflags(write=False)
    idx, _ = O.corner_indices(pts, dims, net_res)                                               # (B, 7, N, 3) base voxels (z, y, x)
    return {"dims": dims, "align": align, "N": N, "B": B, "disp": disp, "net_res": net_res, "pts": pts, "dh": dh, "ref": ref,
            "base": idx, "pts_g": pts.cuda(), "dh_g": dh.cuda()}


def _decode(cs, ic):
    """b, j, lattice coordinates (base + 1) and the in-volume mask of the items `ic` (long, CPU)."""
    B, N, (D, H, W) = cs["B"], cs["N"], cs["dims"]
    pn, j = ic // 7, ic % 7
    base = cs["base"][pn // N, j, pn % N].long()
    inside = ((base >= -1).all(1)) & (base[:, 0] < D) & (base[:, 1] < H) & (base[:, 2] < W)
    return pn // N, j, base[:, 0] + 1, base[:, 1] + 1, base[:, 2] + 1, inside


def _scatter(cs, items):
    ops = _ops()
    return ops.gather_project_bwd(cs["pts_g"], cs["dh_g"], cs["dims"], items, cs["disp"], cs["align"]).cpu().numpy()


def _check(cs, dP, what):
    for j in range(7):
        e = G.rel_err(dP[:, :, j], cs["ref"][:, :, j])
        assert e < 1e-5, f"{what}: displacement {j}: rel err {e:.2e}"


@pytest.mark.parametrize("c,K", CASE_K)
def test_block_order_with_hand_over_matches_autograd_and_two_pass(c, K):
    ops = _ops()
    cs = _case(c)
    items = ops.item_order(cs["pts_g"], cs["dims"], cs["disp"], cs["align"], x_block=K)
    dP = _scatter(cs, items)
    _check(cs, dP, f"x-block order K={K}")
    plan = ops.project_plan(cs["pts_g"], cs["dims"], cs["disp"], cs["align"])
    runs = [ops.gather_project_bwd(cs["pts_g"], cs["dh_g"], cs["dims"], plan, cs["disp"], cs["align"]) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])                      # the two-pass form never hands over: still bit-reproducible
    e = G.rel_err(runs[0].cpu().numpy(), dP)
    assert e < 1e-5, f"two-pass form vs x-block order K={K}: {e:.2e}"


@pytest.mark.parametrize("c,K", CASE_K + [(c, 1) for c in range(len(CASES))])
def test_block_order_is_sorted_permutation(c, K):
    ops = _ops()
    cs = _case(c)
    B, N, (D, H, W) = cs["B"], cs["N"], cs["dims"]
    items = ops.item_order(cs["pts_g"], cs["dims"], cs["disp"], cs["align"], x_block=K)
    ic = items.cpu().long()
    assert sorted(ic.tolist()) == list(range(7 * B * N)), "not a permutation"
    b, j, z, y, x, inside = _decode(cs, ic)
    nb = (W + 1 + K - 1) // K
    key = ((((b * (D + 1) + z) * (H + 1) + y) * nb + x // K) * 8 + j) * K + x % K
    n_in = int(inside.sum())
    assert bool(inside[:n_in].all()), "items that touch no voxel must come last"
    assert bool((key[1:n_in] >= key[:n_in - 1]).all()), "block key not non-decreasing"
    if K == 1:
        assert torch.equal(items, ops.item_order(cs["pts_g"], cs["dims"], cs["disp"], cs["align"], with_j=True))


@pytest.mark.parametrize("c", range(len(CASES)))
def test_any_item_order_gives_the_same_sums(c):
    cs = _case(c)
    B, N, (D, H, W) = cs["B"], cs["N"], cs["dims"]
    T = 7 * B * N
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(5 + c)).int()
    _check(cs, _scatter(cs, perm.cuda()), "random permutation")
    # whole rows, displacement-major, x DESCENDING inside the row: the successor's key is cur - 1, which must not hand over
    ic = torch.arange(T)
    b, j, z, y, x, inside = _decode(cs, ic)
    key = ((((b * (D + 1) + z) * (H + 1) + y) * 8 + j) * (W + 1) + (W - x))
    key = torch.where(inside, key, torch.full_like(key, int(key.max()) + 1))
    desc = torch.sort(key, stable=True)[1].int()
    _check(cs, _scatter(cs, desc.cuda()), "x-descending rows")
