"""A numpy model of bn_stats_partial_kernel / bn_stats_final_kernel's summation (csrc/bn_pool.hip), no GPU needed.

The kernel sums x - p and (x - p)^2 per thread in float32 runs of 16 rows (the square-and-add is one fused multiply-add,
as the compiler emits it), carries the runs in float64, and finishes with mean = p + s/n, var = ss/n - (s/n)^2, where the
pivot p is the channel's value in row 0.  This file holds the ill-conditioned inputs and the gate of
tests/test_gpu_bn_paths.py::test_ill_conditioned_statistics, and shows on any machine that the pivoted scheme meets the
gate and that the un-pivoted one (p = 0: E[x^2] - mean^2) misses it on the same inputs, i.e. that the inputs discriminate.
"""
import numpy as np
import pytest
import torch

EPS = 1e-5
ILL_SHAPES = [(2, 1, 1, 1), (2, 1, 2, 2), (1, 1, 8, 8), (1, 1, 64, 64)]     # (B, D, H, W): 2, 8, 64, 4096 rows
ILL_C = 32
MEAN_OVER_STD = (0, 1, -10, 10, 100, -100, 1000)
CONST_CH, ALT_CH = 30, 31
CONST_VALUE, ALT_VALUES = 1000.1, (3.0, 3.01)


def gate(stock_err):
    """what the kernel may err where stock float32 batch norm errs `stock_err`: 4x (another, equally sound summation
    order), or the 1e-6 the suite asks of the running statistics, whichever is larger"""
    return max(4.0 * stock_err, 1e-6)


def ill_conditioned_input(shape):
    """-> x (B, 32, D, H, W), gamma, beta (float32 tensors, drawn in float64), {group name: channel indices}.
    Channel c < 30 is randn * s_c + s_c * r_c, r_c cycling through MEAN_OVER_STD; channel 30 is constant at 1000.1;
    channel 31 alternates between 3.0 and 3.01 from row to row."""
    B, D, H, W = shape
    rows = B * D * H * W
    g = torch.Generator().manual_seed(4000 + rows)
    C = ILL_C
    s = 0.5 * 4.0 ** torch.rand(C, generator=g, dtype=torch.float64)
    r = torch.tensor([MEAN_OVER_STD[c % len(MEAN_OVER_STD)] for c in range(C)], dtype=torch.float64)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * s + s * r
    x[:, CONST_CH] = CONST_VALUE
    x[:, ALT_CH] = torch.tensor(ALT_VALUES, dtype=torch.float64)[torch.arange(rows) % 2]
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    groups = {f"r={m}": [c for c in range(C - 2) if MEAN_OVER_STD[c % len(MEAN_OVER_STD)] == m] for m in MEAN_OVER_STD}
    groups["const"] = [CONST_CH]
    groups["alt"] = [ALT_CH]
    x = x.view(B, D, H, W, C).permute(0, 4, 1, 2, 3).contiguous()
    return x.float(), gamma.float(), beta.float(), groups


def _stats_blocks(rows):
    b = min(max(-(-rows // 256), 1), 2048)
    rpb = -(-rows // b)
    return -(-rows // rpb), rpb


def model_statistics(x2d, pivoted):
    """x2d (rows, C) float32 -> mean (float64), unbiased variance and invstd (rounded to float32 as the kernel stores them)"""
    rows, C = x2d.shape
    RL = 256 // (C // 4)
    p = x2d[0].copy() if pivoted else np.zeros(C, np.float32)
    blocks, rpb = _stats_blocks(rows)
    s, ss = np.zeros(C, np.float64), np.zeros(C, np.float64)
    for b in range(blocks):
        xb = x2d[b * rpb:min(rows, (b + 1) * rpb)]
        for rl in range(min(RL, len(xb))):
            mine = xb[rl::RL]
            for r0 in range(0, len(mine), 16):
                fs, fss = np.zeros(C, np.float32), np.zeros(C, np.float32)
                for v in mine[r0:r0 + 16]:
                    d = (v - p).astype(np.float32)
                    fs = (fs + d).astype(np.float32)
                    fss = (fss.astype(np.float64) + d.astype(np.float64) * d.astype(np.float64)).astype(np.float32)   # fma
                s += fs
                ss += fss
    m = s / rows
    mean = p.astype(np.float64) + m
    var = np.maximum(ss / rows - m * m, 0.0)
    unb = var * rows / (rows - 1)
    return mean, unb.astype(np.float32), (1.0 / np.sqrt(var + EPS)).astype(np.float32)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


@pytest.mark.parametrize("shape", ILL_SHAPES, ids=[f"rows{np.prod(s)}" for s in ILL_SHAPES])
def test_pivoted_sums_meet_the_gate_and_plain_sums_do_not(shape):
    x, gamma, beta, groups = ill_conditioned_input(shape)
    C = x.shape[1]
    rows = x.numel() // C
    x2d = x.permute(0, 2, 3, 4, 1).reshape(rows, C)
    var64 = x2d.double().var(0, unbiased=False).numpy()
    unb64 = var64 * rows / (rows - 1)
    inv64 = 1.0 / np.sqrt(var64 + EPS)
    mean64 = x2d.double().mean(0).numpy()
    rm, rv = torch.zeros(C), torch.ones(C)
    _, _, inv_s = torch.native_batch_norm(x, gamma, beta, rm, rv, True, 1.0, EPS)
    rated = [c for c in range(C) if c != CONST_CH]                 # the constant channel has var64 = 0
    stock = {"var": _rel(rv.numpy(), unb64), "inv": _rel(inv_s.numpy(), inv64)}
    err = {}
    for pivoted in (True, False):
        mean, unb, inv = model_statistics(x2d.numpy(), pivoted)
        err[pivoted] = {"var": _rel(unb, unb64), "inv": _rel(inv, inv64)}
        if pivoted:
            assert np.all(np.abs(mean - mean64) <= 1e-7 * np.sqrt(var64 + EPS) + 1e-12 * np.abs(mean64))
            assert unb[CONST_CH] == 0.0 and abs(float(inv[CONST_CH]) * EPS ** 0.5 - 1.0) < 1e-6
    for name, chans in groups.items():
        print(f"rows={rows} {name:>7}: " + "  ".join(
            f"{q} pivot {err[True][q][chans].max():.1e} plain {err[False][q][chans].max():.1e} stock {stock[q][chans].max():.1e}"
            for q in ("var", "inv")))
    miss = {p: [(q, c) for q in ("var", "inv") for c in rated if not err[p][q][c] <= gate(stock[q][c])] for p in (True, False)}
    assert not miss[True], miss[True]
    # E[x^2] - mean^2 of float32 squares loses (mean/std)^2 * 2^-24 of the variance: every |mean/std| >= 100 group misses
    for m in (100, -100, 1000):
        assert any(c in groups[f"r={m}"] for q, c in miss[False] if q == "var"), (m, miss[False])
