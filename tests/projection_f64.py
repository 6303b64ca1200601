"""numpy float64 references of the projection kernels (csrc/projection.hip), one function per kernel operation.

Nothing here comes from the package.  Every function takes the float32 arrays the kernel receives, widens them and
evaluates the kernel's formula in float64.  The ``*_wrong_*`` functions at the end are mistakes a kernel could make;
tests/test_projection_f64_cpu.py uses them to show that the test inputs tell right from wrong, nothing else calls them."""
import numpy as np

F32, F64 = np.float32, np.float64


# ---- unproject (csrc/unproject.h) ---------------------------------------------------------------------------------------
def _consts64(consts):
    """The 12 kernel constants (f, cx, cy, s00, t0, s11, t1, s22, t2, d0, d1, d2): rounded to float32, as the kernel
    receives them, then widened."""
    c = [float(F32(v)) for v in consts]
    assert len(c) == 12
    return c


def _pixels(Hi, Wi):
    return np.arange(Wi, dtype=F64)[None, None, :], np.arange(Hi, dtype=F64)[None, :, None]


def unproject(depth, consts, normalize):
    """depth (B, Hi, Wi) -> (B, Hi * Wi, 3) grid-space points, normalised to (p - d / 2) / d on request."""
    f, cx, cy, s00, t0, s11, t1, s22, t2, d0, d1, d2 = _consts64(consts)
    z = np.asarray(depth, dtype=F64)
    B, Hi, Wi = z.shape
    u, v = _pixels(Hi, Wi)
    with np.errstate(invalid="ignore"):
        X = (u * z - cx * z) / f
        Y = -((v * z - cy * z) / f)
        g = np.stack([s00 * X + t0, s11 * Y + t1, s22 * z + t2], axis=-1)
        if normalize:
            d = np.array([d0, d1, d2], dtype=F64)
            g = (g - d / 2.0) / d
    return g.reshape(B, Hi * Wi, 3)


def _unproject_bwd(gpc, shape, consts, normalize, exchange_uv=False):
    f, cx, cy, s00, _, s11, _, s22, _, d0, d1, d2 = _consts64(consts)
    B, Hi, Wi = shape
    g = np.asarray(gpc, dtype=F64).reshape(B, Hi, Wi, 3)
    u, v = _pixels(Hi, Wi)
    if exchange_uv:
        u, v = np.broadcast_to(v, (1, Hi, Wi)), np.broadcast_to(u, (1, Hi, Wi))
    a0 = s00 * ((u - cx) / f)
    a1 = -s11 * ((v - cy) / f)
    a2 = s22
    if normalize:
        a0, a1, a2 = a0 / d0, a1 / d1, a2 / d2
    return g[..., 0] * a0 + g[..., 1] * a1 + g[..., 2] * a2


def unproject_bwd(gpc, shape, consts, normalize):
    """Cotangent gpc (B, Hi * Wi, 3) -> gradient of the depth (B, Hi, Wi).  The map is linear in the depth, so the depth
    itself does not enter."""
    return _unproject_bwd(gpc, shape, consts, normalize)


# ---- splat backward ------------------------------------------------------------------------------------------------------
def splat_decisions(pts, dims):
    """The integer decisions, taken in float32 as oracle/projection_oracle.py::splat_indices takes them: valid (B, N),
    base voxel (B, N, 3) int64 (zeros where a coordinate is NaN) and g = (p + 0.5) * (D - 1) (B, N, 3) float32."""
    p = np.asarray(pts, dtype=F32)
    hi, lo = F32(0.5 - 1e-6), F32(-0.5 + 1e-6)
    with np.errstate(invalid="ignore"):
        valid = ((p < hi) & (p > lo)).all(-1)
        g = ((p + F32(0.5)) * (np.asarray(dims, dtype=F32) - F32(1.0))).astype(F32)
        base = np.clip(np.nan_to_num(np.floor(g), nan=0.0), -2.0e9, 2.0e9).astype(np.int64)
    base[np.isnan(p).any(-1)] = 0
    return valid, base, g


def _splat_bwd(pts, gacc, dims, factors):
    dims = tuple(int(d) for d in dims)
    valid, base, g = splat_decisions(pts, dims)
    B, N = valid.shape
    ga = np.asarray(gacc, dtype=F64)
    with np.errstate(invalid="ignore"):
        r = g.astype(F64) - base.astype(F64)
    r[~valid] = 0.0
    w = np.stack([1.0 - r, r], axis=0)                      # w[corner][b, n, axis]
    b_idx = np.broadcast_to(np.arange(B)[:, None], (B, N))
    out = np.zeros((B, N, 3), dtype=F64)
    for k in range(2):
        for j in range(2):
            for l in range(2):
                z, y, x = base[..., 0] + k, base[..., 1] + j, base[..., 2] + l
                m = valid & (z >= 0) & (z < dims[0]) & (y >= 0) & (y < dims[1]) & (x >= 0) & (x < dims[2])
                gv = np.zeros((B, N), dtype=F64)
                gv[m] = ga[b_idx[m], z[m], y[m], x[m]]      # corners outside the grid are dropped
                out[..., 0] += (gv if k else -gv) * w[j][..., 1] * w[l][..., 2]
                out[..., 1] += (gv if j else -gv) * w[k][..., 0] * w[l][..., 2]
                out[..., 2] += (gv if l else -gv) * w[k][..., 0] * w[j][..., 1]
    out *= np.asarray(factors, dtype=F64)
    out[~valid] = 0.0
    return out


def splat_bwd(pts, gacc, dims):
    """Gradient of sum(acc * gacc) with respect to the points, acc being the UNCLAMPED trilinear splat (B, D0, D1, D2).
    Remainders, weights and the three sums in float64; invalid points give exactly 0."""
    return _splat_bwd(pts, gacc, dims, [int(d) - 1 for d in dims])


# ---- clamp(scale * x, 0, 1) backward, float32 like the kernel (it is compared bit for bit) --------------------------------
def _scale_clamp01_bwd(x, gout, scale, exclusive):
    x, gout, s = np.asarray(x, dtype=F32), np.asarray(gout, dtype=F32), F32(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * s
        inside = ((v > 0) & (v < 1)) if exclusive else ((v >= 0) & (v <= 1))
        return np.where(inside, gout * s, F32(0.0)).astype(F32)


def scale_clamp01_bwd(x, gout, scale):
    """gin = scale * gout where 0 <= scale * x <= 1 (bounds included, NaN excluded), else 0."""
    return _scale_clamp01_bwd(x, gout, scale, exclusive=False)


# ---- blur, one axis: correlation with zero padding K / 2, by slices ------------------------------------------------------
def _shifted(a, o, axis):
    """s[i] = a[i + o] along `axis` (1 + the spatial axis of a (B, D0, D1, D2) array), zero outside."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    if abs(o) >= n:
        return out
    src, dst = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    src[axis] = slice(max(o, 0), n + min(o, 0))
    dst[axis] = slice(max(-o, 0), n + min(-o, 0))
    out[tuple(dst)] = a[tuple(src)]
    return out


def _offsets(K, negate=False):
    return [(K // 2 - t) if negate else (t - K // 2) for t in range(K)]


def blur_axis(x, taps, axis):
    """out[i] = sum_t x[i + (t - K/2)] * taps[t] along spatial axis `axis` of x (B, D0, D1, D2)."""
    x, taps = np.asarray(x, dtype=F64), np.asarray(taps, dtype=F64)
    return sum(_shifted(x, o, axis + 1) * taps[t] for t, o in enumerate(_offsets(len(taps))))


def blur_axis_adjoint(gout, taps, axis):
    """gin[i] = sum_t gout[i - (t - K/2)] * taps[t]: the transpose of blur_axis."""
    g, taps = np.asarray(gout, dtype=F64), np.asarray(taps, dtype=F64)
    return sum(_shifted(g, o, axis + 1) * taps[t] for t, o in enumerate(_offsets(len(taps), negate=True)))


def blur_taps_grad(x, gout, K, axis):
    """gtaps[t] = sum_i gout[i] * x[i + (t - K/2)]."""
    x, g = np.asarray(x, dtype=F64), np.asarray(gout, dtype=F64)
    return np.array([np.sum(g * _shifted(x, o, axis + 1)) for o in _offsets(K)], dtype=F64)


# ---- named wrong variants: for tests/test_projection_f64_cpu.py only ------------------------------------------------------
def wrong_blur_axis_adjoint_no_flip(gout, taps, axis):
    """The adjoint that forgets to flip the taps (t - K/2 where K/2 - t belongs): the forward pass applied to gout."""
    return blur_axis(gout, taps, axis)


def wrong_blur_taps_grad_negated(x, gout, K, axis):
    """The tap gradient with the offset negated."""
    x, g = np.asarray(x, dtype=F64), np.asarray(gout, dtype=F64)
    return np.array([np.sum(g * _shifted(x, o, axis + 1)) for o in _offsets(K, negate=True)], dtype=F64)


def wrong_unproject_bwd_uv_exchanged(gpc, shape, consts, normalize):
    """The column index where the row index belongs and the other way round."""
    return _unproject_bwd(gpc, shape, consts, normalize, exchange_uv=True)


def wrong_splat_bwd_factors_exchanged(pts, gacc, dims):
    """The (D - 1) factors of two axes exchanged: the first two axes whose sizes differ (none: the true result)."""
    f = [int(d) - 1 for d in dims]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        if f[a] != f[b]:
            f[a], f[b] = f[b], f[a]
            break
    return _splat_bwd(pts, gacc, dims, f)


def wrong_splat_bwd_no_factor(pts, gacc, dims):
    """The (D - 1) factor left out."""
    return _splat_bwd(pts, gacc, dims, [1, 1, 1])


def wrong_scale_clamp01_bwd_exclusive(x, gout, scale):
    """The gradient cut at 0 < scale * x < 1: wrong exactly at the two bounds, which torch.clamp lets through."""
    return _scale_clamp01_bwd(x, gout, scale, exclusive=True)
