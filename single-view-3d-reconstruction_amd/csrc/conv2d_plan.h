// Launch plans of the UNet's 2-D convolutions (host side).  Which kernel family, loader form, tile / split counts, epilogue
// form and grid a conv2d entry point of conv2d_igemm.hip (forward, backward-data), gemm_bf16x3.hip (weight gradient) and
// conv2d.hip (1..4 output channels) takes for a shape and the low address bits of its operands, and the refusal it answers with
// otherwise.  The launchers and the workspace-size functions call the cv2_*_plan() function of their family and act on the
// result; svr_conv2d_variant (conv2d_igemm.hip) exports the same calls, so for everything the HOST decides -- family, loader
// template, classes, tiles, splits, grids, workspace sizes -- the answer cannot drift from what runs.  Three fields are decided
// by the KERNELS from their own arguments and only restated here: `epilogue` coal / lane (conv2d_igemm_kernel's `coal`
// predicate: TN, N % 4, the output's address), reduce_v4 / reduce_scalar (ig_reduce_kernel's `v4`: N % 4, split_stride % 4)
// and `dy_vec4` (the dY loader of linear_tn_x3_tr_kernel<.., CONV>: VEC4 && N % 4 == 0).  A change to one of those predicates
// must be made here too; tests/test_gpu_conv2d_paths.py runs every value of the three fields against float64, so a kernel
// that took another path than the plan says would still be checked, under the wrong name.  Nothing here touches the device or
// includes anything from ROCm.
#pragma once
#include <algorithm>
#include <stdint.h>
#include "error.h"  // SVR_CHECK, svr_hip.h (svr_conv2d_plan, SVR_CV2_*)

namespace svr {

struct Cv2Query {
  int op;                      // SVR_CV2_FWD / SVR_CV2_BWD_DATA / SVR_CV2_BWD_WEIGHT
  int B, H, W, C0, C1, Cout, k, stride, act, upsample;
  unsigned lo0, lo1, lody, loout;   // low four address bits of src0, src1, dY and the output (Y / dIn)
};

constexpr int CV2_SM_MAXW = 8192;     // floats of LDS the 1..4-channel kernels keep their weights in
constexpr int CV2_TM = 128;           // tile rows of conv2d_igemm_kernel
constexpr int CV2_GK = 16;            // reduction elements per k-step of conv2d_igemm_kernel
constexpr int CV2_WG_TILE = 128;      // linear_tn_x3_tr_kernel: 128 x 128 output tiles ...
constexpr int CV2_WG_XK = 32;         // ... and k-steps of 32 rows
constexpr int CV2_SM_FWD_GRID = 2048, CV2_SM_BWD_GRID = 4096;

inline unsigned cv2_lo4(const void *p) { return (unsigned)((uintptr_t)p & 15); }
inline int64_t cv2_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int cv2_pad16(int c) { return (c + 15) / 16 * 16; }
inline bool cv2_small_supported(int Cout, int C, int k) { return Cout >= 1 && Cout <= 4 && (int64_t)Cout * C * k * k <= CV2_SM_MAXW; }

// reduction splits of the implicit GEMM: enough workgroups to fill the chip (512 four-wave or 1 024 two-wave ones: two waves per
// SIMD -- a k-step is a dependent chain load -> split -> LDS -> MFMA, and with one wave per SIMD the 512-tile layers ran at
// 2.8 us per k-step; profiles/r04_unet_split_target.txt), at least 8 k-steps each
inline int cv2_ig_splits(int64_t tiles, int ksteps, int n_out, int *ksplit) {
  const int target = n_out <= 64 ? 1024 : 512;
  int splits = (int)std::min<int64_t>(std::max<int64_t>(1, target / std::max<int64_t>(tiles, 1)), std::max(1, ksteps / 8));
  splits = std::min(splits, 64);
  *ksplit = (int)cv2_cdiv(ksteps, splits);
  return (int)cv2_cdiv(ksteps, *ksplit);
}
// row slabs of the weight gradient: the slabs are written and read once each -- few, long splits
inline int cv2_wgrad_splits(int64_t M, int64_t N, int64_t K, int64_t *rows_per_split) {
  const int64_t tiles = cv2_cdiv(N, CV2_WG_TILE) * cv2_cdiv(K, CV2_WG_TILE);
  const int64_t want = std::max<int64_t>(1, 384 / tiles);
  int64_t rps = cv2_cdiv(cv2_cdiv(M, want), CV2_WG_XK) * CV2_WG_XK;
  rps = std::max<int64_t>(rps, 4 * CV2_WG_XK);
  *rows_per_split = rps;
  return (int)cv2_cdiv(M, rps);
}
inline int cv2_sm_rows_per_block(int64_t M) { return (int)std::max<int64_t>(64, cv2_cdiv(cv2_cdiv(M, 1024), 4) * 4); }

// output size of a padded convolution; refuses an input smaller than the window (C division truncates toward zero:
// (H + 2 pad - k) / stride + 1 would answer 1 row for H = 1 at k4 s2 where the true count is 0)
inline int cv2_out_dims(const Cv2Query &q, int pad, const char *what, int *Ho, int *Wo) {
  SVR_CHECK(q.H + 2 * pad >= q.k && q.W + 2 * pad >= q.k, SVR_E_BADSHAPE, "%s: input %d x %d (padding %d) is smaller than the %d x %d window: no output",
            what, q.H, q.W, pad, q.k, q.k);
  *Ho = (q.H + 2 * pad - q.k) / q.stride + 1;
  *Wo = (q.W + 2 * pad - q.k) / q.stride + 1;
  return SVR_OK;
}
inline int cv2_common_checks(const Cv2Query &q, const char *what) {
  SVR_CHECK(q.B > 0 && q.H > 0 && q.W > 0 && q.C0 > 0 && q.C1 >= 0 && q.Cout > 0, SVR_E_BADARG, "%s: bad descriptor", what);
  return SVR_OK;
}

// svr_conv2d_fwd / svr_conv2d_bwd_data (conv2d_igemm.hip)
inline int cv2_ig_plan(const Cv2Query &q, svr_conv2d_plan &p) {
  const bool fwd = q.op == SVR_CV2_FWD;
  const char *what = fwd ? "conv2d_fwd" : "conv2d_bwd_data";
  p = svr_conv2d_plan{};
  if (int rc = cv2_common_checks(q, what)) return rc;
  SVR_CHECK((q.k == 4 && q.stride == 2) || (q.k == 3 && q.stride == 1) || (q.k == 1 && q.stride == 1), SVR_E_UNSUPPORTED,
            "%s: k=%d stride=%d (k4 s2 p1 / k3 s1 p1 / k1 s1 p0)", what, q.k, q.stride);
  SVR_CHECK(fwd || q.k != 1, SVR_E_UNSUPPORTED, "%s: k = 1 has forward planes only", what);
  SVR_CHECK(q.act >= 0 && q.act <= 2, SVR_E_BADARG, "%s: act %d", what, q.act);
  SVR_CHECK(!q.upsample, SVR_E_UNSUPPORTED, "%s: the x2 upsample is materialised first (svr_conv2d_virtual)", what);
  SVR_CHECK((int64_t)q.B * q.H * q.W < (1 << 24), SVR_E_UNSUPPORTED, "%s: %ld pixels (row decode limit 2^24)", what,
            (long)q.B * q.H * q.W);
  const int pad = q.k == 1 ? 0 : 1, C = q.C0 + q.C1;
  int Ho, Wo;
  if (int rc = cv2_out_dims(q, pad, what, &Ho, &Wo)) return rc;
  p.Ho = Ho; p.Wo = Wo;
  const int N = fwd ? q.Cout : C;                      // output columns of the GEMM
  const int mode2 = !fwd && q.stride == 2;
  p.classes = mode2 ? 4 : 1;
  p.family = N <= 64 ? SVR_CV2_IGEMM64 : SVR_CV2_IGEMM128;
  const int tn = N <= 64 ? 64 : 128;
  int64_t rows, outs;
  if (fwd) {
    p.vec4 = q.C0 % 4 == 0 && q.C1 % 4 == 0 && ((q.lo0 | q.lo1) & 15) == 0;
    p.ksteps = q.k * q.k * cv2_pad16(C) / CV2_GK;
    rows = (int64_t)q.B * Ho * Wo;
    outs = rows * N;
  } else {
    p.vec4 = q.Cout % 4 == 0 && (q.lody & 15) == 0;   // the gathered operand is dY
    p.ksteps = (mode2 ? 4 : q.k * q.k) * cv2_pad16(q.Cout) / CV2_GK;
    rows = (int64_t)q.B * cv2_cdiv(q.H, mode2 ? 2 : 1) * cv2_cdiv(q.W, mode2 ? 2 : 1);   // the largest parity class
    outs = (int64_t)q.B * q.H * q.W * N;
  }
  p.mtiles = cv2_cdiv(rows, CV2_TM);
  p.tiles = p.mtiles * cv2_cdiv(N, tn) * p.classes;
  p.splits = cv2_ig_splits(p.tiles, p.ksteps, N, &p.ksplit);
  p.split_stride = outs;
  if (p.splits > 1) {
    p.epilogue = N % 4 == 0 ? SVR_CV2_EPI_REDUCE_V4 : SVR_CV2_EPI_REDUCE_SCALAR;
    p.reduce_grid = (int32_t)std::min<int64_t>(cv2_cdiv(outs, 1024), 1024);
    p.workspace_bytes = (int64_t)p.splits * outs * 4;
  } else {
    p.epilogue = tn == 128 && N % 4 == 0 && (q.loout & 15) == 0 ? SVR_CV2_EPI_COAL : SVR_CV2_EPI_LANE;
  }
  return SVR_OK;
}

// svr_conv2d_bwd_weight (gemm_bf16x3.hip)
inline int cv2_wgrad_plan(const Cv2Query &q, svr_conv2d_plan &p) {
  const char *what = "conv2d_bwd_weight";
  p = svr_conv2d_plan{};
  if (int rc = cv2_common_checks(q, what)) return rc;
  SVR_CHECK((q.k == 4 && q.stride == 2) || (q.k == 3 && q.stride == 1), SVR_E_UNSUPPORTED, "%s: k=%d stride=%d", what, q.k, q.stride);
  SVR_CHECK(q.act >= 0 && q.act <= 2, SVR_E_BADARG, "%s: act %d", what, q.act);
  SVR_CHECK(!q.upsample, SVR_E_UNSUPPORTED, "%s: the x2 upsample is materialised first (svr_conv2d_virtual)", what);
  int Ho, Wo;
  if (int rc = cv2_out_dims(q, 1, what, &Ho, &Wo)) return rc;
  p.Ho = Ho; p.Wo = Wo;
  const int C = q.C0 + q.C1;
  const int64_t M = (int64_t)q.B * Ho * Wo, K = (int64_t)q.k * q.k * cv2_pad16(C), N = q.Cout;
  SVR_CHECK(M > 0 && M < (1 << 24) && (int64_t)q.B * q.H * q.W < (1 << 24), SVR_E_UNSUPPORTED,
            "%s: %ld output pixels, %ld input pixels (row decode limit 2^24)", what, (long)M, (long)q.B * q.H * q.W);
  p.family = SVR_CV2_WGRAD_TR;
  p.classes = 1;
  p.vec4 = q.C0 % 4 == 0 && q.C1 % 4 == 0 && ((q.lo0 | q.lo1 | q.lody) & 15) == 0;
  p.dy_vec4 = p.vec4 && N % 4 == 0;
  p.tiles = cv2_cdiv(K, CV2_WG_TILE) * cv2_cdiv(N, CV2_WG_TILE);
  p.splits = cv2_wgrad_splits(M, N, K, &p.rows_per_split);
  p.last_rows = M - (int64_t)(p.splits - 1) * p.rows_per_split;
  return SVR_OK;
}

// svr_conv2d_small_fwd / _bwd_data / _bwd_weight (conv2d.hip)
inline int cv2_small_plan(const Cv2Query &q, svr_conv2d_plan &p) {
  const char *what = q.op == SVR_CV2_FWD ? "conv2d_small_fwd" : (q.op == SVR_CV2_BWD_DATA ? "conv2d_small_bwd_data" : "conv2d_small_bwd_weight");
  p = svr_conv2d_plan{};
  SVR_CHECK(q.B > 0 && q.H > 0 && q.W > 0 && q.C0 > 0 && q.C1 >= 0, SVR_E_BADARG, "%s: bad descriptor", what);
  SVR_CHECK((q.k == 4 && q.stride == 2) || (q.k == 3 && q.stride == 1), SVR_E_UNSUPPORTED, "%s: k=%d stride=%d", what, q.k, q.stride);
  SVR_CHECK(!q.upsample, SVR_E_UNSUPPORTED, "%s: the x2 upsample is materialised first (svr_conv2d_virtual)", what);
  SVR_CHECK((int64_t)q.B * q.H * q.W < (1 << 24), SVR_E_UNSUPPORTED, "%s: %ld pixels (row decode limit 2^24)", what, (long)q.B * q.H * q.W);
  const int C = q.C0 + q.C1;
  SVR_CHECK(cv2_small_supported(q.Cout, C, q.k), SVR_E_UNSUPPORTED, "%s: Cout=%d C=%d (1..4 output channels, Cout*C*k*k <= %d)", what,
            q.Cout, C, CV2_SM_MAXW);
  int Ho, Wo;
  if (int rc = cv2_out_dims(q, 1, what, &Ho, &Wo)) return rc;
  p.Ho = Ho; p.Wo = Wo;
  p.family = SVR_CV2_SMALL;
  p.classes = 1;
  p.co = q.Cout;
  p.kk = q.k;
  p.vec4 = q.op != SVR_CV2_BWD_DATA && q.C0 % 4 == 0 && q.C1 % 4 == 0 && ((q.lo0 | q.lo1) & 15) == 0;   // (backward-data gathers dY per channel)
  const int64_t M = (int64_t)q.B * Ho * Wo;
  if (q.op == SVR_CV2_FWD) {
    p.grid = (int32_t)std::min<int64_t>(cv2_cdiv(M, 16), CV2_SM_FWD_GRID);
    p.capped = cv2_cdiv(M, 16) > CV2_SM_FWD_GRID;
  } else if (q.op == SVR_CV2_BWD_DATA) {
    const int64_t total = (int64_t)q.B * q.H * q.W * ((C + 3) / 4);
    p.grid = (int32_t)std::min<int64_t>(cv2_cdiv(total, 256), CV2_SM_BWD_GRID);
    p.capped = cv2_cdiv(total, 256) > CV2_SM_BWD_GRID;
  } else {
    p.rows_per_block = cv2_sm_rows_per_block(M);
    p.parts = (int32_t)cv2_cdiv(M, p.rows_per_block);
    const int items = q.k * q.k * ((C + 3) / 4);
    p.ipg = std::min(1024, (items + 63) / 64 * 64);     // items per group, groups per workgroup
    p.groups = std::max(1, 1024 / p.ipg);
    p.grid = p.parts;
    p.grid_y = (int32_t)cv2_cdiv(items, p.ipg);
    p.workspace_bytes = (int64_t)p.parts * ((int64_t)q.k * q.k * C * q.Cout + q.Cout) * 4;
  }
  return SVR_OK;
}

// what svr_amd.ops runs for the layer: the plain-FMA kernels where the weight fits them, else the GEMMs
inline int cv2_plan(const Cv2Query &q, svr_conv2d_plan &p) {
  if (q.Cout >= 1 && q.C0 > 0 && q.C1 >= 0 && q.k > 0 && cv2_small_supported(q.Cout, q.C0 + q.C1, q.k)) return cv2_small_plan(q, p);
  return q.op == SVR_CV2_BWD_WEIGHT ? cv2_wgrad_plan(q, p) : cv2_ig_plan(q, p);
}

}  // namespace svr
