/*
 * svr_hip.h -- C ABI of libsvr_hip.so: the MI355X (gfx950) kernels behind the IF-Net
 * occupancy-query hot path of nihalsid/single-view-3d-reconstruction.
 *
 * The reference has no FFI layer of its own: the path sits behind torch nn.Modules
 * (model/ifnet.py:10-199, model/projection.py:21-218) and every arithmetic step is a stock
 * torch op.  Each entry point below therefore names the torch call site(s) it replaces.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes, no torch types; the CALLER owns every buffer
 *     (inputs, outputs, workspaces) and keeps it alive until the stream work completes;
 *   - asynchronous: work is only enqueued on `stream` (a hipStream_t passed as void*),
 *     no device synchronisation, no allocation, no default-stream work;
 *   - return 0 on success, a negative SVR_E_* code for a bad argument, or a positive
 *     hipError_t for a launch failure; svr_last_error() gives the text (thread local);
 *   - volumes are channels-last: (B, D, H, W, C) float32, C contiguous;
 *   - "feature rows": (B*N, FS) float32, FS = row stride >= svr_feature_width(); column
 *     layout is level-major, see svr_feature_layout().
 */
#ifndef SVR_HIP_H
#define SVR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_OK 0
#define SVR_E_BADARG (-1)
#define SVR_E_BADSHAPE (-2)
#define SVR_E_ALIGN (-3)
#define SVR_E_UNSUPPORTED (-4)
#define SVR_E_IO (-5)
#define SVR_E_NOTFOUND (-6)
#define SVR_E_INTERNAL (-7) /* a bound that the design rules out was reached; nothing was written out of bounds */

#define SVR_MAX_LEVELS 6

int svr_version(void); /* 100 = round 1, 200 = this header (svr_level / svr_gather_desc grew: check svr_sizeof_*) */
const char *svr_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Trilinear multi-level feature gather  (replaces: coordinate prep model/ifnet.py:156-161,
 * the six F.grid_sample calls :162,168,175,181,187,193, torch.cat :197 and the reshape
 * model/ifnet.py:43-45; 32-variant :93-118).
 * ------------------------------------------------------------------------------------- */
/* Backward plan of one level for the atomic-free "pull" scatter (svr_gather_pull_plan): the 7*B*N (point,
 * displacement) items sorted by the row-major key of their base cell, one 16-byte record per item and the first
 * item of every occupied cell.  All three arrays are device memory owned by the caller.                    */
typedef struct svr_pull_plan {
  const uint32_t *keys;  /* (7*B*N) sorted cell keys; items that touch no voxel carry the largest key      */
  const void *recs;      /* (7*B*N) x {float fx, fy, fz; int32 gfeat_offset} in sorted order               */
  const int32_t *heads;  /* (B*(D+1)*(H+1)*(W+1) + 1) CSR offsets: heads[c] = number of items with a key < c     */
  int64_t n_items;       /* 7*B*N                                                                          */
} svr_pull_plan;

typedef struct svr_level {
  const float *vol; /* (B, D, H, W, C) channels-last                                  */
  float *gvol;      /* backward only: gradient volume, same shape, accumulated into   */
  int32_t C, D, H, W;
  int32_t col;      /* first column of this level inside a feature row                */
  const int32_t *order; /* backward only, optional: (B*N) visiting order for THIS level from
                           svr_points_voxel_order (overrides svr_gather_desc.order)   */
  const int32_t *item_order; /* backward only, optional: (7*B*N) item ids from svr_gather_item_order -- the atomic
                           scatter then walks (point, displacement) items sorted jointly by base cell (7x longer
                           runs on the coarse levels); overrides `order`             */
  const svr_pull_plan *plan; /* backward only, optional (host pointer, read at call time): scatter this level
                           atomic-free in pull form.  gvol is then OVERWRITTEN (it need not be zeroed) and
                           `order` is ignored.  C in {1, 16, 32, 64} (C = 1: the raw grid of level 0,
                           one scalar per voxel).                                      */
} svr_level;

typedef struct svr_gather_desc {
  int32_t n_levels;
  int32_t B, N;           /* batch, query points per sample                          */
  int32_t row_stride;     /* FS: floats per feature row (>= used width, multiple of 4) */
  int32_t align_corners;  /* 0: 128-architecture, 1: 32-architecture                   */
  float displacement;     /* 0.0722 / 0.035 (model/ifnet.py:144,82)                    */
  const int32_t *order;   /* optional (B*N) processing order from svr_points_morton_order, or NULL */
  svr_level level[SVR_MAX_LEVELS];
  int32_t flags;          /* SVR_GATHER_* bits, 0 = production defaults                */
} svr_gather_desc;

/* flags: test / measurement switches; results are the same with or without them.
 *   WIDE_OFFSETS   forward: take the 64-bit-offset gather body that is otherwise only selected when a
 *                  volume or the feature matrix has >= 2^31 elements (so tests can reach it at small sizes);
 *   DETERMINISTIC  backward: scatter without float atomics in a fixed summation order (one wave per
 *                  (sample, level), serial over the points like ATen's CPU grid_sampler_3d_backward):
 *                  bit-reproducible run to run, orders of magnitude slower -- for tests only.          */
#define SVR_GATHER_WIDE_OFFSETS 1
#define SVR_GATHER_DETERMINISTIC 2

/* Layout pin for bindings in other languages: sizeof(svr_level) / sizeof(svr_gather_desc) as this library was
 * compiled; a binding asserts its own struct sizes against these before the first call.                   */
int64_t svr_sizeof_level(void);
int64_t svr_sizeof_gather_desc(void);

/* order[i] = index (b*N+n) of the i-th point in (sample, Morton code at 64^3) order.  Not a
 * reference op: it only changes the order in which the gather / scatter kernels visit points
 * (L2 locality, run-combining of atomics); outputs keep the caller's point order.
 * workspace: svr_points_morton_order_workspace() bytes.                                      */
/* order[i] = index of the i-th point in (sample, row-major index, x fastest, of the BASE VOXEL of its undisplaced
 * trilinear sample in a D x H x W volume) order: points that scatter into the same 8 corners of that
 * level become consecutive, which is what the backward run-combining needs (the base-voxel lattice is
 * shifted by half a voxel, differently at every level, so one global order cannot serve all levels).
 * Same workspace size as svr_points_morton_order.                                               */
int svr_points_voxel_order(const float *points, int32_t *order, int32_t B, int32_t N, int32_t D, int32_t H,
                           int32_t W, int32_t align_corners, void *workspace, void *stream);
int64_t svr_points_morton_order_workspace(int32_t B, int32_t N);
int svr_points_morton_order(const float *points, int32_t *order, float *sorted_points /* (B,N,3) or NULL */,
                            int32_t B, int32_t N, void *workspace, void *stream);

/* Plan for the pull-form backward scatter of ONE level (volume D x H x W, C channels at feature column `col`).
 * The scatter of a sparse level is bound by the float-atomic rate (~1.3 TB/s); in pull form every voxel sums the
 * items of its <= 8 neighbouring base cells in a fixed order and is written once with plain stores: no atomics, no
 * zero-initialised gradient volume, bit-reproducible.  Not a reference op (ATen's CPU backward scatters serially).
 * keys / recs / heads: see svr_pull_plan (heads needs B*(D+1)*(H+1)*(W+1)+1 int32).  B*N*row_stride and the cell
 * count must be below 2^31.  workspace: svr_gather_pull_plan_workspace(B, N) +
 * svr_gather_pull_plan_workspace_cells(B, D, H, W) bytes.                                                    */
int64_t svr_gather_pull_plan_workspace(int32_t B, int32_t N);
int64_t svr_gather_pull_plan_workspace_cells(int32_t B, int32_t D, int32_t H, int32_t W);
int svr_gather_pull_plan(const float *points, int32_t B, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C,
                         int32_t col, int32_t row_stride, int32_t align_corners, float displacement,
                         uint32_t *keys, void *recs, int32_t *heads, int32_t *items /* optional (7*B*N): the sorted item
                         ids = svr_level.item_order of the same level */, int32_t *stats /* optional, 2 device ints:
                         [0] = longest serial walk of the pull kernel (items in one (row, x strip) range) */,
                         void *workspace, void *stream);

/* items[i] = id (b*N+n)*7 + j of the i-th (point, displacement) item in (sample, row-major base cell of ITS displaced
 * sample in a D x H x W volume) order; items that touch no voxel come last.  For svr_level.item_order.
 * workspace: svr_gather_pull_plan_workspace(B, N) bytes.                                                     */
int svr_gather_item_order(const float *points, int32_t B, int32_t N, int32_t D, int32_t H, int32_t W,
                          int32_t align_corners, float displacement, int32_t with_j /* 1: order by (cell, j) */,
                          int32_t *items, void *workspace, void *stream);
/* The x-BLOCK order of the projected scatter's atomic form: items sorted by
 *   (sample, z, y, x / block, j, x % block)        (x, y, z = base cell + 1; block in [1, W + 1])
 * so that inside a block of `block` x-adjacent cells the runs of ONE displacement follow each other and
 * svr_gather_project_bwd hands the shared face of two neighbours over in registers instead of adding it to dP twice.
 * block = 1 is exactly svr_gather_item_order(with_j = 1).  The scatter's result does not depend on the order (it finds
 * its runs from the points), only its speed does.  Same workspace, same key width limits as svr_gather_item_order.   */
int svr_gather_item_order_xblock(const float *points, int32_t B, int32_t N, int32_t D, int32_t H, int32_t W,
                                 int32_t align_corners, float displacement, int32_t block, int32_t *items,
                                 void *workspace, void *stream);
/* Backward-only projection of a wide level (gather.hip, gather_bwd_proj_kernel): the scatter commutes with fc_0's
 * product, so the level's 7*C feature columns need neither dX nor dW of the point MLP over all points:
 *   dP[b][v][j][0:256] += w(item, v) * dh[(b*N+n)][0:256]   for every item (n, j) of svr_gather_item_order(with_j = 1)
 * or svr_gather_item_order_xblock (fewer float atomics; any permutation of the item ids gives the same sums)
 * (dP: (B, D*H*W, 7, 256) float32, zero-initialised by the caller; dh: the gradient wrt fc_0's pre-activation, row
 * stride lddh >= 256).  The caller finishes with two GEMMs over VOXELS: dvol = dP W0_l, dW0_l = dP^T vol.       */
int svr_gather_project_bwd(const float *points, const float *dh, int64_t lddh, int32_t B, int32_t N, int32_t D, int32_t H,
                           int32_t W, int32_t align_corners, float displacement, const int32_t *items, float *dP,
                           void *stream);

/* Two-pass form of svr_gather_project_bwd (no float atomics, no memset of dP, bit-reproducible): pass 1 stores the 8 corner
 * sums of every run -- a maximal stretch of equal (sample, cell, displacement) keys inside a 256-item chunk of the sorted
 * items -- to partials[slot][8][256]; pass 2 gives every (voxel, displacement) row of dP the sum of the <= 8 cells that touch
 * it, with plain stores (dP is OVERWRITTEN).  svr_gather_project_plan sorts the items (as svr_gather_item_order with_j = 1)
 * and builds keys (7*B*N sorted u32), sidx (7*B*N + 1: run starts in front of an item) and first_slot
 * (B*(D+1)*(H+1)*(W+1)*8 + 1); partials needs svr_gather_project_slots(...) * 8 * 256 floats (not initialised).
 * workspace: svr_gather_project_plan_workspace(B, N) bytes.                                                              */
int64_t svr_gather_project_plan_workspace(int32_t B, int32_t N);
int64_t svr_gather_project_slots(int32_t B, int32_t N, int32_t D, int32_t H, int32_t W);
int svr_gather_project_plan(const float *points, int32_t B, int32_t N, int32_t D, int32_t H, int32_t W, int32_t align_corners,
                            float displacement, int32_t *items, uint32_t *keys, int32_t *sidx, int32_t *first_slot,
                            void *workspace, void *stream);
int svr_gather_project_bwd2(const float *points, const float *dh, int64_t lddh, int32_t B, int32_t N, int32_t D, int32_t H,
                            int32_t W, int32_t align_corners, float displacement, const int32_t *items, const int32_t *sidx,
                            const int32_t *first_slot, float *partials, float *dP, void *stream);

/* features[b*N+n][level.col + j*C + c] = trilinear sample j of channel c (zeros padding);
 * columns past the last level (up to row_stride) are written as zeros.                      */
int svr_gather_trilinear_fwd(const svr_gather_desc *d, const float *points /*(B,N,3)*/,
                             float *features, void *stream);
/* Fused gather -> first point-MLP layer (gather_fc0.hip): the feature rows of svr_gather_trilinear_fwd are produced
 * 128 points x one K-slab at a time in LDS and multiplied straight into fc_0's 128 x 256 output tile (3-product f16
 * split, as svr_linear_fwd_f16x3), so the (B*N, row_stride) feature matrix is never written or read:
 *   Y[b*N+n][0:n_out] = epi( features[b*N+n][:] . W[0:n_out][:]^T )         (model/ifnet.py:156-197 + :43-45,55)
 * W (n_out, >= last used column), row stride ldw, in the feature row's column layout (svr_level.col); n_out = 256.
 * keep_levels: bit l set = the gathered values of level l are ALSO stored to `features` -- the rows a backward still
 * needs; 0 = inference, `features` may be NULL.  The kept matrix has row stride ldf floats (<= 0: d->row_stride) and
 * level l starts at column keep_cols[l] (host array of n_levels entries, read at call time; NULL: svr_level.col, i.e.
 * the layout of svr_gather_trilinear_fwd) -- a compact matrix of the kept levels only (800 columns instead of a
 * 2592-wide row for the 128-architecture's training step).  With any bit set the columns behind the last kept level
 * (keep_cols given) / the last level (NULL) up to ldf are zero-filled.  d->order must be NULL (sort the points instead);
 * channel counts 1 (at most one level), 16, 32 or multiples of 64; every volume < 2^30 elements;
 * svr_gather_fc0_supported(d) tells.  workspace: svr_gather_fc0_workspace(d, n_out) bytes.                       */
int32_t svr_gather_fc0_supported(const svr_gather_desc *d);
int64_t svr_gather_fc0_workspace(const svr_gather_desc *d, int32_t n_out);
int svr_gather_fc0_fwd(const svr_gather_desc *d, const float *points, const float *W, int64_t ldw, const float *bias, float *Y,
                       int64_t ldy, int32_t n_out, float *features, int64_t ldf, const int32_t *keep_cols, uint32_t keep_levels,
                       int32_t epilogue, void *workspace, void *stream);
/* The same in two calls, for callers that query ONE pyramid with ONE weight matrix many times (dense-grid inference,
 * model/ifnet.py:215-229: one chunk of the lattice per call): svr_gather_fc0_prepare splits W into the kernel's f16
 * planes and stores the slab table in `workspace` (three small launches), svr_gather_fc0_run is the gather -> fc_0
 * kernel alone and may be repeated with other points / B*N <= the prepared descriptor's, same volumes, same layout.
 * svr_gather_fc0_fwd = prepare + run.                                                                             */
int svr_gather_fc0_prepare(const svr_gather_desc *d, const float *W, int64_t ldw, int32_t n_out, float *features, int64_t ldf,
                           const int32_t *keep_cols, uint32_t keep_levels, void *workspace, void *stream);
int svr_gather_fc0_run(const svr_gather_desc *d, const float *points, const float *bias, float *Y, int64_t ldy, int32_t n_out,
                       float *features, int64_t ldf, const int32_t *keep_cols, uint32_t keep_levels, int32_t epilogue,
                       void *workspace, void *stream);
/* bf16-STORAGE variant of the fused kernel (the throughput mode of svr_gather_trilinear_fwd_bf16 + svr_linear_fwd_bf16 in
 * one launch; never the default): the levels' `vol` pointers are bf16 volumes (8-byte aligned), W (n_out, ldw) is given in
 * f32 and rounded to bf16 (round to nearest even), the feature values are rounded to bf16 once -- the bits
 * svr_gather_trilinear_fwd_bf16 writes -- and multiplied on the bf16 matrix cores with f32 accumulation; Y (B*N, ldy) bf16.
 * workspace: svr_gather_fc0_workspace(d, n_out) bytes; prepare once per pyramid and weight, run per point set.            */
int svr_gather_fc0_bf16_prepare(const svr_gather_desc *d, const float *W, int64_t ldw, int32_t n_out, void *workspace,
                                void *stream);
int svr_gather_fc0_bf16_run(const svr_gather_desc *d, const float *points, const float *bias, uint16_t *Y, int64_t ldy,
                            int32_t n_out, int32_t epilogue, void *workspace, void *stream);
/* gvol[level] += scatter of gfeatures (autograd of grid_sample wrt the volume);
 * levels with gvol == NULL are skipped.  gpoints (B,N,3) may be NULL; when given it is
 * OVERWRITTEN with the gradient wrt the query points.                                   */
int svr_gather_trilinear_bwd(const svr_gather_desc *d, const float *points, const float *gfeatures,
                             float *gpoints, void *stream);
/* Integer base corner (z0,y0,x0) of every sample: out (B,7,N,3) int32 -- the bit-exact gate. */
int svr_gather_corner_indices(const svr_gather_desc *d, int32_t level, const float *points,
                              int32_t *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * bf16-STORAGE throughput mode of the query path (north_star "bf16 occupancy logits", BASELINE configs[1];
 * reference hooks: the dtype-generic grid_sample / Conv1d calls model/ifnet.py:161-193,55-59 under
 * util/arguments.py:30 --precision 16).  Volumes, feature rows and MLP activations are bf16 in memory; corner
 * weights, sums, MFMA accumulators, bias and ReLU are f32; every stored value is rounded once (nearest even).
 * The sample geometry is the f32 code of the default path: corner indices stay bit-exact.  A separate mode --
 * never the default, never held to the fp32 1e-4 gate (bf16_path.hip).
 * ------------------------------------------------------------------------------------- */
int svr_cast_f32_to_bf16(const float *in, uint16_t *out, int64_t n, void *stream);
/* As svr_gather_trilinear_fwd, with svr_level.vol pointing to bf16 volumes (B,D,H,W,C) and bf16 feature rows
 * (row_stride in ELEMENTS, multiple of 8).  One of the levels must have C == 1 (its kernel writes the padding
 * columns) unless the levels fill the row.                                                               */
int svr_gather_trilinear_fwd_bf16(const svr_gather_desc *d, const float *points, uint16_t *features, void *stream);
/* Y[M,N] (bf16) = epi( X[M,K] (bf16, ldx) W[N,K]^T (bf16, ldw) ), f32 accumulation on v_mfma_f32_32x32x16_bf16;
 * epilogue NONE / BIAS / BIAS_RELU with an f32 bias; 32 | K, rows 16-byte aligned.                         */
int svr_linear_fwd_bf16(const uint16_t *X, int64_t ldx, const uint16_t *W, int64_t ldw, const float *bias, uint16_t *Y,
                        int64_t ldy, int64_t M, int64_t N, int64_t K, int epilogue, void *stream);
/* logits[r(m)] (f32) = H[m,:] (bf16) . w (f32) + b,  r(m) = row_map[m] or m (see svr_fc_out_fwd)           */
int svr_fc_out_fwd_bf16(const uint16_t *H, int64_t ldh, const float *w, const float *b, float *logits,
                        const int32_t *row_map, int64_t M, int64_t K, void *stream);

/* ---------------------------------------------------------------------------------------
 * Dense f32 GEMMs on MFMA (replaces nn.Conv1d(.,.,1) fc_0/fc_1/fc_2 model/ifnet.py:19-21,55-57
 * and their autograd).  Row-major everywhere.
 * ------------------------------------------------------------------------------------- */
#define SVR_EPI_NONE 0
#define SVR_EPI_BIAS 1       /* + bias[n]                       */
#define SVR_EPI_BIAS_RELU 2  /* relu(. + bias[n])               */
#define SVR_EPI_MASK 3       /* . * (mask[m][n] > 0)  (ReLU backward with the saved output) */

/* Y[M,N] = epi( X[M,K](ldx) * W[N,K](ldw)^T )                                           */
int svr_linear_fwd(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                   float *Y, int64_t ldy, int64_t M, int64_t N, int64_t K, int epilogue,
                   const float *mask, int64_t ldmask, void *stream);
/* dX[M,K] = epi( dY[M,N](lddy) * W[N,K](ldw) ), epilogue NONE or MASK (mask is [M,K])    */
int svr_linear_bwd_data(const float *dY, int64_t lddy, const float *W, int64_t ldw, float *dX,
                        int64_t lddx, int64_t M, int64_t N, int64_t K, int epilogue,
                        const float *mask, int64_t ldmask, void *stream);
/* dW[N,K](lddw) = dY[M,N]^T * X[M,K];  db[N] = column sums of dY (db may be NULL).
 * workspace: svr_linear_bwd_weight_workspace() bytes.  Deterministic (slab + ordered sum). */
int64_t svr_linear_bwd_weight_workspace(int64_t M, int64_t N, int64_t K);
int svr_linear_bwd_weight(const float *dY, int64_t lddy, const float *X, int64_t ldx, float *dW,
                          int64_t lddw, float *db, int64_t M, int64_t N, int64_t K,
                          void *workspace, void *stream);

/* Forward product at f32 accuracy on the bf16 matrix cores: x = hi + mid + lo (three bf16 terms = 24
 * mantissa bits), six MFMA products, f32 accumulation; agrees with svr_linear_fwd to ~2e-7 relative.
 * epilogue NONE / BIAS / BIAS_RELU.  workspace: svr_linear_fwd_bf16x6_workspace(N, K) bytes.          */
int64_t svr_linear_fwd_bf16x6_workspace(int64_t N, int64_t K);
int svr_linear_fwd_bf16x6(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                          float *Y, int64_t ldy, int64_t M, int64_t N, int64_t K, int epilogue,
                          void *workspace, void *stream);
/* Same result with the 3-product f16 split (x = hi + lo in f16: 22 mantissa bits; W normalised by a power of two,
 * lo terms kept normal by exact 2^11 scaling, see gemm_f16x3.hip): as accurate as an f32 GEMM (~3e-7 of f64) at
 * half the matrix-core work of bf16x6.  Domain: |X| < 65504 (f16 range).
 * workspace: svr_linear_fwd_f16x3_workspace(N, K) bytes.
 * PREPARE / RUN (the four split-precision entry points svr_linear_fwd_f16x3, svr_linear_bwd_data_bf16x3,
 * svr_conv3d_k3_fwd_f16x3, svr_conv3d_k3_bwd_data_bf16x3): with the data operand (X / dY / in / dout) NULL the call only
 * prepares the workspace from W (scale + split planes: the launches that depend on the parameters alone); with W NULL it
 * runs on a workspace an earlier call prepared.  A training step prepares every layer once, on a side stream, while the
 * first kernels of the step run (model/ifnet.py), instead of 2-4 launch-bound kernels in front of every layer.         */
int64_t svr_linear_fwd_f16x3_workspace(int64_t N, int64_t K);
int svr_linear_fwd_f16x3(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                          float *Y, int64_t ldy, int64_t M, int64_t N, int64_t K, int epilogue,
                          void *workspace, void *stream);

/* The same two backward products on the bf16 matrix cores with a 3-term split (x = hi + mid, products
 * hi*hi + hi*mid + mid*hi, f32 accumulation): ~1.5e-5 relative error per product, ~5x fewer matrix-core
 * cycles than the exact-f32 MFMA.  Backward only -- the forward pass (logits, ReLU masks) stays exact f32.
 * bwd_data workspace: svr_linear_bwd_data_bf16x3_workspace(N, K) bytes (split + transposed weight planes).
 * bwd_data needs N % 32 == 0, K % 4 == 0, and dX and the mask float4-able (16-byte aligned, leading dimensions multiples
 * of 4: SVR_E_ALIGN / SVR_E_BADSHAPE otherwise); bwd_weight takes any K and any X layout (a slower path where K % 4 != 0
 * or X is not float4-able).                                                                                              */
int64_t svr_linear_bwd_data_bf16x3_workspace(int64_t N, int64_t K);
int svr_linear_bwd_data_bf16x3(const float *dY, int64_t lddy, const float *W, int64_t ldw, float *dX,
                               int64_t lddx, int64_t M, int64_t N, int64_t K, int epilogue,
                               const float *mask, int64_t ldmask, void *workspace, void *stream);
int64_t svr_linear_bwd_weight_bf16x3_workspace(int64_t M, int64_t N, int64_t K);
int svr_linear_bwd_weight_bf16x3(const float *dY, int64_t lddy, const float *X, int64_t ldx, float *dW,
                                 int64_t lddw, float *db, int64_t M, int64_t N, int64_t K,
                                 void *workspace, void *stream);

/* The same two backward products at f32 LEVEL on the f16 matrix cores ("f16x3s": the scaled 3-product f16 split).  The
 * reference computes its backward in fp32 (util/arguments.py:30, precision 32); bf16x3 above carries 16 mantissa bits per
 * operand, this carries 22 -- at the same three matrix instructions per block.  f16 has 5 exponent bits, so a gradient
 * operand is first multiplied by an exact power of two that brings its |max| into [2^13, 2^14):
 *   svr_amax_f32: amax[0] = bit pattern of max |X[m][n]| (one pass; N, ld multiples of 4, rows 16-byte aligned), or the
 *   amax_dx output of svr_linear_bwd_data_f16x3 (|max| of the dX it stored: the next layer's dY needs no extra pass).
 * Every amax OUTPUT (svr_amax_f32's, amax_dx, amax_din, ...) is an atomic maximum: the word must hold 0 (or a lower
 * bound) on entry -- the library launches no memset for it.
 * amax_dy == NULL: no scaling (values must then lie in f16's range).  The weight operand is normalised the same way when
 * its planes are prepared (PREPARE / RUN as above: dY NULL = prepare from W, W NULL = run); the activation operand X of
 * the weight gradient is taken as it is (|x| < 65504; below |x| ~ 1e-4 its correction term has an absolute error floor of
 * 1.5e-11 |dY|).  Errors against f64: ~3e-7 (the exact-f32 kernels' own level), bf16x3: ~1e-5.                              */
int svr_amax_f32(const float *X, int64_t ld, int64_t M, int64_t N, uint32_t *amax, void *stream);
int64_t svr_linear_bwd_data_f16x3_workspace(int64_t N, int64_t K);
int svr_linear_bwd_data_f16x3(const float *dY, int64_t lddy, const float *W, int64_t ldw, float *dX,
                              int64_t lddx, int64_t M, int64_t N, int64_t K, int epilogue,
                              const float *mask, int64_t ldmask, const uint32_t *amax_dy, uint32_t *amax_dx,
                              void *workspace, void *stream);
int64_t svr_linear_bwd_weight_f16x3_workspace(int64_t M, int64_t N, int64_t K);
int svr_linear_bwd_weight_f16x3(const float *dY, int64_t lddy, const float *X, int64_t ldx, float *dW,
                                int64_t lddw, float *db, int64_t M, int64_t N, int64_t K,
                                const uint32_t *amax_dy, void *workspace, void *stream);

/* What a linear entry point above does with a call (the launchers ask the same function).  Host only: no device memory is
 * touched, callable without a GPU.  op = SVR_LIN_*; M, N, K as the entry point takes them (x (M,K), w (N,K), dy (M,N));
 * ld_a / ld_b / ld_out / ld_mask and lo_a / lo_b / lo_out / lo_mask are the leading dimensions and the low four address bits
 * of the first operand (X forward, dY backward), the second (W; X of backward-weight), the output (Y / dX / dW) and the
 * mask; epilogue = SVR_EPI_*; want_bias: backward-weight is asked for db.  Outputs (each may be NULL):
 *   kernel: SVR_LIN_K_*;  coalesced: 1 = the tile leaves through LDS as float4 rows, 0 = one dword per lane;
 *   splits / rows_per_split: reduction splits of backward-weight (1 / M elsewhere);
 *   bias_form: SVR_LIN_BIAS_* -- where db comes from;
 *   status: what the entry point would return for these operands, SVR_OK or its refusal (outputs past the refused check
 *   are not meaningful).  The return value is SVR_E_BADARG for an unknown op, else SVR_OK.                                   */
#define SVR_LIN_FWD_F32 0
#define SVR_LIN_FWD_F16X3 1
#define SVR_LIN_FWD_BF16X6 2
#define SVR_LIN_BWD_DATA_F32 3
#define SVR_LIN_BWD_DATA_F16X3S 4
#define SVR_LIN_BWD_DATA_BF16X3 5
#define SVR_LIN_BWD_WEIGHT_F32 6
#define SVR_LIN_BWD_WEIGHT_F16X3S 7
#define SVR_LIN_BWD_WEIGHT_BF16X3 8
#define SVR_LIN_K_NT 0          /* exact f32: linear_nt_kernel                                              */
#define SVR_LIN_K_NN 1          /*            linear_nn_kernel                                              */
#define SVR_LIN_K_TN 2          /*            linear_tn_kernel + slab_reduce_kernel                         */
#define SVR_LIN_K_NT128 3       /* linear_nt_h3_kernel<128>                                                 */
#define SVR_LIN_K_NT64 4        /* linear_nt_h3_kernel<64> (N <= 64)                                        */
#define SVR_LIN_K_NT128_BWD 5   /* linear_nt_h3_kernel<128, BWD> on transposed planes                       */
#define SVR_LIN_K_NN_X3 6       /* linear_nn_x3_kernel (bf16 or scaled f16 split)                           */
#define SVR_LIN_K_TN_TR 7       /* linear_tn_x3_tr_kernel + slab_reduce_x3_kernel                           */
#define SVR_LIN_K_TN_PREPASS 8  /* dy_planes_kernel + linear_tn_x3_kernel + slab_reduce_x3_kernel           */
#define SVR_LIN_K_NT_X6 9       /* linear_nt_x6_kernel                                                      */
#define SVR_LIN_BIAS_NONE 0
#define SVR_LIN_BIAS_KERNEL 1       /* column sums of the dY rows the weight-gradient kernel loads          */
#define SVR_LIN_BIAS_COLSUM_VEC 2   /* colsum_partial_kernel (float4)                                       */
#define SVR_LIN_BIAS_COLSUM_SLOW 3  /* colsum_partial_slow_kernel (one thread per column)                   */
int svr_linear_variant(int32_t op, int64_t M, int64_t N, int64_t K, int64_t ld_a, int64_t ld_b, int64_t ld_out,
                       int64_t ld_mask, int32_t lo_a, int32_t lo_b, int32_t lo_out, int32_t lo_mask, int32_t epilogue,
                       int32_t want_bias, int32_t *kernel, int32_t *coalesced, int32_t *splits, int64_t *rows_per_split,
                       int32_t *bias_form, int32_t *status);

/* fc_out (Conv1d(hidden,1,1), model/ifnet.py:35,58-59): logits[r(m)] = H[m,:].w + b, where
 * r(m) = row_map[m] if row_map != NULL (rows were processed in Morton order: scatter the logits back
 * to the caller's point order) else m.                                                            */
int svr_fc_out_fwd(const float *H, int64_t ldh, const float *w, const float *b, float *logits,
                   const int32_t *row_map, int64_t M, int64_t K, void *stream);
/* With g[m] = dlogits[r(m)]:  dH[m,k] = g[m]*w[k]*(H[m,k]>0);  dw[k] = sum_m g[m]*H[m,k];
 * db = sum g.  workspace: svr_fc_out_bwd_workspace() bytes.  amax_dh (may be NULL; must hold 0 on entry):
 * receives the bit pattern of max |dH| -- the scale of the next layer's "f16x3s" products, see
 * svr_linear_bwd_data_f16x3.                                                                 */
int64_t svr_fc_out_bwd_workspace(int64_t M, int64_t K);
int svr_fc_out_bwd(const float *H, int64_t ldh, const float *w, const float *dlogits,
                   const int32_t *row_map, float *dH, int64_t lddh, float *dw, float *db, int64_t M,
                   int64_t K, uint32_t *amax_dh, void *workspace, void *stream);

/* The tail of the point MLP in one kernel (mlp_tail.hip): h1 = relu(h0 W1^T + b1), h2 = relu(h1 W2^T + b2),
 * logits[r(m)] = h2[m,:].w_out + b_out -- bit for bit what svr_linear_fwd_f16x3 (twice, BIAS_RELU) and svr_fc_out_fwd
 * return, without reading h1 and h2 back (both are still written: the backward needs them).  W1, W2 (hidden, hidden)
 * contiguous; h0, h1, h2 (M, hidden) with leading dimensions ldh*.  hidden == 256 only; h0 / h1 / h2 rows 16-byte aligned,
 * leading dimensions multiples of 4, w_out 16-byte aligned: SVR_E_UNSUPPORTED otherwise (run the three ops instead).
 * PREPARE / RUN as svr_linear_fwd_f16x3: h0 == NULL prepares the workspace from W1 and W2 only, W1 == NULL (then W2 == NULL
 * too) runs on a prepared workspace.  workspace: svr_mlp_tail_fwd_workspace(hidden) bytes (SVR_E_UNSUPPORTED for a width
 * the kernel is not built for).                                                                                       */
int64_t svr_mlp_tail_fwd_workspace(int64_t hidden);
int svr_mlp_tail_fwd(const float *h0, int64_t ldh0, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *w_out, const float *b_out, float *h1, int64_t ldh1, float *h2, int64_t ldh2,
                     float *logits, const int32_t *row_map, int64_t M, int64_t hidden, void *workspace, void *stream);

/* BCE-with-logits, reduction 'none' -> sum over points -> mean over batch
 * (trainer/trainer_ifnet.py:46).  loss: 1 float; dlogits (B,N) = gscale*(sigmoid(z)-y)/B
 * (dlogits may be NULL).  workspace: B doubles.                                           */
int svr_bce_logits_sum_mean(const float *logits, const float *targets, float *loss, float *dlogits,
                            int64_t B, int64_t N, float gscale, void *workspace, void *stream);
/* The same loss and gradient with the sum in a fixed order (no atomics): every block of a sample leaves its float64
 * partial in workspace[b][block], one thread adds a sample's partials in ascending block order and then the samples in
 * ascending b.  workspace: svr_bce_ordered_workspace(B) bytes.                                                  */
int64_t svr_bce_ordered_workspace(int64_t B);
int svr_bce_logits_sum_mean_ordered(const float *logits, const float *targets, float *loss, float *dlogits,
                                    int64_t B, int64_t N, float gscale, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * 3x3x3 convolution, padding 1, channels-last (replaces nn.Conv3d(.,.,3,padding=1) + ReLU
 * model/ifnet.py:126-135,164-191 and autograd).  Weights in the packed layout made by
 * svr_conv3d_pack_weight: fwd  Wp[tap][ci][co],  bwd-data  Wp[tap'][co][ci] (flipped taps).
 * ------------------------------------------------------------------------------------- */
int svr_conv3d_pack_weight(const float *W /*(Co,Ci,3,3,3)*/, float *Wp_fwd, float *Wp_bwd,
                           int32_t Ci, int32_t Co, void *stream);
int svr_conv3d_unpack_wgrad(const float *dWp /*[tap][ci][co]*/, float *dW /*(Co,Ci,3,3,3)*/,
                            int32_t Ci, int32_t Co, void *stream);
/* out(B,D,H,W,Co) = epi( conv(in(B,D,H,W,Ci), Wp) ): epilogue BIAS / BIAS_RELU / NONE / MASK.
 * Used for forward (Wp_fwd) and for backward-data (Wp_bwd, Ci<->Co swapped by the caller). */
int svr_conv3d_k3(const float *in, const float *Wp, const float *bias, float *out, int32_t B,
                  int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co, int epilogue,
                  const float *mask, void *stream);
/* conv_in (Ci == 1, model/ifnet.py:126,165) forward with the statistics of the following BatchNorm3d fused in:
 * out(B,D,H,W,Co) = epi(conv(in(B,D,H,W,1), Wp[27][1][Co]) + bias), stats[0:Co] = mean, stats[Co:2Co] = biased variance
 * of `out` (float64: what svr_bn_stats(out) returns) without re-reading the output.  Co in {16, 32}.
 * workspace: svr_conv3d_c1_fwd_stats_workspace(B, D, H, W, Co) bytes.                                       */
int64_t svr_conv3d_c1_fwd_stats_workspace(int32_t B, int32_t D, int32_t H, int32_t W, int32_t Co);
int svr_conv3d_c1_fwd_stats(const float *in, const float *Wp, const float *bias, float *out, double *stats,
                            int32_t B, int32_t D, int32_t H, int32_t W, int32_t Co, int epilogue,
                            void *workspace, void *stream);
/* Forward at f32 accuracy on the bf16 matrix cores (bf16x6, see svr_linear_fwd_bf16x6): takes the UNPACKED
 * weights W(Co,Ci,3,3,3); epilogue NONE / BIAS / BIAS_RELU; Ci % 16 == 0.
 * workspace: svr_conv3d_fwd_bf16x6_workspace(Ci, Co) bytes.                                              */
int64_t svr_conv3d_fwd_bf16x6_workspace(int32_t Ci, int32_t Co);
int svr_conv3d_k3_fwd_bf16x6(const float *in, const float *W, const float *bias, float *out, int32_t B,
                             int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue,
                             void *workspace, void *stream);
/* Same contract with the 3-product f16 split (see svr_linear_fwd_f16x3): f32-level accuracy for |in| < 65504 at half
 * the matrix-core work of bf16x6.  workspace: svr_conv3d_fwd_f16x3_workspace(Ci, Co) bytes.               */
int64_t svr_conv3d_fwd_f16x3_workspace(int32_t Ci, int32_t Co);
int svr_conv3d_k3_fwd_f16x3(const float *in, const float *W, const float *bias, float *out, int32_t B,
                             int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue,
                             void *workspace, void *stream);
/* ... + the BatchNorm statistics of `out` from the kernel's epilogue: part[blocks][2][Co] float64 partial sums (sum, sum of
 * squares of the stored values), blocks = svr_conv3d_fwd_f16x3_stats_blocks(same shape); finish with svr_bn_finalize_parts.
 * (model/ifnet.py:170-172 etc.: the last convolution of a stage -> ReLU -> BatchNorm3d.)                              */
int32_t svr_conv3d_fwd_f16x3_stats_blocks(int32_t B, int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co);
int svr_conv3d_k3_fwd_f16x3_stats(const float *in, const float *W, const float *bias, float *out, double *part, int32_t B,
                                  int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue,
                                  void *workspace, void *stream);
/* Backward-data on the bf16 matrix cores with the 3-term split (see svr_linear_bwd_data_bf16x3):
 * din(B,D,H,W,Ci) = epi( conv^T(dout(B,D,H,W,Co), W(Co,Ci,3,3,3)) ), epilogue NONE or MASK (mask like din).
 * Takes the UNPACKED weights; workspace: svr_conv3d_bwd_data_bf16x3_workspace(Ci, Co) bytes.  Ci even.   */
int64_t svr_conv3d_bwd_data_bf16x3_workspace(int32_t Ci, int32_t Co);
int svr_conv3d_k3_bwd_data_bf16x3(const float *dout, const float *W, float *din, int32_t B, int32_t D,
                                  int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue,
                                  const float *mask, void *workspace, void *stream);
/* dWp[tap][ci][co] = sum_m in[m+tap][ci]*dout[m][co]; db[co] = sum_m dout[m][co] (may be NULL). */
int64_t svr_conv3d_k3_bwd_weight_workspace(int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci,
                                           int32_t Co);
int svr_conv3d_k3_bwd_weight(const float *in, const float *dout, float *dWp, float *db, int32_t B,
                             int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                             void *workspace, void *stream);
/* Same result on the bf16 matrix cores with the 3-term split (voxels are the MFMA reduction; ~1e-5 relative);
 * Ci, Co % 4 == 0.  workspace: svr_conv3d_k3_bwd_weight_bf16x3_workspace(...) bytes.                      */
int64_t svr_conv3d_k3_bwd_weight_bf16x3_workspace(int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci,
                                                  int32_t Co);
int svr_conv3d_k3_bwd_weight_bf16x3(const float *in, const float *dout, float *dWp, float *db, int32_t B,
                                    int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                                    void *workspace, void *stream);
/* The same, written straight in the parameter's layout dW(Co,Ci,3,3,3) (autograd's layout of nn.Conv3d.weight.grad):
 * the slab reduction, the layout change and the bias-gradient reduction are one launch.                          */
int svr_conv3d_k3_bwd_weight_bf16x3_param(const float *in, const float *dout, float *dW, float *db, int32_t B,
                                          int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                                          void *workspace, void *stream);
/* The encoder's two backward products at f32 LEVEL on the scaled f16 split ("f16x3s", see svr_linear_bwd_data_f16x3):
 * amax_dout = svr_amax_f32 of dout (or the amax output of the kernel that made it; NULL: no scaling), amax_din (may be
 * NULL) receives |max| of the stored din.  bwd_data: PREPARE / RUN like the bf16x3 entry (dout NULL = prepare from W,
 * W NULL = run), workspace svr_conv3d_bwd_data_f16x3_workspace(Ci, Co) bytes, Co % 16 == 0, Ci even.  bwd_weight:
 * workspace svr_conv3d_k3_bwd_weight_bf16x3_workspace(...) bytes, Ci, Co % 4 == 0; param_layout != 0: dW(Co,Ci,3,3,3),
 * else the packed [tap][ci][co].                                                                                    */
int64_t svr_conv3d_bwd_data_f16x3_workspace(int32_t Ci, int32_t Co);
int svr_conv3d_k3_bwd_data_f16x3(const float *dout, const float *W, float *din, int32_t B, int32_t D,
                                 int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue,
                                 const float *mask, const uint32_t *amax_dout, uint32_t *amax_din,
                                 void *workspace, void *stream);
int svr_conv3d_k3_bwd_weight_f16x3(const float *in, const float *dout, float *dW, float *db, int32_t B,
                                   int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co, int32_t param_layout,
                                   const uint32_t *amax_dout, void *workspace, void *stream);
/* Which kernel instantiation the split-precision 3x3x3 entry points above take for a shape (the launchers ask the same
 * function).  Host only: no device memory is touched, callable without a GPU.  op = SVR_CONV_*; shapes as the entry point
 * takes them (Ci / Co of the CONVOLUTION; backward-data writes Ci columns and reduces over Co).  Outputs (each may be NULL):
 *   ck: channels of the reduction side per LDS chunk (16 / 32);  tn: 32-column output tiles per workgroup (1 / 2 / 4);
 *   vt: z-slices per wave (2 = the 8x4x8 double-brick tile, 32 columns);  persistent: 1 = conv3d_brick_p_kernel (bricks
 *   handed to resident workgroups; SVR_CONV_PERSISTENT=0 in the environment turns it off), 0 = one brick per workgroup;
 *   workgroup_rows: bricks of the volume = grid.x of the one-brick kernels = partial-sum rows of the stats epilogue
 *   (svr_conv3d_fwd_f16x3_stats_blocks).  SVR_E_UNSUPPORTED for channel counts the entry point refuses.            */
#define SVR_CONV_FWD_F16X3 0
#define SVR_CONV_BWD_DATA_F16X3S 1
#define SVR_CONV_BWD_DATA_BF16X3 2
#define SVR_CONV_FWD_BF16X6 3
int svr_conv3d_k3_variant(int32_t op, int32_t B, int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int32_t *ck,
                          int32_t *tn, int32_t *vt, int32_t *persistent, int64_t *workgroup_rows);
/* Which kernel a 3x3x3 weight-gradient entry point runs for a shape (each launcher asks the same function).  Host only: no
 * device memory is touched, callable without a GPU.  op = SVR_CONV_BWD_WEIGHT_*: F32 = svr_conv3d_k3_bwd_weight, F16X3S =
 * svr_conv3d_k3_bwd_weight_f16x3, BF16X3 = svr_conv3d_k3_bwd_weight_bf16x3 and its _param form.  Outputs (each may be NULL):
 *   kernel: SVR_WGRAD_*.  The f32 entry: C1_CO16_LDS (Ci == 1, Co == 16, W <= 128: input rows in LDS), C1_CO16 (wider rows),
 *     C1 (Ci == 1, other Co <= 32), BRICK (Ci, Co % 4 == 0).  The split entries: WS_PAIR / WS = the wave-specialised kernel
 *     (paired-row tiles for Ci <= 16) where every workgroup gets 8 bricks or more, X3 = the 8-wave kernel otherwise;
 *   parts: workgroups (per 32 x 32 channel-tile pair for BRICK / WS_PAIR / WS / X3) among which the volume is dealt;
 *   max_bricks_per_part: 4x4x8-voxel bricks the busiest of them walks (1 for the Ci == 1 kernels: one chunk of rows each).
 * Returns what the entry point returns for the shape (SVR_E_BADSHAPE / SVR_E_UNSUPPORTED), SVR_E_BADARG for an unknown op.  */
#define SVR_CONV_BWD_WEIGHT_F32 0
#define SVR_CONV_BWD_WEIGHT_F16X3S 1
#define SVR_CONV_BWD_WEIGHT_BF16X3 2
#define SVR_WGRAD_C1_CO16_LDS 0
#define SVR_WGRAD_C1_CO16 1
#define SVR_WGRAD_C1 2
#define SVR_WGRAD_BRICK 3
#define SVR_WGRAD_WS_PAIR 4
#define SVR_WGRAD_WS 5
#define SVR_WGRAD_X3 6
int svr_conv3d_k3_bwd_weight_variant(int32_t op, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                                     int32_t *kernel, int32_t *parts, int64_t *max_bricks_per_part);

/* ---------------------------------------------------------------------------------------
 * BatchNorm3d (training or eval) + MaxPool3d(2), channels-last
 * (replaces nn.BatchNorm3d model/ifnet.py:138-142,165-192 and nn.MaxPool3d(2) :136,169-188).
 * ------------------------------------------------------------------------------------- */
/* stats[0:C] = mean, stats[C:2C] = biased variance over (B,D,H,W) in float64.
 * workspace: svr_bn_stats_workspace() bytes.                                              */
int64_t svr_bn_stats_workspace(int64_t rows, int32_t C);
int svr_bn_stats(const float *x, double *stats, int64_t rows /*B*D*H*W*/, int32_t C,
                 void *workspace, void *stream);
/* svr_bn_stats followed by svr_bn_finalize(training = 1) in two launches instead of three (stats may be NULL).
 * mean_lo (C floats, may be NULL): mean - mean_f32, so that mean_f32 + mean_lo is the mean to ~2^-48; the backward
 * centres x with both (svr_bn_bwd_*), which keeps xhat accurate where |mean| >> std.                                */
int svr_bn_stats_finalize(const float *x, double *stats, const float *gamma, const float *beta, float *running_mean,
                          float *running_var, float *scale_shift, float *mean_f32, float *mean_lo, int64_t rows,
                          int32_t C, float eps, float momentum, void *workspace, void *stream);
/* The same from per-workgroup partial sums part[blocks][2][C] (float64 sum / sum of squares of the BatchNorm's input, left by
 * svr_conv3d_k3_fwd_f16x3_stats): no pass over the tensor at all.                                                   */
int svr_bn_finalize_parts(const double *part, int32_t blocks, double *stats, const float *gamma, const float *beta,
                          float *running_mean, float *running_var, float *scale_shift, float *mean_f32, float *mean_lo,
                          int64_t rows, int32_t C, float eps, float momentum, void *stream);
/* scale_shift[0:C] = gamma*invstd, [C:2C] = beta - mean*gamma*invstd, [2C:3C] = invstd (f32);
 * training != 0 also updates running_mean/var (momentum, unbiased var) like torch.          */
int svr_bn_finalize(const double *stats, const float *gamma, const float *beta, float *running_mean,
                    float *running_var, float *scale_shift, float *mean_f32, int64_t rows,
                    int32_t C, float eps, float momentum, int training, void *stream);
/* y = x*scale + shift (full resolution);  pooled (B,D/2,H/2,W/2,C) = 2x2x2 max of y (floor),
 * argmax (uint8 0..7, first maximum in z,y,x scan order) -- pooled/argmax may be NULL.
 * With mean_f32 (else NULL, and mean_lo / beta NULL too): y = ((x - mean_f32) - mean_lo)*scale + beta (mean_lo, beta may
 * be NULL = 0), which has no f32 shift of the size of mean*scale in it: accurate where |mean| >> std, y = beta exactly
 * on a constant channel.                                                                      */
int svr_bn_apply_pool(const float *x, const float *scale_shift, const float *mean_f32, const float *mean_lo,
                      const float *beta, float *y, float *pooled, uint8_t *argmax, int32_t B, int32_t D, int32_t H,
                      int32_t W, int32_t C, void *stream);
/* Backward of [ReLU ->] BN -> {sample, pool}:
 *   dy_total = dy (may be NULL = 0) + unpool(dpooled via argmax) (dpooled may be NULL)
 *   sums[0:C] = sum dy_total, sums[C:2C] = sum dy_total*xhat   (float64, step 1)
 *   dx = gamma*invstd*(dy_total - sum1/n - xhat*sum2/n) * (x > 0 if relu_mask & 1)  (step 2)
 *   dgamma = sum2, dbeta = sum1.
 * relu_mask bit 1 (value 2): the forward used FROZEN statistics (eval mode, running mean / var from
 * svr_bn_finalize(training = 0)): autograd of F.batch_norm(training=False) is dx = gamma*invstd*dy_total;
 * dgamma / dbeta are the same sums.
 * xhat = ((x - mean_f32) - mean_lo) * invstd; mean_lo may be NULL (= 0: the forward left none).   */
int svr_bn_bwd_reduce(const float *x, const float *dy, const float *dpooled, const uint8_t *argmax,
                      const float *mean_f32, const float *mean_lo, const float *scale_shift, double *sums, int32_t B,
                      int32_t D, int32_t H, int32_t W, int32_t C, void *workspace, void *stream);
int svr_bn_bwd_apply(const float *x, const float *dy, const float *dpooled, const uint8_t *argmax,
                     const float *mean_f32, const float *mean_lo, const float *scale_shift, const float *gamma,
                     const double *sums, float *dx, float *dgamma, float *dbeta, int32_t B,
                     int32_t D, int32_t H, int32_t W, int32_t C, int relu_mask, uint32_t *amax_dx,
                     void *stream);   /* amax_dx (may be NULL; 0 on entry): bit pattern of max |dx|, as svr_fc_out_bwd's */

/* ---------------------------------------------------------------------------------------
 * First encoder stage of the 128-architecture as one recomputed unit (stage1.hip):
 *   a = relu(conv_in(x) + bias), y = BatchNorm3d(a), pooled = MaxPool3d(2)(y)
 * (replaces model/ifnet.py:126,138,136 as called at :165-166,169, and their autograd).  `a` -- one input channel, 27 taps,
 * 16 outputs -- is recomputed from x in every pass instead of being stored: the forward reads x and writes y / pooled /
 * argmax only, the backward reads x, dy, dpooled and writes the parameter gradients only.
 *   svr_stage1_supported: Co == 16 and 32-bit offsets inside one sample.
 *   svr_stage1_fwd:  training != 0: batch statistics (stats[0:16] mean, [16:32] biased variance, float64; running
 *                    statistics updated like torch), else the running statistics; outputs as svr_bn_finalize +
 *                    svr_bn_apply_pool (scale_shift 3 x 16, mean_f32 16, y, pooled / argmax may be NULL).
 *   svr_stage1_bwd:  dy_total = dy (may be NULL) + unpool(dpooled via argmax) (may be NULL); sums (float64, 2 x 16) =
 *                    sum dy_total, sum dy_total*xhat; dgamma, dbeta; dW(16,1,3,3,3) (the PARAMETER's layout) and db[16]
 *                    (may be NULL) of conv_in; dout (may be NULL)
 *                    = d(loss)/d(conv_in output) for a caller that needs d(loss)/d(x).  relu_mask as svr_bn_bwd_apply.
 *   f16x3 != 0: the recomputed convolution runs as the 3-product f16 split of svr_conv3d_k3_fwd_f16x3 (f32-level
 *                    accuracy for |x| < 65504, 3 matrix instructions per 16 voxels instead of 7 exact-f32 ones); 0: exact
 *                    f32.  The backward must be called with the flag the forward was called with (it recomputes the same
 *                    activation: ReLU mask and xhat bit for bit).
 *   workspace: svr_stage1_workspace(B, D, H, W) bytes.  Wp = svr_conv3d_pack_weight's Wp_fwd ([27][1][16]).          */
int32_t svr_stage1_supported(int32_t B, int32_t D, int32_t H, int32_t W, int32_t Co);
int64_t svr_stage1_workspace(int32_t B, int32_t D, int32_t H, int32_t W);
int svr_stage1_fwd(const float *x, const float *Wp, const float *bias, const float *gamma, const float *beta,
                   float *running_mean, float *running_var, float *y, float *pooled, uint8_t *argmax,
                   float *scale_shift, float *mean_f32, double *stats, int32_t B, int32_t D, int32_t H, int32_t W,
                   int32_t Co, float eps, float momentum, int training, int f16x3, void *workspace, void *stream);
int svr_stage1_bwd(const float *x, const float *Wp, const float *bias, const float *dy, const float *dpooled,
                   const uint8_t *argmax, const float *mean_f32, const float *scale_shift, double *sums,
                   float *dgamma, float *dbeta, float *dW, float *db, float *dout, int32_t B, int32_t D,
                   int32_t H, int32_t W, int32_t Co, int relu_mask, int f16x3, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Depth -> point cloud -> voxel grid  (model/projection.py).
 * ------------------------------------------------------------------------------------- */
/* pc[b][v*Wi+u] = (c2f * [X,Y,Z,1]) then optionally (p - dims/2)/dims  (projection.py:150-163,
 * 199-206, 124-132).  consts: f, cx, cy, c2f[0][0], c2f[0][3], c2f[1][1], c2f[1][3], c2f[2][2],
 * c2f[2][3], dims0, dims1, dims2 (12 floats, host memory).  gdepth/gpc for the backward.   */
int svr_unproject_fwd(const float *depth, float *pc, int32_t B, int32_t Hi, int32_t Wi,
                      const float *consts, int normalize, void *stream);
int svr_unproject_bwd(const float *depth, const float *gpc, float *gdepth, int32_t B, int32_t Hi,
                      int32_t Wi, const float *consts, int normalize, void *stream);
/* acc (B,D0,D1,D2) += trilinear splat of valid points (projection.py:39-78); acc must be zeroed
 * by the caller.  base (B,N,3) int32 and valid (B,N) uint8 are optional outputs (bit-exact gate). */
int svr_voxelize_splat_fwd(const float *pts, float *acc, int32_t *base, uint8_t *valid, int32_t B,
                           int32_t N, int32_t D0, int32_t D1, int32_t D2, void *stream);
/* gpts (B,N,3) = gradient wrt the normalised points given gacc (gradient wrt acc).          */
int svr_voxelize_splat_bwd(const float *pts, const float *gacc, float *gpts, int32_t B, int32_t N,
                           int32_t D0, int32_t D1, int32_t D2, void *stream);
/* out = clamp(scale*in, 0, 1): scale 8 = the reference's x8 alias quirk (projection.py:75-80),
 * scale 1 = the final clamp of the blur (:116).  bwd: gin = scale*gout where 0 <= scale*in <= 1.
 * NaN is loud, as in torch.clamp: fwd gives NaN for a NaN input (never a clean 0), bwd gives 0.  */
int svr_scale_clamp01_fwd(const float *in, float *out, int64_t n, float scale, void *stream);
int svr_scale_clamp01_bwd(const float *in, const float *gout, float *gin, int64_t n, float scale,
                          void *stream);
/* One axis pass of the separable blur (projection.py:96-114): out = correlation along `axis`
 * (0 = first spatial) with taps[K] (device memory, K odd <= 15), zero padding K/2.           */
int svr_blur_axis_fwd(const float *in, const float *taps, float *out, int32_t B, int32_t D0,
                      int32_t D1, int32_t D2, int32_t axis, int32_t K, void *stream);
/* gin = adjoint pass of gout (gin may be NULL); gtaps[K] (float64, zeroed by the caller) +=
 * sum_i gout[i]*in[i + t - K/2]  (gtaps may be NULL).                                        */
int svr_blur_axis_bwd(const float *in, const float *taps, const float *gout, float *gin,
                      double *gtaps, int32_t B, int32_t D0, int32_t D1, int32_t D2, int32_t axis,
                      int32_t K, void *stream);

/* ---- ordered (bit-reproducible) forms of the two reductions above: DESIGN.md section 16 ----
 *
 * svr_voxelize_splat_fwd_ordered: the splat without float atomics, in a FIXED SUMMATION ORDER that is a function of
 * the point array and the shape alone:
 *   - a point's base voxel (i0, i1, i2), fractions (r0, r1, r2) and validity are those of svr_voxelize_splat_fwd
 *     (same device function); its weight for corner (k, j, l) is (w0[k] * w1[j]) * w2[l] in float32 with
 *     w[0] = 1 - r, w[1] = r, as there;
 *   - voxel (z, y, x) of sample b holds eight partial sums P[k][j][l], k, j, l in {0, 1}: P[k][j][l] is the float32
 *     sum, starting from +0 and taken SEQUENTIALLY IN ASCENDING POINT INDEX n, of the corner-(k, j, l) weights of the
 *     valid points of sample b whose base voxel is (z - k, y - j, x - l);
 *   - acc[b][z][y][x] = ((P000 + P001) + (P010 + P011)) + ((P100 + P101) + (P110 + P111)).
 * Implementation: the points are keyed by (b, i0 + 1, i1 + 1, i2 + 1) in a (D0+1) x (D1+1) x (D2+1) lattice (invalid
 * and NaN points: a sentinel key), sorted with the stable 32-bit radix sort, and a pull kernel in which a thread owns
 * a strip of consecutive x voxels walks the CSR ranges of the contributing cells.  EVERY voxel of acc is written (it
 * need not be zeroed).  vox (may be NULL, acc's shape) = clamp(8 * acc, 0, 1), svr_scale_clamp01_fwd's arithmetic, from
 * the same kernel.  base / valid: as svr_voxelize_splat_fwd.  Needs B*(D0+1)*(D1+1)*(D2+1) < 2^31 - 1 and
 * B*N < 2^31 (SVR_E_UNSUPPORTED otherwise; svr_voxelize_splat_ordered_workspace then returns SVR_E_UNSUPPORTED too).
 * workspace: svr_voxelize_splat_ordered_workspace(B, N, D0, D1, D2) bytes.                                         */
int64_t svr_voxelize_splat_ordered_workspace(int32_t B, int32_t N, int32_t D0, int32_t D1, int32_t D2);
int svr_voxelize_splat_fwd_ordered(const float *pts, float *acc, float *vox, int32_t *base, uint8_t *valid, int32_t B,
                                   int32_t N, int32_t D0, int32_t D1, int32_t D2, void *workspace, void *stream);
/* svr_blur_axis_bwd with the tap gradient in a fixed order: the same grid and per-thread float32 grid-stride partials,
 * the same float64 tree inside a block; the block sums go to workspace[block][K] (float64) and one small kernel adds
 * them in a fixed order (per tap: lane i of 64 adds blocks i, i + 64, ... in ascending order, then a fixed tree over the
 * lanes).  gtaps[K] (float64) is WRITTEN (no zero fill).  workspace:
 * svr_blur_axis_bwd_ordered_workspace(B, D0, D1, D2, K) bytes (only read when gtaps is given).                      */
int64_t svr_blur_axis_bwd_ordered_workspace(int32_t B, int32_t D0, int32_t D1, int32_t D2, int32_t K);
int svr_blur_axis_bwd_ordered(const float *in, const float *taps, const float *gout, float *gin, double *gtaps,
                              int32_t B, int32_t D0, int32_t D1, int32_t D2, int32_t axis, int32_t K, void *workspace,
                              void *stream);

/* ---------------------------------------------------------------------------------------
 * 2-D convolution blocks of the UNet depth regressor (replaces nn.Conv2d(k4,s2,p1) / nn.Conv2d(k3,s1,p1),
 * nn.LeakyReLU(0.2) / nn.ReLU, nn.Upsample(scale_factor=2, mode="bilinear") and torch.cat of model/unet.py:38-60,
 * 66-118 and their autograd).  Channels-last (B,H,W,C) float32.  A block's input is  act( cat(src0, src1) ), optionally
 * upsampled x2 (align_corners False); svr_conv2d_im2col writes its patch matrix
 *   col[(b,oy,ox)][(ky*k+kx)*C + c],  C = C0 + C1,  (B*Ho*Wo) x (k*k*C),  Ho = (Hv + 2 - k)/stride + 1
 * and the convolution itself is svr_linear_fwd* on it (weights repacked to [Cout][(ky*k+kx)*C + c]); backward:
 * svr_linear_bwd_weight* on (dY, col), svr_linear_bwd_data* -> dcol, then svr_conv2d_col2im sums dcol back in gather
 * form (workspace dvirt: B*Hv*Wv*C floats), applies the upsample adjoint and the activation mask and writes the
 * gradients of the two sources (either may be NULL).  act: 0 none, 1 LeakyReLU(0.2), 2 ReLU.
 * ------------------------------------------------------------------------------------- */
typedef struct svr_conv2d_desc {
  const float *src0, *src1; /* (B,H,W,C0), (B,H,W,C1) or NULL */
  int32_t B, H, W, C0, C1;
  int32_t k, stride;        /* (4,2) or (3,1); padding 1 */
  int32_t act, upsample;
} svr_conv2d_desc;
int svr_conv2d_im2col(const svr_conv2d_desc *d, float *col, void *stream);
int svr_conv2d_col2im(const svr_conv2d_desc *d, const float *dcol, float *dvirt, float *dsrc0, float *dsrc1, void *stream);

/* The same blocks as IMPLICIT GEMMs (round 4; the default of model/unet.py's hip backend, conv2d_igemm.hip): no patch matrix.
 * The A operand of the split-precision MFMA GEMM is gathered from the channels-last input -- a reduction step is 16 channels of
 * one tap; activation and concatenation are applied on the way in.  Descriptors here have upsample = 0: a decoder block first
 * writes its input  V = upsample_x2(act(cat(src0, src1)))  once with svr_conv2d_virtual (1x the activation; any descriptor)
 * and convolves {src0 = V, act = 0}.
 *   svr_conv2d_prepare   W (Cout, C, k, k) as nn.Conv2d holds it -> f16 hi / lo planes of the forward product and (want_bwd)
 *                        of the backward-data product in `planes` (svr_conv2d_planes_bytes); amax: one device word, left with
 *                        max|W| (the scale of the split).  Once per weight version.
 *   svr_conv2d_fwd       Y (B, Ho, Wo, Cout) = conv(act(cat(src0, src1))) + bias (bias may be NULL).  amax_x (may be NULL): word
 *                        holding max|input| -- the input is then a GRADIENT operand, scaled by a power of two into f16's range
 *                        (f16x3s); amax_y (may be NULL): zeroed word, left with max|Y|.  k = 1, stride 1 (no padding) is a plain
 *                        row-major GEMM Y (M, Cout) = X (M, C) W^T with the reduction split of the deep layers: B = H = 1, W = M
 *                        (svr_amd.ops.linear_bwd_data_splitk: few output tiles, long reductions).
 *   svr_conv2d_bwd_data  dIn (B, H, W, C0 + C1) = gradient of the convolution's (activated, concatenated) input from
 *                        dY (B, Ho, Wo, Cout); amax_dy: word holding max|dY| (scaled f16 split), NULL = unscaled.  Stride-2
 *                        layers run as four stride-1 problems, one per parity class of the input pixel.
 *   svr_conv2d_finish_bwd  dIn (or, for an upsampled block, the gradient of V) -> gradients of src0 / src1: upsample adjoint
 *                        (gather form), activation derivative, channel split.  `d` is the BLOCK's descriptor (upsample as is).
 *   svr_conv2d_bwd_weight  dW (Cout, C, k, k) in the parameter's own layout and db (Cout, may be NULL) from dY and the gathered
 *                        input; workspace svr_conv2d_bwd_weight_workspace bytes.
 * Layers with few output tiles split the reduction over workgroups and sum the partial outputs in a fixed order (workspace
 * svr_conv2d_workspace_bytes; deterministic, no atomics).  Limits: B*H*W and B*Ho*Wo < 2^24.                                  */
/* Blocks with 1..4 output channels (the UNet's last layer, 64 -> channels_out: a GEMM tile would be 1/64 full) run on the vector
 * ALUs in plain f32 FMAs straight from W (Cout, C, k, k): no planes, no amax words.  svr_conv2d_small_supported: Cout in 1..4 and
 * Cout*C*k*k <= 8192 (the weights live in LDS).  Same descriptors (upsample = 0) and the same results layout as above.             */
int svr_conv2d_small_supported(int32_t Cout, int32_t C, int32_t k);
int svr_conv2d_small_fwd(const svr_conv2d_desc *d, const float *W, const float *bias, float *Y, int32_t Cout, void *stream);
int svr_conv2d_small_bwd_data(const svr_conv2d_desc *d, const float *W, const float *dY, int32_t Cout, float *dIn, void *stream);
int64_t svr_conv2d_small_bwd_weight_workspace(const svr_conv2d_desc *d, int32_t Cout);
int svr_conv2d_small_bwd_weight(const svr_conv2d_desc *d, const float *dY, int32_t Cout, float *dW, float *db, void *workspace,
                                void *stream);
int64_t svr_conv2d_planes_bytes(int32_t Cout, int32_t C, int32_t k);
int svr_conv2d_prepare(const float *W, int32_t Cout, int32_t C, int32_t k, int32_t stride, int32_t want_bwd, uint32_t *amax,
                       void *planes, void *stream);
/* All layers of a network at once (n <= 16; three launches instead of four per layer): arrays of n weights / shapes / plane
 * buffers; amax_base: n words 256 bytes apart (layer i's word = amax_base + 64 i), zeroed here.  Same planes as n single calls. */
int svr_conv2d_prepare_many(int32_t n, const float *const *W, const int32_t *Cout, const int32_t *C, const int32_t *k,
                            const int32_t *stride, const int32_t *want_bwd, uint32_t *amax_base, void *const *planes, void *stream);
int64_t svr_conv2d_workspace_bytes(const svr_conv2d_desc *d, int32_t Cout);
int svr_conv2d_virtual(const svr_conv2d_desc *d, float *V, void *stream);
int svr_conv2d_fwd(const svr_conv2d_desc *d, const void *planes, const uint32_t *amax_w, const float *bias, float *Y, int32_t Cout,
                   const uint32_t *amax_x, uint32_t *amax_y, void *workspace, void *stream);
int svr_conv2d_bwd_data(const svr_conv2d_desc *d, const void *planes, const uint32_t *amax_w, const float *dY,
                        const uint32_t *amax_dy, int32_t Cout, float *dIn, void *workspace, void *stream);
int svr_conv2d_finish_bwd(const svr_conv2d_desc *d, const float *dvirt, float *dsrc0, float *dsrc1, void *stream);
int64_t svr_conv2d_bwd_weight_workspace(const svr_conv2d_desc *d, int32_t Cout);
int svr_conv2d_bwd_weight(const svr_conv2d_desc *d, const float *dY, const uint32_t *amax_dy, int32_t Cout, float *dW, float *db,
                          void *workspace, void *stream);
/* What the conv2d entry points above do with a layer (the launchers and the workspace-size functions ask the same functions).
 * Host only: no device memory is touched, callable without a GPU.  op = SVR_CV2_*; the shape as the descriptor holds it
 * (act = 0, upsample = 0); lo_src0 / lo_src1 / lo_dy / lo_out: the low four address bits of the two sources, of dY and of the
 * output (Y / dIn).  The layer runs on the plain-FMA kernels where svr_conv2d_small_supported says so (as svr_amd.ops routes it),
 * else on the GEMMs.  plan (may be NULL) receives:
 *   family: SVR_CV2_SMALL / IGEMM64 / IGEMM128 (conv2d_igemm_kernel<64 / 128>) / WGRAD_TR (linear_tn_x3_tr_kernel<true, true, *>);
 *   vec4: the gathered operand (the input; dY for backward-data) goes through the 16-byte loader;  Ho, Wo: output size;
 *   forward / backward-data GEMMs: classes (4: the parity classes of a stride-2 backward), mtiles (row tiles of the largest
 *     class), tiles (workgroups per reduction split), ksteps, splits, ksplit (k-steps per split), epilogue (SVR_CV2_EPI_*: COAL /
 *     LANE = the kernel's own epilogue, float4 rows through LDS or one dword per lane; REDUCE_V4 / REDUCE_SCALAR = partial tiles
 *     summed by ig_reduce_kernel), reduce_grid (its workgroups; it strides where split_stride > 1024 * reduce_grid),
 *     split_stride (floats of the output), workspace_bytes (the partial outputs; 0 unsplit);
 *   weight gradient: dy_vec4 (dY through the float4 loader), tiles, splits (row slabs), rows_per_split, last_rows;
 *   small kernels: co, kk (kernel size), grid (grid.x), capped (forward / backward-data: the grid is at its cap and workgroups
 *     stride), rows_per_block, parts, ipg, groups, grid_y (weight gradient), workspace_bytes (its partials).
 * Returns SVR_OK or the entry point's own refusal (SVR_E_BADARG for an unknown op), its text in svr_last_error().               */
#define SVR_CV2_FWD 0
#define SVR_CV2_BWD_DATA 1
#define SVR_CV2_BWD_WEIGHT 2
#define SVR_CV2_SMALL 0
#define SVR_CV2_IGEMM64 1
#define SVR_CV2_IGEMM128 2
#define SVR_CV2_WGRAD_TR 3
#define SVR_CV2_EPI_COAL 0
#define SVR_CV2_EPI_LANE 1
#define SVR_CV2_EPI_REDUCE_V4 2
#define SVR_CV2_EPI_REDUCE_SCALAR 3
typedef struct svr_conv2d_plan {
  int32_t family, vec4, Ho, Wo;
  int32_t classes, ksteps, splits, ksplit, epilogue, reduce_grid;
  int32_t dy_vec4;
  int32_t co, kk, grid, capped, rows_per_block, parts, ipg, groups, grid_y;
  int64_t mtiles, tiles, split_stride, rows_per_split, last_rows, workspace_bytes;
} svr_conv2d_plan;
int svr_conv2d_variant(int32_t op, int32_t B, int32_t H, int32_t W, int32_t C0, int32_t C1, int32_t Cout, int32_t k, int32_t stride,
                       int32_t lo_src0, int32_t lo_src1, int32_t lo_dy, int32_t lo_out, svr_conv2d_plan *plan);

/* ---------------------------------------------------------------------------------------
 * Occupancy labelling against a triangle mesh (replaces check_mesh_contains,
 * data_processing/libmesh/inside_mesh.py:5-155, and the Cython TriangleHash, libmesh/triangle_hash.pyx:8-85,
 * called per training step by data_processing/mesh_occupancies.py:24-53 when subsample_points > 0).
 * Host side (plain C++, no device work): the 2-D triangle hash as a CSR table.
 *   svr_mesh_hash_entries: number of (cell, triangle) entries; writes scale[3], translate[3] of the mesh rescale to
 *                          [0.5, res-0.5]^3 (inside_mesh.py:17-22) to scale_translate[6].  Negative = SVR_E_*.
 *   svr_mesh_hash_build:   tri (n_faces*9 rescaled float64 coordinates), cell_start (res*res+1), tri_ids (entries;
 *                          triangles in index order inside a cell, like the reference's push_back order).
 * verts (n_verts,3) float64 and faces (n_faces,3) int32 are HOST arrays; all outputs are HOST arrays the caller
 * then copies to the device.
 * Device side: svr_mesh_contains -- points (n,3) float32 (points_f64 = 0) or float64 (1) on the device;
 * contains[i] = inside by both z-ray directions, holes[i] = the two directions disagree (uint8 0/1).  float64
 * arithmetic in the reference's operation order: the booleans equal the reference's bit for bit.
 * ------------------------------------------------------------------------------------- */
int64_t svr_mesh_hash_entries(const double *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int32_t res,
                              double *scale_translate);
int svr_mesh_hash_build(const double *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int32_t res,
                        double *tri, int32_t *cell_start, int32_t *tri_ids, int64_t entries);
int svr_mesh_contains(const void *points, int32_t points_f64, int64_t n, const double *tri, const int32_t *cell_start,
                      const int32_t *tri_ids, int32_t res, const double *scale_translate, uint8_t *contains,
                      uint8_t *holes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Marching cubes (replaces marching_cubes.marching_cubes + export_obj of util/visualize.py:23-25, behind
 * implicit_to_mesh, model/ifnet.py:232-234, and visualize_sdf).  field: (X, Y, Z) float32, C order, on the device;
 * output: a welded, indexed triangle mesh in the field's index space (a vertex (x, y, z) has x along axis 0).
 *   - a lattice point is inside iff (double)v < level (NaN: outside); every cell (i, j, k), i < X-1, j < Y-1,
 *     k < Z-1, is polygonised; any extent below 2 gives an empty mesh; the border is not padded (open surfaces);
 *   - one vertex per crossing lattice edge (exactly one endpoint inside), shared by the cells around it, at
 *     (float)((double)p_axis + fmin(fmax((level - a) / (b - a), 0), 1)), a at the lower endpoint p, b at p + e_axis;
 *   - vertices ordered by owner point (lower endpoint, C order), then axis 0, 1, 2; faces by cell (C order of the
 *     minimum corner), then case-table order; normals point from inside to outside.
 *   svr_mc_workspace_bytes: device workspace for a lattice (negative = SVR_E_BADSHAPE: 2^31 points or more).
 *   svr_mc_count:  classify + scan; writes the device int64 totals[2] = {V, F}.  The caller reads them back and
 *                  allocates verts (V, 3) float32 and faces (F, 3) int32; faces are int32, so V, F < 2^31 is the
 *                  caller's check before svr_mc_emit.
 *   svr_mc_emit:   fills verts / faces from the same field, level and workspace (after svr_mc_count on the stream).
 *   svr_mc_case_table: host only; out[256 * 16] = the kernels' case table, 3 edge ids per triangle, -1 padded
 *                  (edge 4 * axis + (o_u | o_v << 1), corner c at offset (c & 1, c >> 1 & 1, c >> 2 & 1)).
 * ------------------------------------------------------------------------------------- */
int64_t svr_mc_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
int svr_mc_count(const float *field, int32_t X, int32_t Y, int32_t Z, double level, void *ws, int64_t ws_bytes,
                 int64_t *totals, void *stream);
int svr_mc_emit(const float *field, int32_t X, int32_t Y, int32_t Z, double level, void *ws, float *verts, int32_t *faces,
                void *stream);
int svr_mc_case_table(int8_t *out);

/* ---------------------------------------------------------------------------------------
 * Block-sparse evaluation of the occupancy lattice in front of svr_mc_* (not a reference op: a coarse-to-fine
 * extractor in the manner of MISE; driven by util/sparse_grid.py, restated in numpy by tests/sparse_lattice_oracle.py).
 * The network is queried only in blocks the surface passes through; the field handed to svr_mc_* stays a dense
 * (X, Y, Z) float32 array.  Errors, ownership and streams as for svr_mc_*.
 *   - lattice (X, Y, Z), every extent >= 2, fewer than 2^31 points; block edge s >= 2 cells (else SVR_E_BADSHAPE).
 *     Per axis with n points: nb = ceil((n-1)/s) blocks; coarse indices c[i] = min(i*s, n-1), i = 0..nb; lattice
 *     index i is owned by block min(i / s, nb-1) (the last block also owns index n-1).  Blocks, coarse points and the
 *     owned points of a block are all numbered in C order (z fastest);
 *   - inside(v) := (double)v < level (NaN: outside), the rule of svr_mc_*;
 *   - coordinates: tx, ty, tz are device tables of X, Y, Z float32 (torch.linspace(-0.5, 0.5, n), the tensors
 *     make_3d_grid expands); the kernels copy table entries and never compute a coordinate;
 *   - 1. C = f at the (nbx+1)(nby+1)(nbz+1) coarse points; 2. fill: every lattice point takes C at the minimum
 *     corner of its owner block; 3. round 1 selects the blocks whose 8 corner flags inside(C) are not all equal;
 *     4. a round lists the selected blocks in C order of block index, lists their owned points block by block,
 *     has f evaluated on that list, stores the values into the field and sets the blocks' state to the round
 *     number (>= 1; 0 = never evaluated); 5. leak check, over the blocks of this round only: every lattice edge
 *     (p, q) along an axis with p in such a block, q in a block with state 0 and inside(field[p]) !=
 *     inside(field[q]) selects q's block for the next round and counts once; 6. rounds repeat until one selects
 *     nothing; after `max_rounds` rounds the caller selects every block with state 0 (all = 1), which ends leak-free.
 *     At exit no edge with differing sides has an unevaluated endpoint.
 *   svr_sl_workspace_bytes: device workspace (negative = SVR_E_BADSHAPE).
 *   svr_sl_coarse_points:  pts (coarse points, 3) float32.
 *   svr_sl_fill_seed:      coarse (coarse points) float32 -> field (X, Y, Z), state (nbx, nby, nbz) uint8 = 0, and the
 *                          selection of round 1 in the workspace.
 *   svr_sl_select:         consumes the pending selection (all = 1: every block with state 0 instead): one exclusive
 *                          scan of the per-block owned-point counts; the block list and each block's first row go to
 *                          the workspace; totals[0] = listed blocks, totals[1] = listed points (device int64[3]).
 *                          The caller reads totals back, once per round, to size the point list.
 *   svr_sl_block_points:   pts (totals[1], 3) float32, the owned points of the n_blocks listed blocks.
 *   svr_sl_scatter:        vals (totals[1]) float32 -> field; state of the listed blocks = round (1..255).
 *   svr_sl_leak_check:     step 5 for the listed blocks: marks the next selection, totals[2] = counted edges (read
 *                          back with the next round's totals).
 * ------------------------------------------------------------------------------------- */
int64_t svr_sl_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t s);
int svr_sl_coarse_points(const float *tx, const float *ty, const float *tz, int32_t X, int32_t Y, int32_t Z, int32_t s,
                         float *pts, void *stream);
int svr_sl_fill_seed(const float *coarse, int32_t X, int32_t Y, int32_t Z, int32_t s, double level, float *field,
                     uint8_t *state, void *ws, int64_t ws_bytes, void *stream);
int svr_sl_select(int32_t X, int32_t Y, int32_t Z, int32_t s, int32_t all, const uint8_t *state, void *ws, int64_t *totals,
                  void *stream);
int svr_sl_block_points(const float *tx, const float *ty, const float *tz, int32_t X, int32_t Y, int32_t Z, int32_t s,
                        const void *ws, int64_t n_blocks, float *pts, void *stream);
int svr_sl_scatter(const float *vals, int32_t X, int32_t Y, int32_t Z, int32_t s, const void *ws, int64_t n_blocks,
                   int32_t round, float *field, uint8_t *state, void *stream);
int svr_sl_leak_check(const float *field, int32_t X, int32_t Y, int32_t Z, int32_t s, double level, const uint8_t *state,
                      void *ws, int64_t n_blocks, int64_t *totals, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mesh evaluation: IoU, Chamfer-L2, normal consistency (replaces what util/evaluate.py:9-119 takes from trimesh --
 * mesh.sample, face_normals -- and from pykdtree's KDTree.query, and the sampler of data_processing/
 * mesh_occupancies.py:9-22).  Every rule below is restated in numpy by tests/eval_oracle.py; one rounding per
 * operation (no contraction).
 *
 * svr_mesh_face_table: HOST only.  verts (n_verts,3) float64, faces (n_faces,3) int32; face f = (A, B, C):
 *     e1 = B - A, e2 = C - A, n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x),
 *     len = sqrt((nx*nx + ny*ny) + nz*nz), area = 0.5 * len, normals_out[f] = n / len (each component divided);
 *     a face whose len is not > 0 (zero area, NaN) gets a zero normal and area 0;
 *     cum_area_out[f] = cum_area_out[f-1] + area, summed sequentially from f = 0 (numpy: np.cumsum).
 *     SVR_E_BADARG for null pointers, counts <= 0 or a face index outside [0, n_verts).
 * svr_mesh_sample: tri (n_faces,3,3) float64 = verts[faces], cum_area (n_faces), uniforms (n,3) float64 in [0,1),
 *     all on the device.  Sample i: x = u0 * cum_area[F-1]; face = the first j with cum_area[j] > x (a face without
 *     area is never chosen); if there is none (x rounded up to the total), the first j with cum_area[j] >= the total;
 *     (w1, w2) = (u1, u2), or (1 - u1, 1 - u2) if u1 + u2 > 1;
 *     p = (A + w1 * (B - A)) + w2 * (C - A) per coordinate in float64, stored as float32.  points_out (n,3) float32,
 *     face_out (n) int32.  n == 0 is a no-op; n < 0 or n_faces outside [1, 2^31) is SVR_E_BADARG.
 * svr_nn_search: exact nearest target of every query; queries (Q,3), targets (T,3) float32 on the device.
 *     d2(q, t) = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), dx = fl(qx - tx) ..., all float32.  The winner is the
 *     smallest d2; ties go to the LOWEST target index; a NaN d2 never wins against a number (+inf is a number).
 *     dist_out[q] = sqrt(d2) correctly rounded to float32, idx_out[q] = the winner.  A query all of whose d2 are NaN
 *     gets dist NaN and idx -1.  The result does not depend on how the work is split: bit-identical run to run.
 *     workspace: svr_nn_search_workspace(Q) = 8 * Q bytes on the device.  T == 0 or T >= 2^31: SVR_E_BADSHAPE;
 *     Q < 0, a null pointer or a short workspace: SVR_E_BADARG; Q == 0: no-op.
 * svr_nn_normals_dot: dot_out[q] = |n_q / |n_q|  .  n_t[idx[q]] / |n_t[idx[q]]||  in float64 (normals_f64 = 0: both
 *     normal arrays are float32 and are widened first; 1: float64); |n| = sqrt((x*x + y*y) + z*z), the dot is
 *     (x*x' + y*y') + z*z'.  idx[q] outside [0, T) gives NaN.
 * svr_eval_sums: sums_out[3] (device float64) = sum d, sum d*d (d widened to float64 first), sum dot (NaN when
 *     dot == NULL), over n entries, in a fixed order (fixed grid, fixed trees): bit-identical run to run.
 *     workspace: SVR_EVAL_SUMS_WORKSPACE_BYTES on the device.
 * svr_iou_counts: counts_out[2] (device int64) = number of i with a[i] && b[i], with a[i] || b[i] (uint8, 0 = false).
 * All argument checks return before the first HIP call.
 * ------------------------------------------------------------------------------------- */
#define SVR_EVAL_SUMS_WORKSPACE_BYTES 6144
int svr_mesh_face_table(const double *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, double *normals_out,
                        double *cum_area_out);
int svr_mesh_sample(const double *tri, const double *cum_area, int64_t n_faces, const double *uniforms, int64_t n,
                    float *points_out, int32_t *face_out, void *stream);
int64_t svr_nn_search_workspace(int64_t Q);
int svr_nn_search(const float *queries, int64_t Q, const float *targets, int64_t T, float *dist_out, int32_t *idx_out,
                  void *workspace, int64_t workspace_bytes, void *stream);
int svr_nn_normals_dot(const void *normals_q, const void *normals_t, int32_t normals_f64, const int32_t *idx, int64_t Q,
                       int64_t T, double *dot_out, void *stream);
int svr_eval_sums(const float *dist, const double *dot, int64_t n, double *sums_out, void *workspace, int64_t workspace_bytes,
                  void *stream);
int svr_iou_counts(const uint8_t *a, const uint8_t *b, int64_t n, int64_t *counts_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Unsigned distance field of a triangle mesh on a lattice (no reference op: the reference's distance_field.df came
 * from a tool that was never shipped; data_processing/mesh_to_df.py drives this, tests/df_oracle.py restates it in
 * numpy).  Errors, ownership and streams as for svr_mc_*; one rounding per operation (no contraction).
 *   tri: (F, 9) float64 on the device, a, b, c per face, in grid index space (what svr_mc_emit writes: x along
 *   axis 0).  Lattice (X, Y, Z), every extent >= 1, fewer than 2^31 points; point (i, j, k) sits at p = (i, j, k).
 *   dot(u, v) := (ux*vx + uy*vy) + uz*vz.  Per pair (p, face), all float64, in this order:
 *     ab = b - a;  ac = c - a;  ap = p - a;  bp = p - b;  cp = p - c                 (per component)
 *     d1 = dot(ab, ap);  d2 = dot(ac, ap);  d3 = dot(ab, bp);  d4 = dot(ac, bp);  d5 = dot(ab, cp);  d6 = dot(ac, cp)
 *     vc = d1*d4 - d3*d2;  vb = d5*d2 - d1*d6;  va = d3*d6 - d5*d4;  e43 = d4 - d3;  e56 = d5 - d6
 *     (v, w) := the FIRST line whose condition holds (a comparison with NaN is false):
 *       1. d1 <= 0 and d2 <= 0                     (0, 0)                                vertex a
 *       2. d3 >= 0 and d4 <= d3                    (1, 0)                                vertex b
 *       3. vc <= 0 and d1 >= 0 and d3 <= 0         (d1 / (d1 - d3), 0)                   edge ab
 *       4. d6 >= 0 and d5 <= d6                    (0, 1)                                vertex c
 *       5. vb <= 0 and d2 >= 0 and d6 <= 0         (0, d2 / (d2 - d6))                   edge ac
 *       6. va <= 0 and e43 >= 0 and e56 >= 0       w = e43 / (e43 + e56), v = 1 - w      edge bc
 *       7. otherwise                               den = (va + vb) + vc, (vb / den, vc / den)   face interior
 *     q = (a + v*ab) + w*ac;  e = p - q  (per component);  dd = dot(e, e)            (the pair's squared distance)
 *   A face whose ab x ac = (aby*acz - abz*acy, abz*acx - abx*acz, abx*acy - aby*acx) is exactly (0, 0, 0) is skipped.
 *   Per point: best = min dd over the other faces in ascending index with a strict `<` (the lowest index wins a tie,
 *   a NaN dd never wins).  field[i, j, k] = (float)sqrt(best), float32, C order (X, Y, Z); face[i, j, k] = the winner
 *   (int32, optional; -1 when no dd was a number).  truncate = T > 0: where field > (float)T, field = (float)T and
 *   face = -1; truncate <= 0: untruncated (the .df format's rule).
 *   The lattice is cut into bricks of s^3 points, s in {4, 8} (else SVR_E_BADSHAPE), numbered in C order of
 *   (bx, by, bz); the last brick per axis is partial.  Per brick a candidate list of face indices, ascending, that
 *   holds at least every face that wins a point of the brick; the field does not depend on s,
 *   on the lists or on how the bricks are batched: bit-identical to the rule above.
 *   svr_mesh_df_bricks:      number of bricks (negative = SVR_E_BADSHAPE).
 *   svr_mesh_df_workspace_bytes: device workspace of svr_mesh_df_count (negative = SVR_E_BADSHAPE).
 *   svr_mesh_df_valid_faces: counts the faces that are not skipped; SYNCHRONISES the stream and writes the count to
 *                            the HOST int64 *n_valid.  ws: 8 device bytes.  F == 0 or no face with area: SVR_E_BADSHAPE.
 *   svr_mesh_df_count:       the cull sweep: per brick the squared threshold (kept in ws) and the candidate count, then
 *                            an exclusive scan: offsets (bricks + 1 int64, device) -- offsets[bricks] is the total.
 *                            With c the centre and r the half diagonal of the points the brick holds, and dmin the
 *                            smallest sqrt(dd(c, face)): a face is a candidate iff sqrt(dd(c, face)) <= min(dmin, T) +
 *                            2 r + slack (T only when truncate > 0).  `slack` >= 0 covers the rounding of dd and of this
 *                            comparison (DESIGN.md section 18 derives the value the Python driver passes).
 *                            The caller reads offsets back and walks the bricks in batches whose lists fit its buffer.
 *   svr_mesh_df_emit:        lists of bricks [b0, b1) into list (int32, `capacity` entries: no write goes past it; the
 *                            caller sizes it offsets[b1] - offsets[b0]); the list of brick b starts at offsets[b] -
 *                            offsets[b0].  Same tri, lattice, s and ws as the count that filled ws and offsets.
 *   svr_mesh_df_eval:        field / face (face may be NULL) of bricks [b0, b1) from their lists.  list == NULL: every
 *                            face is a candidate of every brick (brute force; offsets is not read).
 * ------------------------------------------------------------------------------------- */
int64_t svr_mesh_df_bricks(int32_t X, int32_t Y, int32_t Z, int32_t s);
int64_t svr_mesh_df_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t s);
int svr_mesh_df_valid_faces(const double *tri, int64_t F, void *ws, int64_t *n_valid, void *stream);
int svr_mesh_df_count(const double *tri, int64_t F, int32_t X, int32_t Y, int32_t Z, int32_t s, double truncate, double slack,
                      void *ws, int64_t ws_bytes, int64_t *offsets, void *stream);
int svr_mesh_df_emit(const double *tri, int64_t F, int32_t X, int32_t Y, int32_t Z, int32_t s, const void *ws,
                     const int64_t *offsets, int64_t b0, int64_t b1, int32_t *list, int64_t capacity, void *stream);
int svr_mesh_df_eval(const double *tri, int64_t F, int32_t X, int32_t Y, int32_t Z, int32_t s, double truncate,
                     const int64_t *offsets, const int32_t *list, int64_t b0, int64_t b1, float *field, int32_t *face,
                     void *stream);

/* ---------------------------------------------------------------------------------------
 * Ray casting a triangle mesh through the pipeline's pinhole camera: depth, distance, face and normal maps (no reference
 * op: the reference's distance.exr came from a renderer that was never shipped; data_processing/render_view.py drives
 * this, tests/raycast_oracle.py restates it in numpy).  Errors, ownership and streams as for svr_mc_*; one rounding per
 * operation (no contraction).
 *   tri: (F, 9) float64 on the device, a, b, c per face, in grid index space (the space of svr_mesh_df_*).
 *   consts: the 12 float32 constants of svr_unproject_fwd in HOST memory, f, cx, cy, s00, t0, s11, t1, s22, t2, dims (dims
 *   unused); each is widened to float64 first.  Image (H, W), 1 <= H, W <= 32768; pixel (u = column, v = row).
 *   unproject_point sends pixel (u, v) at depth z to (s00*(u-cx)/f*z + t0, -s11*(v-cy)/f*z + t1, s22*z + t2), so the
 *   pixel's ray has
 *     o = (t0, t1, t2);   d = (s00 * (((double)u - cx) / f),  -(s11 * (((double)v - cy) / f)),  s22)
 *   and the ray parameter is the depth in metres.  dot(x, y) := (x0*y0 + x1*y1) + x2*y2; cross products component by
 *   component, (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0).  Per pair (pixel, face), all float64, in this order
 *   (Moeller-Trumbore, two-sided; a comparison with NaN is false, so a NaN anywhere rejects the pair):
 *     e1 = b - a;  e2 = c - a;  p = d x e2;  det = dot(e1, p);          det == 0: the face is skipped (edge-on, zero area)
 *     inv = 1 / det;  s = o - a;  bu = dot(s, p) * inv;                 rejected unless 0 <= bu <= 1
 *     q = s x e1;  bv = dot(d, q) * inv;                                rejected unless bv >= 0 and bu + bv <= 1
 *     z = dot(e2, q) * inv;                                             accepted when near < z <= far
 *   Per pixel: best = min z over the accepted faces in ascending index with a strict `<` (the lowest index wins a tie, a
 *   NaN never wins).  Outputs, C order:
 *     depth    (H, W) float32: (float)best; `miss` where no face was accepted (0.0 in the Python driver: svr_depth_grid_mark
 *              sends it to index -8 on axis 2 and counts it out of range);
 *     face     (H, W) int32, optional: the winner, -1 for a miss;
 *     distance (H, W) float32, optional: the inverse of svr_distance_to_depth in the same float32 operations,
 *              distance = depth * sqrt((float)(r*r + c*c) / (f*f) + 1), r = row - H/2, c = col - W/2 (integer division; f
 *              the float32 constant), applied to the stored depth, `miss` included.  The ray uses cx, cy, the distance the
 *              integer centres: exactly what unprojection and svr_distance_to_depth undo;
 *     normal   (H, W, 3) float32, optional: n = e1 x e2 of the winner, len = sqrt(dot(n, n)), m = n / len per component,
 *              m = -m when dot(m, d) > 0; (float)m; 0 for a miss;
 *     shade    (H, W) uint8, optional: rint((255 * |dot(m, d)|) / sqrt(dot(d, d))) (half to even), 0 for a miss or NaN.
 *   Cracks: a ray through a shared edge or vertex may be accepted by both faces, by one or by neither -- the two faces
 *   round bu, bv independently.  Rays go through pixel centres, which makes this rare.  A face without area whose det
 *   rounds to a non-zero value is not skipped; its bu, bv are then noise of size 1 / eps and all but never in range.
 *   The image is cut into tiles of T x T pixels, T in {8, 16} (else SVR_E_BADSHAPE), numbered row by row; the last tile
 *   per axis is partial.  Per tile a candidate list of face indices, ascending, that holds every face accepted by a pixel
 *   of the tile (DESIGN.md section 19 has the argument and what it assumes); the maps do not depend on T, on the lists or
 *   on how the tiles are batched: bit-identical to the rule above.
 *   svr_raycast_tiles:           number of tiles (negative = SVR_E_BADSHAPE).
 *   svr_raycast_workspace_bytes: device workspace of svr_raycast_count (negative = SVR_E_BADSHAPE).
 *   svr_raycast_face_bounds:     rects (F, 4) int32 on the device, {x0, x1, y0, y1} inclusive: per vertex g
 *                                zc = (g2 - t2) / s22, u = cx + (f*(g0 - t0)) / (s00*zc), v = cy - (f*(g1 - t1)) / (s11*zc);
 *                                [floor(min u) - 1, ceil(max u) + 1] x [floor(min v) - 1, ceil(max v) + 1], each side clamped
 *                                to +-2^30.  A face with a zc not above 2^-20, a |u| or |v| not <= 2^30 (NaN, inf) or
 *                                max zc > 1024 * min zc gets {-2^30, 2^30, -2^30, 2^30}: every tile.
 *   svr_raycast_count:           per tile the number of faces whose rectangle overlaps the tile's pixels, then an exclusive
 *                                scan: offsets (tiles + 1 int64, device) -- offsets[tiles] is the total.  The caller reads
 *                                offsets back and walks the tiles in batches whose lists fit its buffer.
 *   svr_raycast_emit:            lists of tiles [b0, b1) into list (int32, `capacity` entries: no write goes past it; the
 *                                caller sizes it offsets[b1] - offsets[b0]); the list of tile t starts at offsets[t] -
 *                                offsets[b0].  Same rects, image and T as the count that filled offsets.
 *   svr_raycast_eval:            the maps of tiles [b0, b1) from their lists (face, distance, normal, shade may be NULL).
 *                                list == NULL: every face is a candidate of every tile (brute force; offsets is not read).
 *                                A list entry outside [0, F) is ignored.
 * ------------------------------------------------------------------------------------- */
int64_t svr_raycast_tiles(int32_t H, int32_t W, int32_t T);
int64_t svr_raycast_workspace_bytes(int32_t H, int32_t W, int32_t T);
int svr_raycast_face_bounds(const double *tri, int64_t F, const float *consts /*[12]*/, int32_t *rects, void *stream);
int svr_raycast_count(const int32_t *rects, int64_t F, int32_t H, int32_t W, int32_t T, void *ws, int64_t ws_bytes,
                      int64_t *offsets, void *stream);
int svr_raycast_emit(const int32_t *rects, int64_t F, int32_t H, int32_t W, int32_t T, const int64_t *offsets, int64_t b0,
                     int64_t b1, int32_t *list, int64_t capacity, void *stream);
int svr_raycast_eval(const double *tri, int64_t F, const float *consts /*[12]*/, int32_t H, int32_t W, int32_t T, double near_z,
                     double far_z, float miss, const int64_t *offsets, const int32_t *list, int64_t b0, int64_t b1,
                     float *depth, int32_t *face, float *distance, float *normal, uint8_t *shade, void *stream);

/* ---------------------------------------------------------------------------------------
 * Vertex colours of a mesh from the image it was reconstructed from (no reference op: the reference shows coloured results
 * but ships no code for them; util/mesh_color.py drives this, tests/vertex_color_oracle.py restates it in numpy).  Errors,
 * ownership and streams as for svr_mc_*.  All arithmetic is float64, one rounding per operation (no contraction); a
 * comparison with NaN is false.
 *   verts: (V, 3) float32 on the device, grid index space (the space of svr_raycast_*: the caller divides lattice indices
 *   by inf_res first).  consts: the 12 float32 constants of svr_unproject_fwd in HOST memory, each widened first (dims
 *   unused).  depth: (H, W) float32 on the device, the SAME mesh seen from the same camera (svr_raycast_eval's depth with
 *   miss = 0).  image: (Hi, Wi, 3) uint8 on the device.  map: {ax, bx, ay, by}, HOST float64: depth-map pixel (u, v) lies at
 *   image position (ax*u + bx, ay*v + by), pixel centres at integers in both.  fill: 3 HOST uint8.  bias: metres.
 *   svr_vertex_color_sample, per vertex g, in this order:
 *     1. zc = (g2 - t2) / s22;  u = cx + (f*(g0 - t0)) / (s00*zc);  v = cy - (f*(g1 - t1)) / (s11*zc)
 *        (svr_raycast_face_bounds' projection);
 *     2. in frame iff zc > 0 and -0.5 <= u <= W - 0.5 and -0.5 <= v <= H - 0.5;
 *     3. seen iff one of the up to four pixels (floor(u) + a, floor(v) + b), a, b in {0, 1}, that lie inside
 *        [0, W) x [0, H) has D > 0 and zc <= (double)D + bias.  A miss is 0 in such a map and never counts; neither does a
 *        negative or NaN D; D = inf sees every vertex in front of it;
 *     4. x = ax*u + bx;  y = ay*v + by;  inside iff -0.5 <= x <= Wi - 0.5 and -0.5 <= y <= Hi - 0.5 (the border that
 *        SquarePad adds around the image is outside);
 *     5. x0 = floor(x), wx = x - x0, columns clamp(x0, 0, Wi-1) and clamp(x0 + 1, 0, Wi-1); rows likewise from y0, wy;
 *        per channel, p{column}{row} the four pixels: top = p00 + wx*(p10 - p00); bot = p01 + wx*(p11 - p01);
 *        val = top + wy*(bot - top); the colour is (uint8)rint(val), half to even;
 *     6. colors (V, 3) uint8 = that colour and state (V) uint8 = 1 when 2, 3 and 4 hold; else colors = fill, state = 0.
 *     V == 0 is a no-op.  H, W, Hi, Wi outside [1, 32768]: SVR_E_BADSHAPE.
 *   svr_vertex_color_spread: vertices the camera does not see take colour along mesh edges.  One pass goes over every face
 *     (i0, i1, i2) and each of its six ordered corner pairs (s, d): if state[s] != 0 and state[d] == 0 AT THE START OF THE
 *     PASS, colors[s] is added per channel into sum[d] and 1 into count[d] (uint32 both; an edge shared by two faces counts
 *     twice).  After the pass every vertex with count > 0 gets colors = (2*sum + count) / (2*count) per channel, in integer
 *     division (the mean, rounded half up), and state = 2.  Passes repeat until one changes nothing or until max_passes
 *     (negative: no limit; V passes always suffice).  Vertices never reached -- components without a seen vertex, vertices
 *     of no face -- keep their colour and state 0.  A face with an index outside [0, V) is ignored.  The sums are integers,
 *     so the order in which the atomics arrive cannot change a bit: the result is the same on every run.
 *     faces: (F, 3) int32 on the device; colors / state: svr_vertex_color_sample's outputs, updated in place; ws:
 *     svr_vertex_color_workspace_bytes(V) device bytes (negative = SVR_E_BADSHAPE: V outside [0, 2^31)), need not be
 *     zeroed.  The host reads a device counter of changed vertices back after every check_every (>= 1) passes and stops when
 *     it has not moved; passes past the fixed point change nothing, so the result does not depend on check_every.  *passes
 *     (HOST, optional): the passes launched: whole intervals up to and including the first in which nothing changed, never
 *     more than max_passes or V + 1.  The call synchronises the stream.
 * ------------------------------------------------------------------------------------- */
int64_t svr_vertex_color_workspace_bytes(int64_t V);
int svr_vertex_color_sample(const float *verts, int64_t V, const float *consts /*[12]*/, const float *depth, int32_t H, int32_t W,
                            double bias, const uint8_t *image, int32_t Hi, int32_t Wi, const double *map /*[4]*/,
                            const uint8_t *fill /*[3]*/, uint8_t *colors, uint8_t *state, void *stream);
int svr_vertex_color_spread(const int32_t *faces, int64_t F, int64_t V, uint8_t *colors, uint8_t *state, void *ws, int64_t ws_bytes,
                            int64_t max_passes, int32_t check_every, int64_t *passes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Connected components of a mesh, their statistics, and the filter that keeps some of them (no reference op: the reference
 * writes raw marching-cubes output, floaters included; util/mesh_clean.py drives this, tests/mesh_components_oracle.py restates
 * it in numpy).  Errors, ownership and streams as for svr_mc_*.  No float operation takes part: every
 * output is the same bits on every run, whichever way the atomics arrive.
 *   verts: (V, 3) float32, faces: (F, 3) int32, on the device, 0 <= V, F < 2^31 (else SVR_E_BADSHAPE).
 *   The rule:
 *     1. a face is VALID iff its three indices lie in [0, V).  An invalid face joins nothing; its face label is -1.  A face
 *        that repeats an index ((a, a, b), (a, a, a)) is valid and joins what it names; duplicate faces change nothing.
 *     2. two vertices are in one COMPONENT iff a chain of valid faces connects them; a vertex of no valid face is a
 *        component of its own, with 0 faces.
 *     3. a component's ROOT is its smallest vertex index; components are numbered 0 .. C-1 in ascending order of root.
 *        vertex_label[i] = the number of i's component; face_label[f] = vertex_label[first index of f], -1 when f is invalid.
 *     4. per component, int32: root; vertex_count; face_count = its valid faces; marked_count = its vertices with
 *        mark[i] != 0 (mark: (V) uint8, NULL = all 0).
 *     5. per component, float32 x 3: bbox_min = fmin, bbox_max = fmax over its vertices' coordinates, per axis: a NaN
 *        coordinate is skipped, +-inf take part, an axis without a non-NaN value holds +inf / -inf.  Computed as the unsigned
 *        minimum / maximum of key(bits) = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000), whose order is the floats' (so of
 *        -0.0 and +0.0 the minimum is -0.0 and the maximum +0.0: compare the box by value), and decoded.
 *     6. FILTER, given keep[c] (uint8, nonzero = keep) per component: a face is kept iff it is valid and keep[its label];
 *        a vertex is kept iff keep[its label] and it lies in at least one valid face.  Kept vertices and kept faces keep
 *        their relative order; out_faces holds the new indices; vertex_index[j] = the old index of kept vertex j, so any
 *        per-vertex attribute follows as attr[vertex_index]; out_verts[j] = the three words of verts[vertex_index[j]], copied.
 *     7. SELECTION is the host's, over the C rows read back once (util/mesh_clean.py select_components; no entry point
 *        here): a component is kept iff face_count >= max(1, min_faces) and extent >= min_extent and, if require_mark,
 *        marked_count >= 1; with keep_largest only the one with the most faces among those, the lowest label on a tie.
 *        extent = sqrt(sum over the axes of (max - min)^2) in float64 from the float32 box; an axis with max <= min (one
 *        value, or none: +inf / -inf) adds 0.  Keeping nothing is an empty mesh, not an error.
 *        Face area is deliberately no statistic: a float sum per component would depend on the order of arrival.
 *   ws: svr_mesh_components_workspace_bytes(V, F) device bytes (negative = SVR_E_BADSHAPE); one buffer serves the three
 *   stages in turn, needs no zeroing, and must be the same, untouched, between svr_mesh_filter_count and svr_mesh_filter_emit.
 *   svr_mesh_components_label: vertex_label (V), face_label (F) int32; *count (DEVICE int64) = C.  V == 0: C = 0 and every
 *     face label is -1; F == 0: C = V, vertex_label[i] = i.  Lock-free union-find, then one scan: no host synchronisation.
 *   svr_mesh_components_stats: C = what the label call counted; the six outputs hold C rows.  C == 0 is a no-op.  A label
 *     outside [0, C) adds nothing.  uniform_path: nonzero lets a wave whose vertices (faces) share one label fold its values
 *     before it issues atomics; 0 issues them per lane.  The outputs are the same bits either way.
 *   svr_mesh_filter_count: totals (DEVICE int64 x 2) = kept vertices, kept faces; V == 0 or F == 0: both 0.
 *   svr_mesh_filter_emit: out_verts (V', 3), out_faces (F', 3), vertex_index (V') as the totals size them; call it only
 *     when they are not 0.
 * ------------------------------------------------------------------------------------- */
int64_t svr_mesh_components_workspace_bytes(int64_t V, int64_t F);
int svr_mesh_components_label(const int32_t *faces, int64_t F, int64_t V, void *ws, int64_t ws_bytes, int32_t *vertex_label,
                              int32_t *face_label, int64_t *count, void *stream);
int svr_mesh_components_stats(const float *verts, int64_t V, const int32_t *vertex_label, const int32_t *face_label, int64_t F,
                              const uint8_t *mark, int64_t C, void *ws, int64_t ws_bytes, int32_t *root, int32_t *vertex_count,
                              int32_t *face_count, int32_t *marked_count, float *bbox_min, float *bbox_max, int32_t uniform_path,
                              void *stream);
int svr_mesh_filter_count(const int32_t *faces, int64_t F, int64_t V, const int32_t *vertex_label, const uint8_t *keep, int64_t C,
                          void *ws, int64_t ws_bytes, int64_t *totals, void *stream);
int svr_mesh_filter_emit(const float *verts, int64_t V, const int32_t *faces, int64_t F, void *ws, int64_t ws_bytes, float *out_verts,
                         int32_t *out_faces, int32_t *vertex_index, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mesh simplification by vertex clustering, Rossignac-Borrel (no reference op: the reference writes raw marching-cubes output,
 * every triangle smaller than a lattice cell; util/mesh_simplify.py drives this, tests/mesh_simplify_oracle.py restates it in
 * numpy).  Errors, ownership and streams as for svr_mc_*.  Wherever threads meet the values are integers
 * (cells, vertex indices, int64 fixed-point sums), so every output is the same bits on every run, whichever way the atomics
 * arrive.  The unit is built with -ffp-contract=off.
 *   verts: (V, 3) float32, faces: (F, 3) int32, on the device, 0 <= V, F < 2^31 (else SVR_E_BADSHAPE).
 *   cell: the cluster edge, a float32, finite with 2^-10 <= cell <= 2^16 (else SVR_E_BADARG, and nothing is launched).
 *   The rule:
 *     1. a vertex is CLUSTERABLE iff its three coordinates are finite and each |v_a| < 2^16.  The others belong to no cluster
 *        and are counted (`bad`).
 *     2. its CELL is q_a = floor((double)v_a / (double)cell), computed in float64; |q_a| < 2^27 by the limits, an int32.  Two
 *        clusterable vertices are in one CLUSTER iff their (q_x, q_y, q_z) are equal.
 *     3. a cluster's ROOT is its smallest member vertex index; clusters are numbered in ascending order of root.
 *     4. POSITION: s_a(i) = (int64) rint((double)v_a * 65536), ties to even (the product is exact); S_a = the int64 sum over
 *        the members and n = their number (|S_a| < 2^63 by the limits); the cluster's vertex is
 *        (float)(((double)S_a / (double)n) / 65536.0).  A cluster with n == 1 keeps the three words of its one vertex, copied:
 *        a cell no larger than the vertex spacing is the identity on positions, bit for bit.
 *     5. a face is VALID iff its three indices lie in [0, V) and name clusterable vertices (the indices are compared before
 *        any of them addresses memory); its MAPPED triple is the three cluster numbers; it is DEGENERATE iff two of them are
 *        equal.
 *     6. the CANONICAL triple is the mapped triple rotated so that its smallest number comes first (a rotation keeps the
 *        orientation).  Two non-degenerate faces are DUPLICATES iff their canonical triples are equal; of a set of duplicates
 *        only the face with the smallest index is kept.  (A, B, C) and (A, C, B) are no duplicates: both stay, a two-sided sheet.
 *     7. OUTPUT: a face is kept iff it is valid, not degenerate and the first of its duplicates; a cluster is kept iff a kept
 *        face names it.  Kept clusters keep their relative order and are renumbered 0 .. V'-1; kept faces keep their relative
 *        order and their own rotation, with the new numbers.  vertex_cluster[i] (V, int32) = the output vertex of i's cluster,
 *        -1 if i is not clusterable or its cluster was dropped; cluster_size[j] (V', int32) = n.  Any per-vertex attribute can
 *        be pooled by the caller over vertex_cluster.
 *   Consequences: every member moves by less than `cell` per axis (its cluster's vertex lies in the closed hull of the cell's
 *   members), plus the fixed-point step (2^-17 per member, so at most that for the mean) and half a float32 ulp of the result.
 *   A closed input can lose manifoldness where a feature is thinner than a cell (two sheets collapse into a two-sided sheet or
 *   an edge shared by four faces): simplification trades topology for size, and nothing here repairs it.
 *   ws: svr_mesh_simplify_workspace_bytes(V, F) device bytes (negative = SVR_E_BADSHAPE); needs no zeroing, and must be the
 *   same buffer, untouched, between svr_mesh_simplify_count and svr_mesh_simplify_emit.
 *   svr_mesh_simplify_count: totals (DEVICE int64 x 3) = V', F', bad.  V == 0 or F == 0: (0, 0, bad), ws may be null.
 *     uniform_path: nonzero lets a wave whose vertices share one cluster fold its sums before it issues atomics; 0 issues them
 *     per lane.  The outputs are the same bits either way.  Reading the totals is the caller's one host synchronisation.  The
 *     call is asynchronous, so the one failure it can only meet on the device -- a hash set without an empty slot, which a
 *     half-empty table rules out -- arrives in the totals: all three hold SVR_E_INTERNAL, and no kernel has left its buffers.
 *   svr_mesh_simplify_emit: out_verts (V', 3), out_faces (F', 3), cluster_size (V') as the totals size them (not touched, and
 *     may be null, when the totals are 0), vertex_cluster (V).  V == 0 or F == 0: only vertex_cluster is filled, with -1.
 * ------------------------------------------------------------------------------------- */
int64_t svr_mesh_simplify_workspace_bytes(int64_t V, int64_t F);
int svr_mesh_simplify_count(const float *verts, int64_t V, const int32_t *faces, int64_t F, float cell, void *ws, int64_t ws_bytes,
                            int32_t uniform_path, int64_t *totals, void *stream);
int svr_mesh_simplify_emit(const float *verts, int64_t V, const int32_t *faces, int64_t F, void *ws, int64_t ws_bytes, float *out_verts,
                           int32_t *out_faces, int32_t *vertex_cluster, int32_t *cluster_size, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mesh smoothing, Taubin's lambda|mu iteration by an all-integer rule (no reference op: the reference writes raw marching-cubes
 * output, terraced where the network's field is near-binary; util/mesh_smooth.py drives this, tests/mesh_smooth_oracle.py
 * restates it in numpy).  Errors, ownership and streams as for svr_mc_*.  The iteration is all integers,
 * so every output bit is independent of the order of atomics and of FP contraction; the only floating-point operations are
 * the two conversions at either end.  The unit is built with -ffp-contract=off.
 *   verts: (V, 3) float32, faces: (F, 3) int32, on the device, 0 <= V < 2^31, 0 <= F <= 2^28 (else SVR_E_BADSHAPE).
 *   iterations: 0 <= n <= 1024.  lam, mu: float32 with 0 < lam <= 1 and -1 <= mu <= 0 after the rounding of point 1; mu = 0
 *   is plain Laplacian smoothing, one pass per iteration.  fix_boundary: nonzero keeps the vertices of point 5 in place.
 *   Anything else is SVR_E_BADARG, and so are out_verts overlapping verts (a pass reads every old position) and a workspace
 *   that is too small; every refusal happens before anything is enqueued.
 *   The rule:
 *     1. the step weights are fixed point: L_lam = rint((double)lam * 65536) and L_mu = rint((double)mu * 65536), integers,
 *        with 1 <= L_lam <= 65536 and -65536 <= L_mu <= 0.
 *     2. a vertex is USABLE iff its three coordinates are finite and each |v_a| < 2^16 (svr_mesh_simplify's "clusterable").
 *     3. a face is VALID iff its three indices lie in [0, V), are pairwise distinct, and name usable vertices (the indices are
 *        compared before any of them addresses memory).  Repeated valid faces each count.
 *     4. every valid face (a, b, c) gives a the ENTRY (next b, prev c), b the entry (c, a) and c the entry (a, b); m_i is the
 *        number of entries of vertex i.
 *     5. i is INTERIOR iff for every j the number of its entries with next = j equals the number with prev = j (equality of
 *        multisets, exact): every edge that leaves i on one face comes back on another.
 *     6. STATE (uint8), the first that applies: 3 = not usable; 1 = m_i is 0; 2 = fix_boundary is set and i is not interior;
 *        0 = movable.
 *     7. every usable vertex gets q_a = (int64) rint((double)v_a * 65536) per axis, ties to even (the product is exact).
 *     8. n times: one Jacobi pass with L = L_lam, then one with L = L_mu (omitted when L_mu = 0).  A pass reads the old q of
 *        every vertex and gives each movable vertex i, per axis,
 *          S = the sum over i's entries of (q[next] + q[prev]),  c = 2 m_i,
 *          mean = floor((S + m_i) / c)            -- floor division; S + m_i can be negative,
 *          step = (L * (mean - q) + 32768) >> 16  -- an arithmetic shift (floor),
 *          q' = clamp(q + step, -2^33, 2^33).
 *        The other vertices keep q.  |S + m_i| <= 2^29 * 2^33 + 2^28 < 2^63 and |L * (mean - q)| < 2^52.
 *     9. OUTPUT: a movable vertex, when n > 0, becomes (float)((double)q_a / 65536.0); every other vertex keeps its three
 *        input words, NaN payloads included; n = 0 is the identity, bit for bit.  Faces are not touched.  state (V, uint8) as
 *        in 6; counts (DEVICE int64 x 4) = the number of vertices in states 0, 1, 2, 3.
 *   Consequences: a negative mu extrapolates, so a coordinate can leave +-2^16 although every input lies inside; the clamp
 *   keeps the sums inside int64, so an output can be as large as +-131072.0 (= 2^33 / 2^16), and never larger.  On a closed
 *   manifold every vertex is interior; where the lattice border cuts a surface open, the rim is what fix_boundary holds.
 *   ws: svr_mesh_smooth_workspace_bytes(V, F) device bytes (negative = SVR_E_BADSHAPE); needs no zeroing.
 *   svr_mesh_smooth is asynchronous and synchronises nothing with the host: the output sizes are known.  V == 0: only
 *   counts is written.  F == 0: out_verts is a copy, every state is 1 or 3, ws may be null.
 * ------------------------------------------------------------------------------------- */
int64_t svr_mesh_smooth_workspace_bytes(int64_t V, int64_t F);
int svr_mesh_smooth(const float *verts, int64_t V, const int32_t *faces, int64_t F, int32_t iterations, float lam, float mu,
                    int32_t fix_boundary, void *ws, int64_t ws_bytes, float *out_verts, uint8_t *state, int64_t *counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * Shaded previews of a mesh: area-weighted vertex normals, a shading pass over the ray caster's face map, and the box
 * filter behind supersampling (no reference op: the reference shows pictures of its meshes but ships no code for them;
 * util/mesh_render.py drives this, tests/mesh_render_oracle.py restates it in numpy).  Errors,
 * ownership and streams as for svr_mc_*.  Both units are built with -ffp-contract=off: one rounding per float64 operation.
 *
 * svr_mesh_vertex_normals.  verts: (V, 3) float32, faces: (F, 3) int32, on the device, 0 <= V < 2^31, 0 <= F <= 2^28 (else
 * SVR_E_BADSHAPE).  The rule is all-integer up to the final normalisation, so no output bit depends on the order of atomics:
 *     1. a vertex is USABLE iff its three coordinates are finite and each |v_a| < 2^16 (svr_mesh_smooth's rule).
 *     2. a face is VALID iff its three indices lie in [0, V), are pairwise distinct, and name usable vertices (the indices are
 *        compared before any of them addresses memory).  Repeated valid faces each count.
 *     3. q_a = (int64) rint((double)v_a * 1024), ties to even (the product is exact), so |q_a| <= 2^26.
 *     4. per valid face (a, b, c): e1 = q_b - q_a, e2 = q_c - q_a, n = e1 x e2 component by component in int64,
 *        (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x), each |n_a| <= 2^55; n is added to the accumulators of a, of b
 *        and of c.  The sums are taken modulo 2^64 (two's complement wrap), so they are defined, and equal to numpy's int64,
 *        even where they overflow; below 256 faces per vertex no overflow is possible.
 *     5. per vertex: x, y, z = (double) of the three sums (read as signed); len = sqrt((x*x + y*y) + z*z); if len > 0 the
 *        normal is ((float)(x / len), (float)(y / len), (float)(z / len)), else (0, 0, 0).
 *     6. STATE (uint8), the first that applies: 3 = not usable; 1 = in no valid face, or a zero sum (len is not > 0);
 *        0 = has a normal.  counts (DEVICE int64 x 3) = the number of vertices in states 0, 1, 3, in this order.
 *   The direction follows the faces' winding (counter-clockwise seen from the side the normal points to); nothing is flipped.
 *   out: (V, 3) float32; state: (V,) uint8.  out overlapping verts and a workspace that is too small are SVR_E_BADARG; every
 *   refusal happens before anything is enqueued.  ws: svr_mesh_vertex_normals_workspace_bytes(V, F) device bytes (negative =
 *   SVR_E_BADSHAPE); needs no zeroing.  Asynchronous, no host synchronisation.  V == 0: only counts is written.  F == 0:
 *   every normal is 0, every state 1 or 3, ws may be null.
 *
 * svr_mesh_shade.  tri: the ray caster's (F, 9) float64 table; faces: (F, 3) int32 (may be null when normals and colors are);
 * face_map: the `face` output of svr_raycast_eval for the SAME tri, consts and image, (H, W) int32, negative = miss; consts:
 * the 12 float32 constants in HOST memory, widened first; normals: (V, 3) float32 or null; colors: (V, 3) uint8 or null;
 * albedo, background: 3 HOST uint8 each; ambient: float32 with 0 <= ambient <= 1 (else SVR_E_BADARG); rgb: (H, W, 3) uint8.
 * All of tri ... rgb but consts, albedo and background are on the device.  Per pixel (u = column, v = row), float64, one
 * rounding per operation, dot and cross as for svr_raycast_*:
 *     1. a miss, or a face index outside [0, F): rgb = background.
 *     2. d = the ray direction of svr_raycast_*; o = (t0, t1, t2); with a, b, c of the face, by the expressions of the pair test:
 *        e1 = b - a; e2 = c - a; p = d x e2; det = dot(e1, p); inv = 1 / det; s = o - a; bu = dot(s, p) * inv; q = s x e1;
 *        bv = dot(d, q) * inv; w0 = (1 - bu) - bv.  det == 0 cannot occur for a face the caster accepted; in a map from
 *        elsewhere such a pixel takes background.
 *     3. the shading normal: with normals and the face's three indices i0, i1, i2 in [0, V): N_a = (w0*n0_a + bu*n1_a) + bv*n2_a
 *        (the float32 normals widened), len = sqrt(dot(N, N)), and N / len per component when len > 0.  In every other case (no
 *        normals, len not > 0 -- NaN included --, an index outside [0, V)): the face's unit normal turned against the ray, as
 *        svr_raycast_eval's `normal` computes it (m = (e1 x e2) / |e1 x e2|, negated when dot(m, d) > 0).
 *     4. c = |dot(N, d)| / sqrt(dot(d, d)): the light is at the camera and the surface is two-sided, so it is never black from
 *        behind;  I = a + (1 - a) * c  with a = (double)ambient.
 *     5. the base colour per channel: with colors and the three indices in [0, V), (w0*c0 + bu*c1) + bv*c2 of the three
 *        vertices' bytes widened; else albedo.
 *     6. rgb = rint(base * I), half to even, clamped to [0, 255]; NaN gives 0.
 *   One thread per pixel, no LDS, no atomics; a face or vertex index outside its range never becomes an address.  F == 0: every
 *   pixel is background.
 *
 * svr_box_downsample_rgb8.  src (s*H, s*W, 3) uint8 -> dst (H, W, 3) uint8, s in {1, 2, 3, 4} (else SVR_E_BADARG), on the
 * device, not overlapping: per channel (sum of the s x s block + s*s/2) / (s*s) in integers -- the mean rounded half up.
 * Supersampling: the fine image is rendered with f' = s*f, cx' = s*cx + (s - 1)/2, cy' = s*cy + (s - 1)/2, computed in float64
 * on the host from the float32 constants and rounded to float32 (the other nine unchanged).  Fine pixel s*u + i then sees the
 * direction of coarse position u + (i - (s - 1)/2) / s: sub-pixel i lies at offset (i - (s - 1)/2) / s from the pixel centre,
 * the s x s sub-pixels tile the pixel evenly.
 * ------------------------------------------------------------------------------------- */
int64_t svr_mesh_vertex_normals_workspace_bytes(int64_t V, int64_t F);
int svr_mesh_vertex_normals(const float *verts, int64_t V, const int32_t *faces, int64_t F, void *ws, int64_t ws_bytes, float *out,
                            uint8_t *state, int64_t *counts, void *stream);
int svr_mesh_shade(const double *tri, const int32_t *faces, int64_t F, int64_t V, const int32_t *face_map, const float *consts /*[12]*/,
                   int32_t H, int32_t W, const float *normals, const uint8_t *colors, const uint8_t *albedo /*[3]*/,
                   const uint8_t *background /*[3]*/, float ambient, uint8_t *rgb, void *stream);
int svr_box_downsample_rgb8(const uint8_t *src, int32_t H, int32_t W, int32_t s, uint8_t *dst, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sample wire formats (replaces the Python loaders of dataset/implicit_dataset.py:24-56,
 * data_processing/volume_reader.py:36-45 and the np.load calls on process_sample.py:19-30's outputs).
 * The files are read on the host (svr_df_* / svr_npz_*: File formats, below).
 * Device side: x-fastest -> C-order transpose of a .df payload, casts to float32, and the random row subset of
 * implicit_dataset.py:40-43 as a gather with cast (idx: device int64; rows outside [0, n_rows) set *bad_flag).
 * ------------------------------------------------------------------------------------- */
#define SVR_DT_F32 0
#define SVR_DT_F64 1
#define SVR_DT_BOOL 2
#define SVR_DT_U8 3
#define SVR_DT_I32 4
#define SVR_DT_I64 5
int svr_df_to_grid(const float *payload, float *out /*(X,Y,Z) C order*/, int32_t X, int32_t Y, int32_t Z, void *stream);
int svr_cast_to_f32(const void *in, int32_t dtype, float *out, int64_t n, void *stream);
int svr_subsample_rows(const void *rows, int32_t dtype, int64_t n_rows, int32_t cols, const int64_t *idx, int64_t n_idx,
                       float *out, int32_t *bad_flag, void *stream);
/* svr_subsample_rows_batched: the row subsets of a whole collated batch in one launch.  `segments` (DEVICE, n_segments
 *   entries) describes one (item, sigma, array) each: out[out_offset + i * cols + c] = (float)rows[idx[idx_offset + i] * cols + c]
 *   for i < n_idx, c < cols; dtype is SVR_DT_F32 / F64 / BOOL / U8 as in svr_subsample_rows, a row outside [0, n_rows)
 *   writes 0 and sets *bad_flag (may be NULL).  `elem_prefix` (DEVICE, n_segments + 1 int64): elem_prefix[0] = 0,
 *   elem_prefix[s + 1] = elem_prefix[s] + n_idx[s] * cols[s]; `total` = elem_prefix[n_segments] (the HOST's copy: it sizes the
 *   launch).  `idx` is the shared int64 index buffer, `out` the shared float32 output; the caller guarantees that every
 *   segment's index and output range lies inside them and that output ranges do not overlap.  The struct is six 8-byte
 *   words, so table, prefix and indices can travel in ONE int64 host buffer and one copy.  n_segments <= 0 or total <= 0:
 *   no-op. */
typedef struct svr_row_segment {
  const void *rows;
  int64_t n_rows;
  int64_t idx_offset;
  int64_t n_idx;
  int64_t out_offset;
  int32_t dtype;
  int32_t cols;
} svr_row_segment;
int svr_subsample_rows_batched(const svr_row_segment *segments, const int64_t *elem_prefix, int32_t n_segments, int64_t total,
                               const int64_t *idx, float *out, int32_t *bad_flag, void *stream);

/* ---------------------------------------------------------------------------------------
 * Raw views (data_processing/distance_to_depth.py, process_sample.py:17-21, dataset/scene_net_data.py:77-84).  The .exr
 * files are read on the host (svr_exr_*: File formats, below).
 *
 * Device side (raw_sample.hip):
 *   svr_distance_to_depth: depth = sqrt(d*d / ((r*r + c*c) / (f*f) + 1)) over (B, H, W), r = row - H/2, c = col - W/2
 *     (integer division; the reference centres on these integers, not on cx / cy).  r*r + c*c is an integer converted to
 *     float32; every float32 operation is rounded on its own, in this order; the square root is correctly rounded.
 *   svr_depth_grid_mark: one (H, W) map, a distance map (is_distance = 1: the rule above with `focal` first) or a depth
 *     map -> the un-normalised grid-space coordinate of svr_unproject_fwd (same device function, same 12 consts) ->
 *     round half to even -> grid[i0][i1][i2] = 1 (grid: D0*D1*D2 uint8, zeroed by the caller; plain stores of 1).
 *     A pixel whose rounded index leaves [0, D) on any axis (NaN / inf included; indices in [-D, 0) are NOT wrapped) is
 *     not written and adds 1 to *out_of_range (device int32, zeroed by the caller).  coords (optional): (H*W, 3) float32.
 * ------------------------------------------------------------------------------------- */
int svr_distance_to_depth(const float *distance, float *depth, int32_t B, int32_t H, int32_t W, float focal, void *stream);
int svr_depth_grid_mark(const float *map, int32_t is_distance, float focal, int32_t H, int32_t W, const float *consts /*[12]*/,
                        uint8_t *grid, int32_t D0, int32_t D1, int32_t D2, int32_t *out_of_range, float *coords, void *stream);

/* ---------------------------------------------------------------------------------------
 * Stage visualisation of the scene trainer (replaces util/visualize.py:10-20,28-49: to_point_list + trimesh's multibox,
 * numpy + PIL + pyexr; called by trainer/trainer_scene_net.py:170-188).  Errors, ownership and streams as for svr_mc_*.
 *
 * Voxel-box mesher.  field: (X, Y, Z) float32, C order, on the device; output: the welded boundary surface of the union
 * of unit cubes centred on the occupied indices, in the field's index space (x along axis 0, as marching cubes).
 *   - voxel (i, j, k) is occupied iff (double)v >= threshold (NaN: not occupied) and is the cube [i-1/2, i+1/2] x
 *     [j-1/2, j+1/2] x [k-1/2, k+1/2]; a cube face is emitted iff the voxel across it is unoccupied or outside the lattice
 *     (multibox's triangle set minus the faces shared by two boxes);
 *   - vertices: points (a, b, c) of the (X+1)(Y+1)(Z+1) corner lattice at (a-1/2, b-1/2, c-1/2); a corner is emitted once
 *     iff an emitted face touches it (the 8 voxels around it, outside = empty, are neither all empty nor all occupied);
 *     ordered by the corner's C-order index;
 *   - faces: by voxel (C order), then direction -x, +x, -y, +y, -z, +z; each a quad q0 q1 q2 q3, counter-clockwise from
 *     outside, as the triangles (q0, q1, q2), (q0, q2, q3); corner offsets (x y z) from the voxel's minimum corner:
 *       -x: 000 001 011 010   +x: 100 110 111 101   -y: 000 100 101 001
 *       +y: 010 011 111 110   -z: 000 010 110 100   +z: 001 101 111 011
 *   svr_voxel_mesh_workspace_bytes: device workspace (negative = SVR_E_BADSHAPE: a corner lattice of 2^31 points or more).
 *   svr_voxel_mesh_count: classify + scan; writes the device int64 totals[2] = {V, F} (F triangles).  The caller reads
 *                  them back, checks V, F < 2^31 and allocates verts (V, 3) float32 and faces (F, 3) int32.
 *   svr_voxel_mesh_emit: fills verts / faces from the same workspace (after svr_voxel_mesh_count on the stream).  An
 *                  extent of 0 gives an empty mesh.
 *
 * Depth-map image planes (map: (H, W) float32 on the device):
 *   svr_depth_minmax: stats[4] (device uint32; [0] = ~key(min), [1] = key(max), [2] = 1 if any value is NaN / inf (such
 *     values take no part in min / max), [3] unused; key(v) = the float's bits with the sign bit set for v >= 0 and all
 *     bits flipped for v < 0, whose unsigned order is the floats' order).
 *   svr_depth_planes: plane_f32[r][c] = d = map[r][flip ? W-1-c : c]; plane_u8[r][c] = (uint8)(255.0f / max * (d - min)):
 *     float32 division, subtraction and product, each rounded on its own, then truncation toward zero (a value past 255
 *     keeps its low 8 bits).  min / max are read from `stats` on the device.
 * ------------------------------------------------------------------------------------- */
int64_t svr_voxel_mesh_workspace_bytes(int32_t X, int32_t Y, int32_t Z);
int svr_voxel_mesh_count(const float *field, int32_t X, int32_t Y, int32_t Z, double threshold, void *ws, int64_t ws_bytes,
                         int64_t *totals, void *stream);
int svr_voxel_mesh_emit(const float *field, int32_t X, int32_t Y, int32_t Z, double threshold, void *ws, float *verts,
                        int32_t *faces, void *stream);
int svr_depth_minmax(const float *map, int64_t n, uint32_t *stats /*[4]*/, void *stream);
int svr_depth_planes(const float *map, int32_t H, int32_t W, int32_t flip, const uint32_t *stats, float *plane_f32,
                     uint8_t *plane_u8, void *stream);

/* ---------------------------------------------------------------------------------------
 * Depth head of the UNet regressor (replaces trainer/trainer_unet.py:43-61: F.interpolate(size=S, bilinear) -> crop of
 * rows r0:r1 -> sigmoid -> renormalise -> F.mse_loss, and their autograd).  raw: (B, 1, Hs, Ws) float32, contiguous.
 *   S > 0 : y = F.interpolate(raw, size=S, mode='bilinear', align_corners=False)[:, :, r0:r1, :], (B, 1, r1-r0, S).  Per
 *           axis, in float32, every operation rounded on its own:  scale = (float)in / (float)S;
 *           src = max(scale * (dst + 0.5f) - 0.5f, 0);  i0 = (int)src;  i1 = i0 + (i0 < in-1);  l1 = src - i0;  l0 = 1 - l1;
 *           y = l0y*(l0x*a00 + l1x*a01) + l1y*(l0x*a10 + l1x*a11).  Rows outside r0:r1 are never computed.
 *   S == 0: y = raw (r0, r1 ignored), output (B, 1, Hs, Ws).
 *   depth = min(sigmoid(y) * (float)(max_z - min_z) + (float)min_z, (float)max_z)      (the bound only takes back a last
 *           rounding past max_z).
 * svr_depth_head_fwd: writes depth.  target (may be NULL; depth's shape): loss[0] = mean((depth - target)^2), summed in
 *   float64: one partial per block in `workspace` (svr_depth_head_workspace(B, Ho, Wo) bytes, Ho x Wo the output's plane;
 *   it need not be zeroed), added in a fixed order.  gdst (may be NULL; needs target; depth's shape) receives
 *   d loss / d y = 2/n * (depth - target) * (max_z - min_z) * s * (1 - s); with S == 0 that is d loss / d raw.
 * svr_depth_head_bwd (S > 0): draw (B, 1, Hs, Ws) = the transposed interpolation of gdst, in gather form: every source
 *   pixel sums, in a fixed order, the cropped destination pixels whose taps touch it (found with the forward's own index
 *   function).  No atomics: the same bits on every run; a source pixel that no cropped destination pixel touches gets
 *   an exact 0.  draw is overwritten (it need not be zeroed).
 * At most three launches for a training step (forward, loss sum, backward); no synchronisation, no allocation.
 * ------------------------------------------------------------------------------------- */
int64_t svr_depth_head_workspace(int32_t B, int32_t Ho, int32_t Wo);
int svr_depth_head_fwd(const float *raw, const float *target, float *depth, float *loss, float *gdst, int32_t B, int32_t Hs,
                       int32_t Ws, int32_t S, int32_t r0, int32_t r1, double min_z, double max_z, void *workspace,
                       void *stream);
int svr_depth_head_bwd(const float *gdst, float *draw, int32_t B, int32_t Hs, int32_t Ws, int32_t S, int32_t r0, int32_t r1,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * RGB preprocessing of the scene network's input (replaces the torchvision chain of dataset/scene_net_data.py:30-38 on a
 * PIL image: SquarePad -> Resize((W, W)) -> ToTensor -> Normalize(0.5, 0.5), and the FLIP_LEFT_RIGHT of
 * dataset/scenes_dataset.py in front of it), bit for bit what Pillow's 8-bit BILINEAR resize gives.
 *
 * Per axis with input size `in` and output size `out` (all in double, every operation rounded on its own):
 *   scale = in / out;  fs = max(scale, 1);  support = 1.0 * fs;  ss = 1 / fs
 *   for xx in 0..out-1:  center = (xx + 0.5) * scale
 *     xmin = max(0, (int)(center - support + 0.5));  xmax = min(in, (int)(center + support + 0.5))
 *     w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|)  for x in 0..xmax-xmin-1;   w[x] /= sum(w)
 *     k[x] = (int)(w[x] * 2^22 + 0.5)
 *   out[xx] = clamp((2^21 + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)     per band, int32
 * Host only:
 *   svr_rgb_resize_taps: the largest tap count of (in, out), (int)ceil(support) * 2 + 1 (3 when out >= in, 7 for 640 -> 256).
 *   svr_rgb_resize_table: table (out, K + 2) int32 in HOST memory, row xx = {xmin, xmax - xmin, k[0..K-1]} (unused taps 0);
 *     K >= svr_rgb_resize_taps(in, out).  The caller uploads it; a table depends on (in, out, K) alone.
 * svr_rgb_preprocess: src (B, H, W, C) uint8, C 1 or 3.
 *   Wout > 0: the image (columns mirrored first when `flip`) is padded with hp = (max(H, W) - W) / 2 zero columns and
 *     vp = (max(H, W) - H) / 2 zero rows on BOTH sides (integer division: an odd difference leaves Hp = H + 2 vp and
 *     Wp = W + 2 hp different, 5 x 8 -> 7 x 8) and resized to Wout x Wout: columns first with table_x = the table of
 *     (Wp, Wout) into tmp (B, Hp, Wout, C) uint8, then rows with table_y = the table of (Hp, Wout).  A pass whose sizes
 *     agree is skipped and needs no table; tmp is needed only when both run.  Kx / Ky: the K of each table.  The padded
 *     zeros take part in the filter; no padded image is stored.
 *   Wout == 0: no pad and no resize, the output is H x W (flip still applies).
 *   out_u8 (B, Ho, Wo, C) uint8 and out_f32 (B, C, Ho, Wo) float32 = norm[byte]; either may be NULL, not both.  norm: 256
 *     floats in device memory, the value of every byte: filled by the caller with the operations to reproduce
 *     (u / 255, then (x - 0.5) / 0.5, in float32).
 *   One or two launches.  Source reads outside the image give 0 and a row's count is capped at K, whatever the tables hold.
 * svr_grid_to_camera: dst[i][a] = (src[i][a] - t_a) / s_a for (n, 3) float32 points, scale_shift = {s0, t0, s1, t1, s2, t2} in
 *   host memory: the inverse of the camera -> grid affine  g = s * c + t  of svr_unproject_fwd (consts[3..8]); dst may be src.
 * ------------------------------------------------------------------------------------- */
int32_t svr_rgb_resize_taps(int32_t in, int32_t out);
int svr_rgb_resize_table(int32_t in, int32_t out, int32_t K, int32_t *table);
int svr_rgb_preprocess(const uint8_t *src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Wout, int32_t flip,
                       const int32_t *table_x, int32_t Kx, const int32_t *table_y, int32_t Ky, const float *norm, uint8_t *tmp,
                       uint8_t *out_u8, float *out_f32, void *stream);
int svr_grid_to_camera(const float *src, float *dst, int64_t n, const float *scale_shift, void *stream);

/* ---------------------------------------------------------------------------------------
 * File formats (csrc/io_*.cpp, plain C++ + zlib): the readers and writers of the files the project shares with the
 * reference's tools.  One contract for every entry point of this section: HOST pointers only (pinned memory is fine), no
 * stream, no GPU needed -- nothing of ROCm is called and the files build with any C++17 compiler; the return value is 0
 * or a negative SVR_E_* code with its text in svr_last_error() (thread local); no C++ exception crosses the ABI, and a
 * malformed file is an error code, never a read outside the file's bytes or the caller's buffers.
 *
 * Meshes and images, written (svr_mc_*, svr_voxel_mesh_*, svr_vertex_color_*, svr_depth_planes make the arrays):
 *   svr_write_obj: host only; verts (nv, 3) float32 and faces (nf, 3) int32 HOST arrays -> `v x y z` lines (%.9g,
 *                  float32 round trip) then `f a b c` lines (1-based).  SVR_E_IO on a failed open / write.
 *   svr_write_obj_normals: the same with normals (nv, 3) float32, one per vertex: the `v` lines, then `vn x y z` lines
 *                  (%.9g), then `f a//a b//b c//c` lines (1-based; a vertex and its normal share the index).
 *   svr_write_ply: host only; verts (nv, 3) float32, colors (nv, 3) uint8 and faces (nf, 3) int32 HOST arrays -> a binary
 *     little-endian PLY: the header below (LF line ends, the two counts in decimal), then per vertex 12 + 3 bytes (x, y, z,
 *     red, green, blue), then per face 1 + 12 bytes (the count 3, three indices, 0-based).  SVR_E_IO on a failed open / write.
 *       ply
 *       format binary_little_endian 1.0
 *       element vertex <nv>
 *       property float x
 *       property float y
 *       property float z
 *       property uchar red
 *       property uchar green
 *       property uchar blue
 *       element face <nf>
 *       property list uchar int vertex_indices
 *       end_header
 *   svr_write_png_gray8: data (H, W) uint8 -> a PNG file: signature, IHDR (bit depth 8, colour type 0, no interlace), one
 *     zlib-deflated IDAT with filter type 0 on every scanline, IEND, CRC-32 on every chunk.
 *   svr_write_png_rgb8: data (H, W, 3) uint8 -> the same format with colour type 2 (RGB), three bytes per pixel.
 *   svr_write_obj_points: pts (n, 3) float32 -> one line `v %f %f %f %f %f %f` per point: the coordinates + 0.5 (added in
 *     float32, then widened) and the colour 1 1 1 (visualize_point_list, util/visualize.py:14-20).  n == 0: an empty file.
 *
 * Samples (`out` / `payload` ideally pinned; dtype codes: SVR_DT_*, above):
 *   .df  = 3 x uint64 dims (X, Y, Z) + X*Y*Z float32, x fastest;
 *   .npz = zip of .npy members (stored by np.savez, deflated by np.savez_compressed; zip64 local headers).
 *
 * OpenEXR subset:
 *   read: single-part scanline files; compression NONE (0), ZIPS (2), ZIP (3); pixel types UINT (0), HALF (1),
 *   FLOAT (2); any channel count (the file's alphabetical order); lineOrder 0 / 1; any data-window origin; blocks stored
 *   raw because deflate did not shrink them.  Refused by name: tiled / multi-part / deep files, subsampled channels, every
 *   other compression.  A truncated file or an offset beyond it is SVR_E_IO, never a read outside the file's bytes.
 *   svr_exr_info: width, height, origin[2] = the data window's (x, y) minimum, the channel count, compression, lineOrder;
 *     names (optional) receives the channel names, each NUL terminated, back to back (names_bytes of room);
 *     pixel_types (optional) one code per channel; both need max_channels >= the channel count.
 *   svr_exr_read_channel: one channel as float32 (HALF widened, UINT converted), (H, W) row major, top scanline of the
 *     data window first, into `out` (host, n = W * H values; pinned memory is fine).  Unknown name: SVR_E_NOTFOUND.
 *   svr_exr_write: data = (n_channels, H, W) float32 planes in the order of `names` (NUL terminated, back to back) ->
 *     an uncompressed FLOAT scanline file, data window (0,0)-(W-1,H-1), channels sorted by name.
 * ------------------------------------------------------------------------------------- */
int svr_write_obj(const char *path, const float *verts, int64_t nv, const int32_t *faces, int64_t nf);
int svr_write_ply(const char *path, const float *verts, const uint8_t *colors, int64_t nv, const int32_t *faces, int64_t nf);
int svr_write_png_gray8(const char *path, const uint8_t *data, int32_t H, int32_t W);
int svr_write_png_rgb8(const char *path, const uint8_t *data, int32_t H, int32_t W);
int svr_write_obj_normals(const char *path, const float *verts, const float *normals, int64_t nv, const int32_t *faces, int64_t nf);
int svr_write_obj_points(const char *path, const float *pts, int64_t n);
int svr_df_dims(const char *path, int64_t *dims /*[3]*/);
int svr_df_read(const char *path, float *payload, int64_t n);
/* svr_df_write: host only; the inverse of svr_df_dims + svr_df_read: three little-endian uint64 extents, then the X*Y*Z
 *   float32 values of `payload` (HOST, x fastest).  SVR_E_IO on a failed open or write, SVR_E_BADARG for an extent outside [1, 2^20), the range
 *   svr_df_dims accepts. */
int svr_df_write(const char *path, const float *payload, int64_t X, int64_t Y, int64_t Z);
int svr_npz_member_info(const char *path, const char *member, int32_t *dtype, int32_t *ndim, int64_t *shape /*[8]*/,
                        int32_t *fortran_order);
int svr_npz_member_read(const char *path, const char *member, void *out, int64_t nbytes);
int svr_exr_info(const char *path, int32_t *width, int32_t *height, int32_t *origin /*[2]*/, int32_t *n_channels, char *names,
                 int64_t names_bytes, int32_t *pixel_types, int32_t max_channels, int32_t *compression, int32_t *line_order);
int svr_exr_read_channel(const char *path, const char *name, float *out, int64_t n);
int svr_exr_write(const char *path, const float *data, int32_t H, int32_t W, const char *names, int32_t n_channels);

#ifdef __cplusplus
}
#endif
#endif /* SVR_HIP_H */
