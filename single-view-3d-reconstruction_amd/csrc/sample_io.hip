// Sample wire formats of the reference's datasets, device side, gfx950.
//
// The reference loads every sample in Python (dataset/implicit_dataset.py:24-56): np.load of a zlib-compressed float64
// grid (depth_grid.npz, key 'grid', data_processing/process_sample.py:19-22), read_df (data_processing/
// volume_reader.py:36-45: 3 x uint64 dims + float32 payload, x fastest, unpacked one float at a time through
// struct.unpack into a tuple), and two occupancy_<sigma>.npz files (keys points / occupancies / grid_coords,
// process_sample.py:28-30) whose random subset is assembled through Python lists.  At ~22 ms per training step that
// loader is the next bottleneck.  The files are read on the host by io_df.cpp and io_npz.cpp into caller buffers
// (pinned memory); here is what follows on the device: the x-fastest -> C-order transpose of the .df payload, float64 ->
// float32 casts, and the per-sample random row subset (gather by index with cast: points float64 -> float32,
// occupancies bool -> float32).
// Given the same files and the same indices the tensors equal the reference's __getitem__ outputs bit for bit.
#include "common.h"

using namespace svr;

namespace {

__global__ __launch_bounds__(256) void df_to_grid_kernel(const float *__restrict__ payload, float *__restrict__ out, int X, int Y, int Z) {
  // out[x][y][z] (C order) = payload[x + X * (y + Y * z)]; 32 x 32 tiles through LDS over the (x, z) plane of one y
  __shared__ float tile[32][33];
  const int y = blockIdx.z, x0 = blockIdx.x * 32, z0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int x = x0 + tx, z = z0 + r;
    tile[r][tx] = (x < X && z < Z) ? payload[x + (int64_t)X * (y + (int64_t)Y * z)] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int x = x0 + r, z = z0 + tx;
    if (x < X && z < Z) out[((int64_t)x * Y + y) * Z + z] = tile[tx][r];
  }
}

template <typename T>
__device__ __forceinline__ float as_f32(T v) { return (float)v; }

template <typename T>
__global__ __launch_bounds__(256) void cast_to_f32_kernel(const T *__restrict__ in, float *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = as_f32(in[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void subsample_rows_kernel(const T *__restrict__ rows, int64_t n_rows, int cols,
                                                             const int64_t *__restrict__ idx, int64_t n_idx, float *__restrict__ out,
                                                             int *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_idx * cols) return;
  const int64_t r = idx[i / cols];
  if (r < 0 || r >= n_rows) {
    if (bad) atomicExch(bad, 1);
    out[i] = 0.f;
    return;
  }
  out[i] = as_f32(rows[r * cols + i % cols]);
}

// Batched row subset: every (item, sigma, array) of a collated batch is one svr_row_segment; the segments' output elements
// are numbered back to back (elem_prefix), one thread per element, 256 per block.  A block finds the segment of its FIRST
// element with one block-uniform bisection of elem_prefix (scalar loads, the same for all 256 lanes); a lane then only walks
// forward over the segments that begin inside its block.  Stores are coalesced within a segment (consecutive lanes,
// consecutive floats); the row reads are scattered by the indices.
__global__ __launch_bounds__(256) void subsample_rows_batched_kernel(const svr_row_segment *__restrict__ seg,
                                                                     const int64_t *__restrict__ elem_prefix, int n_seg, int64_t total,
                                                                     const int64_t *__restrict__ idx, float *__restrict__ out,
                                                                     int *__restrict__ bad) {
  const int64_t first = (int64_t)blockIdx.x * 256, i = first + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = n_seg - 1;  // the last segment with elem_prefix[s] <= first (elem_prefix[0] = 0)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (elem_prefix[mid] <= first) lo = mid; else hi = mid - 1;
  }
  int s = lo;
  while (i >= elem_prefix[s + 1]) ++s;  // i < total = elem_prefix[n_seg]: stops at n_seg - 1 at the latest
  const svr_row_segment sg = seg[s];
  const int64_t e = i - elem_prefix[s];
  const int64_t r = idx[sg.idx_offset + e / sg.cols];
  float *dst = out + sg.out_offset + e;
  if (r < 0 || r >= sg.n_rows) {
    if (bad) atomicExch(bad, 1);
    *dst = 0.f;
    return;
  }
  const int64_t at = r * sg.cols + e % sg.cols;
  switch (sg.dtype) {
    case SVR_DT_F64: *dst = as_f32(((const double *)sg.rows)[at]); break;
    case SVR_DT_F32: *dst = ((const float *)sg.rows)[at]; break;
    default: *dst = as_f32(((const uint8_t *)sg.rows)[at]); break;  // SVR_DT_BOOL / SVR_DT_U8 (the launcher's contract)
  }
}

}  // namespace

extern "C" int svr_df_to_grid(const float *payload, float *out, int32_t X, int32_t Y, int32_t Z, void *stream) {
  SVR_CHECK(payload && out && X > 0 && Y > 0 && Z > 0 && Y < 65536 && cdiv(Z, 32) < 65536, SVR_E_BADARG, "df_to_grid: bad argument");
  hipLaunchKernelGGL(df_to_grid_kernel, dim3((unsigned)cdiv(X, 32), (unsigned)cdiv(Z, 32), (unsigned)Y), dim3(256), 0,
                     (hipStream_t)stream, payload, out, X, Y, Z);
  return launch_status("df_to_grid");
}

extern "C" int svr_cast_to_f32(const void *in, int32_t dtype, float *out, int64_t n, void *stream) {
  if (n <= 0) return SVR_OK;
  SVR_CHECK(in && out, SVR_E_BADARG, "cast_to_f32: null pointer");
  const dim3 g((unsigned)cdiv(n, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case SVR_DT_F64: hipLaunchKernelGGL(cast_to_f32_kernel<double>, g, b, 0, s, (const double *)in, out, n); break;
    case SVR_DT_F32: hipLaunchKernelGGL(cast_to_f32_kernel<float>, g, b, 0, s, (const float *)in, out, n); break;
    case SVR_DT_BOOL: case SVR_DT_U8: hipLaunchKernelGGL(cast_to_f32_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)in, out, n); break;
    case SVR_DT_I32: hipLaunchKernelGGL(cast_to_f32_kernel<int32_t>, g, b, 0, s, (const int32_t *)in, out, n); break;
    case SVR_DT_I64: hipLaunchKernelGGL(cast_to_f32_kernel<int64_t>, g, b, 0, s, (const int64_t *)in, out, n); break;
    default: SVR_CHECK(false, SVR_E_UNSUPPORTED, "cast_to_f32: dtype %d", dtype);
  }
  return launch_status("cast_to_f32");
}

extern "C" int svr_subsample_rows(const void *rows, int32_t dtype, int64_t n_rows, int32_t cols, const int64_t *idx, int64_t n_idx,
                                  float *out, int32_t *bad_flag, void *stream) {
  if (n_idx <= 0) return SVR_OK;
  SVR_CHECK(rows && idx && out && cols > 0 && n_rows > 0, SVR_E_BADARG, "subsample_rows: bad argument");
  const dim3 g((unsigned)cdiv(n_idx * cols, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case SVR_DT_F64: hipLaunchKernelGGL(subsample_rows_kernel<double>, g, b, 0, s, (const double *)rows, n_rows, cols, idx, n_idx, out, bad_flag); break;
    case SVR_DT_F32: hipLaunchKernelGGL(subsample_rows_kernel<float>, g, b, 0, s, (const float *)rows, n_rows, cols, idx, n_idx, out, bad_flag); break;
    case SVR_DT_BOOL: case SVR_DT_U8: hipLaunchKernelGGL(subsample_rows_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)rows, n_rows, cols, idx, n_idx, out, bad_flag); break;
    default: SVR_CHECK(false, SVR_E_UNSUPPORTED, "subsample_rows: dtype %d", dtype);
  }
  return launch_status("subsample_rows");
}

extern "C" int svr_subsample_rows_batched(const svr_row_segment *segments, const int64_t *elem_prefix, int32_t n_segments,
                                          int64_t total, const int64_t *idx, float *out, int32_t *bad_flag, void *stream) {
  if (n_segments <= 0 || total <= 0) return SVR_OK;
  SVR_CHECK(segments && elem_prefix && idx && out, SVR_E_BADARG, "subsample_rows_batched: null pointer");
  SVR_CHECK(cdiv(total, 256) < (int64_t)1 << 31, SVR_E_BADARG, "subsample_rows_batched: %ld elements exceed one launch", (long)total);
  hipLaunchKernelGGL(subsample_rows_batched_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, segments,
                     elem_prefix, n_segments, total, idx, out, bad_flag);
  return launch_status("subsample_rows_batched");
}
