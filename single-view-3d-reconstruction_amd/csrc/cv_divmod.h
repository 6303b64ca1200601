// Row decode of the UNet's weight-gradient kernels (gemm_bf16x3.hip, conv2d.hip): pixel index -> (sample, row, column) without
// an integer division.  Plain C++ on the host (tests/host/cv_divmod_driver.cpp checks the claim below), __device__ under hipcc.
#pragma once
#if defined(__HIPCC__)
#define CV_HD __host__ __device__ __forceinline__
#else
#define CV_HD inline
#endif

// n / d and n % d for 0 <= n < 2^24, 0 < d < 2^24 through one float multiply (rcp = 1.0f / d) and one correction step
CV_HD void cv_divmod(int n, int d, float rcp, int &q, int &r) {
  q = (int)((float)n * rcp);
  r = n - q * d;
  if (r < 0) { --q; r += d; }
  else if (r >= d) { ++q; r -= d; }
}
