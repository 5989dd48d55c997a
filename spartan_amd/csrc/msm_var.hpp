// spartan_amd: what the variable-base multiplications share between their translation units — msm_var.hip (sp_msm_var, sp_points,
// sp_msm_points: one multiplication a call) and msm_many.hip (sp_msm_var_many, sp_msm_points_many: K of them in one launch chain).
#pragma once
#include "internal.hpp"

constexpr size_t MV_MAX_N = 65536;
constexpr int MV_BLOCK = 256;

struct sp_points {
  int dev;
  size_t n;
  Pt* table;  // [64 windows][n][8]: table[(w * n + j) * 8 + m - 1] = m 16^w P[j]
};

__device__ __forceinline__ Pt pt_shfl_down(const Pt& p, int delta) {
  Pt r;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    r.X.v[i] = __shfl_down((unsigned long long)p.X.v[i], delta, 64);
    r.Y.v[i] = __shfl_down((unsigned long long)p.Y.v[i], delta, 64);
    r.Z.v[i] = __shfl_down((unsigned long long)p.Z.v[i], delta, 64);
    r.T.v[i] = __shfl_down((unsigned long long)p.T.v[i], delta, 64);
  }
  return r;
}

// The sum of one term per lane over a block of MV_BLOCK lanes, shared by the window kernels of sp_msm_var and sp_msm_points: 6 wavefront
// shuffle levels, then the 4 wavefront sums through LDS; lane 0 writes the block's sum. EVERY lane of the block must call it (no early exit
// before it): lane 0 of each wavefront ends with the sum of its 64 terms.
__device__ __forceinline__ void msmv_block_sum(Pt p, Pt* sm /*[MV_BLOCK / 64], shared*/, Pt* __restrict__ out) {
  const int t = threadIdx.x;
#pragma unroll 1
  for (int delta = 32; delta > 0; delta >>= 1) p = pt_add(p, pt_shfl_down(p, delta));
  if ((t & 63) == 0) sm[t >> 6] = p;
  __syncthreads();
  if (t == 0) *out = pt_add(pt_add(sm[0], sm[1]), pt_add(sm[2], sm[3]));
}
