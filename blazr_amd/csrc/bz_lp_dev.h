// bz_lp_dev.h -- what the two users of a logits row's log-sum-exp and top list share (bz_logprobs.hip: the batched sampler's rows; bz_score.hip: prompt rows): the
// composite key that IS the order (logit descending, id ascending) and the block reductions of their 256-thread kernels; the integer term of the sum as a function
// (k_lp_sum spells the same expression out in its loop).  The key and the term are host + device, so the public host evaluation (bz_score_row_spec) runs the
// expressions the kernels run.
#pragma once
#include "bz_internal.h"

typedef unsigned long long u64;

__host__ __device__ __forceinline__ unsigned lp_bits(float x) { unsigned b; __builtin_memcpy(&b, &x, 4); return b; }
__host__ __device__ __forceinline__ float lp_float(unsigned b) { float x; __builtin_memcpy(&x, &b, 4); return x; }
// larger = earlier in (x descending, id ascending); 0 = no entry (a NaN logit maps there: never listed)
__host__ __device__ __forceinline__ u64 lp_composite(float x, long long i) {
  if (x != x) return 0;
  unsigned b = x == 0.0f ? 0u : lp_bits(x);                     // -0 orders as +0: equal logits tie on the id alone
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)b << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
}
__host__ __device__ __forceinline__ float lp_logit_of(u64 c) {
  const unsigned k = (unsigned)(c >> 32);
  return lp_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// q = floor(bz_expf(x - M) * 2^40): the row's sum is an integer, so it does not depend on the order of its terms.  e <= 1: at most 2^40; a NaN (a row of -inf) adds nothing
__host__ __device__ __forceinline__ u64 lp_term(float x, float M) {
  const float e = bz_expf(x - M);
  return e > 0.0f ? (u64)((double)e * 1099511627776.0) : 0ull;
}
__host__ __device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

#ifdef __HIPCC__
// every thread of the 256 gets the block's maximum (two barriers; red: 4 words of LDS)
__device__ __forceinline__ u64 block_max_u64(u64 v, u64* red) {
  for (int k = 32; k >= 1; k >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, k, 64), hi = __shfl_xor((unsigned)(v >> 32), k, 64);
    v = umax64(v, ((u64)hi << 32) | lo);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const u64 t = umax64(umax64(red[0], red[1]), umax64(red[2], red[3]));
  __syncthreads();
  return t;
}
// every thread of the 256 gets the block's (integer, therefore exact) sum
__device__ __forceinline__ u64 block_sum_u64(u64 s, u64* red) {
  for (int k = 32; k >= 1; k >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)s, k, 64), hi = __shfl_xor((unsigned)(s >> 32), k, 64);
    s += ((u64)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const u64 t = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return t;
}
__device__ __forceinline__ float block_max_f(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float t = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return t;
}
#endif  // __HIPCC__
