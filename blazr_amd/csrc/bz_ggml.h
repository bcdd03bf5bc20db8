// bz_ggml.h -- device decoders of RAW ggml blocks (the bytes of a GGUF file, public GGML block spec).  One definition per format: the load-time repack
// (bz_kernels.hip k_repack_gq) and the quantised token-embedding gathers (k_embed, bz_prefill.hip k_pf_embed) both read raw blocks through these.
//   Q4_0 : { f16 d; u8 qs[16] }                                                      18 B / 32    (weight j < 16: low nibble of qs[j], j + 16: its high nibble)
//   Q4_1 : { f16 d, m; u8 qs[16] }                                                   20 B / 32
//   Q5_0 : { f16 d; u8 qh[4]; u8 qs[16] }                                            22 B / 32    (5th bit of weight j = bit j of qh as a little-endian u32)
//   Q5_1 : { f16 d, m; u8 qh[4]; u8 qs[16] }                                         24 B / 32
//   Q8_0 : { f16 d; int8 qs[32] }                                                   34 B / 32
//   Q4_K : { f16 d, dmin; u8 scales[12]; u8 qs[128] }                              144 B / 256
//   Q5_K : { f16 d, dmin; u8 scales[12]; u8 qh[32]; u8 qs[128] }                   176 B / 256   (5th bit of element l of sub-block j = bit j of qh[l])
//   Q6_K : { u8 ql[128]; u8 qh[64]; int8 scales[16]; f16 d }                       210 B / 256
// Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/blazr_hip.h"

__device__ __forceinline__ unsigned q4k_raw_nib(const unsigned char* blk, int k) {   // weight k (0..255) of a raw block_q4_K
  const int j64 = k >> 6, l = k & 63;
  const unsigned char b = blk[16 + j64 * 32 + (l & 31)];
  return l < 32 ? (b & 15u) : (unsigned)(b >> 4);
}
__device__ __forceinline__ unsigned q5k_raw(const unsigned char* blk, int k) {       // 5-bit value (0..31) of weight k of a raw block_q5_K
  const int j64 = k >> 6, l = k & 63;
  const unsigned char b = blk[48 + j64 * 32 + (l & 31)];
  const unsigned lo = l < 32 ? (b & 15u) : (unsigned)(b >> 4);
  return lo | (((unsigned)(blk[16 + (k & 31)] >> (k >> 5)) & 1u) << 4);
}
__device__ __forceinline__ unsigned q6k_raw(const unsigned char* blk, int k) {       // 6-bit value (0..63) of weight k of a raw block_q6_K
  const int n128 = k >> 7, l = k & 127, quad = l >> 5, pos = l & 31;
  const unsigned char qlb = blk[n128 * 64 + (quad & 1) * 32 + pos];
  const unsigned lo = quad < 2 ? (qlb & 15u) : (unsigned)(qlb >> 4);
  const unsigned hi = (blk[128 + n128 * 32 + pos] >> (2 * quad)) & 3u;
  return lo | (hi << 4);
}
// the 4- / 5-bit value of weight j (0..31) of a raw legacy block (values: Q4_0 (q - 8) d, Q4_1 q d + m, Q5_0 (q - 16) d, Q5_1 q d + m)
__device__ __forceinline__ unsigned q4_0_raw(const unsigned char* blk, int j) { const unsigned char b = blk[2 + (j & 15)]; return j < 16 ? (b & 15u) : (unsigned)(b >> 4); }
__device__ __forceinline__ unsigned q4_1_raw(const unsigned char* blk, int j) { const unsigned char b = blk[4 + (j & 15)]; return j < 16 ? (b & 15u) : (unsigned)(b >> 4); }
__device__ __forceinline__ unsigned q5_0_raw(const unsigned char* blk, int j) {
  const unsigned char b = blk[6 + (j & 15)];
  return (j < 16 ? (b & 15u) : (unsigned)(b >> 4)) | ((((unsigned)blk[2 + (j >> 3)] >> (j & 7)) & 1u) << 4);
}
__device__ __forceinline__ unsigned q5_1_raw(const unsigned char* blk, int j) {
  const unsigned char b = blk[8 + (j & 15)];
  return (j < 16 ? (b & 15u) : (unsigned)(b >> 4)) | ((((unsigned)blk[4 + (j >> 3)] >> (j & 7)) & 1u) << 4);
}
__host__ __device__ __forceinline__ bool ggml_is_legacy(int type) {
  return type == BZ_GGML_Q4_0 || type == BZ_GGML_Q4_1 || type == BZ_GGML_Q5_0 || type == BZ_GGML_Q5_1;
}
// 6-bit scale / min of sub-block j from the 12 packed bytes of a Q4_K / Q5_K block (GGML get_scale_min_k4)
__device__ __forceinline__ void qk_raw_scale_min(const unsigned char* s, int j, int& sc, int& mn) {
  if (j < 4) { sc = s[j] & 63; mn = s[j + 4] & 63; }
  else { sc = (s[j + 4] & 15) | ((s[j - 4] >> 6) << 4); mn = (s[j + 4] >> 4) | ((s[j] >> 6) << 4); }
}
__device__ __forceinline__ float f16_at(const unsigned char* p) { return __half2float(__ushort_as_half((unsigned short)(p[0] | (p[1] << 8)))); }

// weights per block: 32 for Q8_0 and the legacy formats, 256 for the k-quants
__host__ __device__ __forceinline__ int ggml_blk_k(int type) { return type == BZ_GGML_Q8_0 || ggml_is_legacy(type) ? 32 : 256; }
__host__ __device__ __forceinline__ size_t ggml_blk_row_bytes(int type, int K) {
  if (ggml_is_legacy(type)) return (size_t)(K / 32) * (type == BZ_GGML_Q4_0 ? 18 : type == BZ_GGML_Q4_1 ? 20 : type == BZ_GGML_Q5_0 ? 22 : 24);
  return type == BZ_GGML_Q8_0 ? (size_t)(K / 32) * 34 : type == BZ_GGML_Q4_K ? (size_t)(K / 256) * 144 : type == BZ_GGML_Q5_K ? (size_t)(K / 256) * 176
       : type == BZ_GGML_Q6_K ? (size_t)(K / 256) * 210 : 0;
}
// weight k of a raw ggml row, exactly as ggml's dequantize_row_* computes it (its products and differences in its order, no contraction)
__device__ __forceinline__ float ggml_row_elem(int type, const unsigned char* row, int k) {
  if (type == BZ_GGML_Q8_0) {
    const unsigned char* b = row + (size_t)(k >> 5) * 34;
    return __fmul_rn(f16_at(b), (float)(signed char)b[2 + (k & 31)]);
  }
  if (ggml_is_legacy(type)) {   // Q4_0 / Q5_0: y = (q - 8 | 16) * d ; Q4_1 / Q5_1: y = q * d + m
    const unsigned char* b = row + (size_t)(k >> 5) * ggml_blk_row_bytes(type, 32);
    const int j = k & 31;
    if (type == BZ_GGML_Q4_0) return __fmul_rn((float)((int)q4_0_raw(b, j) - 8), f16_at(b));
    if (type == BZ_GGML_Q5_0) return __fmul_rn((float)((int)q5_0_raw(b, j) - 16), f16_at(b));
    const float q = (float)(type == BZ_GGML_Q4_1 ? q4_1_raw(b, j) : q5_1_raw(b, j));
    return __fadd_rn(__fmul_rn(q, f16_at(b)), f16_at(b + 2));
  }
  if (type == BZ_GGML_Q6_K) {
    const unsigned char* b = row + (size_t)(k >> 8) * 210;
    const int kk = k & 255;
    return __fmul_rn(__fmul_rn(f16_at(b + 208), (float)(signed char)b[192 + (kk >> 4)]), (float)((int)q6k_raw(b, kk) - 32));
  }
  const bool five = type == BZ_GGML_Q5_K;   // Q4_K / Q5_K: y = (d * sc) * q - (dmin * m)
  const unsigned char* b = row + (size_t)(k >> 8) * (five ? 176 : 144);
  const int kk = k & 255;
  int sc, mn;
  qk_raw_scale_min(b + 4, kk >> 5, sc, mn);
  const float q = (float)(five ? q5k_raw(b, kk) : q4k_raw_nib(b, kk));
  return __fsub_rn(__fmul_rn(__fmul_rn(f16_at(b), (float)sc), q), __fmul_rn(f16_at(b + 2), (float)mn));
}
