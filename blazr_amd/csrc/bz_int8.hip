// bz_int8.hip -- INT8 W8A8 (compressed-tensors "int-quantized"): int8 weights, row-major [N][K], one f32 scale per output row; the activations are quantised to
// int8 per row (per token), dynamically and symmetrically, by the kernels themselves.  For an input row x (rounded to the activation dtype, held as f32):
//
//   amax = max_k |x[k]|        sx = amax == 0 ? 1 : amax / 127        a[k] = clamp(rint(x[k] / sx), -127, 127)        (f32 divisions, ties to even)
//   acc[n] = sum_k a[k] q[n][k]                                         (int32, exact: K <= 131072 keeps |acc| <= 131072 . 127 . 128 < 2^31)
//   y[n] = R_act( f32( acc[n] . (sx . sw[n]) ) + b[n] )                 (both products in double, one rounding to f32, the bias in f32)
//
// Every sum is an integer, so a row's value does not depend on lanes, chunks, slices, tiles or the kernel that formed it: the GEMM's row i IS the GEMV of row i.
//
//   k_gemv_i8        decode GEMV, the quantiser in its prologue: direct output, or split-K with integer partials in the ring's 64-bit accumulator
//   k_i8_quant_rows  rows of 16-bit activations -> int8 codes and row scales (the GEMV prologue's arithmetic)
//   k_gemm_i8a8      prompt / decode-batch GEMM, both operands int8 on v_mfma_i32_32x32x32_i8
//   k_dequant_i8     op-level read-back of the device layout
#include "bz_internal.h"
#include "bz_dev.h"
#include <algorithm>

typedef int i8_i32x4 __attribute__((ext_vector_type(4)));
typedef int i8_i32x16 __attribute__((ext_vector_type(16)));

// the three pieces of the arithmetic above, shared by every kernel of this file
__device__ __forceinline__ float i8_row_scale(float amax) { return amax == 0.f ? 1.f : __fdiv_rn(amax, 127.f); }
__device__ __forceinline__ int i8_code(float x, float sx) { return (int)fminf(fmaxf(rintf(__fdiv_rn(x, sx)), -127.f), 127.f); }
__device__ __forceinline__ unsigned i8_pack4(float a, float b, float c, float d, float sx) {
  return ((unsigned)i8_code(a, sx) & 255u) | (((unsigned)i8_code(b, sx) & 255u) << 8) | (((unsigned)i8_code(c, sx) & 255u) << 16) | ((unsigned)i8_code(d, sx) << 24);
}
__device__ __forceinline__ float i8_finish(int acc, float sx, float sw) { return (float)((double)acc * ((double)sx * (double)sw)); }

// ---------------------------------------------------------------------------------------------------------
// decode GEMV.  The weight stream is k_gemv_f8's: 256 threads, a wave walks its rows four at a time (row = lane / 16), one 256-k chunk per step (16 lanes x 16
// bytes = one row's 256 bytes), wave-wide 16-byte non-temporal loads of 1 KiB, two buffers of four loads in flight (~40 KiB per CU).  What differs is
// everything behind the load.  The prologue builds the WHOLE row as f32 in LDS (every slice of the split form needs the row's maximum), reduces amax over the
// workgroup, and writes the int8 codes as words: K bytes, zero beyond K (K % 64 == 0 leaves a ragged last chunk; its loads are clamped to a valid address and
// meet zero codes).  The codes keep the row's own order, so the sixteen lanes of a weight row read sixteen consecutive 16-byte pieces -- 256 contiguous bytes,
// all 64 banks once -- and the four rows of a wave read the same addresses (a broadcast).  Per 16-byte piece: four V_DOT4_I32_I8 into four independent int32
// chains, then a 16-lane integer reduction per row.
// SPLIT: blockIdx = row block * SK + ks; slice ks covers KCs chunks.  Partials are integers: they go to the ring's 64-bit accumulator with integer atomics,
// unscaled, and the workgroup that finishes a row block LAST (a counter per row block, reset by that workgroup) applies the finish once.  It leaves the
// consumer's fixed-point value, as k_gemv_f8<true> does -- or, where the caller asked for it (GemvOut::split_f32: the op-level entry, whose f32 results have no grid),
// stores the f32 value there and hands the accumulator back zeroed.  Either way the value is the direct form's: the same integer, the same finish.
// ---------------------------------------------------------------------------------------------------------
#define I8_SMEM_MAX (152 * 1024)               // dynamic LDS a launch may ask for (the kernel's static words come on top: 160 KiB per workgroup)

template <bool SPLIT>
__global__ __launch_bounds__(256) void k_gemv_i8(const signed char* __restrict__ W, const float* __restrict__ scale, const float* __restrict__ bias, int N, int K,
                                                 int rows_per_wg, Pro pro, float* out, int act, long long* zero_buf, int zero_n, int SK, long long* accbuf,
                                                 unsigned* cnt) {
  extern __shared__ __attribute__((aligned(16))) char i8_smem[];
  __shared__ float i8_am[4];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, sub = lane >> 4, l16 = lane & 15;
  const int bid = blockIdx.x;
  const int rb = SPLIT ? bid / SK : bid, ks = SPLIT ? bid % SK : 0;
  const int rpw = rows_per_wg >> 2;
  const int rbeg = rb * rows_per_wg + wave * rpw, rend = min(rbeg + rpw, N);
  const int KCall = (K + 255) >> 8, KCs = SPLIT ? (KCall + SK - 1) / SK : KCall;
  const int kc0 = ks * KCs;
  const int KC = max(min(KCs, KCall - kc0), 0);
  float* xs = (float*)i8_smem;                  // [K] the row as f32
  unsigned* cw = (unsigned*)(xs + K);           // [KCall * 64] its codes, four per word, lowest k in the lowest byte (the weights' byte order)
  float* red = (float*)(cw + KCall * 64);       // [16]
  const int ngroups = rend > rbeg ? (rend - rbeg + 3) >> 2 : 0;
  const int nsteps = ngroups * KC;
  // issue cursor (clamped at the last step: a few redundant loads at the tail, never a branch around a load)
  int ig = 0, ikc = 0, ist = 0;
  auto issue = [&](uint4 (&q)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int row = min(rbeg + ig * 4 + sub, N - 1);
      const int k = (kc0 + ikc) * 256 + l16 * 16;
      q[j] = ldnt((const uint4*)(W + (size_t)row * K + (k < K ? k : 0)));
      if (ist + 1 < nsteps) { ist++; if (++ikc == KC) { ikc = 0; ig++; } }
    }
  };
  uint4 q0[4], q1[4];
  issue(q0);
  __builtin_amdgcn_sched_barrier(0);
  if (zero_buf)                                 // the ring protocol's side duty: zero the buffer the NEXT accumulate launch adds into
    for (int i = bid * 256 + tid; i < zero_n; i += gridDim.x * 256) zero_buf[i] = 0;
  // the quantiser: the whole row, its maximum, its codes
  build_x_simple<0>(pro, 0, K, xs, red, bid == 0);
  float am = 0.f;
  for (int i = tid * 4; i < K; i += 1024) {
    const float4 v = *(const float4*)(xs + i);
    am = fmaxf(fmaxf(am, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  am = wave_max(am);
  if (lane == 0) i8_am[wave] = am;
  __syncthreads();
  const float sx = i8_row_scale(fmaxf(fmaxf(i8_am[0], i8_am[1]), fmaxf(i8_am[2], i8_am[3])));
  for (int i = tid * 4; i < KCall * 256; i += 1024) {
    unsigned w = 0u;
    if (i < K) { const float4 v = *(const float4*)(xs + i); w = i8_pack4(v.x, v.y, v.z, v.w, sx); }
    cw[i >> 2] = w;
  }
  __syncthreads();
  int acc[4] = {0, 0, 0, 0};
  int cg = 0, ckc = 0, cst = 0;
  auto consume = [&](const uint4 (&q)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (cst < nsteps) {
        cst++;
        const uint4 c = *(const uint4*)(cw + (kc0 + ckc) * 64 + l16 * 4);
        acc[0] = __builtin_amdgcn_sdot4((int)q[j].x, (int)c.x, acc[0], false);
        acc[1] = __builtin_amdgcn_sdot4((int)q[j].y, (int)c.y, acc[1], false);
        acc[2] = __builtin_amdgcn_sdot4((int)q[j].z, (int)c.z, acc[2], false);
        acc[3] = __builtin_amdgcn_sdot4((int)q[j].w, (int)c.w, acc[3], false);
        if (++ckc == KC) {
          ckc = 0;
          const int v = grp_reduce<16, OpAdd>((acc[0] + acc[1]) + (acc[2] + acc[3]));
          acc[0] = acc[1] = acc[2] = acc[3] = 0;
          const int row = rbeg + cg * 4 + sub;
          if (l16 == 0 && row < rend) {
            if (SPLIT) {
              atomicAdd((unsigned long long*)(accbuf + row), (unsigned long long)(long long)v);
            } else {
              float y = i8_finish(v, sx, scale[row]);
              if (bias) y += bias[row];
              out[row] = round_act(y, act);
            }
          }
          cg++;
        }
      }
    }
  };
  for (int st = 0; st < nsteps; st += 8) {
    issue(q1); consume(q0);
    issue(q0); consume(q1);
  }
  if (SPLIT) {
    // the last workgroup of this row block to arrive turns the complete integer sums into the consumer's values
    __shared__ int i8_last;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      const unsigned old = atomicAdd(cnt + rb, 1u);
      i8_last = old == (unsigned)(SK - 1);
      if (i8_last) cnt[rb] = 0u;
    }
    __syncthreads();
    if (i8_last) {
      __threadfence();
      const int row = rb * rows_per_wg + tid;
      if (tid < rows_per_wg && row < N) {
        const long long a = __hip_atomic_load(accbuf + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float y = i8_finish((int)a, sx, scale[row]);
        if (bias) y += bias[row];
        // the ring gets the value ALREADY rounded to the activation dtype: a 16-bit float is exact on the ring's grid (f16: 2^-44 lies under its smallest
        // subnormal; bf16: 2^-40, exact from 2^-33 up), so the consumer's R_act(fix2f(.)) returns the direct form's bits, not a second rounding of y
        if (out) { out[row] = round_act(y, act); accbuf[row] = 0; }
        else accbuf[row] = d2fix((double)round_act(y, act), pro.act);
      }
    }
  }
}

static int i8_rows_per_wg(int N) {
  int r = 16;
  while (r < 256 && (N + r - 1) / r > 1024) r <<= 1;    // ~1000 workgroups when N is large (each runs the prologue), at least four rows per wave
  return r;
}
// split count of an int8 [N, K] GEMV: the rows are FP8's bytes, so the rule is FP8's (bzk_f8_choose_sk)
int bzk_i8_choose_sk(int N, int K) { return bzk_f8_choose_sk(N, K); }

int bzk_gemv_i8(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act) {
  if (pro.mode != PRO_PLAIN && pro.mode != PRO_NORM && pro.mode != PRO_SILU) BZ_FAIL(BZ_E_UNSUPPORTED, "int8 gemv: prologue mode %d is not built (plain, norm, silu are)", pro.mode);
  if (pro.perm || out.amax_val || out.shift.cs) BZ_FAIL(BZ_E_UNSUPPORTED, "int8 gemv: act-order / argmax partials / conv shift are not built");
  if (L.K % 64 || L.N % 64 || L.K > 131072 || !L.scales) BZ_FAIL(BZ_E_INVALID, "int8 gemv: N=%d K=%d must be multiples of 64, K <= 131072, with scales", L.N, L.K);
  if (pro.mode == PRO_NORM && (pro.H != L.K || pro.H % 4)) BZ_FAIL(BZ_E_INVALID, "int8 gemv: norm prologue over %d elements, K=%d", pro.H, L.K);
  const int KCall = (L.K + 255) / 256;
  const int SK = L.sk > 1 ? L.sk : 1;           // (more slices than chunks: the surplus slices are empty and only count)
  const char* lbl = pro.mode == PRO_NORM ? "gemv_i8<norm>" : pro.mode == PRO_SILU ? "gemv_i8<silu>" : "gemv_i8";
  const size_t smem = (size_t)L.K * 4 + (size_t)KCall * 256 + 64;      // the f32 row, its codes, the prologue's words
  if (smem > I8_SMEM_MAX) BZ_FAIL(BZ_E_UNSUPPORTED, "K=%d too large for the int8 GEMV", L.K);
  static bool attr_done = false;      // a long row takes more than the 64 KiB a launch gets without asking
  if (!attr_done) {
    BZ_HIP(hipFuncSetAttribute((const void*)k_gemv_i8<true>, hipFuncAttributeMaxDynamicSharedMemorySize, I8_SMEM_MAX));
    BZ_HIP(hipFuncSetAttribute((const void*)k_gemv_i8<false>, hipFuncAttributeMaxDynamicSharedMemorySize, I8_SMEM_MAX));
    attr_done = true;
  }
  if (SK > 1) {
    if (!out.acc || !L.zeros) BZ_FAIL(BZ_E_INVALID, "split-K int8 gemv needs a fixed-point accumulator and its row-block counters");
    BZ_LAUNCH(lbl, L.algo_bytes, (k_gemv_i8<true>), dim3((L.N / 16) * SK), dim3(256), smem, s, (const signed char*)L.w, (const float*)L.scales, L.bias, L.N, L.K, 16, pro,
              out.split_f32, act, out.zero_buf, out.zero_n, SK, out.acc, (unsigned*)L.zeros);
  } else {
    if (!out.direct) BZ_FAIL(BZ_E_INVALID, "int8 gemv needs a direct output");
    const int rpw = i8_rows_per_wg(L.N);
    BZ_LAUNCH(lbl, L.algo_bytes, (k_gemv_i8<false>), dim3((L.N + rpw - 1) / rpw), dim3(256), smem, s, (const signed char*)L.w, (const float*)L.scales, L.bias, L.N, L.K, rpw, pro,
              out.direct, act, out.zero_buf, out.zero_n, 1, (long long*)nullptr, (unsigned*)nullptr);
  }
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// out[n][k] = f32(sw[n] q[n][k]): one rounding.  Four weights per thread.
__global__ void k_dequant_i8(const unsigned* __restrict__ W, const float* __restrict__ scale, int K, size_t words, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
    const float sc = scale[(i * 4) / (size_t)K];
    const unsigned w = W[i];
    *(float4*)(out + i * 4) = make_float4(__fmul_rn(sc, (float)(signed char)(w & 255u)), __fmul_rn(sc, (float)(signed char)((w >> 8) & 255u)),
                                          __fmul_rn(sc, (float)(signed char)((w >> 16) & 255u)), __fmul_rn(sc, (float)(signed char)(w >> 24)));
  }
}
int bzk_dequant_i8(hipStream_t s, const LinearDev& L, float* out) {
  hipLaunchKernelGGL(k_dequant_i8, dim3(2048), dim3(256), 0, s, (const unsigned*)L.w, (const float*)L.scales, L.K, (size_t)L.N * L.K / 4, out);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// k_i8_quant_rows: S rows of 16-bit activations -> codes [S][K] int8 and sx[S] f32, the GEMV prologue's arithmetic (i8_row_scale, i8_code), so the same bits.
// One workgroup per row; a thread reads eight elements (16 bytes) per pass, twice: once for the maximum, once (from cache) for the codes.  K % 64 == 0.
// ---------------------------------------------------------------------------------------------------------
template <int DT> __device__ __forceinline__ float i8_from16(unsigned h16) {
  if constexpr (DT == BZ_BF16) return __uint_as_float(h16 << 16);
  else return (float)__builtin_bit_cast(_Float16, (unsigned short)h16);
}
template <int DT>
__global__ __launch_bounds__(256) void k_i8_quant_rows(const unsigned short* __restrict__ X, int K, signed char* __restrict__ codes, float* __restrict__ sxs) {
  __shared__ float qr_am[4];
  const int tid = threadIdx.x;
  const unsigned short* xr = X + (size_t)blockIdx.x * K;
  float am = 0.f;
  for (int e = tid * 8; e < K; e += 2048) {
    const uint4 raw = *(const uint4*)(xr + e);
    const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; i++) am = fmaxf(am, fmaxf(fabsf(i8_from16<DT>(u[i] & 0xffffu)), fabsf(i8_from16<DT>(u[i] >> 16))));
  }
  am = wave_max(am);
  if ((tid & 63) == 0) qr_am[tid >> 6] = am;
  __syncthreads();
  const float sx = i8_row_scale(fmaxf(fmaxf(qr_am[0], qr_am[1]), fmaxf(qr_am[2], qr_am[3])));
  if (tid == 0) sxs[blockIdx.x] = sx;
  for (int e = tid * 8; e < K; e += 2048) {
    const uint4 raw = *(const uint4*)(xr + e);
    uint2 o;
    o.x = i8_pack4(i8_from16<DT>(raw.x & 0xffffu), i8_from16<DT>(raw.x >> 16), i8_from16<DT>(raw.y & 0xffffu), i8_from16<DT>(raw.y >> 16), sx);
    o.y = i8_pack4(i8_from16<DT>(raw.z & 0xffffu), i8_from16<DT>(raw.z >> 16), i8_from16<DT>(raw.w & 0xffffu), i8_from16<DT>(raw.w >> 16), sx);
    *(uint2*)(codes + (size_t)blockIdx.x * K + e) = o;
  }
}
int bzk_i8_quant_rows(hipStream_t s, int dt, const void* x16, int S, int K, void* codes, float* sx) {
  if ((dt != BZ_F16 && dt != BZ_BF16) || S <= 0 || K < 64 || K % 64) BZ_FAIL(BZ_E_INVALID, "i8_quant_rows: 16-bit rows with K %% 64 == 0 (S=%d K=%d)", S, K);
  if (dt == BZ_F16) BZ_LAUNCH("i8_quant_rows", (double)S * K * 2.0, (k_i8_quant_rows<BZ_F16>), dim3(S), dim3(256), 0, s, (const unsigned short*)x16, K, (signed char*)codes, sx);
  else BZ_LAUNCH("i8_quant_rows", (double)S * K * 2.0, (k_i8_quant_rows<BZ_BF16>), dim3(S), dim3(256), 0, s, (const unsigned short*)x16, K, (signed char*)codes, sx);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// k_gemm_i8a8: Y[S][N] = R(f32(acc . (sx[s] . sw[n])) + b[n]), acc = XQ[S][K] . Q[N][K]^T on v_mfma_i32_32x32x32_i8.  A lane's A or B operand of that instruction is
// sixteen consecutive k-bytes of one row (row = lane & 31, k = 16 (lane / 32) ..), and both arrays are row-major bytes: one 16-byte read each, nothing to
// unpack or transpose.  256 threads, 2 x 2 waves; a workgroup tile of 64 TM x 128 x 64 (TM = 2: 128 rows; 1 for at most 64 rows), a wave owns 32 TM x 64:
// TM x 2 MFMA tiles, 32 TM accumulator registers.  Tiles go global -> registers -> LDS into two buffers: thread t carries the 16-byte piece t % 4 of rows
// t / 4 (+ 64 per pass), four lanes reading one row's 64 contiguous bytes; the NEXT k-step's global loads are issued before this step's MFMAs and stored
// after them, one barrier per step.  LDS rows are padded to 80 bytes: the fragment reads of 16 lanes (rows r .. r + 15, 80 bytes apart) start at banks
// 20 r mod 64 -- sixteen disjoint groups of four, all 64 banks.  Rows past S or N are clamped to the last valid row and their results dropped.
// Epilogue: the C layout (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) gives a lane one column n and sixteen rows per tile: sw[n] and b[n]
// are per-lane scalars, sx[m] a broadcast load.  No split-K: the sums are integers, so one would change nothing but the launch count.
// ---------------------------------------------------------------------------------------------------------
#define I8G_LD 80          // bytes of an LDS tile row (64 data + 16 pad)

template <int TM>
__global__ __launch_bounds__(256) void k_gemm_i8a8(const signed char* __restrict__ XQ, const float* __restrict__ SX, const signed char* __restrict__ W, const float* __restrict__ scale,
                                                   const float* __restrict__ bias, int S, int N, int K, int act, float* __restrict__ Y, int mtiles) {
  constexpr int BM = 64 * TM, ABYTES = BM * I8G_LD, TILE = ABYTES + 128 * I8G_LD;
  __shared__ __attribute__((aligned(16))) unsigned char sm[2 * TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int mt = blockIdx.x % mtiles, nt = blockIdx.x / mtiles;      // the row tiles of one column tile sit side by side: its weights are read from HBM once
  const int m0 = mt * BM, n0 = nt * 128;
  const int nsteps = K >> 6;
  const int lrow = tid >> 2, piece = tid & 3;
  const signed char* ap[TM]; const signed char* bp[2];
#pragma unroll
  for (int i = 0; i < TM; i++) ap[i] = XQ + (size_t)min(m0 + 64 * i + lrow, S - 1) * K + 16 * piece;
#pragma unroll
  for (int i = 0; i < 2; i++) bp[i] = W + (size_t)min(n0 + 64 * i + lrow, N - 1) * K + 16 * piece;
  i8_i32x4 ga[TM], gb[2];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < TM; i++) ga[i] = *(const i8_i32x4*)(ap[i] + (size_t)kt * 64);
#pragma unroll
    for (int i = 0; i < 2; i++) gb[i] = *(const i8_i32x4*)(bp[i] + (size_t)kt * 64);
  };
  auto lstore = [&](int buf) {
    unsigned char* base = sm + buf * TILE + lrow * I8G_LD + 16 * piece;
#pragma unroll
    for (int i = 0; i < TM; i++) *(i8_i32x4*)(base + 64 * i * I8G_LD) = ga[i];
#pragma unroll
    for (int i = 0; i < 2; i++) *(i8_i32x4*)(base + ABYTES + 64 * i * I8G_LD) = gb[i];
  };
  i8_i32x16 acc[TM][2];
#pragma unroll
  for (int t = 0; t < TM; t++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][j][i] = 0;
  gload(0);
  lstore(0);
  const int aoff = (wm * 32 * TM + r) * I8G_LD + 16 * h, boff = ABYTES + (wn * 64 + r) * I8G_LD + 16 * h;
  for (int it = 0; it < nsteps; it++) {
    __syncthreads();                                         // tile `it` is in LDS; everyone is done reading the buffer this step's stores overwrite
    gload(min(it + 1, nsteps - 1));                          // clamped: one redundant reload at the tail, never a branch around a load
    const unsigned char* tb = sm + (it & 1) * TILE;
#pragma unroll
    for (int s2 = 0; s2 < 2; s2++) {                         // MFMA step: k = 32 s2 + 16 h .. + 15 of rows r (+ 32 per tile)
      i8_i32x4 af[TM], bf[2];
#pragma unroll
      for (int t = 0; t < TM; t++) af[t] = *(const i8_i32x4*)(tb + aoff + t * 32 * I8G_LD + 32 * s2);
#pragma unroll
      for (int j = 0; j < 2; j++) bf[j] = *(const i8_i32x4*)(tb + boff + j * 32 * I8G_LD + 32 * s2);
#pragma unroll
      for (int t = 0; t < TM; t++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[t][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[t], bf[j], acc[t][j], 0, 0, 0);
    }
    if (it + 1 < nsteps) lstore((it + 1) & 1);
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int n = n0 + wn * 64 + 32 * j + r;
    if (n < N) {
      const float sw = scale[n], bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int t = 0; t < TM; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int m = m0 + wm * 32 * TM + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m < S) {
            float y = i8_finish(acc[t][j][i], SX[m], sw);
            if (bias) y += bv;
            Y[(size_t)m * N + n] = round_act(y, act);
          }
        }
    }
  }
}

bool bzk_gemm_i8a8_ok(const LinearDev& L, int xdt) {
  return L.kind == LK_I8 && (xdt == BZ_F16 || xdt == BZ_BF16) && L.K % 64 == 0 && L.K >= 64 && L.K <= 131072 && L.N % 64 == 0 && L.scales != nullptr;
}

// codes [S][K] int8 and sx [S] as bzk_i8_quant_rows wrote them; act: rounding of the output (BZ_F32: none)
int bzk_gemm_i8a8(hipStream_t s, const LinearDev& L, const void* codes, const float* sx, int S, int act, float* y) {
  const int N = L.N, K = L.K;
  if (!bzk_gemm_i8a8_ok(L, BZ_F16)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_i8a8: int8 weights with N %% 64 == 0 and K %% 64 == 0 only");
  if (S <= 0 || N <= 0 || !codes || !sx) BZ_FAIL(BZ_E_INVALID, "gemm_i8a8: S=%d N=%d", S, N);
  const double flops = 2.0 * S * (double)N * K;
  const int TM = S <= 64 ? 1 : 2, BM = 64 * TM;
  const int mtiles = (S + BM - 1) / BM, ntiles = (N + 127) / 128;
  if ((long long)mtiles * ntiles >= (1ll << 31)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_i8a8: 2^31 tiles or more");
  const unsigned grid = (unsigned)mtiles * (unsigned)ntiles;
#define LAUNCH_I8A8(M) BZ_LAUNCH("gemm_i8a8_mfma", flops, (k_gemm_i8a8<M>), dim3(grid), dim3(256), 0, s, (const signed char*)codes, sx, (const signed char*)L.w, \
    (const float*)L.scales, L.bias, S, N, K, act, y, mtiles)
  if (TM == 1) LAUNCH_I8A8(1); else LAUNCH_I8A8(2);
#undef LAUNCH_I8A8
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
