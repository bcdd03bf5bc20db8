// bz_fp8.hip -- FP8 (OCP E4M3) weights, W8A16: one byte per weight, row-major [N][K], one f32 scale per output row, 16-bit (or f32) activations.
//
//   y[n] = R_act( f32( s[n] . sum_k x[k] e4m3(q[n][k]) ) + b[n] )
//
// Every E4M3 value is exact in f16 and in bf16 and every product x e4m3(q) has at most 15 significant bits, so an FP8 linear is a dense 16-bit linear with
// one-byte storage: the decode kernel carries the sum the way the dense rows kernels do (f32 products, exact; double sum) and applies the scale ONCE, to the
// finished sum.  NaN codes (0x7F / 0xFF) are refused when a tensor is added, so the conversion below never meets one.
//
//   k_gemv_f8     decode GEMV: direct output, or split-K through the 64-bit fixed-point accumulator with the finish (scale, bias) in the launch
//   k_gemm_f8w    prompt / decode-batch GEMM on the 16-bit matrix cores: weight tiles staged as bytes, expanded to f16 / bf16 fragments in registers
//   k_dequant_f8  op-level read-back of the device layout
#include "bz_internal.h"
#include "bz_dev.h"
#include <algorithm>

typedef float f8_f32x2 __attribute__((ext_vector_type(2)));
// four E4M3 bytes of one word -> four floats, lowest byte (= lowest k) first: V_CVT_PK_F32_FP8, two per instruction, OCP e4m3fn on gfx950
// (subnormals included; the two NaN codes never reach a kernel)
__device__ __forceinline__ void f8x4_to_f32(unsigned w, float (&f)[4]) {
  const f8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo.x; f[1] = lo.y; f[2] = hi.x; f[3] = hi.y;
}

// ---------------------------------------------------------------------------------------------------------
// decode GEMV.  256 threads; a wave walks its rows four at a time (row = lane / 16), one 256-k chunk per step (16 lanes x 16 bytes = one row's 256 bytes),
// so a wave-wide 16-byte load reads 1 KiB: four rows' contiguous 256 bytes.  Two buffers of four loads: 4-8 KiB in flight per wave, 16-32 KiB per
// workgroup (~40 KiB per CU is what HBM can use).  x sits in LDS as f32, zero beyond K (K % 64 == 0 leaves a ragged last chunk; its loads are
// clamped to a valid address and meet zeros), padded by four floats after every sixteen (xs_pos<2>): a lane's sixteen activations are four float4 reads, and
// sixteen lanes 80 bytes apart cover all 64 banks.  Four independent double sums per lane: the adds of one 16-byte piece do not wait for each other.
// SPLIT: blockIdx = row block * SK + ks; slice ks covers KCs chunks.  The partial sums stay in UNSCALED units: they go to the ring's accumulator on a grid
// of their own (2^-24: the unscaled sums reach 448 |x| K), and the workgroup that finishes a row block LAST (a counter per row block, reset by that
// workgroup: nothing to zero between launches, graph replays included) reads the complete sums, applies scale and bias once and leaves the accumulator
// holding R_f32(s sum) + b on the consumer's grid -- what every fixed-point consumer of the step expects to find.
// ---------------------------------------------------------------------------------------------------------
#define F8_SMEM_MAX (152 * 1024)               // dynamic LDS a launch may ask for (the kernel's static words come on top: 160 KiB per workgroup)
#define F8_XCHUNK 320                         // LDS floats per 256-k chunk (xs_pos<2>)
#define F8_PART_SCALE 16777216.0              // 2^24
#define F8_PART_INV 5.9604644775390625e-08    // 2^-24

template <bool SPLIT>
__global__ __launch_bounds__(256) void k_gemv_f8(const unsigned char* __restrict__ W, const float* __restrict__ scale, const float* __restrict__ bias, int N, int K,
                                                 int rows_per_wg, Pro pro, float* out, int act, long long* zero_buf, int zero_n, int SK, long long* accbuf,
                                                 unsigned* cnt) {
  extern __shared__ __attribute__((aligned(16))) char f8_smem[];
  float* xs = (float*)f8_smem;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, sub = lane >> 4, l16 = lane & 15;
  const int bid = blockIdx.x;
  const int rb = SPLIT ? bid / SK : bid, ks = SPLIT ? bid % SK : 0;
  const int rpw = rows_per_wg >> 2;
  const int rbeg = rb * rows_per_wg + wave * rpw, rend = min(rbeg + rpw, N);
  const int KCall = (K + 255) >> 8, KCs = SPLIT ? (KCall + SK - 1) / SK : KCall;
  const int kc0 = ks * KCs;
  const int KC = max(min(KCs, KCall - kc0), 0);
  const int kb = kc0 * 256;
  float* red = xs + KCs * F8_XCHUNK;            // [16]
  const int ngroups = rend > rbeg ? (rend - rbeg + 3) >> 2 : 0;
  const int nsteps = ngroups * KC;
  // issue cursor (clamped at the last step: a few redundant loads at the tail, never a branch around a load)
  int ig = 0, ikc = 0, ist = 0;
  auto issue = [&](uint4 (&q)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int row = min(rbeg + ig * 4 + sub, N - 1);
      const int k = kb + ikc * 256 + l16 * 16;
      q[j] = ldnt((const uint4*)(W + (size_t)row * K + (k < K ? k : 0)));
      if (ist + 1 < nsteps) { ist++; if (++ikc == KC) { ikc = 0; ig++; } }
    }
  };
  uint4 q0[4], q1[4];
  issue(q0);
  __builtin_amdgcn_sched_barrier(0);
  if (zero_buf)                                 // the ring protocol's side duty: zero the buffer the NEXT accumulate launch adds into
    for (int i = bid * 256 + threadIdx.x; i < zero_n; i += gridDim.x * 256) zero_buf[i] = 0;
  const int KR = max(min(K - kb, KC * 256), 0);
  for (int i = KR + threadIdx.x; i < KCs * 256; i += 256) xs[xs_pos<2>(i)] = 0.f;
  build_x_simple<2>(pro, kb, KR, xs, red, bid == 0);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};                             // exact products, double sum: a row's value does not depend on the lane / chunk / slice decomposition
  int cg = 0, ckc = 0, cst = 0;
  auto consume = [&](const uint4 (&q)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (cst < nsteps) {
        cst++;
        const float4* xp = (const float4*)(xs + ckc * F8_XCHUNK + l16 * 20);
        const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float4 xv = xp[i];
          float f[4];
          f8x4_to_f32(w[i], f);
          acc[0] += (double)__fmul_rn(f[0], xv.x);
          acc[1] += (double)__fmul_rn(f[1], xv.y);
          acc[2] += (double)__fmul_rn(f[2], xv.z);
          acc[3] += (double)__fmul_rn(f[3], xv.w);
        }
        if (++ckc == KC) {
          ckc = 0;
          const double vd = grp_sum_d<16>((acc[0] + acc[1]) + (acc[2] + acc[3]));
          acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
          const int row = rbeg + cg * 4 + sub;
          if (l16 == 0 && row < rend) {
            if (SPLIT) {
              atomicAdd((unsigned long long*)(accbuf + row), (unsigned long long)__double2ll_rn(vd * F8_PART_SCALE));
            } else {
              float v = (float)(vd * (double)scale[row]);   // the scale meets the finished sum, one rounding to f32, then the bias in f32 (the oracle's order)
              if (bias) v += bias[row];
              out[row] = round_act(v, act);
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
    // the last workgroup of this row block to arrive turns the complete unscaled sums into the consumer's fixed-point values
    __shared__ int f8_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned old = atomicAdd(cnt + rb, 1u);
      f8_last = old == (unsigned)(SK - 1);
      if (f8_last) cnt[rb] = 0u;
    }
    __syncthreads();
    if (f8_last) {
      __threadfence();
      const int row = rb * rows_per_wg + threadIdx.x;
      if (threadIdx.x < rows_per_wg && row < N) {
        const long long a = __hip_atomic_load(accbuf + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float v = (float)(((double)a * F8_PART_INV) * (double)scale[row]);
        if (bias) v += bias[row];
        accbuf[row] = d2fix((double)v, pro.act);
      }
    }
  }
}

static int f8_rows_per_wg(int N) {
  int r = 16;
  while (r < 256 && (N + r - 1) / r > 1024) r <<= 1;    // ~1000 workgroups when N is large (each runs the prologue), at least four rows per wave
  return r;
}
// split count of an FP8 [N, K] GEMV: bzk_rows_choose_sk's rule for one-byte rows -- enough (16-row x K-slice) workgroups to fill the chip when N alone gives
// fewer than 256, a slice keeps at least four 256-byte chunks of a row (below that the prologue dominates).  From 256 row blocks on the direct form runs:
// measured on the 8B widths, the split form's hand-off (a device-scope fence per workgroup) costs more than the second workgroup per CU gains
int bzk_f8_choose_sk(int N, int K) {
  const int rbs = (N + 15) / 16, KC = (K + 255) / 256;
  if (rbs >= 256 || KC < 8) return 1;
  int sk = std::min((512 + rbs - 1) / rbs, KC / 4);
  if (sk < 2) return 1;
  const int kcs = (KC + sk - 1) / sk;
  return (KC + kcs - 1) / kcs;
}

int bzk_gemv_f8(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act) {
  if (pro.mode != PRO_PLAIN && pro.mode != PRO_NORM && pro.mode != PRO_SILU) BZ_FAIL(BZ_E_UNSUPPORTED, "fp8 gemv: prologue mode %d is not built (plain, norm, silu are)", pro.mode);
  if (pro.perm || out.amax_val || out.shift.cs) BZ_FAIL(BZ_E_UNSUPPORTED, "fp8 gemv: act-order / argmax partials / conv shift are not built");
  if (L.K % 64 || L.N % 64 || !L.scales) BZ_FAIL(BZ_E_INVALID, "fp8 gemv: N=%d K=%d must be multiples of 64, with scales", L.N, L.K);
  if (pro.mode == PRO_NORM && (pro.H != L.K || pro.H % 4)) BZ_FAIL(BZ_E_INVALID, "fp8 gemv: norm prologue over %d elements, K=%d", pro.H, L.K);
  const int KCall = (L.K + 255) / 256;
  const int SK = L.sk > 1 ? L.sk : 1;           // (more slices than chunks: the surplus slices are empty and only count)
  const char* lbl = pro.mode == PRO_NORM ? "gemv_f8<norm>" : pro.mode == PRO_SILU ? "gemv_f8<silu>" : "gemv_f8";
  static bool attr_done = false;      // a long row's activations take more than the 64 KiB a launch gets without asking
  if (!attr_done) {
    BZ_HIP(hipFuncSetAttribute((const void*)k_gemv_f8<true>, hipFuncAttributeMaxDynamicSharedMemorySize, F8_SMEM_MAX));
    BZ_HIP(hipFuncSetAttribute((const void*)k_gemv_f8<false>, hipFuncAttributeMaxDynamicSharedMemorySize, F8_SMEM_MAX));
    attr_done = true;
  }
  if (SK > 1) {
    if (!out.acc || !L.zeros) BZ_FAIL(BZ_E_INVALID, "split-K fp8 gemv needs a fixed-point accumulator and its row-block counters");
    const int KCs = (KCall + SK - 1) / SK;
    const size_t smem = (size_t)KCs * F8_XCHUNK * 4 + 64;
    if (smem > F8_SMEM_MAX) BZ_FAIL(BZ_E_UNSUPPORTED, "K=%d too large for the fp8 GEMV in %d slices", L.K, SK);
    BZ_LAUNCH(lbl, L.algo_bytes, (k_gemv_f8<true>), dim3((L.N / 16) * SK), dim3(256), smem, s, (const unsigned char*)L.w, (const float*)L.scales, L.bias, L.N, L.K, 16, pro,
              (float*)nullptr, act, out.zero_buf, out.zero_n, SK, out.acc, (unsigned*)L.zeros);
  } else {
    if (!out.direct) BZ_FAIL(BZ_E_INVALID, "fp8 gemv needs a direct output");
    const int rpw = f8_rows_per_wg(L.N);
    const size_t smem = (size_t)KCall * F8_XCHUNK * 4 + 64;
    if (smem > F8_SMEM_MAX) BZ_FAIL(BZ_E_UNSUPPORTED, "K=%d too large for the fp8 GEMV", L.K);
    BZ_LAUNCH(lbl, L.algo_bytes, (k_gemv_f8<false>), dim3((L.N + rpw - 1) / rpw), dim3(256), smem, s, (const unsigned char*)L.w, (const float*)L.scales, L.bias, L.N, L.K, rpw, pro,
              out.direct, act, out.zero_buf, out.zero_n, 1, (long long*)nullptr, (unsigned*)nullptr);
  }
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// out[n][k] = f32(s[n] e4m3(q[n][k])): the product has up to 28 significant bits, formed in double and rounded once.  Four weights per thread, through the
// conversion the GEMV and the GEMM use.
__global__ void k_dequant_f8(const unsigned* __restrict__ W, const float* __restrict__ scale, int K, size_t words, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
    const double sc = (double)scale[(i * 4) / (size_t)K];
    float f[4];
    f8x4_to_f32(W[i], f);
    *(float4*)(out + i * 4) = make_float4((float)(sc * (double)f[0]), (float)(sc * (double)f[1]), (float)(sc * (double)f[2]), (float)(sc * (double)f[3]));
  }
}
int bzk_dequant_f8(hipStream_t s, const LinearDev& L, float* out) {
  hipLaunchKernelGGL(k_dequant_f8, dim3(2048), dim3(256), 0, s, (const unsigned*)L.w, (const float*)L.scales, L.K, (size_t)L.N * L.K / 4, out);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// W8A16 GEMM on the 16-bit matrix cores: Y[S][N] = R(s[n] (X16[S][K] . e4m3(Q[N][K])^T) + b[n]).  The structure of k_gemm_nt2 (bz_prefill.hip): 128 x 128 x 64
// tiles (64 x 128 for <= 64 rows), 2 x 2 waves, both operands global -> LDS by LDS-DMA into two buffers, split-K partials summed in a fixed order.  What differs
// is the weight tile: 128 rows x 64 BYTES (8 KiB against 16: half the staging traffic), one wave-instruction fills 16 rows, the four 16-byte pieces of a row
// XOR-swizzled by (row / 4) & 3 so that the fragment reads (ds_read_b128, rows 64 bytes apart) spread over the banks.  A lane's 16 bytes are k = 32 h + 16 jj
// .. + 15 of its row: two MFMA steps' worth, expanded in registers to two f16 / bf16 fragments -- exactly, every E4M3 value being a 16-bit float.
// ---------------------------------------------------------------------------------------------------------
typedef float f8_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 f8_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f8_f16x8 __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ f8_f32x16 f8_mfma16(const uint4& a, const uint4& b, f8_f32x16 c) {
  if constexpr (DT == BZ_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(f8_bf16x8, a), __builtin_bit_cast(f8_bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f8_f16x8, a), __builtin_bit_cast(f8_f16x8, b), c, 0, 0, 0);
}
// two exact floats -> one word of two f16 / bf16 (the conversion cannot round: four significant bits, exponents inside both formats)
template <int DT> __device__ __forceinline__ unsigned f8_pack2(float a, float b) {
  if constexpr (DT == BZ_F16) return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a, b));
  else return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u);
}
// eight E4M3 bytes (two words) -> one MFMA operand fragment of eight 16-bit values
template <int DT> __device__ __forceinline__ uint4 f8_frag(unsigned w0, unsigned w1) {
  float a[4], b[4];
  f8x4_to_f32(w0, a);
  f8x4_to_f32(w1, b);
  return make_uint4(f8_pack2<DT>(a[0], a[1]), f8_pack2<DT>(a[2], a[3]), f8_pack2<DT>(b[0], b[1]), f8_pack2<DT>(b[2], b[3]));
}
// one 1 KiB LDS-DMA: lane i's 16 bytes at `gsrc` land at LDS byte address ldst + 16 i (ldst wave-uniform); inline asm for the reason given at glds16 in
// bz_prefill.hip (the builtin's alias tracking drains vmcnt per k-step).  M0 is saved and restored inside the statement.
__device__ __forceinline__ void f8_glds16(const void* gsrc, const unsigned char* ldst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(const __attribute__((address_space(3))) unsigned char*)ldst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

template <int DT, int TM>
__global__ __launch_bounds__(256) void k_gemm_f8w(const unsigned short* __restrict__ X, const unsigned char* __restrict__ W, const float* __restrict__ scale,
                                                  const float* __restrict__ bias, int S, int N, int K, int act, float* __restrict__ Y, float* __restrict__ part, int KS,
                                                  int mtiles, int ntiles) {
  constexpr int BM = 64 * TM, ABYTES = BM * 128, TILE = ABYTES + 128 * 64;
  extern __shared__ __attribute__((aligned(1024))) unsigned char f8_smem2[];   // the only LDS object of this kernel
  const int xcd = blockIdx.x & 7, jj0 = blockIdx.x >> 3;
  const int mt = jj0 % mtiles, rest = jj0 / mtiles, ks = rest % KS, nt = (rest / KS) * 8 + xcd;
  if (nt >= ntiles) return;                                  // (whole workgroup: no barrier is skipped by part of it)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = mt * BM, n0 = nt * 128;
  const int nk = K >> 6, k_beg = (int)((long long)ks * nk / KS), k_end = (int)((long long)(ks + 1) * nk / KS), nsteps = k_end - k_beg;
  // staging.  A: wave w fills row groups 2 TM w .. (8 rows x 128 B each), lane -> (row lane / 8, slot lane % 8), the slot holds piece slot ^ row.
  // B: wave w fills row groups 2 w, 2 w + 1 (16 rows x 64 B each), lane -> (row lane / 4, slot lane % 4), the slot holds piece slot ^ ((row / 4) & 3)
  const int lrow = lane >> 3, piece = (lane & 7) ^ lrow;
  const int brow = lane >> 2, bpiece = (lane & 3) ^ ((lane >> 4) & 3);
  unsigned xo[2 * TM], wo[2];                                // element / byte offsets (S K and N K < 2^32 on this path); rows past the edge are clamped, their results dropped
#pragma unroll
  for (int i = 0; i < 2 * TM; i++) xo[i] = (unsigned)min(m0 + (wave * 2 * TM + i) * 8 + lrow, S - 1) * (unsigned)K + 8u * piece;
#pragma unroll
  for (int i = 0; i < 2; i++) wo[i] = (unsigned)min(n0 + (wave * 2 + i) * 16 + brow, N - 1) * (unsigned)K + 16u * bpiece;
  auto issue = [&](int kt, int buf) {
    unsigned char* base = f8_smem2 + buf * TILE;
#pragma unroll
    for (int i = 0; i < 2 * TM; i++) f8_glds16(X + xo[i] + (size_t)kt * 64, base + (wave * 2 * TM + i) * 1024);
#pragma unroll
    for (int i = 0; i < 2; i++) f8_glds16(W + wo[i] + (size_t)kt * 64, base + ABYTES + (wave * 2 + i) * 1024);
  };
  f8_f32x16 acc[TM][2];
#pragma unroll
  for (int t = 0; t < TM; t++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][j][i] = 0.f;
  if (nsteps > 0) {
    issue(k_beg, 0);
    const int aoff = (wm * 32 * TM + r) * 128, boff = ABYTES + (wn * 64 + r) * 64, sw = r & 7, bsw = (r >> 2) & 3;
    for (int it = 0; it < nsteps; it++) {
      // this wave's pieces of tile `it` have landed; after the barrier everyone's have, and everyone is done reading the buffer the next issue overwrites
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      issue(min(k_beg + it + 1, k_end - 1), (it + 1) & 1);   // clamped: one redundant reload at the tail, never a branch around a load
      const unsigned char* tb = f8_smem2 + (it & 1) * TILE;
#pragma unroll
      for (int jj = 0; jj < 2; jj++) {
        uint4 bq[2];                                         // lane (r, h): bytes k = 32 h + 16 jj .. + 15 of rows r and 32 + r of this wave's 64
#pragma unroll
        for (int j = 0; j < 2; j++) bq[j] = *(const uint4*)(tb + boff + j * 32 * 64 + (((2 * h + jj) ^ bsw) * 16));
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
          const int sidx = 2 * jj + s2;                      // MFMA step: k = 32 h + 8 sidx .. + 7 (A and B alike)
          const int po = ((4 * h + sidx) ^ sw) * 16;
          uint4 af[TM], bf[2];
#pragma unroll
          for (int t = 0; t < TM; t++) af[t] = *(const uint4*)(tb + aoff + t * 32 * 128 + po);
#pragma unroll
          for (int j = 0; j < 2; j++) bf[j] = s2 == 0 ? f8_frag<DT>(bq[j].x, bq[j].y) : f8_frag<DT>(bq[j].z, bq[j].w);
#pragma unroll
          for (int t = 0; t < TM; t++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[t][j] = f8_mfma16<DT>(af[t], bf[j], acc[t][j]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the tail's redundant LDS-DMA lands before the LDS allocation is released
  }
  // C layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int n = n0 + wn * 64 + 32 * j + r;
    if (n < N) {
      const float sc = part ? 1.f : scale[n], bv = (!part && bias) ? bias[n] : 0.f;
#pragma unroll
      for (int t = 0; t < TM; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int m = m0 + wm * 32 * TM + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m < S) {
            if (part) part[((size_t)ks * S + m) * N + n] = acc[t][j][i];
            else Y[(size_t)m * N + n] = round_act(__fadd_rn(__fmul_rn(acc[t][j][i], sc), bv), act);
          }
        }
    }
  }
}

// split-K partials (unscaled) summed in a fixed order, then the epilogue of the unsplit form
__global__ void k_gemm_f8w_reduce(const float* __restrict__ part, int KS, size_t SN, int N, const float* __restrict__ scale, const float* __restrict__ bias, int act,
                                  float* __restrict__ Y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < SN; i += (size_t)gridDim.x * 256) {
    float v = 0.f;
    for (int z = 0; z < KS; z++) v += part[(size_t)z * SN + i];
    const int n = (int)(i % (size_t)N);
    Y[i] = round_act(__fadd_rn(__fmul_rn(v, scale[n]), bias ? bias[n] : 0.f), act);
  }
}

bool bzk_gemm_f8w_ok(const LinearDev& L, int xdt) { return L.kind == LK_F8 && (xdt == BZ_F16 || xdt == BZ_BF16) && L.K % 64 == 0 && L.K >= 64 && L.scales != nullptr; }

// dt: the 16-bit dtype of x16 (and of the expanded weight fragments); act: rounding of the output (BZ_F32: none); ws: split-K partials (optional)
int bzk_gemm_f8w(hipStream_t s, const LinearDev& L, int dt, const void* x16, int S, int act, float* y, float* ws, size_t ws_bytes) {
  const int N = L.N, K = L.K;
  if (!bzk_gemm_f8w_ok(L, dt)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_f8w: fp8 weights with K %% 64 == 0 and 16-bit activations only");
  if (S <= 0 || N <= 0) BZ_FAIL(BZ_E_INVALID, "gemm_f8w: S=%d N=%d", S, N);
  if ((unsigned long long)S * K >= (1ull << 32) || (unsigned long long)N * K >= (1ull << 32)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_f8w: operand of 2^32 elements or more");
  const double flops = 2.0 * S * (double)N * K;
  // tiles and split as bzk_gemm_nt chooses them
  const int TM = S <= 64 ? 1 : 2, BM = 64 * TM;
  const int mtiles = (S + BM - 1) / BM, ntiles = (N + 127) / 128, nk = K / 64;
  const long long tiles = (long long)mtiles * ntiles;
  int KS = 1;
  if (ws) {
    while (KS * 2 * tiles <= 320 && KS * 2 <= nk / 2 && KS < 16 && (size_t)KS * 2 * S * N * 4 <= ws_bytes) KS *= 2;
  }
  float* part = KS > 1 ? ws : nullptr;
  const unsigned grid = 8u * (unsigned)((ntiles + 7) / 8) * (unsigned)mtiles * (unsigned)KS;
#define LAUNCH_F8W(DT, M) BZ_LAUNCH("gemm_f8w_mfma", flops, (k_gemm_f8w<DT, M>), dim3(grid), dim3(256), 2 * (64 * M * 128 + 128 * 64), s, (const unsigned short*)x16, \
    (const unsigned char*)L.w, (const float*)L.scales, L.bias, S, N, K, act, y, part, KS, mtiles, ntiles)
  if (dt == BZ_F16) { if (TM == 1) LAUNCH_F8W(BZ_F16, 1); else LAUNCH_F8W(BZ_F16, 2); }
  else { if (TM == 1) LAUNCH_F8W(BZ_BF16, 1); else LAUNCH_F8W(BZ_BF16, 2); }
#undef LAUNCH_F8W
  BZ_HIP(hipGetLastError());
  if (KS > 1) {
    const size_t SN = (size_t)S * N;
    hipLaunchKernelGGL(k_gemm_f8w_reduce, dim3((unsigned)std::min<size_t>((SN + 255) / 256, 2048)), dim3(256), 0, s, (const float*)ws, KS, SN, N, (const float*)L.scales, L.bias, act, y);
    BZ_HIP(hipGetLastError());
  }
  return BZ_OK;
}
