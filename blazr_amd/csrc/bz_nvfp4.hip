// bz_nvfp4.hip -- NVFP4 weights (compressed-tensors `nvfp4-pack-quantized`), W4A16: E2M1 codes in groups of 16 along K with one E4M3 scale per group and one f32
// factor per tensor, 16-bit activations.
//
//   W[n][k] = e2m1(q[n][k]) e4m3(s[n][k / 16]) r[n]        y[n] = R_act( f32( r[n] sum_k x[k] e2m1(q[n][k]) e4m3(s[n][k / 16]) ) + b[n] )
//
// r[n] = f32(1 / weight_global_scale) of the part row n came from (parts fused along N keep their own), an f32 [N] array beside the tiles.  It never enters an
// inner loop: both kernels apply it once to a row's finished sum.
//
// What the group scale allows.  An E2M1 magnitude (0, 0.5, 1, 1.5, 2, 3, 4, 6) has two significant bits, an E4M3 magnitude (sign clear, NaN refused when a
// tensor is added) at most four, so c = e2m1 . e4m3 has at most six; the largest is 6 . 448 = 2688, the smallest nonzero 0.5 . 2^-9 = 2^-10: c is EXACT and
// normal in f16 (eleven bits) and in bf16 (eight).  The GEMM therefore builds scaled 16-bit fragments and leaves the whole sum to the matrix cores -- no
// multiply-add on partial tiles and no double accumulators (what k_gemm_mx4w pays for E8M0 scales that f16 cannot hold).  The GEMV keeps the exact-sum
// contract: x . e2m1 is exact in f32; a group's sixteen products are summed in double and the group's sum is multiplied by its scale in double -- one multiply
// per GROUP, not per weight.  That keeps the bar because the multiply is a double operation like the adds around it: the scale has four significant bits,
// so the product is exact unless the group's sum needs more than 49, and then it is off by 2^-53 of its magnitude, as any of the row's K adds may be --
// against the 2^-24 of the one rounding to f32 that the row's value gets.
//
// Device layout (bzk_repack_nv4, at finalize): tiles of FOUR ROWS x 512 k, NV4_TILE = 1152 bytes each, [N / 4][ceil(K / 512)] of them.  A tile is what one
// wave consumes per GEMV step: 64 pieces of 16 bytes -- piece l holds the 32 codes of row l / 16, k 32 (l % 16) .. + 31 of the tile, in file order (byte j: low
// nibble element 2 j, high nibble element 2 j + 1) -- followed by the 64 PAIRS of scale bytes of those pieces in the same order (first the group of elements
// 0 .. 15).  A wave-wide 16-byte load and a wave-wide 2-byte load read one contiguous 1152-byte run; the four scale bytes of a row's 64 k are one aligned
// word, which is what the GEMM stages.  K % 512 != 0 pads the last tile of a row with code 0 and scale 0: the padding adds exact zeros.
//
//   k_gemv_nv4     decode GEMV, direct output; the four waves of a workgroup split K tile by tile and their partial sums meet in LDS in a fixed order
//   k_gemm_nv4w    prompt / decode-batch GEMM on the 16-bit matrix cores: code tiles and scale words staged by LDS-DMA, expanded to scaled fragments
//   k_dequant_nv4  op-level read-back of the device layout
#include "bz_internal.h"
#include "bz_dev.h"
#include <algorithm>

#define NV4_TILE 1152                         // bytes of a 4-row x 512-k tile: 1024 code bytes + 128 scale bytes
#define NV4_XCHUNK 640                        // LDS floats per 512-k chunk (xs_pos<2>)
#define NV4_SMEM_MAX (152 * 1024)             // dynamic LDS a launch may ask for

typedef _Float16 nv4_h2 __attribute__((ext_vector_type(2)));

// Elements j and j + 4 (j = 0..3) of an eight-code word as two f16 holding the E2M1 values.  The three magnitude bits of a code, placed at bits 9..11 of an
// f16, read e2m1 . 2^-14 (an f16 subnormal for codes 0 and 1), the sign bit goes to bit 15; a packed multiply by 2^14 (exact; f16 subnormals are kept in every
// kernel mode hipcc builds) gives the values.  This is the one place that reads the nibble order.
__device__ __forceinline__ nv4_h2 nv4_pair(unsigned w, int j) {
  const unsigned mag = (j < 3 ? w << (9 - 4 * j) : w >> 3) & 0x0E000E00u;
  const nv4_h2 k = {(_Float16)16384.0f, (_Float16)16384.0f};
  return __builtin_bit_cast(nv4_h2, mag | ((w << (12 - 4 * j)) & 0x80008000u)) * k;
}
// An admitted E4M3 scale byte b (sign clear, not 0x7F): b << 7 is the f16 holding e4m3(b) . 2^-8 -- the four exponent bits land in f16's five, the bias moves
// from 7 to 15, and an E4M3 subnormal lands on an f16 normal or subnormal of the same ratio.  Times 2^8: the scale itself, exact, in both halves / as a double.
__device__ __forceinline__ nv4_h2 nv4_scale_h2(unsigned b) {
  const nv4_h2 k = {(_Float16)256.0f, (_Float16)256.0f};
  return __builtin_bit_cast(nv4_h2, (b << 7) | (b << 23)) * k;
}
__device__ __forceinline__ double nv4_scale_d(unsigned b) { return (double)((float)__builtin_bit_cast(_Float16, (unsigned short)(b << 7)) * 256.f); }

// ---------------------------------------------------------------------------------------------------------
// load-time repack: file layout (codes [N][K / 2], scales [N][K / 16]) -> tiles.  One thread per piece.
// ---------------------------------------------------------------------------------------------------------
__global__ void k_repack_nv4(const unsigned char* __restrict__ q, const unsigned char* __restrict__ sc, int N, int K, int KC, unsigned char* __restrict__ out) {
  const size_t total = (size_t)(N / 4) * KC * 64;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 63);
    const size_t t = idx >> 6;
    const int row = (int)(t / (size_t)KC) * 4 + (l >> 4), k0 = (int)(t % (size_t)KC) * 512 + (l & 15) * 32;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    unsigned short s = 0;
    if (k0 < K) {                             // (K % 64 == 0: a piece is inside the row or wholly beyond it)
      v = *(const uint4*)(q + (size_t)row * (K / 2) + k0 / 2);
      s = *(const unsigned short*)(sc + (size_t)row * (K / 16) + k0 / 16);
    }
    *(uint4*)(out + t * NV4_TILE + l * 16) = v;
    *(unsigned short*)(out + t * NV4_TILE + 1024 + l * 2) = s;
  }
}
size_t bzk_nv4_bytes(int N, int K) { return (size_t)(N / 4) * ((K + 511) / 512) * NV4_TILE; }
// rows [0, N) of `q` / `sc` -> the tiles at `out` (the caller has offset `out` to the part's first row group)
int bzk_repack_nv4(hipStream_t s, const void* q, const void* sc, int N, int K, void* out) {
  const int KC = (K + 511) / 512;
  const size_t total = (size_t)(N / 4) * KC * 64;
  hipLaunchKernelGGL(k_repack_nv4, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, (const unsigned char*)q, (const unsigned char*)sc, N, K, KC,
                     (unsigned char*)out);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// decode GEMV.  256 threads own rows_per_wg rows (a multiple of four); the workgroup walks them four at a time (row = lane / 16) and SPLITS K OVER ITS WAVES:
// wave w takes the tiles w, w + 4, .. of every row group, so all four waves stream one row group's bytes side by side and a short linear (K = 4096: eight
// tiles) still gives every wave work.  Per step a wave reads one tile (a 16-byte and a 2-byte load per lane), two buffers of four steps in flight.  x sits in
// LDS as f32, zero beyond K, padded by four floats after every sixteen (xs_pos<2>): a lane's 32 activations are eight float4 reads.  A lane sums each of its two
// groups' sixteen exact products in four double chains, scales the group's sum by its E4M3 scale in double and adds it to its row sum; a DPP reduction over
// sixteen lanes ends a wave's share of a row group, which goes to LDS as a double.  After one barrier a thread per row adds the four waves' shares in the order
// (0 + 1) + (2 + 3), multiplies by r[n] in double, rounds to f32 once and adds the bias in f32 (the oracle's order).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gemv_nv4(const unsigned char* __restrict__ W, const float* __restrict__ rs, const float* __restrict__ bias, int N, int K, int rows_per_wg,
                                                  Pro pro, float* __restrict__ out, int act, long long* zero_buf, int zero_n) {
  extern __shared__ __attribute__((aligned(16))) char nv4_smem[];
  float* xs = (float*)nv4_smem;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, sub = lane >> 4, l16 = lane & 15;
  const int bid = blockIdx.x;
  const int rbeg = bid * rows_per_wg, rend = min(rbeg + rows_per_wg, N);        // (multiples of 4: N % 64 == 0)
  const int KC = (K + 511) >> 9;
  float* red = xs + KC * NV4_XCHUNK;            // [16]
  double* part = (double*)(red + 16);           // [4 waves][rows_per_wg]
  const int ngroups = (rend - rbeg) >> 2;
  const int kc0 = min(wave, KC - 1), nkw = wave < KC ? (KC - wave + 3) >> 2 : 0;   // this wave's first tile and how many of a row group's it takes
  const int nsteps = ngroups * nkw;
  // issue cursor (clamped at the last step: a few redundant loads at the tail -- for a wave without a share, of tile KC - 1 -- never a branch around a load)
  int ig = 0, ikc = kc0, ist = 0;
  auto issue = [&](uint4 (&q)[4], unsigned (&sc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int g = min((rbeg >> 2) + ig, (N >> 2) - 1);
      const unsigned char* t = W + ((size_t)g * KC + ikc) * NV4_TILE;
      q[j] = ldnt((const uint4*)(t + lane * 16));
      sc[j] = *(const unsigned short*)(t + 1024 + lane * 2);
      if (ist + 1 < nsteps) { ist++; ikc += 4; if (ikc >= KC) { ikc = kc0; ig++; } }
    }
  };
  uint4 q0[4], q1[4];
  unsigned s0[4], s1[4];
  issue(q0, s0);
  __builtin_amdgcn_sched_barrier(0);
  if (zero_buf)                                 // the ring protocol's side duty: zero the buffer the NEXT accumulate launch adds into
    for (int i = bid * 256 + threadIdx.x; i < zero_n; i += gridDim.x * 256) zero_buf[i] = 0;
  for (int i = lane; i < rows_per_wg; i += 64) part[wave * rows_per_wg + i] = 0.0;   // (a wave without a share of K, rows past rend; the wave's own stores follow in order)
  for (int i = K + threadIdx.x; i < KC * 512; i += 256) xs[xs_pos<2>(i)] = 0.f;
  build_x_simple<2>(pro, 0, K, xs, red, bid == 0);
  double acc = 0.0;
  int cg = 0, ckc = kc0, cst = 0;
  auto consume = [&](const uint4 (&q)[4], const unsigned (&sc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (cst < nsteps) {
        cst++;
        const float4* xp = (const float4*)(xs + ckc * NV4_XCHUNK + l16 * 40);
        const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int g = 0; g < 2; g++) {           // group g: elements 16 g .. 16 g + 15 of the piece, words 2 g and 2 g + 1
          double b[4] = {0.0, 0.0, 0.0, 0.0};   // exact products, double sums
#pragma unroll
          for (int d = 2 * g; d < 2 * g + 2; d++) {
            const float4 xa = xp[2 * d + g], xb = xp[2 * d + g + 1];
            const float xl[4] = {xa.x, xa.y, xa.z, xa.w}, xh[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const nv4_h2 p = nv4_pair(w[d], e);
              b[e] += (double)__fmul_rn((float)p.x, xl[e]);
              b[e] += (double)__fmul_rn((float)p.y, xh[e]);
            }
          }
          acc += ((b[0] + b[1]) + (b[2] + b[3])) * nv4_scale_d((sc[j] >> (8 * g)) & 0xffu);
        }
        ckc += 4;
        if (ckc >= KC) {
          ckc = kc0;
          const double vd = grp_sum_d<16>(acc);
          acc = 0.0;
          if (l16 == 0) part[wave * rows_per_wg + cg * 4 + sub] = vd;
          cg++;
        }
      }
    }
  };
  for (int st = 0; st < nsteps; st += 8) {
    issue(q1, s1); consume(q0, s0);
    issue(q0, s0); consume(q1, s1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < rend - rbeg; i += 256) {
    const int row = rbeg + i;
    const double vd = (part[i] + part[rows_per_wg + i]) + (part[2 * rows_per_wg + i] + part[3 * rows_per_wg + i]);
    float v = (float)(vd * (double)rs[row]);    // one rounding to f32, then the bias in f32
    if (bias) v += bias[row];
    out[row] = round_act(v, act);
  }
}

static int nv4_rows_per_wg(int N) {
  int r = 16;
  while (r < 256 && (N + r - 1) / r > 1024) r <<= 1;    // ~1000 workgroups when N is large (each runs the prologue)
  return r;
}

int bzk_gemv_nv4(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act) {
  if (pro.mode != PRO_PLAIN && pro.mode != PRO_NORM && pro.mode != PRO_SILU) BZ_FAIL(BZ_E_UNSUPPORTED, "nvfp4 gemv: prologue mode %d is not built (plain, norm, silu are)", pro.mode);
  if (pro.perm || out.amax_val || out.shift.cs) BZ_FAIL(BZ_E_UNSUPPORTED, "nvfp4 gemv: act-order / argmax partials / conv shift are not built");
  if (L.K % 64 || L.N % 64 || !L.w || !L.scales) BZ_FAIL(BZ_E_INVALID, "nvfp4 gemv: N=%d K=%d must be multiples of 64", L.N, L.K);
  if (pro.mode == PRO_NORM && (pro.H != L.K || pro.H % 4)) BZ_FAIL(BZ_E_INVALID, "nvfp4 gemv: norm prologue over %d elements, K=%d", pro.H, L.K);
  if (!out.direct) BZ_FAIL(BZ_E_INVALID, "nvfp4 gemv needs a direct output");
  const int KC = (L.K + 511) / 512;
  const char* lbl = pro.mode == PRO_NORM ? "gemv_nv4<norm>" : pro.mode == PRO_SILU ? "gemv_nv4<silu>" : "gemv_nv4";
  static bool attr_done = false;      // a long row's activations take more than the 64 KiB a launch gets without asking
  if (!attr_done) {
    BZ_HIP(hipFuncSetAttribute((const void*)k_gemv_nv4, hipFuncAttributeMaxDynamicSharedMemorySize, NV4_SMEM_MAX));
    attr_done = true;
  }
  const int rpw = nv4_rows_per_wg(L.N);
  const size_t smem = (size_t)KC * NV4_XCHUNK * 4 + 64 + (size_t)4 * rpw * 8;
  if (smem > NV4_SMEM_MAX) BZ_FAIL(BZ_E_UNSUPPORTED, "K=%d too large for the nvfp4 GEMV", L.K);
  BZ_LAUNCH(lbl, L.algo_bytes, (k_gemv_nv4), dim3((L.N + rpw - 1) / rpw), dim3(256), smem, s, (const unsigned char*)L.w, (const float*)L.scales, L.bias, L.N, L.K, rpw, pro, out.direct,
            act, out.zero_buf, out.zero_n);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// out[n][k] = f32(e2m1(q[n][k]) e4m3(s) r[n]), formed in double and rounded once, through the expansion the GEMV and the GEMM use.  One thread per piece.
__global__ void k_dequant_nv4(const unsigned char* __restrict__ W, const float* __restrict__ rs, int N, int K, int KC, float* __restrict__ out) {
  const size_t total = (size_t)(N / 4) * KC * 64;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 63);
    const size_t t = idx >> 6;
    const int row = (int)(t / (size_t)KC) * 4 + (l >> 4), k0 = (int)(t % (size_t)KC) * 512 + (l & 15) * 32;
    if (k0 >= K) continue;
    const uint4 q = *(const uint4*)(W + t * NV4_TILE + l * 16);
    const unsigned s = *(const unsigned short*)(W + t * NV4_TILE + 1024 + l * 2);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    float* o = out + (size_t)row * K + k0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const nv4_h2 sh = nv4_scale_h2((s >> (8 * (d >> 1))) & 0xffu);
      const double r = (double)rs[row];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const nv4_h2 p = nv4_pair(w[d], e) * sh;          // the GEMM's scaled f16 values (exact)
        o[8 * d + e] = (float)(r * (double)(float)p.x);
        o[8 * d + e + 4] = (float)(r * (double)(float)p.y);
      }
    }
  }
}
int bzk_dequant_nv4(hipStream_t s, const LinearDev& L, float* out) {
  const int KC = (L.K + 511) / 512;
  hipLaunchKernelGGL(k_dequant_nv4, dim3(2048), dim3(256), 0, s, (const unsigned char*)L.w, (const float*)L.scales, L.N, L.K, KC, out);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// W4A16 GEMM on the 16-bit matrix cores: Y[S][N] = R(r[n] (X16[S][K] . C[N][K]^T) + b[n]), C = e2m1 . e4m3.  The frame of k_gemm_f8w / k_gemm_mx4w: 128 x 128 x 64
// tiles (64 x 128 for <= 64 rows), 2 x 2 waves, operands global -> LDS by LDS-DMA into two buffers, split-K partials summed in a fixed order.  Per 64-k step
// the weight side of a buffer is 128 rows x 32 BYTES of codes (4 KiB; one wave-instruction fills 32 rows, each lane fetching one 16-byte piece from its place
// in the device tiles) and 128 rows x 4 scale BYTES (512 B; waves 0 and 1 fill 64 rows each with one 4-byte LDS-DMA per lane: the four scales of a row's 64 k
// are one aligned word of the tile).  The MFMA sums over both halves of the wave, so a step's k is laid out with both halves inside ONE GROUP: MFMA step sidx
// covers k = 16 sidx + 8 h .. + 7 (h = lane / 32) -- exactly the group of scale byte sidx.  A lane expands a word of eight codes to eight f16 values, multiplies
// them by the group's scale as packed f16 (exact, see the head of the file) and, for bf16 models, takes the upper halves of their f32 forms (exact: six bits).
// The f32 accumulators of the MFMA are all there is: 32 TM registers, so the kernel fits two waves per SIMD with room to spare.  r[n] and the bias are applied
// in the epilogue (the result column of a lane is one n), or by the reduce kernel when K is split.
// ---------------------------------------------------------------------------------------------------------
typedef float nv4_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 nv4_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 nv4_f16x8 __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ nv4_f32x16 nv4_mfma16(const uint4& a, const uint4& b, nv4_f32x16 c) {
  if constexpr (DT == BZ_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(nv4_bf16x8, a), __builtin_bit_cast(nv4_bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(nv4_f16x8, a), __builtin_bit_cast(nv4_f16x8, b), c, 0, 0, 0);
}
// eight codes (one word) and their group's scale -> one MFMA operand fragment of eight scaled 16-bit values in element order
template <int DT> __device__ __forceinline__ uint4 nv4_frag(unsigned w, nv4_h2 sc) {
  nv4_h2 p[4];
#pragma unroll
  for (int e = 0; e < 4; e++) p[e] = nv4_pair(w, e) * sc;     // (element e, element e + 4)
  if constexpr (DT == BZ_F16) {
    unsigned u[4];
#pragma unroll
    for (int e = 0; e < 4; e++) u[e] = __builtin_bit_cast(unsigned, p[e]);
    return make_uint4((u[0] & 0xffffu) | (u[1] << 16), (u[2] & 0xffffu) | (u[3] << 16), (u[0] >> 16) | (u[1] & 0xffff0000u), (u[2] >> 16) | (u[3] & 0xffff0000u));
  } else {
    auto pk = [](float a, float b) { return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u); };
    return make_uint4(pk((float)p[0].x, (float)p[1].x), pk((float)p[2].x, (float)p[3].x), pk((float)p[0].y, (float)p[1].y), pk((float)p[2].y, (float)p[3].y));
  }
}
// LDS-DMA: lane i's 16 (4) bytes at `gsrc` land at LDS byte address ldst + 16 i (+ 4 i), ldst wave-uniform; see f8_glds16 (bz_fp8.hip) and glds16 (bz_prefill.hip)
__device__ __forceinline__ void nv4_glds16(const void* gsrc, const unsigned char* ldst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(const __attribute__((address_space(3))) unsigned char*)ldst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}
__device__ __forceinline__ void nv4_glds4(const void* gsrc, const unsigned char* ldst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(const __attribute__((address_space(3))) unsigned char*)ldst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

template <int DT, int TM>
__global__ __launch_bounds__(256, 2) void k_gemm_nv4w(const unsigned short* __restrict__ X, const unsigned char* __restrict__ W, const float* __restrict__ rs,
                                                      const float* __restrict__ bias, int S, int N, int K, int act, float* __restrict__ Y, float* __restrict__ part, int KS,
                                                      int mtiles, int ntiles) {
  constexpr int BM = 64 * TM, ABYTES = BM * 128, CBYTES = 128 * 32, TILE = ABYTES + CBYTES + 128 * 4;
  extern __shared__ __attribute__((aligned(1024))) unsigned char nv4_smem2[];   // the only LDS object of this kernel
  const int xcd = blockIdx.x & 7, jj0 = blockIdx.x >> 3;
  const int mt = jj0 % mtiles, rest = jj0 / mtiles, ks = rest % KS, nt = (rest / KS) * 8 + xcd;
  if (nt >= ntiles) return;                                  // (whole workgroup: no barrier is skipped by part of it)
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = mt * BM, n0 = nt * 128;
  const int KC = (K + 511) >> 9;
  const int nk = K >> 6, k_beg = (int)((long long)ks * nk / KS), k_end = (int)((long long)(ks + 1) * nk / KS), nsteps = k_end - k_beg;
  // staging.  A: wave w fills row groups 2 TM w .. (8 rows x 128 B each), lane -> (row lane / 8, slot lane % 8), the slot holds piece slot ^ row.
  // codes: wave w fills rows 32 w .. 32 w + 31 (32 B each), lane -> (row lane / 2, piece lane % 2).  scales: wave w < 2 fills rows 64 w .. 64 w + 63 (4 B each)
  const int lrow = lane >> 3, piece = (lane & 7) ^ lrow;
  unsigned xo[2 * TM];                                       // element offsets (S K < 2^32 on this path); rows past the edge are clamped, their results dropped
#pragma unroll
  for (int i = 0; i < 2 * TM; i++) xo[i] = (unsigned)min(m0 + (wave * 2 * TM + i) * 8 + lrow, S - 1) * (unsigned)K + 8u * piece;
  // byte offset of (row n, k) in the device tiles: ((n / 4) KC + k / 512) NV4_TILE + ((n % 4) 16 + (k % 512) / 32) 16; the two scale bytes of that piece sit at
  // ... NV4_TILE + 1024 + ((n % 4) 16 + (k % 512) / 32) 2.  Rows past N (a 128-row tile over N % 128 == 64) are clamped, their results dropped.
  auto row_base = [&](int n, int per_piece) { n = min(n, N - 1); return (size_t)(n >> 2) * KC * NV4_TILE + (size_t)(n & 3) * 16 * per_piece; };
  const size_t wb = row_base(n0 + wave * 32 + (lane >> 1), 16) + (size_t)(lane & 1) * 16;
  const size_t sb = row_base(n0 + (wave & 1) * 64 + lane, 2) + 1024;
  auto issue = [&](int kt, int buf) {
    unsigned char* base = nv4_smem2 + buf * TILE;
    const int k = kt * 64;
    const size_t to = (size_t)(k >> 9) * NV4_TILE;
    const int pc = (k & 511) >> 5;                           // (even: a step is two pieces, four scale bytes)
#pragma unroll
    for (int i = 0; i < 2 * TM; i++) nv4_glds16(X + xo[i] + (size_t)kt * 64, base + (wave * 2 * TM + i) * 1024);
    nv4_glds16(W + wb + to + (size_t)pc * 16, base + ABYTES + wave * 1024);
    if (wave < 2) nv4_glds4(W + sb + to + (size_t)pc * 2, base + ABYTES + CBYTES + wave * 256);
  };
  nv4_f32x16 acc[TM][2];
#pragma unroll
  for (int t = 0; t < TM; t++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][j][i] = 0.f;
  if (nsteps > 0) {
    issue(k_beg, 0);
    const int aoff = (wm * 32 * TM + r) * 128, boff = ABYTES + (wn * 64 + r) * 32, soff = ABYTES + CBYTES + (wn * 64 + r) * 4, sw = r & 7;
    for (int it = 0; it < nsteps; it++) {
      // this wave's pieces of tile `it` have landed; after the barrier everyone's have, and everyone is done reading the buffer the next issue overwrites
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      issue(min(k_beg + it + 1, k_end - 1), (it + 1) & 1);   // clamped: one redundant reload at the tail, never a branch around a load
      const unsigned char* tb = nv4_smem2 + (it & 1) * TILE;
      // the 32 code bytes and the four scale bytes of rows r (x0) and 32 + r (x1) of this wave's 64
      const uint4 b00 = *(const uint4*)(tb + boff), b01 = *(const uint4*)(tb + boff + 16);
      const uint4 b10 = *(const uint4*)(tb + boff + 32 * 32), b11 = *(const uint4*)(tb + boff + 32 * 32 + 16);
      const unsigned sc0 = *(const unsigned*)(tb + soff), sc1 = *(const unsigned*)(tb + soff + 32 * 4);
#pragma unroll
      for (int sidx = 0; sidx < 4; sidx++) {
        // MFMA step sidx: k = 16 sidx + 8 h .. + 7 -- piece 2 sidx + h of an A row, word 2 (sidx % 2) + h of code piece sidx / 2, scale byte sidx
        const int po = ((2 * sidx + h) ^ sw) * 16;
        uint4 af[TM], bf[2];
#pragma unroll
        for (int t = 0; t < TM; t++) af[t] = *(const uint4*)(tb + aoff + t * 32 * 128 + po);
        const uint4 q0 = sidx >> 1 ? b01 : b00, q1 = sidx >> 1 ? b11 : b10;
        bf[0] = nv4_frag<DT>((sidx & 1) == 0 ? (h ? q0.y : q0.x) : (h ? q0.w : q0.z), nv4_scale_h2((sc0 >> (8 * sidx)) & 0xffu));
        bf[1] = nv4_frag<DT>((sidx & 1) == 0 ? (h ? q1.y : q1.x) : (h ? q1.w : q1.z), nv4_scale_h2((sc1 >> (8 * sidx)) & 0xffu));
#pragma unroll
        for (int t = 0; t < TM; t++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[t][j] = nv4_mfma16<DT>(af[t], bf[j], acc[t][j]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the tail's redundant LDS-DMA lands before the LDS allocation is released
  }
  // C layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int n = n0 + wn * 64 + 32 * j + r;
    if (n < N) {
      const float rn = part ? 1.f : rs[n], bv = (!part && bias) ? bias[n] : 0.f;
#pragma unroll
      for (int t = 0; t < TM; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int m = m0 + wm * 32 * TM + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m < S) {
            if (part) part[((size_t)ks * S + m) * N + n] = acc[t][j][i];
            else Y[(size_t)m * N + n] = round_act(__fadd_rn(__fmul_rn(acc[t][j][i], rn), bv), act);
          }
        }
    }
  }
}

// split-K partials summed in a fixed order (the workspace convention of k_gemm_mx4w_reduce), r[n] applied to the sum, then the epilogue of the unsplit form
__global__ void k_gemm_nv4w_reduce(const float* __restrict__ part, int KS, size_t SN, int N, const float* __restrict__ rs, const float* __restrict__ bias, int act,
                                   float* __restrict__ Y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < SN; i += (size_t)gridDim.x * 256) {
    const int n = (int)(i % (size_t)N);
    double v = 0.0;                      // (the partials are f32; their sum is rounded once, with r)
    for (int z = 0; z < KS; z++) v += (double)part[(size_t)z * SN + i];
    Y[i] = round_act(__fadd_rn((float)(v * (double)rs[n]), bias ? bias[n] : 0.f), act);
  }
}

bool bzk_gemm_nv4w_ok(const LinearDev& L, int xdt) {
  return L.kind == LK_NV4 && (xdt == BZ_F16 || xdt == BZ_BF16) && L.K % 64 == 0 && L.K >= 64 && L.N % 64 == 0 && L.w != nullptr && L.scales != nullptr;
}

// dt: the 16-bit dtype of x16 (and of the expanded weight fragments); act: rounding of the output (BZ_F32: none); ws: split-K partials (optional)
int bzk_gemm_nv4w(hipStream_t s, const LinearDev& L, int dt, const void* x16, int S, int act, float* y, float* ws, size_t ws_bytes) {
  const int N = L.N, K = L.K;
  if (!bzk_gemm_nv4w_ok(L, dt)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_nv4w: nvfp4 weights with K %% 64 == 0 and 16-bit activations only");
  if (S <= 0 || N <= 0) BZ_FAIL(BZ_E_INVALID, "gemm_nv4w: S=%d N=%d", S, N);
  if ((unsigned long long)S * K >= (1ull << 32) || (unsigned long long)N * K >= (1ull << 32)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_nv4w: operand of 2^32 elements or more");
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
#define LAUNCH_NV4W(DT, M) BZ_LAUNCH("gemm_nv4w_mfma", flops, (k_gemm_nv4w<DT, M>), dim3(grid), dim3(256), 2 * (64 * M * 128 + 128 * 32 + 128 * 4), s, (const unsigned short*)x16, \
    (const unsigned char*)L.w, (const float*)L.scales, L.bias, S, N, K, act, y, part, KS, mtiles, ntiles)
  if (dt == BZ_F16) { if (TM == 1) LAUNCH_NV4W(BZ_F16, 1); else LAUNCH_NV4W(BZ_F16, 2); }
  else { if (TM == 1) LAUNCH_NV4W(BZ_BF16, 1); else LAUNCH_NV4W(BZ_BF16, 2); }
#undef LAUNCH_NV4W
  BZ_HIP(hipGetLastError());
  if (KS > 1) {
    const size_t SN = (size_t)S * N;
    hipLaunchKernelGGL(k_gemm_nv4w_reduce, dim3((unsigned)std::min<size_t>((SN + 255) / 256, 2048)), dim3(256), 0, s, (const float*)ws, KS, SN, N, (const float*)L.scales, L.bias, act, y);
    BZ_HIP(hipGetLastError());
  }
  return BZ_OK;
}
