// bz_mxfp4.hip -- OCP microscaling FP4 weights (MXFP4), W4A16: E2M1 codes in blocks of 32 along K with one E8M0 scale per block, 16-bit activations.
//
//   W[n][k] = 2^(s[n][k / 32] - 127) e2m1(q[n][k])        y[n] = R_act( f32( sum_k x[k] W[n][k] ) + b[n] )
//
// E2M1 (codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign) has two significant bits, so every product x e2m1(q) with a 16-bit x is exact in f32 and a
// block's power-of-two scale moves exponents only: the decode kernel sums the UNSCALED products of a block in double and multiplies the block's sum by its
// scale as a double -- exact, so the row's value is the double sum of the exact products x W, rounded to f32 once, as the dense rows kernels and k_gemv_f8
// carry theirs.  Scale codes 253 .. 255 are refused when a tensor is added (255 is NaN, 253 and 254 take 6 . 2^(s - 127) out of f32).
//
// Device layout (bzk_repack_mx4, at finalize): tiles of FOUR ROWS x 512 k, MX4_TILE = 1088 bytes each, [N / 4][ceil(K / 512)] of them.  A tile is what one wave
// consumes per step: 64 pieces of 16 bytes -- piece l holds the 32 codes of row l / 16, block l % 16 of the tile, in file order (byte j: low nibble element
// 2 j, high nibble element 2 j + 1) -- followed by the 64 scale bytes of those pieces in the same order.  A wave-wide 16-byte load and a wave-wide byte load
// read one contiguous 1088-byte run; a lane gets exactly one block and its scale, so no lane ever shares or shuffles a scale.  K % 512 != 0 pads the last
// tile of a row with code 0 (+0) and scale 127: the padding adds exact zeros.
//
//   k_gemv_mx4     decode GEMV, direct output (K is never split: block scales differ along K, so there is no common unit for fixed-point partials)
//   k_gemm_mx4w    prompt / decode-batch GEMM on the 16-bit matrix cores: code tiles staged by LDS-DMA, expanded to UNSCALED f16 / bf16 fragments in registers,
//                  one f32 multiply-add per block applies the scale to the block's 32 x 32 partial tile
//   k_dequant_mx4  op-level read-back of the device layout
#include "bz_internal.h"
#include "bz_dev.h"
#include <algorithm>

#define MX4_TILE 1088                         // bytes of a 4-row x 512-k tile: 1024 code bytes + 64 scale bytes
#define MX4_XCHUNK 640                        // LDS floats per 512-k chunk (xs_pos<2>)
#define MX4_SMEM_MAX (152 * 1024)             // dynamic LDS a launch may ask for
#define MX4_FOLD 2                            // GEMM: 64-k steps between two folds of the f32 accumulators into the double ones (a power of two)

typedef _Float16 mx4_h2 __attribute__((ext_vector_type(2)));

// Elements j and j + 4 (j = 0..3) of an eight-code word as the bit patterns of two f16 holding e2m1 . 2^-14: the three magnitude bits of a code, placed at
// bits 9..11 of an f16, read (1 + m0 / 2) 2^(e - 15) for e = code >> 1 > 0 and m0 2^-15 for e = 0 (an f16 subnormal) -- the E2M1 table times 2^-14 -- and
// the sign bit goes to bit 15.  Both elements take the same shifts, so a pair costs four operations.
__host__ __device__ __forceinline__ unsigned mx4_pair_bits(unsigned w, int j) {
  const unsigned mag = (j < 3 ? w << (9 - 4 * j) : w >> 3) & 0x0E000E00u;
  return mag | ((w << (12 - 4 * j)) & 0x80008000u);
}
// ... and as two f16 holding the E2M1 values themselves (a packed multiply by 2^14: exact, f16 subnormals are kept in every kernel mode hipcc builds)
__device__ __forceinline__ mx4_h2 mx4_pair(unsigned w, int j) {
  const mx4_h2 k = {(_Float16)16384.0f, (_Float16)16384.0f};
  return __builtin_bit_cast(mx4_h2, mx4_pair_bits(w, j)) * k;
}
// 2^(c - 127) as a double (any code) and as a float (code 0 is the f32 subnormal 2^-127)
__device__ __forceinline__ double mx4_scale_d(unsigned c) { return __hiloint2double((int)((c + 896u) << 20), 0); }
__device__ __forceinline__ float mx4_scale_f(unsigned c) { return __uint_as_float(c ? c << 23 : 0x00400000u); }

// ---------------------------------------------------------------------------------------------------------
// load-time repack: file layout (codes [N][K / 2], scales [N][K / 32]) -> tiles.  One thread per piece.
// ---------------------------------------------------------------------------------------------------------
__global__ void k_repack_mx4(const unsigned char* __restrict__ q, const unsigned char* __restrict__ sc, int N, int K, int KC, unsigned char* __restrict__ out) {
  const size_t total = (size_t)(N / 4) * KC * 64;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 63);
    const size_t t = idx >> 6;
    const int row = (int)(t / (size_t)KC) * 4 + (l >> 4), k0 = (int)(t % (size_t)KC) * 512 + (l & 15) * 32;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    unsigned char s = 127;
    if (k0 < K) {
      v = *(const uint4*)(q + (size_t)row * (K / 2) + k0 / 2);
      s = sc[(size_t)row * (K / 32) + k0 / 32];
    }
    *(uint4*)(out + t * MX4_TILE + l * 16) = v;
    out[t * MX4_TILE + 1024 + l] = s;
  }
}
size_t bzk_mx4_bytes(int N, int K) { return (size_t)(N / 4) * ((K + 511) / 512) * MX4_TILE; }
// rows [0, N) of `q` / `sc` -> the tiles at `out` (the caller has offset `out` to the part's first row group)
int bzk_repack_mx4(hipStream_t s, const void* q, const void* sc, int N, int K, void* out) {
  const int KC = (K + 511) / 512;
  const size_t total = (size_t)(N / 4) * KC * 64;
  hipLaunchKernelGGL(k_repack_mx4, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, (const unsigned char*)q, (const unsigned char*)sc, N, K, KC,
                     (unsigned char*)out);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// decode GEMV.  The structure of k_gemv_f8: 256 threads, a wave walks its rows four at a time (row = lane / 16), one tile (four rows x 512 k) per step, two
// buffers of four steps' loads in flight (a 16-byte and a 1-byte load per lane and step: 8.5 KiB per wave).  x sits in LDS as f32, zero beyond K, padded by
// four floats after every sixteen (xs_pos<2>): a lane's 32 activations are eight float4 reads.  Per step a lane sums its block's 32 exact products in four
// independent double chains, scales the block's sum by 2^(s - 127) in double and adds it to its row sum; a DPP reduction over the sixteen lanes ends a row.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gemv_mx4(const unsigned char* __restrict__ W, const float* __restrict__ bias, int N, int K, int rows_per_wg, Pro pro,
                                                  float* __restrict__ out, int act, long long* zero_buf, int zero_n) {
  extern __shared__ __attribute__((aligned(16))) char mx4_smem[];
  float* xs = (float*)mx4_smem;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, sub = lane >> 4, l16 = lane & 15;
  const int bid = blockIdx.x;
  const int rpw = rows_per_wg >> 2;
  const int rbeg = bid * rows_per_wg + wave * rpw, rend = min(rbeg + rpw, N);   // (multiples of 4: N % 64 == 0)
  const int KC = (K + 511) >> 9;
  float* red = xs + KC * MX4_XCHUNK;            // [16]
  const int ngroups = rend > rbeg ? (rend - rbeg) >> 2 : 0;
  const int nsteps = ngroups * KC;
  // issue cursor (clamped at the last step: a few redundant loads at the tail, never a branch around a load)
  int ig = 0, ikc = 0, ist = 0;
  auto issue = [&](uint4 (&q)[4], unsigned (&sc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int g = min((rbeg >> 2) + ig, (N >> 2) - 1);
      const unsigned char* t = W + ((size_t)g * KC + ikc) * MX4_TILE;
      q[j] = ldnt((const uint4*)(t + lane * 16));
      sc[j] = t[1024 + lane];
      if (ist + 1 < nsteps) { ist++; if (++ikc == KC) { ikc = 0; ig++; } }
    }
  };
  uint4 q0[4], q1[4];
  unsigned s0[4], s1[4];
  issue(q0, s0);
  __builtin_amdgcn_sched_barrier(0);
  if (zero_buf)                                 // the ring protocol's side duty: zero the buffer the NEXT accumulate launch adds into
    for (int i = bid * 256 + threadIdx.x; i < zero_n; i += gridDim.x * 256) zero_buf[i] = 0;
  for (int i = K + threadIdx.x; i < KC * 512; i += 256) xs[xs_pos<2>(i)] = 0.f;
  build_x_simple<2>(pro, 0, K, xs, red, bid == 0);
  double acc = 0.0;
  int cg = 0, ckc = 0, cst = 0;
  auto consume = [&](const uint4 (&q)[4], const unsigned (&sc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (cst < nsteps) {
        cst++;
        const float4* xp = (const float4*)(xs + ckc * MX4_XCHUNK + l16 * 40);
        const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
        double b[4] = {0.0, 0.0, 0.0, 0.0};     // exact products, double sums: the block's value does not depend on the order
#pragma unroll
        for (int d = 0; d < 4; d++) {           // word d: elements 8 d .. 8 d + 7 of the block
          const float4 xa = xp[2 * d + (d >> 1)], xb = xp[2 * d + (d >> 1) + 1];
          const float xl[4] = {xa.x, xa.y, xa.z, xa.w}, xh[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const mx4_h2 p = mx4_pair(w[d], e);
            b[e] += (double)__fmul_rn((float)p.x, xl[e]);
            b[e] += (double)__fmul_rn((float)p.y, xh[e]);
          }
        }
        acc += ((b[0] + b[1]) + (b[2] + b[3])) * mx4_scale_d(sc[j]);
        if (++ckc == KC) {
          ckc = 0;
          const double vd = grp_sum_d<16>(acc);
          acc = 0.0;
          const int row = rbeg + cg * 4 + sub;
          if (l16 == 0 && row < rend) {
            float v = (float)vd;                // one rounding to f32, then the bias in f32 (the oracle's order)
            if (bias) v += bias[row];
            out[row] = round_act(v, act);
          }
          cg++;
        }
      }
    }
  };
  for (int st = 0; st < nsteps; st += 8) {
    issue(q1, s1); consume(q0, s0);
    issue(q0, s0); consume(q1, s1);
  }
}

static int mx4_rows_per_wg(int N) {
  int r = 16;
  while (r < 256 && (N + r - 1) / r > 1024) r <<= 1;    // ~1000 workgroups when N is large (each runs the prologue), at least four rows per wave
  return r;
}

int bzk_gemv_mx4(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act) {
  if (pro.mode != PRO_PLAIN && pro.mode != PRO_NORM && pro.mode != PRO_SILU) BZ_FAIL(BZ_E_UNSUPPORTED, "mxfp4 gemv: prologue mode %d is not built (plain, norm, silu are)", pro.mode);
  if (pro.perm || out.amax_val || out.shift.cs) BZ_FAIL(BZ_E_UNSUPPORTED, "mxfp4 gemv: act-order / argmax partials / conv shift are not built");
  if (L.K % 64 || L.N % 64 || !L.w) BZ_FAIL(BZ_E_INVALID, "mxfp4 gemv: N=%d K=%d must be multiples of 64", L.N, L.K);
  if (pro.mode == PRO_NORM && (pro.H != L.K || pro.H % 4)) BZ_FAIL(BZ_E_INVALID, "mxfp4 gemv: norm prologue over %d elements, K=%d", pro.H, L.K);
  if (!out.direct) BZ_FAIL(BZ_E_INVALID, "mxfp4 gemv needs a direct output");
  const int KC = (L.K + 511) / 512;
  const char* lbl = pro.mode == PRO_NORM ? "gemv_mx4<norm>" : pro.mode == PRO_SILU ? "gemv_mx4<silu>" : "gemv_mx4";
  static bool attr_done = false;      // a long row's activations take more than the 64 KiB a launch gets without asking
  if (!attr_done) {
    BZ_HIP(hipFuncSetAttribute((const void*)k_gemv_mx4, hipFuncAttributeMaxDynamicSharedMemorySize, MX4_SMEM_MAX));
    attr_done = true;
  }
  const int rpw = mx4_rows_per_wg(L.N);
  const size_t smem = (size_t)KC * MX4_XCHUNK * 4 + 64;
  if (smem > MX4_SMEM_MAX) BZ_FAIL(BZ_E_UNSUPPORTED, "K=%d too large for the mxfp4 GEMV", L.K);
  BZ_LAUNCH(lbl, L.algo_bytes, (k_gemv_mx4), dim3((L.N + rpw - 1) / rpw), dim3(256), smem, s, (const unsigned char*)L.w, L.bias, L.N, L.K, rpw, pro, out.direct, act, out.zero_buf,
            out.zero_n);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// out[n][k] = f32(2^(s - 127) e2m1(q[n][k])), formed in double and rounded once (exact for every admitted code), through the expansion the GEMV and the GEMM use.
// One thread per piece (32 weights).
__global__ void k_dequant_mx4(const unsigned char* __restrict__ W, int N, int K, int KC, float* __restrict__ out) {
  const size_t total = (size_t)(N / 4) * KC * 64;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(idx & 63);
    const size_t t = idx >> 6;
    const int row = (int)(t / (size_t)KC) * 4 + (l >> 4), k0 = (int)(t % (size_t)KC) * 512 + (l & 15) * 32;
    if (k0 >= K) continue;
    const uint4 q = *(const uint4*)(W + t * MX4_TILE + l * 16);
    const double sc = mx4_scale_d(W[t * MX4_TILE + 1024 + l]);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    float* o = out + (size_t)row * K + k0;
#pragma unroll
    for (int d = 0; d < 4; d++)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const mx4_h2 p = mx4_pair(w[d], e);
        o[8 * d + e] = (float)(sc * (double)(float)p.x);
        o[8 * d + e + 4] = (float)(sc * (double)(float)p.y);
      }
  }
}
int bzk_dequant_mx4(hipStream_t s, const LinearDev& L, float* out) {
  const int KC = (L.K + 511) / 512;
  hipLaunchKernelGGL(k_dequant_mx4, dim3(2048), dim3(256), 0, s, (const unsigned char*)L.w, L.N, L.K, KC, out);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// W4A16 GEMM on the 16-bit matrix cores: Y[S][N] = R((X16[S][K] . W[N][K]^T) + b[n]).  The structure of k_gemm_f8w (and through it k_gemm_nt2): 128 x 128 x 64
// tiles (64 x 128 for <= 64 rows), 2 x 2 waves, both operands global -> LDS by LDS-DMA into two buffers, split-K partials summed in a fixed order.  The weight
// tile is 128 rows x 32 BYTES of codes (4 KiB): one wave-instruction fills 32 rows, each lane fetching one 16-byte piece (one block) from its place in the
// device tiles.  A 64-k step holds two blocks per row.  The MFMA sums over both halves of the wave, so a step's k is laid out with BOTH halves inside one
// block: MFMA step sidx covers k = 16 sidx + 8 h .. + 7 (h = lane / 32), steps 0, 1 are block 0 and steps 2, 3 block 1.  The fragments hold the UNSCALED
// E2M1 values, exact in f16 and in bf16 whatever the scale; the two MFMAs of a block accumulate into a zeroed 32 x 32 tile, and one f32 multiply-add per
// element, acc += tile . 2^(s - 127), applies the scale -- the result column of a lane is one n, so the scale is one register per (lane, block).  No block
// falls outside a 16-bit format's range, because no scaled weight is ever stored in one.  The scales (two bytes per row and step) come by an ordinary load,
// one step ahead, from the tail of the same device tiles.
// ---------------------------------------------------------------------------------------------------------
typedef float mx4_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 mx4_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 mx4_f16x8 __attribute__((ext_vector_type(8)));

template <int DT>
__device__ __forceinline__ mx4_f32x16 mx4_mfma16(const uint4& a, const uint4& b, mx4_f32x16 c) {
  if constexpr (DT == BZ_BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mx4_bf16x8, a), __builtin_bit_cast(mx4_bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(mx4_f16x8, a), __builtin_bit_cast(mx4_f16x8, b), c, 0, 0, 0);
}
// eight codes (one word) -> one MFMA operand fragment of eight 16-bit values in element order
template <int DT> __device__ __forceinline__ uint4 mx4_frag(unsigned w) {
  mx4_h2 p[4];
#pragma unroll
  for (int e = 0; e < 4; e++) p[e] = mx4_pair(w, e);          // (element e, element e + 4)
  if constexpr (DT == BZ_F16) {
    unsigned u[4];
#pragma unroll
    for (int e = 0; e < 4; e++) u[e] = __builtin_bit_cast(unsigned, p[e]);
    return make_uint4((u[0] & 0xffffu) | (u[1] << 16), (u[2] & 0xffffu) | (u[3] << 16), (u[0] >> 16) | (u[1] & 0xffff0000u), (u[2] >> 16) | (u[3] & 0xffff0000u));
  } else {
    // (exact floats: the bf16 of one is its upper half)
    auto pk = [](float a, float b) { return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xffff0000u); };
    return make_uint4(pk((float)p[0].x, (float)p[1].x), pk((float)p[2].x, (float)p[3].x), pk((float)p[0].y, (float)p[1].y), pk((float)p[2].y, (float)p[3].y));
  }
}
// one 1 KiB LDS-DMA: lane i's 16 bytes at `gsrc` land at LDS byte address ldst + 16 i (ldst wave-uniform); see f8_glds16 (bz_fp8.hip) and glds16 (bz_prefill.hip)
__device__ __forceinline__ void mx4_glds16(const void* gsrc, const unsigned char* ldst) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(const __attribute__((address_space(3))) unsigned char*)ldst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

template <int DT, int TM>
__global__ __launch_bounds__(256) void k_gemm_mx4w(const unsigned short* __restrict__ X, const unsigned char* __restrict__ W, const float* __restrict__ bias, int S, int N, int K,
                                                   int act, float* __restrict__ Y, float* __restrict__ part, int KS, int mtiles, int ntiles) {
  constexpr int BM = 64 * TM, ABYTES = BM * 128, TILE = ABYTES + 128 * 32;
  extern __shared__ __attribute__((aligned(1024))) unsigned char mx4_smem2[];   // the only LDS object of this kernel
  const int xcd = blockIdx.x & 7, jj0 = blockIdx.x >> 3;
  const int mt = jj0 % mtiles, rest = jj0 / mtiles, ks = rest % KS, nt = (rest / KS) * 8 + xcd;
  if (nt >= ntiles) return;                                  // (whole workgroup: no barrier is skipped by part of it)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = mt * BM, n0 = nt * 128;
  const int KC = (K + 511) >> 9;
  const int nk = K >> 6, k_beg = (int)((long long)ks * nk / KS), k_end = (int)((long long)(ks + 1) * nk / KS), nsteps = k_end - k_beg;
  // staging.  A: wave w fills row groups 2 TM w .. (8 rows x 128 B each), lane -> (row lane / 8, slot lane % 8), the slot holds piece slot ^ row.
  // B: wave w fills rows 32 w .. 32 w + 31 (32 B each), lane -> (row lane / 2, block lane % 2)
  const int lrow = lane >> 3, piece = (lane & 7) ^ lrow;
  unsigned xo[2 * TM];                                       // element offsets (S K < 2^32 on this path); rows past the edge are clamped, their results dropped
#pragma unroll
  for (int i = 0; i < 2 * TM; i++) xo[i] = (unsigned)min(m0 + (wave * 2 * TM + i) * 8 + lrow, S - 1) * (unsigned)K + 8u * piece;
  // byte offset of (row n, k) in the device tiles: ((n / 4) KC + k / 512) MX4_TILE + ((n % 4) 16 + (k % 512) / 32) 16; the scale byte of that block sits at
  // ... MX4_TILE + 1024 + (n % 4) 16 + (k % 512) / 32
  auto row_base = [&](int n, int per_block) { n = min(n, N - 1); return (size_t)(n >> 2) * KC * MX4_TILE + (size_t)(n & 3) * 16 * per_block; };
  const size_t wb = row_base(n0 + wave * 32 + (lane >> 1), 16) + (size_t)(lane & 1) * 16;
  const size_t sb0 = row_base(n0 + wn * 64 + r, 1) + 1024, sb1 = row_base(n0 + wn * 64 + 32 + r, 1) + 1024;
  unsigned scn0, scn1;                                       // the next step's two scale bytes of each of this lane's two result columns
  auto issue = [&](int kt, int buf) {
    unsigned char* base = mx4_smem2 + buf * TILE;
    const int k = kt * 64;
    const size_t to = (size_t)(k >> 9) * MX4_TILE;
    const int blk = (k & 511) >> 5;
    scn0 = *(const unsigned short*)(W + sb0 + to + blk);
    scn1 = *(const unsigned short*)(W + sb1 + to + blk);
#pragma unroll
    for (int i = 0; i < 2 * TM; i++) mx4_glds16(X + xo[i] + (size_t)kt * 64, base + (wave * 2 * TM + i) * 1024);
    mx4_glds16(W + wb + to + (size_t)blk * 16, base + ABYTES + wave * 1024);
  };
  mx4_f32x16 acc[TM][2];
#pragma unroll
  for (int t = 0; t < TM; t++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[t][j][i] = 0.f;
  // The f32 accumulator is emptied into a double one every MX4_FOLD steps (four blocks).  A row whose blocks differ by many binades -- one block of scale 2^0
  // among blocks of 2^-30 -- has sums as large as sum |x W|, where every later f32 add rounds at the full magnitude; folding bounds those roundings by three
  // per fold instead of K / 32 per row, and the result is rounded to f32 once.  Measured on the wide-range test: without the fold up to 2.2 x the dense
  // GEMM's error, with the fold (every four steps or every two, the same figures) up to 1.93 x.
  double acc64[TM][2][16];
#pragma unroll
  for (int t = 0; t < TM; t++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc64[t][j][i] = 0.0;
  auto fold = [&]() {
#pragma unroll
    for (int t = 0; t < TM; t++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 16; i++) { acc64[t][j][i] += (double)acc[t][j][i]; acc[t][j][i] = 0.f; }
  };
  if (nsteps > 0) {
    issue(k_beg, 0);
    const int aoff = (wm * 32 * TM + r) * 128, boff = ABYTES + (wn * 64 + r) * 32, sw = r & 7;
    for (int it = 0; it < nsteps; it++) {
      // this wave's pieces of tile `it` (and this lane's scales) have landed; after the barrier everyone's have, and everyone is done reading the buffer
      // the next issue overwrites
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const unsigned sc0 = scn0, sc1 = scn1;
      issue(min(k_beg + it + 1, k_end - 1), (it + 1) & 1);   // clamped: one redundant reload at the tail, never a branch around a load
      const unsigned char* tb = mx4_smem2 + (it & 1) * TILE;
      // the 32 code bytes of rows r (b0x) and 32 + r (b1x) of this wave's 64: block 0, block 1
      const uint4 b00 = *(const uint4*)(tb + boff), b01 = *(const uint4*)(tb + boff + 16);
      const uint4 b10 = *(const uint4*)(tb + boff + 32 * 32), b11 = *(const uint4*)(tb + boff + 32 * 32 + 16);
#pragma unroll
      for (int blk = 0; blk < 2; blk++) {
        mx4_f32x16 tmp[TM][2];
#pragma unroll
        for (int t = 0; t < TM; t++)
#pragma unroll
          for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 16; i++) tmp[t][j][i] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
          // MFMA step 2 blk + s2: k = 32 blk + 16 s2 + 8 h .. + 7 -- piece 4 blk + 2 s2 + h of an A row, word (2 s2 + h) of the block's 16 bytes
          const int po = ((4 * blk + 2 * s2 + h) ^ sw) * 16;
          uint4 af[TM], bf[2];
#pragma unroll
          for (int t = 0; t < TM; t++) af[t] = *(const uint4*)(tb + aoff + t * 32 * 128 + po);
          const uint4 q0 = blk ? b01 : b00, q1 = blk ? b11 : b10;
          bf[0] = mx4_frag<DT>(s2 == 0 ? (h ? q0.y : q0.x) : (h ? q0.w : q0.z));
          bf[1] = mx4_frag<DT>(s2 == 0 ? (h ? q1.y : q1.x) : (h ? q1.w : q1.z));
#pragma unroll
          for (int t = 0; t < TM; t++)
#pragma unroll
            for (int j = 0; j < 2; j++) tmp[t][j] = mx4_mfma16<DT>(af[t], bf[j], tmp[t][j]);
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const float f = mx4_scale_f(((j ? sc1 : sc0) >> (8 * blk)) & 0xffu);
#pragma unroll
          for (int t = 0; t < TM; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[t][j][i] = __fmaf_rn(tmp[t][j][i], f, acc[t][j][i]);   // (tile . 2^e is exact: one rounding, the add's)
        }
      }
      if ((it & (MX4_FOLD - 1)) == MX4_FOLD - 1) fold();
    }
    fold();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the tail's redundant LDS-DMA lands before the LDS allocation is released
  }
  // C layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int n = n0 + wn * 64 + 32 * j + r;
    if (n < N) {
      const float bv = (!part && bias) ? bias[n] : 0.f;
#pragma unroll
      for (int t = 0; t < TM; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int m = m0 + wm * 32 * TM + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (m < S) {
            const float v = (float)acc64[t][j][i];
            if (part) part[((size_t)ks * S + m) * N + n] = v;
            else Y[(size_t)m * N + n] = round_act(__fadd_rn(v, bv), act);
          }
        }
    }
  }
}

// split-K partials summed in a fixed order, then the epilogue of the unsplit form
__global__ void k_gemm_mx4w_reduce(const float* __restrict__ part, int KS, size_t SN, int N, const float* __restrict__ bias, int act, float* __restrict__ Y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < SN; i += (size_t)gridDim.x * 256) {
    double v = 0.0;                      // (the partials are f32; their sum is rounded once)
    for (int z = 0; z < KS; z++) v += (double)part[(size_t)z * SN + i];
    Y[i] = round_act(__fadd_rn((float)v, bias ? bias[(int)(i % (size_t)N)] : 0.f), act);
  }
}

bool bzk_gemm_mx4w_ok(const LinearDev& L, int xdt) { return L.kind == LK_MX4 && (xdt == BZ_F16 || xdt == BZ_BF16) && L.K % 64 == 0 && L.K >= 64 && L.N % 64 == 0 && L.w != nullptr; }

// dt: the 16-bit dtype of x16 (and of the expanded weight fragments); act: rounding of the output (BZ_F32: none); ws: split-K partials (optional)
int bzk_gemm_mx4w(hipStream_t s, const LinearDev& L, int dt, const void* x16, int S, int act, float* y, float* ws, size_t ws_bytes) {
  const int N = L.N, K = L.K;
  if (!bzk_gemm_mx4w_ok(L, dt)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_mx4w: mxfp4 weights with K %% 64 == 0 and 16-bit activations only");
  if (S <= 0 || N <= 0) BZ_FAIL(BZ_E_INVALID, "gemm_mx4w: S=%d N=%d", S, N);
  if ((unsigned long long)S * K >= (1ull << 32) || (unsigned long long)N * K >= (1ull << 32)) BZ_FAIL(BZ_E_UNSUPPORTED, "gemm_mx4w: operand of 2^32 elements or more");
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
#define LAUNCH_MX4W(DT, M) BZ_LAUNCH("gemm_mx4w_mfma", flops, (k_gemm_mx4w<DT, M>), dim3(grid), dim3(256), 2 * (64 * M * 128 + 128 * 32), s, (const unsigned short*)x16, \
    (const unsigned char*)L.w, L.bias, S, N, K, act, y, part, KS, mtiles, ntiles)
  if (dt == BZ_F16) { if (TM == 1) LAUNCH_MX4W(BZ_F16, 1); else LAUNCH_MX4W(BZ_F16, 2); }
  else { if (TM == 1) LAUNCH_MX4W(BZ_BF16, 1); else LAUNCH_MX4W(BZ_BF16, 2); }
#undef LAUNCH_MX4W
  BZ_HIP(hipGetLastError());
  if (KS > 1) {
    const size_t SN = (size_t)S * N;
    hipLaunchKernelGGL(k_gemm_mx4w_reduce, dim3((unsigned)std::min<size_t>((SN + 255) / 256, 2048)), dim3(256), 0, s, (const float*)ws, KS, SN, N, L.bias, act, y);
    BZ_HIP(hipGetLastError());
  }
  return BZ_OK;
}
