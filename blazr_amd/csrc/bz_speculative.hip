// bz_speculative.hip -- device side of speculative decoding (include/blazr_hip.h: bz_forward_kv_verify, bz_spec_accept, bz_generate_speculative).
//
//   k_spec_head      the dense 16-bit lm_head for 1..8 activation rows in ONE pass over the weights: every 16-byte weight piece is loaded once and multiplied
//                    into every row.  Row r's logits are the bits k_gemv_rows<WDT, false> (bz_kernels.hip, rows_body) writes for that row alone, by construction:
//                      * the same lane -> k mapping (lane l owns k = kc * 512 + l * 8 .. + 7 of every 512-k chunk) and the chunks in ascending order,
//                      * per lane the same sequence acc += (double)(w * x) over the eight elements of a piece (piece_dot_x: the f32 product of two 16-bit
//                        values is exact, the double carries the sum),
//                      * the same wave_sum_d, then ONE rounding of the sum to f32, the bias in f32, round_act,
//                      * the final RMSNorm as the prologue, restated from norm_pass1 / build_x_simple with the same 256-thread decomposition of the sum of squares.
//                    Which wave or workgroup owns an output row does not enter its value.  Activations are f16 (the only dtype the exact prompt rows exist for), so
//                    the normalised rows sit in LDS as f16: 8 rows x 4096 x 2 B = 64 KiB, two workgroups per CU.
//                    Per-row argmax partials: a wave walks its output rows in ascending order and keeps the first maximum; k_spec_argmax_final breaks ties between
//                    workgroups towards the lower index, as k_argmax_final does.
//   k_spec_row_partials / k_spec_argmax_final   per-row argmax of given logits [R, V] (bz_spec_accept), ties to the lowest index.
//   k_spec_accept    n_accept = longest prefix with draft[i] == argmax[i]; record {n_accept, tokens[0 .. n_accept]}; the correction / bonus token also goes to the
//                    slot the next draft step reads.
#include "bz_internal.h"
#include "bz_dev.h"

// first maximum wins: larger value, then smaller index (bz_kernels.hip `better`)
__device__ __forceinline__ bool spec_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

template <int WDT> struct SpecPiece { uint4 a; };

// the eight f32 weights of a piece, in k order
template <int WDT>
__device__ __forceinline__ void spec_unpack(const uint4& p, float (&w)[8]) {
  const unsigned u[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (WDT == BZ_F16) { w[2 * i] = __half2float(__ushort_as_half((unsigned short)(u[i] & 0xffffu))); w[2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(u[i] >> 16))); }
    else { w[2 * i] = __uint_as_float(u[i] << 16); w[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u); }
  }
}
__device__ __forceinline__ void spec_unpack_x(const uint4& p, float (&x)[8]) {
  const unsigned u[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int i = 0; i < 4; i++) { x[2 * i] = __half2float(__ushort_as_half((unsigned short)(u[i] & 0xffffu))); x[2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(u[i] >> 16))); }
}

// one activation row: v = R(h + prev), ss = the rounded exact sum of v^2, x = R(w * R(v * rs)) -> LDS as f16 (every value is an f16 already)
__device__ __forceinline__ void spec_norm_row(const SpecHeadRows& a, int r, __half* xr, int KP) {
  const int tid = threadIdx.x, H = a.H;
  const float* h_in = a.h + (size_t)r * a.stride;
  const float* prev = a.prev ? a.prev + (size_t)r * a.stride : nullptr;
  double ss = 0.0;
  for (int base = 0; base < H; base += 4096) {        // norm_pass1: the same elements per thread, the same order of additions
    float4 hv[4], pv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = min(base + j * 1024 + tid * 4, H - 4);
      hv[j] = *(const float4*)(h_in + i);
      pv[j] = prev ? *(const float4*)(prev + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = base + j * 1024 + tid * 4;
      float v[4] = {hv[j].x, hv[j].y, hv[j].z, hv[j].w};
      if (prev) {
        const float p[4] = {pv[j].x, pv[j].y, pv[j].z, pv[j].w};
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = round_act(v[e] + p[e], a.act);
      }
      if (i < H) {
        ss += ((double)(v[0] * v[0]) + (double)(v[1] * v[1])) + ((double)(v[2] * v[2]) + (double)(v[3] * v[3]));
#pragma unroll
        for (int e = 0; e < 4; e++) xr[i + e] = __float2half_rn(v[e]);     // exact: v is an f16 value
      }
    }
  }
  const float ssf = (float)block_sum_d<4>(ss);       // (also orders the LDS writes above before the reads below)
  const float rs = rms_scale(ssf, (float)H, a.eps);
  for (int i = tid; i < KP; i += 256) {
    float x = 0.f;                                   // zero beyond K: the tail of the last 512-k chunk
    if (i < H) x = round_act(a.norm_w[i] * round_act(__half2float(xr[i]) * rs, a.act), a.act);
    xr[i] = __float2half_rn(x);
  }
}

// R activation rows (compile time: the accumulators are registers), 4 weight rows per step and wave, 256 threads
template <int WDT, int R>
__global__ __launch_bounds__(256) void k_spec_head(const void* __restrict__ W, const float* __restrict__ bias, int N, int K, int rows_per_wg, SpecHeadRows a,
                                                   float* __restrict__ logits, float* __restrict__ pval, int* __restrict__ pidx, int nb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float bv_s[4][R];
  __shared__ int bi_s[4][R];
  const int KP = (K + 511) & ~511, KC = KP >> 9;
  __half* xh = (__half*)smem;                        // [R][KP]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int rpw = rows_per_wg >> 2;
  const int rbeg = blockIdx.x * rows_per_wg + wave * rpw;
  const int rend = min(rbeg + rpw, N);
  const int ngroups = rend > rbeg ? (rend - rbeg + 3) >> 2 : 0;
  const int nsteps = ngroups * KC;
  struct Stage { uint4 p[4]; };
  // issue cursor (clamped at the last step: a few redundant loads at the tail, never a branch around a load)
  int ir = min(rbeg, N - 1), ikc = 0, ist = 0;
  auto issue = [&](Stage& S) {
    const int k = ikc * 512 + lane * 8;
    const int ko = k < K ? k : 0;                    // x is 0 beyond K
#pragma unroll
    for (int rr = 0; rr < 4; rr++) S.p[rr] = ldnt((const uint4*)((const unsigned short*)W + (size_t)min(ir + rr, N - 1) * K + ko));
    if (ist + 1 < nsteps) { ist++; if (++ikc == KC) { ikc = 0; ir += 4; } }
  };
  Stage s0, s1, s2;
  issue(s0);
  issue(s1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r = 0; r < R; r++) spec_norm_row(a, r, xh + (size_t)r * KP, KP);
  __syncthreads();
  const uint4* xh4 = (const uint4*)xh;
  const int xrow4 = KP >> 3;                         // uint4 per activation row
  float bestv[R]; int besti[R];
  double acc[4][R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    bestv[r] = -INFINITY; besti[r] = 0x7fffffff;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) acc[rr][r] = 0.0;
  }
  int cr = rbeg, ckc = 0, cst = 0;
  auto consume = [&](const Stage& S) {
    if (cst >= nsteps) return;
    cst++;
    float w[4][8];
#pragma unroll
    for (int rr = 0; rr < 4; rr++) spec_unpack<WDT>(S.p[rr], w[rr]);
#pragma unroll
    for (int r = 0; r < R; r++) {
      float x[8];
      spec_unpack_x(xh4[r * xrow4 + ckc * 64 + lane], x);
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
#pragma unroll
        for (int e = 0; e < 8; e++) acc[rr][r] += (double)__fmul_rn(w[rr][e], x[e]);      // piece_dot_x, element by element
      }
    }
    if (++ckc == KC) {
      ckc = 0;
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
#pragma unroll
        for (int r = 0; r < R; r++) {
          const double vd = wave_sum_d(acc[rr][r]);
          acc[rr][r] = 0.0;
          if (cr + rr < rend) {
            float v = (float)vd;                     // one rounding of the exact sum, then the bias in f32
            if (bias) v += bias[cr + rr];
            v = round_act(v, a.act);
            if (lane == 0) logits[(size_t)r * N + cr + rr] = v;
            if (v > bestv[r]) { bestv[r] = v; besti[r] = cr + rr; }
          }
        }
      }
      cr += 4;
    }
  };
  for (int st = 0; st < nsteps; st += 3) {
    issue(s2); consume(s0);
    issue(s0); consume(s1);
    issue(s1); consume(s2);
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; r++) { bv_s[wave][r] = bestv[r]; bi_s[wave][r] = besti[r]; }
  }
  __syncthreads();
  if (threadIdx.x < R) {
    const int r = threadIdx.x;
    float v = bv_s[0][r]; int ix = bi_s[0][r];
    for (int w2 = 1; w2 < 4; w2++) if (bv_s[w2][r] > v) { v = bv_s[w2][r]; ix = bi_s[w2][r]; }     // waves hold ascending row ranges
    pval[(size_t)r * nb + blockIdx.x] = v; pidx[(size_t)r * nb + blockIdx.x] = ix;
  }
}

static int spec_head_rpw(int N) {
  // ~512 workgroups (two per CU at 8 rows x 4096: 64 KiB of LDS each), 16 output rows (4 per wave) at least
  int r = ((N + 511) / 512 + 15) & ~15;
  return r < 16 ? 16 : r;
}
bool bzk_spec_head_ok(const LinearDev& L, int act, int H) {
  return L.kind == LK_ROWS && L.sk <= 1 && (L.wdt == BZ_F16 || L.wdt == BZ_BF16) && act == BZ_F16 && L.K == H && H % 8 == 0 && H >= 8 && L.N >= 1 &&
         (size_t)8 * ((H + 511) & ~511) * 2 <= 128 * 1024;
}
int bzk_spec_head_blocks(const LinearDev& L) { const int r = spec_head_rpw(L.N); return (L.N + r - 1) / r; }

int bzk_spec_head(hipStream_t s, const LinearDev& L, const SpecHeadRows& x, int R, float* logits, float* pval, int* pidx, int nb) {
  if (R < 1 || R > 8 || !bzk_spec_head_ok(L, x.act, x.H)) BZ_FAIL(BZ_E_INVALID, "spec_head: %d rows / lm_head format not eligible", R);
  const int rpw = spec_head_rpw(L.N), grid = (L.N + rpw - 1) / rpw;
  if (grid != nb) BZ_FAIL(BZ_E_INVALID, "spec_head: %d argmax partials per row, the launch writes %d", nb, grid);
  const int KP = (L.K + 511) & ~511;
  const size_t smem = (size_t)R * KP * 2;
#define LAUNCH_SH(DT, R_) BZ_LAUNCH("spec_head<norm+lm_head rows+argmax>", L.algo_bytes, (k_spec_head<DT, R_>), dim3(grid), dim3(256), smem, s, (const void*)L.w, L.bias, L.N, L.K, \
    rpw, x, logits, pval, pidx, nb)
#define LAUNCH_SH_R(DT) do { switch (R) { case 1: LAUNCH_SH(DT, 1); break; case 2: LAUNCH_SH(DT, 2); break; case 3: LAUNCH_SH(DT, 3); break; case 4: LAUNCH_SH(DT, 4); break; \
    case 5: LAUNCH_SH(DT, 5); break; case 6: LAUNCH_SH(DT, 6); break; case 7: LAUNCH_SH(DT, 7); break; default: LAUNCH_SH(DT, 8); break; } } while (0)
  if (L.wdt == BZ_F16) LAUNCH_SH_R(BZ_F16); else LAUNCH_SH_R(BZ_BF16);
#undef LAUNCH_SH_R
#undef LAUNCH_SH
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// per-row argmax partials of given logits [R, V]: grid (nb, R)
__global__ __launch_bounds__(256) void k_spec_row_partials(const float* __restrict__ logits, long long V, float* pval, int* pidx, int nb) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const float* lg = logits + (size_t)blockIdx.y * V;
  float bv = -INFINITY; int bi = 0x7fffffff;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += (long long)nb * 256) {
    const float x = lg[i];
    if (spec_better(x, (int)i, bv, bi)) { bv = x; bi = (int)i; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s && spec_better(sv[threadIdx.x + s], si[threadIdx.x + s], sv[threadIdx.x], si[threadIdx.x])) { sv[threadIdx.x] = sv[threadIdx.x + s]; si[threadIdx.x] = si[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { pval[(size_t)blockIdx.y * nb + blockIdx.x] = sv[0]; pidx[(size_t)blockIdx.y * nb + blockIdx.x] = si[0]; }
}
int bzk_spec_row_partials(hipStream_t s, const float* logits, int R, long long V, float* pval, int* pidx, int nb) {
  hipLaunchKernelGGL(k_spec_row_partials, dim3(nb, R), dim3(256), 0, s, logits, V, pval, pidx, nb);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// row r (= blockIdx.x): the partials [r][nb] -> argmax[r]
__global__ __launch_bounds__(256) void k_spec_argmax_final(const float* __restrict__ pval, const int* __restrict__ pidx, int nb, long long* argmax) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int r = blockIdx.x;
  float bv = -INFINITY; int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < nb; i += 256) {
    const float v = pval[(size_t)r * nb + i]; const int ix = pidx[(size_t)r * nb + i];
    if (spec_better(v, ix, bv, bi)) { bv = v; bi = ix; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s && spec_better(sv[threadIdx.x + s], si[threadIdx.x + s], sv[threadIdx.x], si[threadIdx.x])) { sv[threadIdx.x] = sv[threadIdx.x + s]; si[threadIdx.x] = si[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) argmax[r] = (long long)si[0];
}
int bzk_spec_argmax_final(hipStream_t s, const float* pval, const int* pidx, int nb, int R, long long* argmax) {
  BZ_LAUNCH("spec_argmax_final", 0.0, k_spec_argmax_final, dim3(R), dim3(256), 0, s, pval, pidx, nb, argmax);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// one wave: lane i compares draft[i] with argmax[i].  record = {n_accept, tokens[0 .. n_accept], -1 ...} (R + 1 words); next_slot (nullable) <- tokens[n_accept]
__global__ __launch_bounds__(64) void k_spec_accept(const long long* __restrict__ argmax, const long long* __restrict__ draft, int R, long long* record, long long* next_slot) {
  const int lane = threadIdx.x;
  const bool miss = lane < R - 1 && draft[lane] != argmax[lane];
  const unsigned long long mm = __ballot(miss);
  const int n_accept = mm ? (int)__ffsll((long long)mm) - 1 : R - 1;
  const long long last = argmax[n_accept];
  if (lane == 0) { record[0] = n_accept; if (next_slot) next_slot[0] = last; }
  if (lane < R) record[1 + lane] = lane < n_accept ? draft[lane] : (lane == n_accept ? last : -1ll);
}
int bzk_spec_accept(hipStream_t s, const long long* argmax, const long long* draft, int R, long long* record, long long* next_slot) {
  if (R < 1 || R > 16) BZ_FAIL(BZ_E_INVALID, "spec_accept: R = %d (1..16)", R);
  BZ_LAUNCH("spec_accept", 0.0, k_spec_accept, dim3(1), dim3(64), 0, s, argmax, draft, R, record, next_slot);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
