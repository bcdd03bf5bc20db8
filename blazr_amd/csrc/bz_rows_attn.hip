// bz_rows_attn.hip -- batched decode attention at long contexts: split-KV over block tables, one sequence per row.
//
// A decode batch runs its attention on the scalar prompt kernel (bz_prefill.hip k_pf_attn with row_pos), which keeps the scores of a row's whole context for all
// REP = n_heads / n_kv_heads heads in LDS: (8 REP + (256 / (hd / 8)) REP hd) 4 + REP len 4 + 64 <= 160 KiB, i.e. 38 888 / 18 416 / 8 180 / 3 062 positions at
// REP 1 / 2 / 4 / 8.  Beyond that limit (or from BZ_ROWS_SPLIT_MIN positions on) the step runs the pair below instead:
//   k_rows_attn_split<DT, HD, REP, WIN>   grid (slices, kv head, row): a workgroup walks ONE slice of ONE row's keys through that row's block-table row for all
//                                         REP query heads of the group (a K / V row is read once per group), online softmax over key tiles (no score buffer:
//                                         LDS use does not depend on the slice), and writes one partial per (row, head, slice): m, l, o[HD] relative to m (f32)
//   k_rows_attn_merge<DT, HD>             grid (head, row): M = max m_s, weights exp(m_s - M), o / l rounded and stored as 16-bit rows where k_pf_attn stores
//                                         its output (the o_proj GEMM after it is untouched)
// The grid's slice count comes from the CAPACITY, so a captured graph is valid at every position; a workgroup whose slice starts at or beyond its row's context
// returns at once.  The slice length is derived on the device from that row's own length alone (bzk_rows_slice_len), never from the grid, N, the capacity or
// another row, and the merge derives the live slice count from the same rule: it never reads a partial this launch did not write (the workspace is not zeroed),
// and a row's bits do not depend on what else is in the batch, on the table width, or on eager versus graph.
// Batched decode: process_decode_batch, engine/batch_decode.rs:35-150.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include "bz_dev.h"

#define RA_SLICE_MIN 128        // positions per slice, doubled until at most RA_MAX_SLICES slices cover the row's keys
#define RA_MAX_SLICES 64
#define RA_KPT 4                // consecutive keys per row slot and tile: they span at most two blocks (block_size >= RA_KPT - 1), so two table entries serve them
#define RA_WS_CAP ((size_t)128 << 20)
#define RA_LDS_CAP (160 * 1024)

__host__ __device__ __forceinline__ int ra_slice_len(int keys) {
  int spl = RA_SLICE_MIN;
  while ((keys + spl - 1) / spl > RA_MAX_SLICES) spl *= 2;
  return spl;
}

namespace {

template <int DT> __device__ __forceinline__ unsigned short ra_to16(float x) {
  if (DT == BZ_F16) return __half_as_ushort(f16_cvt(x));
  const __bf16 b = (__bf16)x; return __builtin_bit_cast(unsigned short, b);
}
template <int STEP, class Op> __device__ __forceinline__ float ra_xlane(float v) {     // lane l with l ^ STEP
  if (STEP == 8) return Op::f(v, __shfl_xor(v, 8, 64));
  if (STEP == 16) return xrow16<Op>(v);
  return xrow32<Op>(v);
}
__device__ __forceinline__ float ra_w(float m, float M) { return m == -INFINITY ? 0.f : bz_expf(m - M); }   // weight of a partial with maximum m under M

// merge the (m, l, acc) states of lane l and lane l ^ STEP (same 8-dim piece of another row slot); both lanes end with the same bits
template <int STEP, int REP>
__device__ __forceinline__ void ra_join(float (&m)[REP], float (&l)[REP], float (&acc)[REP][8]) {
#pragma unroll
  for (int h = 0; h < REP; h++) {
    const float M = ra_xlane<STEP, OpMax>(m[h]);
    const float f = ra_w(m[h], M);
    l[h] = ra_xlane<STEP, OpAdd>(l[h] * f);
#pragma unroll
    for (int e = 0; e < 8; e++) acc[h][e] = ra_xlane<STEP, OpAdd>(acc[h][e] * f);
    m[h] = M;
  }
}

// 256 threads: PR = HD / 8 lanes share a cache row (16 bytes each), RPP = 256 / PR row slots, each taking RA_KPT consecutive keys of a tile of TK keys.
// Every row slot carries its own running (m, l, o) over the keys it has seen; the slots are joined once, after the slice.
template <int DT, int HD, int REP, bool WIN>
__global__ __launch_bounds__(256) void k_rows_attn_split(const float* __restrict__ qkv, int nq, int nkv, KvView kv, int layer, float scale, const int* __restrict__ row_pos,
                                                         int table_stride, int window, float* __restrict__ ws) {
  constexpr int PR = HD / 8, RPP = 256 / PR, TK = RPP * RA_KPT, PS = HD + 4;
  __shared__ __attribute__((aligned(16))) float part[4][REP][HD];
  __shared__ float mls[4][REP][2];
  const int s = blockIdx.x, kvh = blockIdx.y, row = blockIdx.z, gs = gridDim.x;
  const int len = row_pos[row] + 1;
  const int lo = WIN ? att_lo(len, window) : 0;
  const int SPL = ra_slice_len(len - lo);                      // from this row's own keys alone
  const int p0 = lo + s * SPL;
  if (p0 >= len) return;                                       // slice beyond the row's context (the grid covers the capacity)
  const int p1 = min(p0 + SPL, len);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = tid % PR, g = tid / PR;                        // this thread's 8-dim piece and row slot
  const int bs = kv.bs;
  const int* __restrict__ btab = kv.block_table + (size_t)row * table_stride;
  const unsigned short* kb = (const unsigned short*)kv.k + (size_t)layer * kv.layer_stride + (size_t)kvh * bs * HD + 8 * c;
  const unsigned short* vb = (const unsigned short*)kv.v + (size_t)layer * kv.layer_stride + (size_t)kvh * bs * HD + 8 * c;
  const size_t blk_stride = (size_t)kv.n_kv * bs * HD;
  uint4 qq[REP];
#pragma unroll
  for (int h = 0; h < REP; h++) {
    const float* qr = qkv + (size_t)row * (nq + 2 * nkv) * HD + (size_t)(kvh * REP + h) * HD + 8 * c;
    const float4 a = *(const float4*)qr, b = *(const float4*)(qr + 4);
    qq[h] = make_uint4(pack2<DT>(a.x, a.y), pack2<DT>(a.z, a.w), pack2<DT>(b.x, b.y), pack2<DT>(b.z, b.w));    // roped and rounded by k_pf_rope_kv: exact in 16 bits
  }
  // the RA_KPT keys of this row slot in the tile at c0 (clamped into the slice: every address is a live key of this row); one table entry per block
  auto load_tile = [&](int c0, uint4 (&kr)[RA_KPT], uint4 (&vr)[RA_KPT]) {
    const int pa = min(c0 + g * RA_KPT, p1 - 1), pb = min(c0 + g * RA_KPT + RA_KPT - 1, p1 - 1);
    const int ba = pa / bs, bb = pb / bs;
    const int ea = btab[ba], eb = btab[bb];
    const int edge = bb * bs, base_a = ba * bs;
#pragma unroll
    for (int j = 0; j < RA_KPT; j++) {
      const int p = min(c0 + g * RA_KPT + j, p1 - 1);
      const bool hi = p >= edge;
      const size_t off = (size_t)(hi ? eb : ea) * blk_stride + (size_t)(p - (hi ? edge : base_a)) * HD;
      kr[j] = *(const uint4*)(kb + off);
      vr[j] = *(const uint4*)(vb + off);
    }
  };
  float m[REP], l[REP], acc[REP][8];
#pragma unroll
  for (int h = 0; h < REP; h++) {
    m[h] = -INFINITY; l[h] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) acc[h][e] = 0.f;
  }
  uint4 kr[RA_KPT], vr[RA_KPT];
  load_tile(p0, kr, vr);
  for (int c0 = p0; c0 < p1; c0 += TK) {
    uint4 nk[RA_KPT], nv[RA_KPT];
    load_tile(min(c0 + TK, p1 - 1), nk, nv);                   // the next tile's rows are requested before this tile's arithmetic
    float sc[REP][RA_KPT];
#pragma unroll
    for (int j = 0; j < RA_KPT; j++) {
      const bool live = c0 + g * RA_KPT + j < p1;
#pragma unroll
      for (int h = 0; h < REP; h++) {
        float d = dot2acc<DT>(kr[j].x, qq[h].x, 0.f);
        d = dot2acc<DT>(kr[j].y, qq[h].y, d); d = dot2acc<DT>(kr[j].z, qq[h].z, d); d = dot2acc<DT>(kr[j].w, qq[h].w, d);
        d = grp_reduce<PR, OpAdd>(d);
        sc[h][j] = live ? d * scale : -INFINITY;
      }
    }
    float fr[REP];
#pragma unroll
    for (int h = 0; h < REP; h++) {
      float mt = sc[h][0];
#pragma unroll
      for (int j = 1; j < RA_KPT; j++) mt = fmaxf(mt, sc[h][j]);
      const float mn = fmaxf(m[h], mt);
      fr[h] = ra_w(m[h], mn);
      m[h] = mn;
      l[h] *= fr[h];
#pragma unroll
      for (int e = 0; e < 8; e++) acc[h][e] *= fr[h];
    }
#pragma unroll
    for (int j = 0; j < RA_KPT; j++) {
      float v[8];
      unpack2<DT>(vr[j].x, v[0], v[1]); unpack2<DT>(vr[j].y, v[2], v[3]); unpack2<DT>(vr[j].z, v[4], v[5]); unpack2<DT>(vr[j].w, v[6], v[7]);
#pragma unroll
      for (int h = 0; h < REP; h++) {
        const float e_ = ra_w(sc[h][j], m[h]);
        l[h] += e_;
#pragma unroll
        for (int e = 0; e < 8; e++) acc[h][e] = fmaf(e_, v[e], acc[h][e]);
      }
    }
#pragma unroll
    for (int j = 0; j < RA_KPT; j++) { kr[j] = nk[j]; vr[j] = nv[j]; }
  }
  // join the row slots of a wave (lanes with the same piece), then the four waves through LDS
  if (PR == 8) ra_join<8, REP>(m, l, acc);
  ra_join<16, REP>(m, l, acc);
  ra_join<32, REP>(m, l, acc);
  if (lane < PR) {
#pragma unroll
    for (int h = 0; h < REP; h++) {
      *(float4*)(&part[wave][h][8 * c]) = make_float4(acc[h][0], acc[h][1], acc[h][2], acc[h][3]);
      *(float4*)(&part[wave][h][8 * c + 4]) = make_float4(acc[h][4], acc[h][5], acc[h][6], acc[h][7]);
      if (c == 0) { mls[wave][h][0] = m[h]; mls[wave][h][1] = l[h]; }
    }
  }
  __syncthreads();
  for (int i = tid; i < REP * HD; i += 256) {
    const int h = i / HD, d = i % HD;
    const float M = fmaxf(fmaxf(mls[0][h][0], mls[1][h][0]), fmaxf(mls[2][h][0], mls[3][h][0]));
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; w++) { const float f = ra_w(mls[w][h][0], M); o = fmaf(f, part[w][h][d], o); L = fmaf(f, mls[w][h][1], L); }
    float* dst = ws + (((size_t)row * nq + kvh * REP + h) * gs + s) * PS;
    dst[4 + d] = o;
    if (d == 0) { dst[0] = M; dst[1] = L; }
  }
}

// grid (head, row), HD threads: thread d owns output dim d
template <int DT, int HD>
__global__ __launch_bounds__(HD) void k_rows_attn_merge(const float* __restrict__ ws, int nq, int gs, const int* __restrict__ row_pos, int window,
                                                        unsigned short* __restrict__ out16) {
  constexpr int PS = HD + 4;
  const int h = blockIdx.x, row = blockIdx.y, d = threadIdx.x;
  const int len = row_pos[row] + 1, wl = len - att_lo(len, window), SPL = ra_slice_len(wl);   // the slices k_rows_attn_split wrote for this row
  const int ns = min((wl + SPL - 1) / SPL, gs);
  const float* base = ws + ((size_t)row * nq + h) * gs * PS;
  float M = -INFINITY;
  for (int s = 0; s < ns; s++) M = fmaxf(M, base[(size_t)s * PS]);
  float o = 0.f, L = 0.f;
  for (int s = 0; s < ns; s++) {
    const float f = ra_w(base[(size_t)s * PS], M);
    L = fmaf(f, base[(size_t)s * PS + 1], L);
    o = fmaf(f, base[(size_t)s * PS + 4 + d], o);
  }
  out16[((size_t)row * nq + h) * HD + d] = ra_to16<DT>(div_rn(o, L));
}

template <int DT>
__global__ __launch_bounds__(256) void k_rows16_to_f32(const unsigned short* __restrict__ x, size_t n, float* __restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const unsigned short b = x[i];
    y[i] = DT == BZ_F16 ? __half2float(__ushort_as_half(b)) : __uint_as_float((unsigned)b << 16);
  }
}

}  // namespace

int bzk_rows_slice_len(int len) { return ra_slice_len(std::max(len, 1)); }
int bzk_rows_split_min() { const char* e = getenv("BZ_ROWS_SPLIT_MIN"); return e ? atoi(e) : (1 << 30); }   // read per call: tests move it; a graph keeps its capture's
bool bzk_rows_attn_ok(int nq, int nkv, int hd, int kv_dtype) {
  const int rep = nkv > 0 && nq % nkv == 0 ? nq / nkv : 0;
  return (hd == 64 || hd == 128) && (rep == 1 || rep == 2 || rep == 4 || rep == 8) && (kv_dtype == BZ_F16 || kv_dtype == BZ_BF16);
}
// last context (positions) whose scores the scalar kernel's LDS formula holds; 0: no such group size / head_dim
int bzk_rows_scalar_limit(int nq, int nkv, int hd) {
  const int rep = nkv > 0 && nq % nkv == 0 ? nq / nkv : 0;
  if (hd <= 0 || hd % 8 || hd > 256 || (rep != 1 && rep != 2 && rep != 4 && rep != 8)) return 0;
  const long long fixed = (long long)bzk_pf_attn_smem(nq, nkv, hd, 0, false);
  return fixed >= RA_LDS_CAP ? 0 : (int)((RA_LDS_CAP - fixed) / (4ll * rep));
}
// what a decode batch of N rows launches for one layer at a decision length of `capacity` positions (the longest live row of an eager step, the capacity of
// a graph) under a window of `window` keys (0: none)
int bzk_rows_attn_plan(int nq, int nkv, int hd, int kv_dtype, int block_size, int window, int N, int capacity, int split_min, BzRowsPlan* out) {
  BzRowsPlan p{};
  p.scalar_limit = bzk_rows_scalar_limit(nq, nkv, hd);
  const int keys = window > 0 ? std::min(capacity, window) : capacity;
  const bool pair_ok = bzk_rows_attn_ok(nq, nkv, hd, kv_dtype) && block_size >= RA_KPT;
  const bool beyond = keys > p.scalar_limit;
  if (!beyond && !(pair_ok && keys >= split_min)) { p.kernel = 0; *out = p; return BZ_OK; }
  if (!pair_ok) { p.kernel = -1; *out = p; return BZ_OK; }
  p.kernel = 1;
  p.grid_slices = std::min((std::max(keys, 1) + RA_SLICE_MIN - 1) / RA_SLICE_MIN, RA_MAX_SLICES);
  const size_t per_row = (size_t)nq * p.grid_slices * (hd + 4) * 4;
  p.rows_per_pass = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(N, 1), RA_WS_CAP / per_row));
  p.ws_bytes = (size_t)p.rows_per_pass * per_row;
  *out = p;
  return BZ_OK;
}

// the pair over rows [0, n) of a decode batch: qkv rows as k_pf_rope_kv leaves them, 16-bit output rows at out16; ws holds plan.ws_bytes
int bzk_rows_attn(hipStream_t st, int dt, const float* qkv, int n, int nq, int nkv, int hd, const KvView& kv, int layer, void* out16, const int* row_pos, int table_stride,
                  int window, const BzRowsPlan& plan, float* ws) {
  if (!bzk_rows_attn_ok(nq, nkv, hd, kv.dtype) || kv.dtype != dt || !kv.paged || kv.bs < RA_KPT || !row_pos || !ws || plan.kernel != 1 || plan.grid_slices < 1 ||
      plan.grid_slices > RA_MAX_SLICES || plan.rows_per_pass < 1)
    BZ_FAIL(BZ_E_UNSUPPORTED, "rows attention: head_dim %d / group size %d / cache dtype %d / block size %d unsupported", hd, nkv > 0 ? nq / nkv : 0, kv.dtype, kv.bs);
  const int REP = nq / nkv, gs = plan.grid_slices;
  const float scale = div_rn(1.0f, sqrt_rn((float)hd));
  for (int r0 = 0; r0 < n; r0 += plan.rows_per_pass) {
    const int nr = std::min(plan.rows_per_pass, n - r0);
    KvView vw = kv;
    vw.block_table = kv.block_table + (size_t)r0 * table_stride;
    const float* q = qkv + (size_t)r0 * (nq + 2 * nkv) * hd;
    const int* rp = row_pos + r0;
    unsigned short* o16 = (unsigned short*)out16 + (size_t)r0 * nq * hd;
    const double bytes = 0.0;
#define LAUNCH_RA_(DT, HD, R, WN) BZ_LAUNCH("rows_attn_split", bytes, (k_rows_attn_split<DT, HD, R, WN>), dim3(gs, nkv, nr), dim3(256), 0, st, q, nq, nkv, vw, layer, scale, rp, table_stride, window, ws)
#define LAUNCH_RA(DT, HD, R) do { if (window > 0) LAUNCH_RA_(DT, HD, R, true); else LAUNCH_RA_(DT, HD, R, false); } while (0)
#define LAUNCH_RA_R(DT, HD) do { if (REP == 1) LAUNCH_RA(DT, HD, 1); else if (REP == 2) LAUNCH_RA(DT, HD, 2); else if (REP == 4) LAUNCH_RA(DT, HD, 4); else LAUNCH_RA(DT, HD, 8); } while (0)
#define LAUNCH_RA_H(DT) do { if (hd == 64) LAUNCH_RA_R(DT, 64); else LAUNCH_RA_R(DT, 128); } while (0)
    if (dt == BZ_F16) LAUNCH_RA_H(BZ_F16); else LAUNCH_RA_H(BZ_BF16);
#undef LAUNCH_RA_H
#undef LAUNCH_RA_R
#undef LAUNCH_RA
#undef LAUNCH_RA_
    BZ_HIP(hipGetLastError());
#define LAUNCH_RM(DT, HD) BZ_LAUNCH("rows_attn_merge", bytes, (k_rows_attn_merge<DT, HD>), dim3(nq, nr), dim3(HD), 0, st, ws, nq, gs, rp, window, o16)
    if (dt == BZ_F16) { if (hd == 64) LAUNCH_RM(BZ_F16, 64); else LAUNCH_RM(BZ_F16, 128); }
    else { if (hd == 64) LAUNCH_RM(BZ_BF16, 64); else LAUNCH_RM(BZ_BF16, 128); }
#undef LAUNCH_RM
    BZ_HIP(hipGetLastError());
  }
  return BZ_OK;
}

int bzk_rows16_to_f32(hipStream_t st, int dt, const void* x16, size_t n, float* y) {
  if (dt != BZ_F16 && dt != BZ_BF16) BZ_FAIL(BZ_E_UNSUPPORTED, "rows16_to_f32: 16-bit rows only");
  const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
  if (dt == BZ_F16) hipLaunchKernelGGL(k_rows16_to_f32<BZ_F16>, dim3(std::max(grid, 1u)), dim3(256), 0, st, (const unsigned short*)x16, n, y);
  else hipLaunchKernelGGL(k_rows16_to_f32<BZ_BF16>, dim3(std::max(grid, 1u)), dim3(256), 0, st, (const unsigned short*)x16, n, y);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
