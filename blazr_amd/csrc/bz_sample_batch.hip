// bz_sample_batch.hip -- per-sequence sampling for a decode batch: what the reference's batched step does by calling logits_to_token_on_device once per
// sequence with its own gen_config (engine/batch_decode.rs:149-168), as ONE fixed sequence of launches over all N rows.  Per row the result is what
// oracle/orc_ops.c::orc_logits_to_token gives for that row alone (sampling.rs:445-460) with the penalty window of sampling.rs:169-191 taken from a
// device-resident ring of the row's last tokens and seed = the row's seed + its draw index.
//
// Shape (21 launches, whatever N and the rows' parameters are; grid.y = row everywhere):
//   prep            [N]        dedupe the row's window in LDS (<= 256 entries) -> unique in-range ids + counts; zero the row's level-1 histogram
//   scale, exp      [128, N]   the single-row kernels' passes (bz_sample.hip) per row: 128 blocks x 256 threads, strided per-thread partials, the same
//                              shuffle tree, the 128 partials combined in index order -- so max, the f64 sum and every p_i are the single-row kernel's bits.
//                              Penalised ids are patched from the deduped list (an LDS bit per (thread, iteration) marks them in the streaming pass).
//   norm            [128, N]   p_i -> its f32 bits (the key); level-1 histogram (count and mass) of the row; count / mass of p >= min_p * p_0
//   select          [N]        cut bin of top-k (by rank) and of top-p (by mass)
//   4 x (level, select)        refine both cuts: 11 more bits of the (key descending, id ascending) order per level
//   4 x (level, select)        the same for the draw u; the last select writes the token, the history ring, the draw counter, next / log / step
// No full-vocabulary sort: selection over radix histograms of the 50-bit composite (30 key bits : 20 bits of ~id).  A target whose bin holds one candidate is
// resolved there and the later levels skip the row; a bin of exact ties is refined through the id bits, which IS the ascending-id order, so no candidate list
// and no LDS sort is needed and no buffer can overflow.  Masses are 64-bit fixed point on a 2^-60 grid, accumulated with integer atomics: exactly associative,
// so nothing depends on arrival order.  Against the single-row kernel the only difference is how cumulative masses are accumulated (<= V * 2^-60 here).
#include <hip/hip_runtime.h>
#include <cstring>
#include <algorithm>

#include "bz_internal.h"

typedef unsigned long long u64;

namespace {
constexpr int NB = 128;        // blocks per row of the streaming passes (the single-row kernels' grid)
constexpr int BINS = 2048;     // 11-bit digits
constexpr int WIN = BZ_SAMPLER_WINDOW_MAX;
constexpr long long VMAX = 1ll << 20;
enum { T_K = 0, T_A = 1, T_C = 2 };
enum { M_RANK = 0, M_GE = 1, M_GT = 2 };
enum { S_ACTIVE = 0, S_DONE = 1, S_NONE = 2 };

struct BsRow {     // device-resident per-row state
  float temperature; int top_k; float top_p, min_p, rp, fp, pp; int last_n;
  u64 seed, draw;
  int head, cnt, pad[2];
  long long ring[WIN];
};
// a selection target: DONE => rank = sorted index of the element, mass = cumulative mass through it, rep = its composite
struct BsTarget { int mode, state; u64 thr, prefix, rank, mass, rep; };
struct BsScr {     // per-row scratch of one call
  int pen_n, greedy, step_snap; unsigned p0key;
  unsigned cnt_ge, pad; u64 mass_ge, total;
  BsTarget t[3];
};
struct BsArgs {
  int N; long long V;
  BsRow* rows; BsScr* scr; const float* logits; float* l2; float* pmax; double* psum; float* amv; int* ami;
  long long* pen_id; int* pen_cnt;
  unsigned* h1c; u64* h1m;          // [N][BINS] level 1
  unsigned* hc; u64* hm; u64* hrep; // [N][2][BINS], [N][2][BINS], [N][BINS]: the level being refined (zero between uses)
  long long* tokens_out; long long* next; long long* log; int* step; int logcap;
};

__device__ __forceinline__ int lvl_shift(int L) { return L == 1 ? 39 : L == 2 ? 28 : L == 3 ? 17 : L == 4 ? 6 : 0; }
__device__ __forceinline__ int lvl_bits(int L) { return L == 5 ? 6 : 11; }
__device__ __forceinline__ u64 composite(unsigned key, long long i) { return ((u64)key << 20) | (u64)(0xFFFFFu - (unsigned)i); }   // larger = earlier in (p desc, id asc)
__device__ __forceinline__ u64 mass_of(unsigned key) { return (u64)((double)__uint_as_float(key) * 1152921504606846976.0); }         // p * 2^60, p in [0, 1]
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// ---- prep: the penalty window of sampling.rs:169-191 from the ring, unique in-range ids + counts -----------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_prep(BsArgs a) {
  __shared__ long long win[WIN];
  __shared__ int n_out;
  const int row = blockIdx.x, tid = threadIdx.x;
  const BsRow& r = a.rows[row];
  BsScr& sc = a.scr[row];
  for (int b = tid; b < BINS; b += 256) { a.h1c[(size_t)row * BINS + b] = 0; a.h1m[(size_t)row * BINS + b] = 0; }
  const bool pen = r.rp != 1.0f || r.fp != 0.0f || r.pp != 0.0f;
  int w = 0;
  if (pen) { w = min(max(r.last_n, 0), min(max(r.cnt, 0), WIN)); }
  if (tid == 0) n_out = 0;
  if (tid < w) win[tid] = r.ring[(r.head - w + tid) & (WIN - 1)];
  __syncthreads();
  if (tid < w) {
    const long long id = win[tid];
    if (id >= 0 && id < a.V) {
      bool first = true; int c = 0;
      for (int j = 0; j < w; j++) { if (win[j] == id) { c++; if (j < tid) first = false; } }
      if (first) { const int s = atomicAdd(&n_out, 1); a.pen_id[(size_t)row * WIN + s] = id; a.pen_cnt[(size_t)row * WIN + s] = c; }   // s < w <= WIN
    }
  }
  __syncthreads();
  if (tid == 0) {
    sc.pen_n = n_out; sc.greedy = r.temperature == 0.0f; sc.cnt_ge = 0; sc.mass_ge = 0; sc.total = 0; sc.p0key = 0;
    for (int t = 0; t < 3; t++) { sc.t[t].mode = M_RANK; sc.t[t].state = S_NONE; sc.t[t].thr = sc.t[t].prefix = sc.t[t].rank = sc.t[t].mass = sc.t[t].rep = 0; }
    if (row == 0) sc.step_snap = a.step ? *a.step : 0;
  }
}

// ---- scale: k_samp_scale per row (penalties -> / temperature -> block maximum), plus the greedy partials (penalised value, lowest index) ---------------
__global__ __launch_bounds__(256) void k_bs_scale(BsArgs a) {
  __shared__ unsigned flag[256];
  __shared__ float red[4];
  __shared__ float sv[256];
  __shared__ int si[256];
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  const BsRow& r = a.rows[row];
  const int n = a.scr[row].pen_n;
  const float* lg = a.logits + (size_t)row * a.V;
  float* l2 = a.l2 + (size_t)row * a.V;
  const bool greedy = r.temperature == 0.0f;
  const float T = greedy ? 1.0f : r.temperature;
  flag[tid] = 0;
  __syncthreads();
  long long pid = -1;
  if (tid < n) {
    const long long id = a.pen_id[(size_t)row * WIN + tid];        // in [0, V), V <= 2^20
    if ((int)((id >> 8) & (NB - 1)) == blk) { pid = id; atomicOr(&flag[id & 255], 1u << (int)(id >> 15)); }
  }
  __syncthreads();
  const unsigned mine = flag[tid];
  float m = -INFINITY, bv = -INFINITY; int bi = 0x7fffffff, k = 0;
  for (long long i = (long long)blk * 256 + tid; i < a.V; i += (long long)NB * 256, k++) {
    if ((mine >> k) & 1u) continue;                                // a penalised id: patched below
    const float x = lg[i];
    if (better(x, (int)i, bv, bi)) { bv = x; bi = (int)i; }
    if (!greedy) { const float y = x / T; l2[i] = y; m = fmaxf(m, y); }
  }
  if (pid >= 0) {
    float x = lg[pid];
    const float rp = r.rp, fp = r.fp, pp = r.pp;
    if (rp != 1.0f) x = (x > 0.f) ? x / rp : x * rp;
    x -= fp * (float)a.pen_cnt[(size_t)row * WIN + tid] + pp;
    if (better(x, (int)pid, bv, bi)) { bv = x; bi = (int)pid; }
    if (!greedy) { const float y = x / T; l2[pid] = y; m = fmaxf(m, y); }
  }
  if (greedy) {
    sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s && better(sv[tid + s], si[tid + s], sv[tid], si[tid])) { sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; }
      __syncthreads();
    }
    if (tid == 0) { a.amv[(size_t)row * NB + blk] = sv[0]; a.ami[(size_t)row * NB + blk] = si[0]; }
    return;
  }
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) a.pmax[(size_t)row * NB + blk] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- exp: k_samp_exp per row --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_exp(BsArgs a) {
  __shared__ double red[4];
  const int row = blockIdx.y, tid = threadIdx.x;
  if (a.scr[row].greedy) return;
  float* l2 = a.l2 + (size_t)row * a.V;
  const float* pmax = a.pmax + (size_t)row * NB;
  float m = -INFINITY;
  for (int b = 0; b < NB; b++) m = fmaxf(m, pmax[b]);
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < a.V; i += (long long)NB * 256) {
    const float e = bz_expf(l2[i] - m);
    l2[i] = e;
    s += (double)e;
  }
  for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) a.psum[(size_t)row * NB + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- norm: k_samp_norm per row; the key replaces e in place; level-1 histogram; the min-p count ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_bs_norm(BsArgs a) {
  __shared__ unsigned hc[BINS];
  __shared__ u64 hm[BINS];
  __shared__ unsigned bc; __shared__ u64 bm;
  const int row = blockIdx.y, tid = threadIdx.x;
  if (a.scr[row].greedy) return;
  const BsRow& r = a.rows[row];
  float* l2 = a.l2 + (size_t)row * a.V;
  const double* psum = a.psum + (size_t)row * NB;
  double sum = 0.0;
  for (int b = 0; b < NB; b++) sum += psum[b];
  for (int b = tid; b < BINS; b += 256) { hc[b] = 0; hm[b] = 0; }
  if (tid == 0) { bc = 0; bm = 0; }
  __syncthreads();
  const float p0 = (float)(1.0 / sum);                 // the largest p: its e is bz_expf(0) = 1
  const float thr = p0 * r.min_p;
  const bool minp = r.min_p > 0.0f;
  unsigned c = 0; u64 cm = 0;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < a.V; i += (long long)NB * 256) {
    const float p = (float)((double)l2[i] / sum);
    const unsigned key = (p > 0.0f && p <= 1.0f) ? __float_as_uint(p) : 0u;   // NaN (a row of -inf) and anything out of range sort last with no mass
    ((unsigned*)l2)[i] = key;
    const u64 q = mass_of(key);
    const int d = (int)(key >> 19);                    // == composite >> 39, < 2033
    atomicAdd(&hc[d], 1u); atomicAdd(&hm[d], q);
    if (minp && !(p < thr)) { c++; cm += q; }
  }
  if (minp && c) { atomicAdd(&bc, c); atomicAdd(&bm, cm); }
  __syncthreads();
  for (int b = tid; b < BINS; b += 256)
    if (hc[b]) { atomicAdd(&a.h1c[(size_t)row * BINS + b], hc[b]); atomicAdd(&a.h1m[(size_t)row * BINS + b], hm[b]); }
  if (tid == 0) {
    if (bc) { atomicAdd(&a.scr[row].cnt_ge, bc); atomicAdd(&a.scr[row].mass_ge, bm); }
    if (blockIdx.x == 0) a.scr[row].p0key = (p0 > 0.0f && p0 <= 1.0f) ? __float_as_uint(p0) : 0u;
  }
}

// ---- level L (2..5): histogram of digit L over the candidates that carry a target's prefix ---------------------------------------------------------------
template <int NT, bool REP>
__global__ __launch_bounds__(256) void k_bs_level(BsArgs a, int L, int t0) {
  __shared__ unsigned hc[NT][BINS];
  __shared__ u64 hm[NT][BINS];
  __shared__ u64 hr[REP ? BINS : 1];
  const int row = blockIdx.y, tid = threadIdx.x;
  const BsScr& sc = a.scr[row];
  if (sc.greedy) return;
  bool act[NT]; u64 pre[NT]; bool any = false;
#pragma unroll
  for (int t = 0; t < NT; t++) { act[t] = sc.t[t0 + t].state == S_ACTIVE; pre[t] = sc.t[t0 + t].prefix; any |= act[t]; }
  if (!any) return;
  for (int b = tid; b < NT * BINS; b += 256) { (&hc[0][0])[b] = 0; (&hm[0][0])[b] = 0; }
  if (REP) for (int b = tid; b < BINS; b += 256) hr[b] = 0;
  __syncthreads();
  const unsigned* keys = (const unsigned*)(a.l2 + (size_t)row * a.V);
  const int shp = lvl_shift(L - 1), sh = lvl_shift(L);
  const unsigned dmask = (1u << lvl_bits(L)) - 1u;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < a.V; i += (long long)NB * 256) {
    const unsigned key = keys[i];
    const u64 C = composite(key, i);
#pragma unroll
    for (int t = 0; t < NT; t++) {
      if (act[t] && (C >> shp) == pre[t]) {
        const int d = (int)((unsigned)(C >> sh) & dmask);
        atomicAdd(&hc[t][d], 1u); atomicAdd(&hm[t][d], mass_of(key));
        if (REP) atomicMax(&hr[d], C);
      }
    }
  }
  __syncthreads();
  for (int b = tid; b < NT * BINS; b += 256) {
    const unsigned c = (&hc[0][0])[b];
    if (c) {
      atomicAdd(&a.hc[(size_t)row * 2 * BINS + b], c); atomicAdd(&a.hm[(size_t)row * 2 * BINS + b], (&hm[0][0])[b]);
      if (REP) atomicMax(&a.hrep[(size_t)row * BINS + b], hr[b]);      // REP => NT == 1: b < BINS
    }
  }
}

// ---- select: walk one histogram in descending digit order to the bin that holds the target -----------------------------------------------------------------
// every thread of the block calls it; hcnt / hmass [BINS] are the row's histogram of digit L under tg->prefix (zeroed afterwards when `zero`)
__device__ void select_target(BsTarget* tg, unsigned* hcnt, u64* hmass, u64* hrep, int L, bool zero, u64* total_out) {
  __shared__ u64 pc[256], pm[256];
  __shared__ int fb; __shared__ u64 fcb, fmb, fc, fm;
  const int tid = threadIdx.x;
  const bool active = tg->state == S_ACTIVE;       // uniform
  if (!active && !total_out) return;
  unsigned c[8]; u64 m[8]; u64 sc_ = 0, sm_ = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) { const int b = BINS - 1 - (tid * 8 + j); c[j] = hcnt[b]; m[j] = hmass[b]; sc_ += c[j]; sm_ += m[j]; }
  pc[tid] = sc_; pm[tid] = sm_;
  if (tid == 0) fb = -1;
  __syncthreads();
  if (tid == 0) { u64 xc = 0, xm = 0; for (int t = 0; t < 256; t++) { const u64 tc = pc[t], tm = pm[t]; pc[t] = xc; pm[t] = xm; xc += tc; xm += tm; } if (total_out) *total_out = xm; }
  __syncthreads();
  if (active) {
    const int mode = tg->mode; const u64 thr = tg->thr;
    u64 cb = tg->rank + pc[tid], mb = tg->mass + pm[tid];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      bool hit = false;
      if (c[j]) {
        if (mode == M_RANK) hit = cb <= thr && thr < cb + c[j];
        else if (mode == M_GE) hit = mb < thr && mb + m[j] >= thr;
        else hit = mb <= thr && mb + m[j] > thr;
      }
      if (hit) { fb = BINS - 1 - (tid * 8 + j); fcb = cb; fmb = mb; fc = c[j]; fm = m[j]; }   // at most one bin satisfies the condition
      cb += c[j]; mb += m[j];
    }
  }
  __syncthreads();
  if (active && tid == 0) {
    if (fb < 0) tg->state = S_NONE;
    else {
      tg->prefix = (tg->prefix << lvl_bits(L)) | (u64)fb;
      const bool single = fc == 1 && (hrep != nullptr || tg->mode != M_GT);   // the draw needs the element itself: its composite comes with the bin
      if (single || L == 5) { tg->state = S_DONE; tg->rank = fcb + fc - 1; tg->mass = fmb + fm; if (hrep) tg->rep = hrep[fb]; }
      else { tg->rank = fcb; tg->mass = fmb; }
    }
  }
  __syncthreads();                                   // hrep[fb] is read above: nobody clears it before that
  if (zero) {
#pragma unroll
    for (int j = 0; j < 8; j++) { const int b = BINS - 1 - (tid * 8 + j); hcnt[b] = 0; hmass[b] = 0; if (hrep) hrep[b] = 0; }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_bs_select(BsArgs a, int L, int phase) {
  __shared__ float sv[NB];
  __shared__ int si[NB];
  __shared__ u64 total;
  const int row = blockIdx.x, tid = threadIdx.x;
  BsRow& r = a.rows[row];
  BsScr& sc = a.scr[row];
  const bool greedy = sc.greedy;
  unsigned* h1c = a.h1c + (size_t)row * BINS; u64* h1m = a.h1m + (size_t)row * BINS;
  unsigned* hc = a.hc + (size_t)row * 2 * BINS; u64* hm = a.hm + (size_t)row * 2 * BINS; u64* hrep = a.hrep + (size_t)row * BINS;
  if (!greedy) {
    if (phase == 1) {
      if (L == 1) {
        const u64 keep_k = (r.top_k > 0 && (long long)r.top_k < a.V) ? (u64)r.top_k : (u64)a.V;
        if (tid == 0) {
          sc.t[T_K].mode = M_RANK; sc.t[T_K].state = S_ACTIVE; sc.t[T_K].thr = keep_k - 1;
          if (r.top_p > 0.0f && r.top_p < 1.0f) { sc.t[T_A].mode = M_GE; sc.t[T_A].state = S_ACTIVE; sc.t[T_A].thr = (u64)ceil((double)r.top_p * 1152921504606846976.0); }
        }
        __syncthreads();
        select_target(&sc.t[T_K], h1c, h1m, nullptr, 1, false, &total);
        if (tid == 0) {
          sc.total = total;
          if (keep_k == (u64)a.V) { sc.t[T_K].state = S_DONE; sc.t[T_K].rank = keep_k - 1; sc.t[T_K].mass = total; }   // no top-k: everything is kept
        }
        __syncthreads();
        select_target(&sc.t[T_A], h1c, h1m, nullptr, 1, false, nullptr);
      } else {
        select_target(&sc.t[T_K], hc, hm, nullptr, L, true, nullptr);
        select_target(&sc.t[T_A], hc + BINS, hm + BINS, nullptr, L, true, nullptr);
      }
      if (L == 5) {   // both cuts are known: the kept prefix, its mass, the draw -- and the draw's level-1 bin
        if (tid == 0) {
          u64 keep = (u64)a.V, tot = sc.total;
          if (sc.t[T_K].state == S_DONE) { keep = sc.t[T_K].rank + 1; tot = sc.t[T_K].mass; }
          if (sc.t[T_A].state == S_DONE && sc.t[T_A].rank + 1 < keep) { keep = sc.t[T_A].rank + 1; tot = sc.t[T_A].mass; }
          if (r.min_p > 0.0f) {
            const u64 cut = sc.cnt_ge ? (u64)sc.cnt_ge : 1;
            if (cut < keep) { keep = cut; tot = sc.cnt_ge ? sc.mass_ge : mass_of(sc.p0key); }
          }
          u64 z = (r.seed + r.draw) + 0x9E3779B97F4A7C15ull;
          z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
          z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
          z = z ^ (z >> 31);
          const double totd = (double)tot * (1.0 / 1152921504606846976.0);
          const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0) * totd;
          u64 uf = (u64)(u * 1152921504606846976.0);
          if (tot && uf > tot - 1) uf = tot - 1;            // u < tot: the draw lands inside the kept prefix
          sc.t[T_C].mode = M_GT; sc.t[T_C].state = tot ? S_ACTIVE : S_NONE; sc.t[T_C].thr = uf;
          sc.t[T_C].prefix = sc.t[T_C].rank = sc.t[T_C].mass = sc.t[T_C].rep = 0;
        }
        __syncthreads();
        select_target(&sc.t[T_C], h1c, h1m, nullptr, 1, false, nullptr);
      }
    } else {
      select_target(&sc.t[T_C], hc, hm, hrep, L, true, nullptr);
    }
  }
  if (!(phase == 2 && L == 5)) return;
  // ---- the token ----
  long long tok = -1;
  if (!greedy && sc.t[T_C].state == S_DONE) tok = (long long)(0xFFFFFu - (unsigned)(sc.t[T_C].rep & 0xFFFFFu));
  if (greedy) {   // lowest index of the largest penalised logit, from the 128 partials of the scale pass
    if (tid < NB) { sv[tid] = a.amv[(size_t)row * NB + tid]; si[tid] = a.ami[(size_t)row * NB + tid]; }
    __syncthreads();
    for (int s = NB / 2; s > 0; s >>= 1) {
      if (tid < s && better(sv[tid + s], si[tid + s], sv[tid], si[tid])) { sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; }
      __syncthreads();
    }
    tok = si[0];
  }
  if (tid == 0) {
    if (tok < 0 || tok >= a.V) tok = 0;                     // a row with no mass at all (all -inf / NaN): some id in range
    r.ring[r.head & (WIN - 1)] = tok;
    r.head = (r.head + 1) & (WIN - 1);
    if (r.cnt < WIN) r.cnt = r.cnt + 1;
    r.draw = r.draw + 1;
    if (a.tokens_out) a.tokens_out[row] = tok;
    if (a.next) a.next[row] = tok;
    const int st = a.scr[0].step_snap;                      // read by prep, before any row advances *step
    if (a.log) a.log[(size_t)(st % a.logcap) * a.N + row] = tok;
    if (a.step && row == 0) *a.step = st + 1;
  }
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct bz_batch_sampler {
  bz_device* dev = nullptr;
  BsArgs a{};
  BzLpState* lp = nullptr;   // per-row logit bias / logprobs (bz_logprobs.hip), after bz_batch_sampler_enable
  bool used = false;         // has sampled or been captured: too late to enable
};
BzLpState*& bzk_batch_sampler_lp(bz_batch_sampler* s) { return s->lp; }
bz_device* bzk_batch_sampler_dev(const bz_batch_sampler* s) { return s->dev; }
bool bzk_batch_sampler_used(const bz_batch_sampler* s) { return s->used; }

int bzk_batch_sampler_dims(const bz_batch_sampler* s, int* N, long long* V) { *N = s->a.N; *V = s->a.V; return BZ_OK; }

// the 21 launches; next / log / step (nullable) are the batch graph's feedback buffer, pinned token log [logcap][N] and step counter
int bzk_batch_sample(hipStream_t st, bz_batch_sampler* s, const float* logits, long long* tokens_out, long long* next, long long* log, int* step, int logcap) {
  s->used = true;
  BsArgs a = s->a;
  a.logits = logits; a.tokens_out = tokens_out; a.next = next; a.log = log; a.step = step; a.logcap = logcap > 0 ? logcap : 1;
  const dim3 rows(a.N), grid(NB, a.N), blk(256);
  hipLaunchKernelGGL(k_bs_prep, rows, blk, 0, st, a);
  hipLaunchKernelGGL(k_bs_scale, grid, blk, 0, st, a);
  hipLaunchKernelGGL(k_bs_exp, grid, blk, 0, st, a);
  hipLaunchKernelGGL(k_bs_norm, grid, blk, 0, st, a);
  hipLaunchKernelGGL(k_bs_select, rows, blk, 0, st, a, 1, 1);
  for (int L = 2; L <= 5; L++) {
    hipLaunchKernelGGL((k_bs_level<2, false>), grid, blk, 0, st, a, L, (int)T_K);
    hipLaunchKernelGGL(k_bs_select, rows, blk, 0, st, a, L, 1);
  }
  for (int L = 2; L <= 5; L++) {
    hipLaunchKernelGGL((k_bs_level<1, true>), grid, blk, 0, st, a, L, (int)T_C);
    hipLaunchKernelGGL(k_bs_select, rows, blk, 0, st, a, L, 2);
  }
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

extern "C" int bz_batch_sampler_free(bz_batch_sampler* s) {
  BZ_API_BEGIN
  if (!s) return BZ_OK;
  if (s->dev) { hipSetDevice(s->dev->id); hipStreamSynchronize(s->dev->stream); }
  BsArgs& a = s->a;
  for (void* p : {(void*)a.rows, (void*)a.scr, (void*)a.l2, (void*)a.pmax, (void*)a.psum, (void*)a.amv, (void*)a.ami, (void*)a.pen_id, (void*)a.pen_cnt,
                  (void*)a.h1c, (void*)a.h1m, (void*)a.hc, (void*)a.hm, (void*)a.hrep}) if (p) hipFree(p);
  bzk_lp_free(s->lp);
  if (s->dev) bz_dev_release(s->dev);
  delete s;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_batch_sampler_create(bz_device* dev, int N, int64_t V, bz_batch_sampler** out) {
  BZ_API_BEGIN
  if (!out) BZ_FAIL(BZ_E_INVALID, "batch sampler create: null output pointer");
  *out = nullptr;
  if (!dev) BZ_FAIL(BZ_E_INVALID, "batch sampler create: null device");
  if (N < 1 || N > 512) BZ_FAIL(BZ_E_INVALID, "batch sampler create: N = %d out of range (1 <= N <= 512)", N);
  if (V < 1 || V > VMAX) BZ_FAIL(BZ_E_INVALID, "batch sampler create: V = %lld out of range (1 <= V <= %lld)", (long long)V, VMAX);
  BZ_HIP(hipSetDevice(dev->id));
  bz_batch_sampler* s = new bz_batch_sampler();
  bz_dev_retain(dev); s->dev = dev;
  BsArgs& a = s->a;
  a.N = N; a.V = V;
  const size_t n = (size_t)N;
  struct { void** p; size_t bytes; } al[] = {
    {(void**)&a.rows, n * sizeof(BsRow)}, {(void**)&a.scr, n * sizeof(BsScr)}, {(void**)&a.l2, n * (size_t)V * 4}, {(void**)&a.pmax, n * NB * 4}, {(void**)&a.psum, n * NB * 8},
    {(void**)&a.amv, n * NB * 4}, {(void**)&a.ami, n * NB * 4}, {(void**)&a.pen_id, n * WIN * 8}, {(void**)&a.pen_cnt, n * WIN * 4},
    {(void**)&a.h1c, n * BINS * 4}, {(void**)&a.h1m, n * BINS * 8}, {(void**)&a.hc, n * 2 * BINS * 4}, {(void**)&a.hm, n * 2 * BINS * 8}, {(void**)&a.hrep, n * BINS * 8}};
  for (auto& e : al) {
    if (hipMalloc(e.p, e.bytes) != hipSuccess) { *e.p = nullptr; (void)hipGetLastError(); bz_batch_sampler_free(s); BZ_FAIL(BZ_E_OOM, "batch sampler create: out of device memory (%zu bytes)", e.bytes); }
    if (hipMemset(*e.p, 0, e.bytes) != hipSuccess) { bz_batch_sampler_free(s); BZ_FAIL(BZ_E_HIP, "batch sampler create: hipMemset failed"); }
  }
  // every row starts greedy, without penalties, with an empty history
  std::vector<BsRow> init(n);
  for (auto& r : init) { memset(&r, 0, sizeof(r)); r.top_p = 1.0f; r.rp = 1.0f; r.last_n = 64; }
  if (hipMemcpy(a.rows, init.data(), n * sizeof(BsRow), hipMemcpyHostToDevice) != hipSuccess) { bz_batch_sampler_free(s); BZ_FAIL(BZ_E_HIP, "batch sampler create: upload failed"); }
  BZ_HIP(hipDeviceSynchronize());
  *out = s;
  return BZ_OK;
  BZ_API_END
}

// the parameter checks of set_row; `who` names the caller in the message
int bzk_batch_sampler_check_row(const bz_row_sampling* p, const char* who) {
  if (!(p->temperature >= 0.0f)) BZ_FAIL(BZ_E_INVALID, "%s: temperature must be >= 0 (got %g)", who, (double)p->temperature);
  const bool pen = p->repeat_penalty != 1.0f || p->frequency_penalty != 0.0f || p->presence_penalty != 0.0f;
  if (pen && (p->repeat_last_n < 1 || p->repeat_last_n > WIN))
    BZ_FAIL(BZ_E_INVALID, "%s: repeat_last_n = %d out of range (1 <= repeat_last_n <= %d while a penalty is active)", who, p->repeat_last_n, WIN);
  return BZ_OK;
}
static void fill_row(BsRow& r, const bz_row_sampling* p, const int64_t* history, int n_history, int64_t draw_index) {
  const bool pen = p->repeat_penalty != 1.0f || p->frequency_penalty != 0.0f || p->presence_penalty != 0.0f;
  memset(&r, 0, sizeof(r));
  r.temperature = p->temperature; r.top_k = p->top_k; r.top_p = p->top_p; r.min_p = p->min_p;
  r.rp = p->repeat_penalty; r.fp = p->frequency_penalty; r.pp = p->presence_penalty; r.last_n = pen ? p->repeat_last_n : 0;
  r.seed = p->seed; r.draw = (u64)draw_index;
  const int w = std::min(n_history, WIN);
  for (int i = 0; i < w; i++) r.ring[i] = history[n_history - w + i];
  r.cnt = w; r.head = w & (WIN - 1);
}
size_t bzk_batch_sampler_row_bytes() { return sizeof(BsRow); }
// set_row without the wait (request engine): the row is built in `stage` (pinned, bzk_batch_sampler_row_bytes(), the caller's until the stream has passed the copy)
int bzk_batch_sampler_stage_row(hipStream_t st, bz_batch_sampler* s, int row, const bz_row_sampling* p, const int64_t* history, int n_history, int64_t draw_index, void* stage) {
  fill_row(*(BsRow*)stage, p, history, n_history, draw_index);
  BZ_HIP(hipMemcpyAsync(s->a.rows + row, stage, sizeof(BsRow), hipMemcpyHostToDevice, st));
  return BZ_OK;
}

extern "C" int bz_batch_sampler_set_row(bz_batch_sampler* s, int row, const bz_row_sampling* p, const int64_t* history, int n_history, int64_t draw_index) {
  BZ_API_BEGIN
  if (!s || !p) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row: null argument");
  if (row < 0 || row >= s->a.N) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row: row %d out of range (N = %d)", row, s->a.N);
  BZ_TRY(bzk_batch_sampler_check_row(p, "batch sampler set_row"));
  if (n_history < 0 || (n_history > 0 && !history)) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row: bad history (n_history = %d)", n_history);
  if (draw_index < 0) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row: negative draw index");
  BsRow r;
  fill_row(r, p, history, n_history, draw_index);
  std::lock_guard<std::mutex> dlock__(s->dev->mu);
  BZ_HIP(hipSetDevice(s->dev->id));
  BZ_HIP(hipMemcpyAsync(s->a.rows + row, &r, sizeof(r), hipMemcpyHostToDevice, s->dev->stream));   // stream-ordered: after the replays already enqueued
  BZ_HIP(hipStreamSynchronize(s->dev->stream));
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_batch_sampler_sample(bz_batch_sampler* s, const bz_tensor* logits, bz_tensor* tokens_out) {
  BZ_API_BEGIN
  if (!s || !logits || !tokens_out) BZ_FAIL(BZ_E_INVALID, "batch sampler sample: null argument");
  const size_t N = (size_t)s->a.N, V = (size_t)s->a.V;
  if (logits->dtype != BZ_F32 || logits->nbytes != N * V * 4) BZ_FAIL(BZ_E_INVALID, "batch sampler sample: logits must be F32 [%zu,%zu] (got dtype %d, %zu bytes)", N, V, logits->dtype, logits->nbytes);
  if (tokens_out->dtype != BZ_I64 || tokens_out->nbytes != N * 8) BZ_FAIL(BZ_E_INVALID, "batch sampler sample: tokens_out must be I64 [%zu] (got dtype %d, %zu bytes)", N, tokens_out->dtype, tokens_out->nbytes);
  std::lock_guard<std::mutex> dlock__(s->dev->mu);
  BZ_HIP(hipSetDevice(s->dev->id));
  // with bz_batch_sampler_enable: logprobs phase A on the raw rows, the bias in place, the pick, the records (nothing is launched for a flag that is off)
  hipStream_t st = s->dev->stream;
  BZ_TRY(bzk_lp_pre(st, s, (const float*)logits->ptr));
  BZ_TRY(bzk_lp_bias(st, s, (float*)logits->ptr));
  BZ_TRY(bzk_batch_sample(st, s, (const float*)logits->ptr, (long long*)tokens_out->ptr, nullptr, nullptr, nullptr, 0));
  return bzk_lp_post(st, s, (const float*)logits->ptr, (const long long*)tokens_out->ptr, nullptr);
  BZ_API_END
}
