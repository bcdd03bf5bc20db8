// bz_logprobs.hip -- per-row logit bias and logprobs for a decode batch, on the device: what the single-sequence loop does on the host with
// bz_apply_logit_bias / bz_compute_logprobs (sampling.rs:464-480, 197-256; config/generation.rs:65-74), as launches around the batched sampler's so that a
// captured step needs no logits row on the host.  The state hangs off the batch sampler handle (bz_batch_sampler_enable); a sampler without it launches nothing here.
//
// Order in a step (sampling.rs:414-431): phase A on the raw logits -> grammar mask -> bias -> the sampler's launches -> phase C.
//   k_lp_max     [128, N]  phase A.  Per block of a row with logprobs on: the maximum of its slice (256 ids out of every 32768).
//   k_lp_sum     [128, N]  phase A.  M = the maximum of the 128 block maxima; q_i = floor(bz_expf(x_i - M) * 2^40) as u64; the block's integer sum goes to the row's
//                          S with one atomic: integer addition is exactly associative, so S does not depend on arrival order.  V <= 2^20: S <= 2^60.
//                          Then the block's candidates for the row's first n entries in (logit descending, id ascending) order.  T = the n-th largest of the 128
//                          block maxima is a floor: n entries of the row are >= T, so nothing below T is among the first n, and a block whose maximum is below T
//                          leaves at once (almost all of them on a real row).  The others run rounds of "largest composite below the previous round's" until the
//                          winner falls below T: composite = (order-preserving bits of x : ~id), so one u64 maximum IS the order, ties included; nothing is
//                          marked, no list can overflow.  A round is a pass over the block's slice and one block reduction; an all-equal row runs all n rounds in
//                          every block (the worst case) and still returns ids 0 .. n-1.
//   k_bias_rows  [2, N]    one thread per entry of the row's bias list: keep the raw logit, add the bias in place.  The host deduplicated the list (unique in-range
//                          ids), so no two threads touch one logit.
//   k_lp_record  [N]       phase C.  lse = (float)log((double)S * 2^-40) + M; the row's n first entries = n rounds over the 128 x n block candidates (the global
//                          first n are among them), each thread's candidates in registers; the picked token's raw logit comes from the bias list's saved values
//                          when the token is in it (a masked token is never picked); one record per row into the pinned ring slot of this step.
// Every logprob is the f32 subtraction x - lse.  The only libm call is the double log, once per row.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "bz_internal.h"
#include "bz_lp_dev.h"

namespace {
constexpr int NB = 128;                         // blocks per row of the streaming passes
constexpr int TOPN = BZ_TOP_LOGPROBS_MAX;
constexpr int BMAX = BZ_LOGIT_BIAS_MAX;
constexpr int CPT = (NB * TOPN + 255) / 256;    // block candidates per thread of k_lp_record

struct LpArgs {
  int N; long long V; unsigned flags;
  unsigned* b_id; float* b_val; float* b_save; int* b_cnt;      // [N][BMAX] x 3, [N]
  int* top_n; float* pmax; u64* S; u64* cand;                   // [N], [N][NB], [N], [N][NB][TOPN]
  bz_logprobs_record* ring; int ringcap;                        // pinned host [ringcap][N]
};

__global__ __launch_bounds__(256) void k_lp_max(LpArgs a, const float* logits) {
  __shared__ float redf[4];
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  if (a.top_n[row] < 0) return;
  const float* x = logits + (size_t)row * a.V;
  if (blk == 0 && tid == 0) a.S[row] = 0;
  float m = -INFINITY;
  for (long long i = (long long)blk * 256 + tid; i < a.V; i += (long long)NB * 256) m = fmaxf(m, x[i]);
  m = block_max_f(m, redf);
  if (tid == 0) a.pmax[(size_t)row * NB + blk] = m;
}

__global__ __launch_bounds__(256) void k_lp_sum(LpArgs a, const float* logits) {
  __shared__ float redf[4];
  __shared__ u64 part[4];
  __shared__ float pm[NB];
  __shared__ float tsh;
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  const int top_n = a.top_n[row];
  if (top_n < 0) return;
  const float* x = logits + (size_t)row * a.V;
  const int n = min(top_n, TOPN);
  u64* out = a.cand + ((size_t)row * NB + blk) * TOPN;
  if (tid < n) out[tid] = 0;                                       // none, until a round below says otherwise (the barriers of the reductions order the two writes)
  if (tid < NB) pm[tid] = a.pmax[(size_t)row * NB + tid];
  const float M = block_max_f(tid < NB ? a.pmax[(size_t)row * NB + tid] : -INFINITY, redf);
  u64 s = 0;
  for (long long i = (long long)blk * 256 + tid; i < a.V; i += (long long)NB * 256) {
    const float e = bz_expf(x[i] - M);
    if (e > 0.0f) s += (u64)((double)e * 1099511627776.0);       // e <= 1: at most 2^40; a NaN (a row of -inf) adds nothing
  }
  for (int k = 32; k >= 1; k >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)s, k, 64), hi = __shfl_xor((unsigned)(s >> 32), k, 64);
    s += ((u64)hi << 32) | lo;
  }
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) { const u64 t = (part[0] + part[1]) + (part[2] + part[3]); if (t) atomicAdd(&a.S[row], t); }
  if (n == 0) return;
  // T = the n-th largest of the row's 128 block maxima: n entries of the row are >= T, so an entry below T is not among the row's first n
  if (tid < NB) {
    const float v = pm[tid];
    int rank = 0;
    for (int j = 0; j < NB; j++) { const float w = pm[j]; rank += (w > v || (w == v && j < tid)) ? 1 : 0; }
    if (rank == n - 1) tsh = v;
  }
  __syncthreads();
  const u64 floor_c = lp_composite(tsh, 0xFFFFFFFFll);            // every entry with a logit >= T has a composite >= this one
  if (lp_composite(pm[blk], 0) < floor_c) return;                 // nothing of this slice reaches T
  u64 prev = ~0ull;
  for (int r = 0; r < n; r++) {
    u64 best = 0;
    for (long long i = (long long)blk * 256 + tid; i < a.V; i += (long long)NB * 256) {
      const u64 c = lp_composite(x[i], i);
      if (c < prev) best = umax64(best, c);
    }
    best = block_max_u64(best, part);
    if (best < floor_c) break;                                    // below T, or the slice is used up: the slots from r on stay none
    if (tid == 0) out[r] = best;
    prev = best;
  }
}

__global__ __launch_bounds__(256) void k_bias_rows(LpArgs a, float* logits) {
  const int row = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  const int cnt = min(a.b_cnt[row], BMAX);
  if (e >= cnt) return;
  const size_t at = (size_t)row * BMAX + e;
  const unsigned id = a.b_id[at];
  if ((long long)id >= a.V) return;                              // the host dropped these already
  float* p = logits + (size_t)row * a.V + id;
  const float v = *p;
  a.b_save[at] = v;
  *p = v + a.b_val[at];
}

__global__ __launch_bounds__(256) void k_lp_record(LpArgs a, const float* logits, const long long* tokens, const int* step) {
  __shared__ u64 red[4];
  __shared__ float redf[4];
  __shared__ float saved; __shared__ int have;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int at = step ? (((*step - 1) % a.ringcap) + a.ringcap) % a.ringcap : 0;   // the pick has counted this step already
  bz_logprobs_record* rec = a.ring + (size_t)at * a.N + row;
  const int top_n = a.top_n[row];
  if (top_n < 0) { if (tid == 0) rec->n_top = -1; return; }
  const float M = block_max_f(tid < NB ? a.pmax[(size_t)row * NB + tid] : -INFINITY, redf);
  const float L = (float)log((double)a.S[row] * (1.0 / 1099511627776.0));
  const float lse = L + M;
  // the picked token's raw logit: the bias list kept it if the bias launch changed it
  const long long tok = tokens[row];
  if (tid == 0) have = 0;
  __syncthreads();
  if (a.b_cnt) {
    const int cnt = min(a.b_cnt[row], BMAX);
    for (int e = tid; e < cnt; e += 256)
      if ((long long)a.b_id[(size_t)row * BMAX + e] == tok) { saved = a.b_save[(size_t)row * BMAX + e]; have = 1; }   // unique ids: one writer at most
  }
  __syncthreads();
  if (tid == 0) {
    float xr = -INFINITY;
    if (tok >= 0 && tok < a.V) xr = have ? saved : logits[(size_t)row * a.V + tok];
    rec->token = tok; rec->logprob = xr - lse; rec->lse = lse;
  }
  // the row's first n entries among the blocks' candidates
  const int n = min(top_n, TOPN);
  u64 c[CPT];
#pragma unroll
  for (int j = 0; j < CPT; j++) {
    const int k = tid + j * 256;
    c[j] = (k < NB * TOPN && (k % TOPN) < n) ? a.cand[(size_t)row * NB * TOPN + k] : 0;   // slots past n hold an earlier step's values
  }
  u64 prev = ~0ull;
  int got = 0;
  for (int r = 0; r < n; r++) {
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < CPT; j++) if (c[j] < prev) best = umax64(best, c[j]);
    best = block_max_u64(best, red);
    if (best == 0) break;
    if (tid == 0) { rec->top_ids[r] = 0xFFFFFFFFu - (unsigned)best; rec->top_logprobs[r] = lp_logit_of(best) - lse; }
    prev = best; got = r + 1;
  }
  if (tid == 0) rec->n_top = got;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
struct BzLpState { LpArgs a{}; };

void bzk_lp_free(BzLpState* lp) {
  if (!lp) return;
  LpArgs& a = lp->a;
  for (void* p : {(void*)a.b_id, (void*)a.b_val, (void*)a.b_save, (void*)a.b_cnt, (void*)a.top_n, (void*)a.pmax, (void*)a.S, (void*)a.cand}) if (p) hipFree(p);
  if (a.ring) hipHostFree(a.ring);
  delete lp;
}
unsigned bzk_lp_flags(bz_batch_sampler* s) { BzLpState* lp = bzk_batch_sampler_lp(s); return lp ? lp->a.flags : 0u; }
const bz_logprobs_record* bzk_lp_ring(bz_batch_sampler* s) { BzLpState* lp = bzk_batch_sampler_lp(s); return lp ? lp->a.ring : nullptr; }
void bzk_lp_row_ptrs(bz_batch_sampler* s, int** b_cnt, int** top_n) {
  BzLpState* lp = s ? bzk_batch_sampler_lp(s) : nullptr;
  *b_cnt = lp ? lp->a.b_cnt : nullptr; *top_n = lp ? lp->a.top_n : nullptr;
}

// the three places of a step; each is nothing on a sampler without the flag
int bzk_lp_pre(hipStream_t st, bz_batch_sampler* s, const float* logits) {
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp || !(lp->a.flags & BZ_BS_LOGPROBS)) return BZ_OK;
  hipLaunchKernelGGL(k_lp_max, dim3(NB, lp->a.N), dim3(256), 0, st, lp->a, logits);
  hipLaunchKernelGGL(k_lp_sum, dim3(NB, lp->a.N), dim3(256), 0, st, lp->a, logits);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
int bzk_lp_bias(hipStream_t st, bz_batch_sampler* s, float* logits) {
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp || !(lp->a.flags & BZ_BS_BIAS)) return BZ_OK;
  hipLaunchKernelGGL(k_bias_rows, dim3(BMAX / 256, lp->a.N), dim3(256), 0, st, lp->a, logits);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
int bzk_lp_post(hipStream_t st, bz_batch_sampler* s, const float* logits, const long long* tokens, const int* step) {
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp || !(lp->a.flags & BZ_BS_LOGPROBS)) return BZ_OK;
  hipLaunchKernelGGL(k_lp_record, dim3(lp->a.N), dim3(256), 0, st, lp->a, logits, tokens, step);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// sampling.rs:470-476 builds a dense bias vector in which later entries of the map overwrite earlier ones and ids >= V find no place: the same list, sparse
static int lp_dedupe(long long V, const uint32_t* ids, const float* vals, int n, std::vector<uint32_t>& oi, std::vector<float>& ov, const char* who) {
  if (n < 0 || (n > 0 && (!ids || !vals))) BZ_FAIL(BZ_E_INVALID, "%s: bad bias arrays (n_logit_bias = %d)", who, n);
  std::map<uint32_t, size_t> at;
  oi.clear(); ov.clear();
  for (int i = 0; i < n; i++) {
    if (!std::isfinite(vals[i])) BZ_FAIL(BZ_E_INVALID, "%s: bias entry %d (id %u) is %g, not a finite number", who, i, ids[i], (double)vals[i]);
    if ((long long)ids[i] >= V) continue;
    auto it = at.find(ids[i]);
    if (it == at.end()) { at[ids[i]] = oi.size(); oi.push_back(ids[i]); ov.push_back(vals[i]); }
    else ov[it->second] = vals[i];
  }
  return BZ_OK;
}
static int lp_check_count(size_t cnt, const char* who) {
  if (cnt > (size_t)BMAX) BZ_FAIL(BZ_E_INVALID, "%s: %zu bias entries after deduplication, at most %d", who, cnt, BMAX);
  return BZ_OK;
}
extern "C" int bz_logit_bias_dedupe(int64_t V, const uint32_t* ids, const float* vals, int n, uint32_t* ids_out, float* vals_out, int* n_out) {
  BZ_API_BEGIN
  if (!n_out || V < 1 || (n > 0 && (!ids_out || !vals_out))) BZ_FAIL(BZ_E_INVALID, "logit_bias_dedupe: bad argument");
  std::vector<uint32_t> oi; std::vector<float> ov;
  BZ_TRY(lp_dedupe(V, ids, vals, n, oi, ov, "logit_bias_dedupe"));
  for (size_t i = 0; i < oi.size(); i++) { ids_out[i] = oi[i]; vals_out[i] = ov[i]; }
  *n_out = (int)oi.size();
  return BZ_OK;
  BZ_API_END
}
// the checks of a request's extras without a device (engine submit); the deduplicated list comes back for the row write
int bzk_lp_check_bias(long long V, const uint32_t* ids, const float* vals, int n, std::vector<uint32_t>& oi, std::vector<float>& ov, const char* who) {
  BZ_TRY(lp_dedupe(V, ids, vals, n, oi, ov, who));
  return lp_check_count(oi.size(), who);
}

extern "C" int bz_batch_sampler_enable(bz_batch_sampler* s, uint32_t flags) {
  BZ_API_BEGIN
  if (!s) BZ_FAIL(BZ_E_INVALID, "batch sampler enable: null sampler");
  if (flags == 0 || (flags & ~(uint32_t)(BZ_BS_BIAS | BZ_BS_LOGPROBS))) BZ_FAIL(BZ_E_INVALID, "batch sampler enable: flags = %u (BZ_BS_BIAS = 1, BZ_BS_LOGPROBS = 2)", flags);
  if (bzk_batch_sampler_lp(s)) BZ_FAIL(BZ_E_INVALID, "batch sampler enable: already enabled (one call, with every flag wanted)");
  if (bzk_batch_sampler_used(s)) BZ_FAIL(BZ_E_INVALID, "batch sampler enable: the sampler has sampled or been captured already");
  bz_device* dev = bzk_batch_sampler_dev(s);
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  BzLpState* lp = new BzLpState();
  LpArgs& a = lp->a;
  bzk_batch_sampler_dims(s, &a.N, &a.V);
  a.flags = flags; a.ringcap = bz_batch_graph::LOGCAP;
  const size_t n = (size_t)a.N;
  struct { void** p; size_t bytes; bool on; int fill; } al[] = {
    {(void**)&a.b_id, n * BMAX * 4, (flags & BZ_BS_BIAS) != 0, 0}, {(void**)&a.b_val, n * BMAX * 4, (flags & BZ_BS_BIAS) != 0, 0},
    {(void**)&a.b_save, n * BMAX * 4, (flags & BZ_BS_BIAS) != 0, 0}, {(void**)&a.b_cnt, n * 4, (flags & BZ_BS_BIAS) != 0, 0},
    {(void**)&a.top_n, n * 4, (flags & BZ_BS_LOGPROBS) != 0, 0xff},           // every row: -1, off
    {(void**)&a.pmax, n * NB * 4, (flags & BZ_BS_LOGPROBS) != 0, 0}, {(void**)&a.S, n * 8, (flags & BZ_BS_LOGPROBS) != 0, 0},
    {(void**)&a.cand, n * NB * TOPN * 8, (flags & BZ_BS_LOGPROBS) != 0, 0}};
  for (auto& e : al) {
    if (!e.on) continue;
    if (hipMalloc(e.p, e.bytes) != hipSuccess) { *e.p = nullptr; (void)hipGetLastError(); bzk_lp_free(lp); BZ_FAIL(BZ_E_OOM, "batch sampler enable: out of device memory (%zu bytes)", e.bytes); }
    if (hipMemset(*e.p, e.fill, e.bytes) != hipSuccess) { bzk_lp_free(lp); BZ_FAIL(BZ_E_HIP, "batch sampler enable: hipMemset failed"); }
  }
  if (flags & BZ_BS_LOGPROBS) {
    const size_t bytes = sizeof(bz_logprobs_record) * (size_t)a.ringcap * n;
    if (hipHostMalloc((void**)&a.ring, bytes, hipHostMallocDefault) != hipSuccess) { a.ring = nullptr; (void)hipGetLastError(); bzk_lp_free(lp); BZ_FAIL(BZ_E_OOM, "batch sampler enable: out of pinned memory (%zu bytes)", bytes); }
    memset(a.ring, 0xff, bytes);                                   // n_top = -1 everywhere
  }
  if (hipDeviceSynchronize() != hipSuccess) { bzk_lp_free(lp); BZ_FAIL(BZ_E_HIP, "batch sampler enable: the device failed"); }
  bzk_batch_sampler_lp(s) = lp;
  return BZ_OK;
  BZ_API_END
}

size_t bzk_lp_stage_bytes() { return 8 + (size_t)BMAX * 8; }
// the row's top_n and bias list without the wait (request engine): built in `stage` (pinned, bzk_lp_stage_bytes(), the caller's until the stream has passed the copies);
// ids / vals: cnt deduplicated entries (bzk_lp_check_bias)
int bzk_lp_stage_row(hipStream_t st, bz_batch_sampler* s, int row, int top_n, const uint32_t* ids, const float* vals, int cnt, void* stage) {
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp) return BZ_OK;
  LpArgs& a = lp->a;
  int* hd = (int*)stage; uint32_t* si = (uint32_t*)((char*)stage + 8); float* sv = (float*)((char*)stage + 8 + (size_t)BMAX * 4);
  hd[0] = top_n; hd[1] = cnt;
  for (int i = 0; i < cnt; i++) { si[i] = ids[i]; sv[i] = vals[i]; }
  if (a.top_n) BZ_HIP(hipMemcpyAsync(a.top_n + row, &hd[0], 4, hipMemcpyHostToDevice, st));
  if (a.b_cnt) {
    if (cnt > 0) {
      BZ_HIP(hipMemcpyAsync(a.b_id + (size_t)row * BMAX, si, (size_t)cnt * 4, hipMemcpyHostToDevice, st));
      BZ_HIP(hipMemcpyAsync(a.b_val + (size_t)row * BMAX, sv, (size_t)cnt * 4, hipMemcpyHostToDevice, st));
    }
    BZ_HIP(hipMemcpyAsync(a.b_cnt + row, &hd[1], 4, hipMemcpyHostToDevice, st));
  }
  return BZ_OK;
}

extern "C" int bz_batch_sampler_set_row_bias(bz_batch_sampler* s, int row, const uint32_t* ids, const float* vals, int n) {
  BZ_API_BEGIN
  if (!s) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_bias: null sampler");
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp || !(lp->a.flags & BZ_BS_BIAS)) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_bias: the sampler did not enable BZ_BS_BIAS (bz_batch_sampler_enable)");
  LpArgs& a = lp->a;
  if (row < 0 || row >= a.N) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_bias: row %d out of range (N = %d)", row, a.N);
  std::vector<uint32_t> oi; std::vector<float> ov;
  BZ_TRY(bzk_lp_check_bias(a.V, ids, vals, n, oi, ov, "batch sampler set_row_bias"));
  const int cnt = (int)oi.size();
  bz_device* dev = bzk_batch_sampler_dev(s);
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  if (cnt > 0) {
    BZ_HIP(hipMemcpyAsync(a.b_id + (size_t)row * BMAX, oi.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, dev->stream));   // stream-ordered: after the replays already enqueued
    BZ_HIP(hipMemcpyAsync(a.b_val + (size_t)row * BMAX, ov.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, dev->stream));
  }
  BZ_HIP(hipMemcpyAsync(a.b_cnt + row, &cnt, 4, hipMemcpyHostToDevice, dev->stream));
  BZ_HIP(hipStreamSynchronize(dev->stream));
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_batch_sampler_set_row_logprobs(bz_batch_sampler* s, int row, int top_n) {
  BZ_API_BEGIN
  if (!s) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_logprobs: null sampler");
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp || !(lp->a.flags & BZ_BS_LOGPROBS)) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_logprobs: the sampler did not enable BZ_BS_LOGPROBS (bz_batch_sampler_enable)");
  if (row < 0 || row >= lp->a.N) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_logprobs: row %d out of range (N = %d)", row, lp->a.N);
  if (top_n < -1 || top_n > TOPN) BZ_FAIL(BZ_E_INVALID, "batch sampler set_row_logprobs: top_n = %d out of range (-1 = off, 0 .. %d)", top_n, TOPN);
  bz_device* dev = bzk_batch_sampler_dev(s);
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  BZ_HIP(hipMemcpyAsync(lp->a.top_n + row, &top_n, 4, hipMemcpyHostToDevice, dev->stream));
  BZ_HIP(hipStreamSynchronize(dev->stream));
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_batch_sampler_read_logprobs(bz_batch_sampler* s, bz_logprobs_record* out) {
  BZ_API_BEGIN
  if (!s || !out) BZ_FAIL(BZ_E_INVALID, "batch sampler read_logprobs: null argument");
  BzLpState* lp = bzk_batch_sampler_lp(s);
  if (!lp || !lp->a.ring) BZ_FAIL(BZ_E_INVALID, "batch sampler read_logprobs: the sampler did not enable BZ_BS_LOGPROBS (bz_batch_sampler_enable)");
  bz_device* dev = bzk_batch_sampler_dev(s);
  BZ_HIP(hipSetDevice(dev->id));
  BZ_HIP(hipStreamSynchronize(dev->stream));
  memcpy(out, lp->a.ring, sizeof(bz_logprobs_record) * (size_t)lp->a.N);     // an eager call has no step counter: slot 0
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_decode_batch_graph_read_logprobs(bz_batch_graph* g, int64_t step, bz_logprobs_record* out) {
  BZ_API_BEGIN
  if (!g || !out || step < 0 || step >= g->replays || step < g->replays - bz_batch_graph::LOGCAP) BZ_FAIL(BZ_E_INVALID, "batch graph read_logprobs: step out of range");
  const bz_logprobs_record* ring = g->sampler ? bzk_lp_ring(g->sampler) : nullptr;
  if (!ring) BZ_FAIL(BZ_E_INVALID, "batch graph read_logprobs: the graph's sampler did not enable BZ_BS_LOGPROBS (bz_batch_sampler_enable before the capture)");
  BZ_HIP(hipSetDevice(g->dev->id));
  BZ_HIP(hipStreamSynchronize(g->dev->stream));
  memcpy(out, ring + (size_t)(step % bz_batch_graph::LOGCAP) * g->N, sizeof(bz_logprobs_record) * (size_t)g->N);
  return BZ_OK;
  BZ_API_END
}
