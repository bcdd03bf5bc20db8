// bz_score.hip -- the sink of a prompt's rows: log-likelihoods of given tokens (bz_score_*) and pooled contextual embeddings (bz_embed_*), plus the two op-level
// calls and the host evaluations of both definitions.  Use cases: echo + logprobs, perplexity and the loglikelihood requests of evaluation harnesses
// (sampling.rs:197-256 is the row arithmetic); /v1/embeddings and /rerank (Executor::get_embeddings, engine/executor_embed.rs:33-55; server/pooling.rs:4-47;
// server/rerank.rs:139-171,206).  bz_host.hip decides WHICH rows arrive here (the tail of a prompt chunk, or the row of a token-by-token step); this file is what
// becomes of them.
//
// Scoring, per row x of F32 [R, V] with a target t (device I64; outside 0 .. V-1: the row is not scored).  The arithmetic is bz_logprobs.hip's, through the shared
// device functions of bz_lp_dev.h; those kernels take the sampler's N <= 512 rows, per-row device parameters and pinned ring, these take any number of rows:
//   k_sc_max     [128, rows]  per block: the maximum of its slice (256 ids out of every 32768); block 0 clears the row's sum and rank.
//   k_sc_sum     [128, rows]  M = the maximum of the 128 block maxima; q_i = floor(bz_expf(x_i - M) * 2^40) as u64; one integer atomic add per non-empty block and
//                             row into S (integer addition is exactly associative: S does not depend on arrival order; V < 2^24 keeps it below 2^64).  In the same
//                             pass the block counts its ids whose composite key (lp_composite: logit descending, id ascending, -0 as +0, NaN nowhere) is greater than
//                             the target's: one integer atomic add into the row's RANK = #{x_j > x_t} + #{x_j == x_t, j < t}.  Then the block's candidates for the
//                             row's first n entries, exactly as k_lp_sum finds them (floor T = the n-th largest block maximum; rounds of "largest key below the
//                             previous round's").
//   k_sc_record  [rows]       lse = (float)log((double)S * 2^-40) + M -- the only libm call, once per row; logit = x_t, logprob = x_t - lse (f32), rank (-1 when
//                             x_t is NaN), the first n entries among the 128 x n candidates; one bz_score_row per row into a device buffer.
// The rows of a call are passed over in sub-batches of 256 (the candidate buffer is [256][128][20] u64 = 5.2 MB instead of 42 MB for a 2048-row chunk): rows are
// independent, so no bit can change.  The records come to the host once per call through pinned staging.  Plain vector loads and stores throughout.
//
// The logits workspace of a scoring call whose head is the chunk GEMM is F32 [min(S, chunk), vocab]: 1.05 GB for a full 2 048-row chunk at a 128 256 vocabulary
// (a model-lifetime allocation, made on first use and grown on demand), against S * vocab * 4 bytes on the caller's side for BZ_FWD_ALL_LOGITS -- 16.8 GB at 32 k.
// Why the head is not fused with the reduction: DESIGN.md section 4 "Scoring and embeddings".
//
// Pooling, hidden F32 [n, H] rows of a chunk -> the call's result: NONE copies, CLS is row 0 of the call, LAST row S - 1; MEAN has one thread per column add
// (double)x[s][j] in ROW ORDER into a device-resident double [H] that persists across the call's chunks, finish (float)(sum / S): the order is fixed, so the result is
// a pure function of the rows.  ASSUMPTION: the reference's mean (pooling.rs) is an f32 running sum in an order its backend decides; this one is deliberately not
// that (the reference's own test vectors come out identical either way).  normalize: norm = sqrt(sum_j (double)v_j^2) (any order: the squares are exact in double),
// v_j = (float)((double)v_j / norm) if norm > 1e-12, else unchanged (pooling.rs:40-47).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "bz_internal.h"
#include "bz_lp_dev.h"

namespace {
constexpr int NB = 128;                         // blocks per row of the streaming passes
constexpr int TOPN = BZ_TOP_LOGPROBS_MAX;
constexpr int CPT = (NB * TOPN + 255) / 256;    // block candidates per thread of k_sc_record
constexpr int RB = 256;                         // rows per sub-batch
constexpr long long VMAX = 1ll << 24;

struct ScArgs {
  long long V; int top_n;
  const float* logits; const long long* targets; bz_score_row* rec;     // first row of the sub-batch
  float* pmax; u64* S; unsigned* rank; u64* cand;                       // [RB][NB], [RB], [RB], [RB][NB][TOPN]
};

__device__ __forceinline__ bool sc_scored(long long t, long long V) { return t >= 0 && t < V; }

__global__ __launch_bounds__(256) void k_sc_max(ScArgs a) {
  __shared__ float redf[4];
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  if (!sc_scored(a.targets[row], a.V)) return;
  const float* x = a.logits + (size_t)row * a.V;
  if (blk == 0 && tid == 0) { a.S[row] = 0; a.rank[row] = 0; }
  float m = -INFINITY;
  for (long long i = (long long)blk * 256 + tid; i < a.V; i += (long long)NB * 256) m = fmaxf(m, x[i]);
  m = block_max_f(m, redf);
  if (tid == 0) a.pmax[(size_t)row * NB + blk] = m;
}

__global__ __launch_bounds__(256) void k_sc_sum(ScArgs a) {
  __shared__ float redf[4];
  __shared__ u64 part[4];
  __shared__ float pm[NB];
  __shared__ float tsh;
  const int row = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  const long long t = a.targets[row];
  if (!sc_scored(t, a.V)) return;
  const float* x = a.logits + (size_t)row * a.V;
  const int n = min(a.top_n, TOPN);
  u64* out = a.cand + ((size_t)row * NB + blk) * TOPN;
  if (tid < n) out[tid] = 0;                                       // none, until a round below says otherwise (the barriers of the reductions order the two writes)
  if (tid < NB) pm[tid] = a.pmax[(size_t)row * NB + tid];
  const float M = block_max_f(tid < NB ? a.pmax[(size_t)row * NB + tid] : -INFINITY, redf);
  const u64 ct = lp_composite(x[t], t);                            // 0: the target's logit is NaN, nothing is counted
  u64 s = 0, above = 0;
  for (long long i = (long long)blk * 256 + tid; i < a.V; i += (long long)NB * 256) {
    const float v = x[i];
    s += lp_term(v, M);
    above += (ct != 0 && lp_composite(v, i) > ct) ? 1 : 0;
  }
  s = block_sum_u64(s, part);
  above = block_sum_u64(above, part);
  if (tid == 0) {
    if (s) atomicAdd(&a.S[row], s);
    if (above) atomicAdd(&a.rank[row], (unsigned)above);
  }
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

__global__ __launch_bounds__(256) void k_sc_record(ScArgs a) {
  __shared__ u64 red[4];
  __shared__ float redf[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  bz_score_row* rec = a.rec + row;
  const long long t = a.targets[row];
  if (tid < TOPN) { rec->top_ids[tid] = 0; rec->top_logprobs[tid] = 0.0f; }
  if (!sc_scored(t, a.V)) {
    if (tid == 0) { rec->target = t; rec->logit = 0.0f; rec->logprob = 0.0f; rec->lse = 0.0f; rec->rank = -1; rec->n_top = -1; }
    return;
  }
  const float M = block_max_f(tid < NB ? a.pmax[(size_t)row * NB + tid] : -INFINITY, redf);   // (its barriers order the clearing above before the entries below)
  const float L = (float)log((double)a.S[row] * (1.0 / 1099511627776.0));
  const float lse = L + M;
  if (tid == 0) {
    const float xt = a.logits[(size_t)row * a.V + t];
    rec->target = t; rec->logit = xt; rec->logprob = xt - lse; rec->lse = lse;
    rec->rank = xt != xt ? -1 : (int)a.rank[row];
  }
  // the row's first n entries among the blocks' candidates
  const int n = min(a.top_n, TOPN);
  u64 c[CPT];
#pragma unroll
  for (int j = 0; j < CPT; j++) {
    const int k = tid + j * 256;
    c[j] = (k < NB * TOPN && (k % TOPN) < n) ? a.cand[(size_t)row * NB * TOPN + k] : 0;   // slots past n hold an earlier sub-batch's values
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

// MEAN: thread j carries column j's sum over the chunk's rows in row order (eight loads in flight, added in order)
__global__ __launch_bounds__(256) void k_pool_mean_acc(const float* __restrict__ rows, int n, int H, double* dsum, int first) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= H) return;
  double acc = first ? 0.0 : dsum[j];
  int r = 0;
  for (; r + 8 <= n; r += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = rows[(size_t)(r + u) * H + j];
#pragma unroll
    for (int u = 0; u < 8; u++) acc += (double)v[u];
  }
  for (; r < n; r++) acc += (double)rows[(size_t)r * H + j];
  dsum[j] = acc;
}
__global__ __launch_bounds__(256) void k_pool_mean_finish(const double* dsum, int S, int H, float* out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < H) out[j] = (float)(dsum[j] / (double)S);
}
// Packed prompt batch: the rows of a chunk (packed rows s0 .. s0 + n - 1) belong to inputs seg0 .. seg0 + gridDim.y - 1, input i owning packed rows off[i] ..
// off[i + 1] - 1.  Thread (column j, input i) walks the input's rows INSIDE this chunk in row order: MEAN carries the column's double sum (from dsum[i][j] when the
// input began in an earlier chunk; to dsum when it goes on in a later one) and stores (float)(sum / len) with the input's last row -- bz_pool_spec of the input's
// rows, bit for bit; CLS / LAST copy the input's first / last row when the chunk holds it.       grid = (ceil(H / 256), inputs in the chunk)
__global__ __launch_bounds__(256) void k_pool_seg(const float* __restrict__ rows, int s0, int n, int H, const int* __restrict__ off, int seg0, int pooling, double* dsum,
                                                  float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = seg0 + blockIdx.y;
  if (j >= H) return;
  const int beg = off[i], end = off[i + 1], a = max(beg, s0), b = min(end, s0 + n);
  if (a >= b) return;
  const float* x = rows + (size_t)(a - s0) * H + j;
  if (pooling == BZ_POOL_CLS) { if (a == beg) out[(size_t)i * H + j] = x[0]; return; }
  if (pooling == BZ_POOL_LAST) { if (b == end) out[(size_t)i * H + j] = x[(size_t)(b - 1 - a) * H]; return; }
  double acc = a == beg ? 0.0 : dsum[(size_t)i * H + j];
  for (int r = 0; r < b - a; r++) acc += (double)x[(size_t)r * H];
  if (b == end) out[(size_t)i * H + j] = (float)(acc / (double)(end - beg));
  else dsum[(size_t)i * H + j] = acc;
}
// one block per vector
__global__ __launch_bounds__(256) void k_pool_normalize(float* v, int H) {
  float* x = v + (size_t)blockIdx.x * H;
  double ss = 0.0;
  for (int j = threadIdx.x; j < H; j += 256) { const double d = (double)x[j]; ss += d * d; }
  ss = block_sum_d<4>(ss);
  const double norm = sqrt(ss);
  if (!(norm > 1e-12)) return;
  for (int j = threadIdx.x; j < H; j += 256) x[j] = (float)((double)x[j] / norm);
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// the buffers
// ---------------------------------------------------------------------------------------------------------
struct BzSinkWs {
  // scoring
  float* lg = nullptr; size_t lg_elems = 0;                       // logits workspace of a GEMM head
  long long* tg = nullptr; bz_score_row* rec = nullptr; int cap = 0;   // targets / records of a call, [cap]
  void* pin = nullptr; size_t pin_bytes = 0;                      // pinned staging: targets down, records up
  float* pmax = nullptr; u64* S = nullptr; unsigned* rank = nullptr; u64* cand = nullptr;   // one sub-batch
  const long long* tg_use = nullptr; int cS = 0; long long cV = 0; int ctop = 0;           // the call in flight
  // pooling
  float* hid = nullptr; size_t hid_elems = 0; double* dsum = nullptr; size_t dsum_elems = 0;   // column sums: H doubles (a single prompt), n_seq * H (MEAN over a packed batch)
  int pS = 0, pH = 0, prows = 0; bz_embed_config pcfg{};
  // pooling per input of a packed batch (n_seq > 0): inputs' first packed rows, [n_seq + 1], on the host and on the device (the caller's; it outlives the call)
  int n_seq = 0; std::vector<int> seg_off; const int* seg_off_dev = nullptr;
};

void bzk_sink_free(BzSinkWs* w) {
  if (!w) return;
  for (void* p : {(void*)w->lg, (void*)w->tg, (void*)w->rec, (void*)w->pmax, (void*)w->S, (void*)w->rank, (void*)w->cand, (void*)w->hid, (void*)w->dsum}) if (p) hipFree(p);
  if (w->pin) hipHostFree(w->pin);
  delete w;
}
// a buffer that is too small is replaced; the stream is idle by then (the caller's wait), so nothing reads the old one
template <class T> static int sink_grow(T** p, size_t bytes, const char* what) {
  if (*p) { hipFree(*p); *p = nullptr; }
  if (hipMalloc((void**)p, std::max<size_t>(bytes, 16)) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); BZ_FAIL(BZ_E_OOM, "%s: out of device memory (%zu bytes)", what, bytes); }
  return BZ_OK;
}

int bzk_check_score_cfg(const bz_score_config* cfg, const int64_t* targets, int S, long long V, const void* rows_out, const char* who) {
  if (!cfg || !targets || !rows_out) BZ_FAIL(BZ_E_INVALID, "%s: null config / targets / rows_out", who);
  if (cfg->top_n < 0 || cfg->top_n > TOPN) BZ_FAIL(BZ_E_INVALID, "%s: top_n = %d out of range (0 .. %d)", who, cfg->top_n, TOPN);
  if (V < 1 || V >= VMAX) BZ_FAIL(BZ_E_INVALID, "%s: vocabulary of %lld ids (1 .. 2^24 - 1: the row's integer sum must stay below 2^64)", who, V);
  for (int i = 0; i < S; i++)
    if (targets[i] < -1 || targets[i] >= V) BZ_FAIL(BZ_E_INVALID, "%s: targets[%d] = %lld out of range (-1 = not scored, 0 .. %lld)", who, i, (long long)targets[i], V - 1);
  return BZ_OK;
}
int bzk_check_embed_cfg(const bz_embed_config* cfg, const bz_tensor* out, int S, int H, const char* who) {
  if (!cfg) BZ_FAIL(BZ_E_INVALID, "%s: null config", who);
  if (cfg->pooling < BZ_POOL_NONE || cfg->pooling > BZ_POOL_LAST) BZ_FAIL(BZ_E_INVALID, "%s: pooling = %d unknown (NONE = 0, MEAN = 1, CLS = 2, LAST = 3)", who, cfg->pooling);
  const size_t need = (cfg->pooling == BZ_POOL_NONE ? (size_t)S : 1) * (size_t)H * 4;
  if (!out || out->dtype != BZ_F32 || out->nbytes < need) BZ_FAIL(BZ_E_INVALID, "%s: out must be F32 with at least %zu bytes (%s, hidden %d), has %zu", who, need,
                                                                  cfg->pooling == BZ_POOL_NONE ? "[S, hidden]" : "[hidden]", H, out ? out->nbytes : (size_t)0);
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// scoring: begin / chunk / end
// ---------------------------------------------------------------------------------------------------------
static int score_begin(hipStream_t st, BzSinkWs** wp, int S, long long V, int logits_rows, const int64_t* targets_host, const long long* targets_dev, int top_n) {
  if (!*wp) *wp = new BzSinkWs();
  BzSinkWs* w = *wp;
  const size_t lg_need = (size_t)logits_rows * (size_t)V;
  const size_t pin_need = (size_t)S * (8 + sizeof(bz_score_row));
  if (lg_need > w->lg_elems || S > w->cap || pin_need > w->pin_bytes || !w->cand) {
    BZ_HIP(hipStreamSynchronize(st));
    if (lg_need > w->lg_elems) { w->lg_elems = 0; BZ_TRY(sink_grow(&w->lg, lg_need * 4, "score: logits workspace")); w->lg_elems = lg_need; }
    if (S > w->cap) {
      w->cap = 0;
      BZ_TRY(sink_grow(&w->tg, (size_t)S * 8, "score: targets"));
      BZ_TRY(sink_grow(&w->rec, (size_t)S * sizeof(bz_score_row), "score: records"));
      w->cap = S;
    }
    if (pin_need > w->pin_bytes) {
      if (w->pin) { hipHostFree(w->pin); w->pin = nullptr; }
      w->pin_bytes = 0;
      if (hipHostMalloc(&w->pin, pin_need, hipHostMallocDefault) != hipSuccess) { w->pin = nullptr; (void)hipGetLastError(); BZ_FAIL(BZ_E_OOM, "score: out of pinned memory (%zu bytes)", pin_need); }
      w->pin_bytes = pin_need;
    }
    if (!w->cand) {
      BZ_TRY(sink_grow(&w->pmax, (size_t)RB * NB * 4, "score: block maxima"));
      BZ_TRY(sink_grow(&w->S, (size_t)RB * 8, "score: sums"));
      BZ_TRY(sink_grow(&w->rank, (size_t)RB * 4, "score: ranks"));
      BZ_TRY(sink_grow(&w->cand, (size_t)RB * NB * TOPN * 8, "score: candidates"));
    }
  }
  w->cS = S; w->cV = V; w->ctop = top_n;
  if (targets_host) {
    memcpy(w->pin, targets_host, (size_t)S * 8);
    BZ_HIP(hipMemcpyAsync(w->tg, w->pin, (size_t)S * 8, hipMemcpyHostToDevice, st));
    w->tg_use = w->tg;
  } else w->tg_use = targets_dev;
  return BZ_OK;
}
int bzk_score_begin(hipStream_t st, BzSinkWs** w, int S, long long V, int logits_rows, const int64_t* targets_host, int top_n) {
  return score_begin(st, w, S, V, logits_rows, targets_host, nullptr, top_n);
}
float* bzk_score_logits_ws(BzSinkWs* w) { return w->lg; }

int bzk_score_chunk(hipStream_t st, BzSinkWs* w, const float* logits, int n, int s0) {
  if (s0 < 0 || n < 0 || s0 + n > w->cS) BZ_FAIL(BZ_E_INVALID, "score: rows %d .. %d outside the call's %d", s0, s0 + n, w->cS);
  for (int r0 = 0; r0 < n; r0 += RB) {
    const int rb = std::min(RB, n - r0);
    ScArgs a{w->cV, w->ctop, logits + (size_t)r0 * w->cV, w->tg_use + s0 + r0, w->rec + s0 + r0, w->pmax, w->S, w->rank, w->cand};
    hipLaunchKernelGGL(k_sc_max, dim3(NB, rb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sc_sum, dim3(NB, rb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sc_record, dim3(rb), dim3(256), 0, st, a);
  }
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

int bzk_score_end(hipStream_t st, BzSinkWs* w, bz_score_row* rows_out, bz_score_total* total) {
  const size_t bytes = (size_t)w->cS * sizeof(bz_score_row);
  BZ_HIP(hipMemcpyAsync(w->pin, w->rec, bytes, hipMemcpyDeviceToHost, st));
  BZ_HIP(hipStreamSynchronize(st));
  memcpy(rows_out, w->pin, bytes);
  if (total) {
    total->sum_logprob = 0.0; total->n_scored = 0;
    for (int i = 0; i < w->cS; i++)
      if (rows_out[i].n_top >= 0 && std::isfinite(rows_out[i].logprob)) { total->sum_logprob += (double)rows_out[i].logprob; total->n_scored++; }
  }
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// pooling: begin / chunk / end
// ---------------------------------------------------------------------------------------------------------
int bzk_pool_begin(hipStream_t st, BzSinkWs** wp, int S, int H, int rows, const bz_embed_config* cfg) {
  if (!*wp) *wp = new BzSinkWs();
  BzSinkWs* w = *wp;
  const size_t hid_need = (size_t)(rows + 2) * H;
  if (hid_need > w->hid_elems || (size_t)H > w->dsum_elems) {
    BZ_HIP(hipStreamSynchronize(st));
    if (hid_need > w->hid_elems) { w->hid_elems = 0; BZ_TRY(sink_grow(&w->hid, hid_need * 4, "embed: rows workspace")); w->hid_elems = hid_need; }
    if ((size_t)H > w->dsum_elems) { w->dsum_elems = 0; BZ_TRY(sink_grow(&w->dsum, (size_t)H * 8, "embed: column sums")); w->dsum_elems = (size_t)H; }
  }
  w->pS = S; w->pH = H; w->prows = rows; w->pcfg = *cfg; w->n_seq = 0;
  return BZ_OK;
}
// a packed batch of n_seq inputs (S = off[n_seq] rows in all): the result is [n_seq, H], one pooled vector per input (NONE: all S rows)
int bzk_pool_begin_seg(hipStream_t st, BzSinkWs** wp, int S, int H, int rows, const bz_embed_config* cfg, const int* seg_off_host, const int* seg_off_dev, int n_seq) {
  BZ_TRY(bzk_pool_begin(st, wp, S, H, rows, cfg));
  BzSinkWs* w = *wp;
  const size_t need = (size_t)n_seq * H;      // only MEAN carries sums (k_pool_seg); CLS / LAST / NONE copy rows
  if (cfg->pooling == BZ_POOL_MEAN && need > w->dsum_elems) {
    BZ_HIP(hipStreamSynchronize(st));
    w->dsum_elems = 0; BZ_TRY(sink_grow(&w->dsum, need * 8, "embed: column sums")); w->dsum_elems = need;
  }
  w->n_seq = n_seq; w->seg_off.assign(seg_off_host, seg_off_host + n_seq + 1); w->seg_off_dev = seg_off_dev;
  return BZ_OK;
}
float* bzk_pool_rows_ws(BzSinkWs* w) { return w->hid; }
void bzk_pool_step_rows(BzSinkWs* w, float** hidden, float** prev) { *hidden = w->hid + (size_t)w->prows * w->pH; *prev = w->hid + (size_t)(w->prows + 1) * w->pH; }

int bzk_pool_chunk(hipStream_t st, BzSinkWs* w, const float* rows, int n, int s0, float* out) {
  const int S = w->pS, H = w->pH;
  if (s0 < 0 || n <= 0 || s0 + n > S) BZ_FAIL(BZ_E_INVALID, "embed: rows %d .. %d outside the call's %d", s0, s0 + n, S);
  const size_t rb = (size_t)H * 4;
  if (w->n_seq > 0 && w->pcfg.pooling != BZ_POOL_NONE) {
    // the inputs with a row in this chunk: the one holding s0 .. the one holding s0 + n - 1
    const int i0 = (int)(std::upper_bound(w->seg_off.begin(), w->seg_off.end(), s0) - w->seg_off.begin()) - 1;
    const int i1 = (int)(std::upper_bound(w->seg_off.begin(), w->seg_off.end(), s0 + n - 1) - w->seg_off.begin()) - 1;
    for (int y0 = i0; y0 <= i1; y0 += 65535) {
      hipLaunchKernelGGL(k_pool_seg, dim3((H + 255) / 256, std::min(65535, i1 - y0 + 1)), dim3(256), 0, st, rows, s0, n, H, w->seg_off_dev, y0, (int)w->pcfg.pooling, w->dsum, out);
    }
    BZ_HIP(hipGetLastError());
    return BZ_OK;
  }
  switch (w->pcfg.pooling) {
    case BZ_POOL_NONE: BZ_HIP(hipMemcpyAsync(out + (size_t)s0 * H, rows, (size_t)n * rb, hipMemcpyDeviceToDevice, st)); break;
    case BZ_POOL_CLS: if (s0 == 0) BZ_HIP(hipMemcpyAsync(out, rows, rb, hipMemcpyDeviceToDevice, st)); break;
    case BZ_POOL_LAST: if (s0 + n == S) BZ_HIP(hipMemcpyAsync(out, rows + (size_t)(n - 1) * H, rb, hipMemcpyDeviceToDevice, st)); break;
    default:
      hipLaunchKernelGGL(k_pool_mean_acc, dim3((H + 255) / 256), dim3(256), 0, st, rows, n, H, w->dsum, s0 == 0 ? 1 : 0);
      BZ_HIP(hipGetLastError());
  }
  return BZ_OK;
}
int bzk_pool_end(hipStream_t st, BzSinkWs* w, float* out) {
  const int S = w->pS, H = w->pH;
  if (w->pcfg.pooling == BZ_POOL_MEAN && w->n_seq == 0) hipLaunchKernelGGL(k_pool_mean_finish, dim3((H + 255) / 256), dim3(256), 0, st, w->dsum, S, H, out);
  if (w->pcfg.normalize) hipLaunchKernelGGL(k_pool_normalize, dim3(w->pcfg.pooling == BZ_POOL_NONE ? S : std::max(w->n_seq, 1)), dim3(256), 0, st, out, H);
  w->n_seq = 0;
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// op level
// ---------------------------------------------------------------------------------------------------------
extern "C" int bz_score_rows(bz_device* dev, const bz_tensor* logits, int64_t R, int64_t V, const bz_tensor* targets, const bz_score_config* cfg, bz_score_row* rows_out) {
  BZ_API_BEGIN
  if (!dev || !cfg || !rows_out) BZ_FAIL(BZ_E_INVALID, "score_rows: null argument");
  if (cfg->top_n < 0 || cfg->top_n > TOPN) BZ_FAIL(BZ_E_INVALID, "score_rows: top_n = %d out of range (0 .. %d)", cfg->top_n, TOPN);
  if (R < 1 || R > INT_MAX || V < 1 || V >= VMAX) BZ_FAIL(BZ_E_INVALID, "score_rows: R = %lld rows of V = %lld ids (R >= 1, 1 <= V < 2^24)", (long long)R, (long long)V);
  if (!logits || logits->dtype != BZ_F32 || logits->nbytes < (size_t)R * (size_t)V * 4) BZ_FAIL(BZ_E_INVALID, "score_rows: logits must be F32 [R,V]");
  if (!targets || targets->dtype != BZ_I64 || targets->nbytes < (size_t)R * 8) BZ_FAIL(BZ_E_INVALID, "score_rows: targets must be I64 [R] on the device");
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  BzSinkWs* w = nullptr;
  int rc = score_begin(dev->stream, &w, (int)R, V, 0, nullptr, (const long long*)targets->ptr, cfg->top_n);
  if (rc == BZ_OK) rc = bzk_score_chunk(dev->stream, w, (const float*)logits->ptr, (int)R, 0);
  if (rc == BZ_OK) rc = bzk_score_end(dev->stream, w, rows_out, nullptr);
  else hipStreamSynchronize(dev->stream);
  bzk_sink_free(w);
  return rc;
  BZ_API_END
}

extern "C" int bz_pool_rows(bz_device* dev, const bz_tensor* hidden, int64_t S, int64_t H, const bz_embed_config* cfg, bz_tensor* out) {
  BZ_API_BEGIN
  if (!dev) BZ_FAIL(BZ_E_INVALID, "pool_rows: null device");
  if (S < 1 || S > INT_MAX || H < 1 || H > INT_MAX) BZ_FAIL(BZ_E_INVALID, "pool_rows: S = %lld rows of H = %lld", (long long)S, (long long)H);
  if (!hidden || hidden->dtype != BZ_F32 || hidden->nbytes < (size_t)S * (size_t)H * 4) BZ_FAIL(BZ_E_INVALID, "pool_rows: hidden must be F32 [S,H]");
  BZ_TRY(bzk_check_embed_cfg(cfg, out, (int)S, (int)H, "pool_rows"));
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  BzSinkWs* w = nullptr;
  int rc = bzk_pool_begin(dev->stream, &w, (int)S, (int)H, 0, cfg);
  if (rc == BZ_OK) rc = bzk_pool_chunk(dev->stream, w, (const float*)hidden->ptr, (int)S, 0, (float*)out->ptr);
  if (rc == BZ_OK) rc = bzk_pool_end(dev->stream, w, (float*)out->ptr);
  hipStreamSynchronize(dev->stream);     // the column sums are this call's
  bzk_sink_free(w);
  return rc;
  BZ_API_END
}

// ---------------------------------------------------------------------------------------------------------
// the definitions on the host
// ---------------------------------------------------------------------------------------------------------
extern "C" int bz_score_row_spec(const float* x, int64_t V, int64_t target, int top_n, bz_score_row* row_out) {
  BZ_API_BEGIN
  if (!x || !row_out || V < 1 || V >= VMAX) BZ_FAIL(BZ_E_INVALID, "score_row_spec: bad row (V = %lld)", (long long)V);
  if (top_n < 0 || top_n > TOPN) BZ_FAIL(BZ_E_INVALID, "score_row_spec: top_n = %d out of range (0 .. %d)", top_n, TOPN);
  if (target < -1 || target >= V) BZ_FAIL(BZ_E_INVALID, "score_row_spec: target = %lld out of range (-1 = not scored, 0 .. %lld)", (long long)target, (long long)V - 1);
  memset(row_out, 0, sizeof(*row_out));
  row_out->target = target;
  if (target < 0) { row_out->rank = -1; row_out->n_top = -1; return BZ_OK; }
  float M = -INFINITY;
  for (int64_t i = 0; i < V; i++) M = fmaxf(M, x[i]);
  u64 S = 0;
  for (int64_t i = 0; i < V; i++) S += lp_term(x[i], M);
  const float L = (float)log((double)S * (1.0 / 1099511627776.0));
  const float lse = L + M;
  const float xt = x[target];
  row_out->logit = xt; row_out->logprob = xt - lse; row_out->lse = lse;
  const u64 ct = lp_composite(xt, target);
  int rank = 0;
  if (ct) for (int64_t i = 0; i < V; i++) rank += lp_composite(x[i], i) > ct ? 1 : 0;
  row_out->rank = ct ? rank : -1;
  u64 prev = ~0ull;
  int got = 0;
  for (int r = 0; r < top_n; r++) {
    u64 best = 0;
    for (int64_t i = 0; i < V; i++) { const u64 c = lp_composite(x[i], i); if (c < prev) best = umax64(best, c); }
    if (best == 0) break;
    row_out->top_ids[r] = 0xFFFFFFFFu - (unsigned)best; row_out->top_logprobs[r] = lp_logit_of(best) - lse;
    prev = best; got = r + 1;
  }
  row_out->n_top = got;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_pool_spec(const float* hidden, int64_t S, int64_t H, const bz_embed_config* cfg, float* out) {
  BZ_API_BEGIN
  if (!hidden || !out || !cfg || S < 1 || H < 1) BZ_FAIL(BZ_E_INVALID, "pool_spec: bad argument");
  if (cfg->pooling < BZ_POOL_NONE || cfg->pooling > BZ_POOL_LAST) BZ_FAIL(BZ_E_INVALID, "pool_spec: pooling = %d unknown (NONE = 0, MEAN = 1, CLS = 2, LAST = 3)", cfg->pooling);
  int64_t nvec = 1;
  switch (cfg->pooling) {
    case BZ_POOL_NONE: memcpy(out, hidden, (size_t)S * H * 4); nvec = S; break;
    case BZ_POOL_CLS: memcpy(out, hidden, (size_t)H * 4); break;
    case BZ_POOL_LAST: memcpy(out, hidden + (size_t)(S - 1) * H, (size_t)H * 4); break;
    default:
      for (int64_t j = 0; j < H; j++) {
        double acc = 0.0;
        for (int64_t s = 0; s < S; s++) acc += (double)hidden[(size_t)s * H + j];
        out[j] = (float)(acc / (double)S);
      }
  }
  if (cfg->normalize)
    for (int64_t v = 0; v < nvec; v++) {
      float* p = out + (size_t)v * H;
      double ss = 0.0;
      for (int64_t j = 0; j < H; j++) { const double d = (double)p[j]; ss += d * d; }
      const double norm = sqrt(ss);
      if (norm > 1e-12) for (int64_t j = 0; j < H; j++) p[j] = (float)((double)p[j] / norm);
    }
  return BZ_OK;
  BZ_API_END
}
