// bz_engine.hip -- continuous batching: a request engine over the batched decode graph.  What the reference's BatchEngine / RequestScheduler do
// (engine/batch_engine.rs:91-169 the run loop, 172-319 admission and the chunked prompt, 322-445 the decode step and its harvest;
// engine/request_scheduler.rs:105-205; config/inference.rs:89-90,136,142: max_batch_size, prefill_chunk_size, kv_pool_blocks), with the row life cycle
// ON THE DEVICE: every row of the captured step is live or idle, and the launch that sees a live row's token ends the row (stop id, or tokens used up), so a
// replay already enqueued behind it neither advances the row nor writes into its blocks.  The host may therefore keep `depth` replays in flight and read
// their records late.
//
//   k_engine_advance   where k_batch_advance sits.  Live row: tok = next, pos + 1, slot from its block-table row.  Idle row: token 0 at position 0 of the
//                      row's own park block (it attends to what it has just written: finite logits, no slot shared with any other row).
//   k_engine_finish    the step's last launch (after the pick and the grammar advance).  Live row: left -= 1; ends on a stop id (reason 1), else on
//                      left == 0 (reason 0).  A row that ends becomes idle here: live = 0, pos = 0, table[row][0] = its park block, its grammar state FREE.
//                      its bias list empty and its logprobs off (the record of this step is written before, by k_lp_record).
//                      One status word per row and the number of rows still live go to pinned rings beside the token log.  One workgroup, N <= 512.
//   k_kv_copy_slots    the prefix cache's copy-on-write: the first j slots of a cached block into a request's own block, every layer, K and V, every KV head;
//                      one launch for all copies of a step, the (source, destination, j) triples read from device memory.
// Parking costs the pool one block per row (the last n_rows blocks).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>
#include <map>
#include <vector>

#include "bz_internal.h"

// ---------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------
__global__ void k_engine_advance(long long* tok, const long long* next, int* pos, int* slot, const int* table, int stride, int bs, int N, const EngRow* rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (rows[i].live) {
    tok[i] = next[i];
    const int p = pos[i] + 1;
    pos[i] = p;
    slot[i] = table[(size_t)i * stride + p / bs] * bs + p % bs;
  } else {
    tok[i] = 0;
    pos[i] = 0;                                  // the park position: it does not move
    slot[i] = rows[i].park_block * bs;
  }
}
__global__ __launch_bounds__(512) void k_engine_finish(EngRow* rows, const long long* next, int* pos, int* table, int stride, const int* step, int logcap, int N,
                                                       int* status, int* nlive, uint32_t* gstate, int* row_lora, int* bias_cnt, int* lp_top_n) {
  const int i = threadIdx.x;
  const int st = *step - 1;                      // the pick has counted this replay already
  const int at = ((st % logcap) + logcap) % logcap;
  int still = 0;
  if (i < N) {
    EngRow& r = rows[i];
    int word = ENG_IDLE;
    if (r.live) {
      const int left = r.left - 1;
      const long long t = next[i];
      int reason = -1;
      const int ns = min(max(r.n_stop, 0), BZ_ENGINE_MAX_STOP);
      for (int k = 0; k < ns; k++) if (r.stop[k] == t) reason = 1;
      if (reason < 0 && left <= 0) reason = 0;
      r.left = left;
      if (reason >= 0) {
        r.live = 0;
        pos[i] = 0;
        table[(size_t)i * stride] = r.park_block;
        if (gstate) gstate[i] = BZ_GRAMMAR_ROW_FREE;
        if (row_lora) row_lora[i] = -1;
        if (bias_cnt) bias_cnt[i] = 0;
        if (lp_top_n) lp_top_n[i] = -1;
        word = ENG_FINISHED | (reason << 2);
      } else { word = ENG_TOKEN; still = 1; }
    }
    status[(size_t)at * N + i] = word;
  }
  const int cnt = __syncthreads_count(still);
  if (i == 0) nlive[at] = cnt;
}
// The pool is [layer][block][kv_head][block_size][hd]: per (layer, K|V, head) the first j slots of a block are one contiguous run of j * hd elements, a multiple
// of 16 bytes (hd % 8 == 0, elements of 2 or 4 bytes).  blockIdx.y = the triple, blockIdx.x * 256 + threadIdx.x = the 16-byte vector within the triple's
// layers * 2 * n_kv runs; the grid is sized by the host for the step's largest j, a thread beyond its own triple's bytes leaves.  A triple out of range copies nothing.
__global__ __launch_bounds__(256) void k_kv_copy_slots(uint4* k, uint4* v, const int* triples, int layers, int num_blocks, int n_kv, int bs, int row_vecs) {
  const int* t = triples + 3 * blockIdx.y;
  const int src = t[0], dst = t[1], j = t[2];
  if (src < 0 || src >= num_blocks || dst < 0 || dst >= num_blocks || src == dst || j < 1 || j > bs) return;
  const long long run_vecs = (long long)j * row_vecs;                  // 16-byte vectors per (layer, K|V, head)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= run_vecs * layers * 2 * n_kv) return;
  const long long run = i / run_vecs, off = i % run_vecs;
  const int head = (int)(run % n_kv), which = (int)((run / n_kv) & 1), layer = (int)(run / (2 * n_kv));
  const long long head_vecs = (long long)bs * row_vecs;
  uint4* base = which ? v : k;
  const long long lb = (long long)layer * num_blocks;
  base[((lb + dst) * n_kv + head) * head_vecs + off] = base[((lb + src) * n_kv + head) * head_vecs + off];
}
// n triples (int32 x 3, device memory), max_j = the largest slot count among them (sizes the grid)
int bzk_kv_copy_slots(hipStream_t s, bz_paged_kv* kv, const int* d_triples, int n, int max_j) {
  if (n < 1) return BZ_OK;
  const size_t row_bytes = (size_t)kv->hd * bz_dtype_size(kv->dtype);
  if (row_bytes % 16) BZ_FAIL(BZ_E_INVALID, "kv copy_slots: a row of %zu bytes (head_dim = %d) is no multiple of 16", row_bytes, kv->hd);
  if (max_j < 1 || max_j > kv->block_size) BZ_FAIL(BZ_E_INVALID, "kv copy_slots: %d slots outside 1 .. block_size = %d", max_j, kv->block_size);
  const int row_vecs = (int)(row_bytes / 16);
  const long long vecs = (long long)max_j * row_vecs * kv->layers * 2 * kv->n_kv;
  hipLaunchKernelGGL(k_kv_copy_slots, dim3((unsigned)((vecs + 255) / 256), n), dim3(256), 0, s, (uint4*)kv->k, (uint4*)kv->v, d_triples, kv->layers, kv->num_blocks, kv->n_kv,
                     kv->block_size, row_vecs);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
int bzk_engine_advance(hipStream_t s, long long* tok, const long long* next, int* pos, int* slot, const int* table, int stride, int bs, int N, const EngRow* rows) {
  hipLaunchKernelGGL(k_engine_advance, dim3((N + 63) / 64), dim3(64), 0, s, tok, next, pos, slot, table, stride, bs, N, rows);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}
int bzk_engine_finish(hipStream_t s, EngRow* rows, const long long* next, int* pos, int* table, int stride, const int* step, int logcap, int N, int* status,
                      int* nlive, uint32_t* gstate, int* row_lora, int* bias_cnt, int* lp_top_n) {
  if (N > 512) BZ_FAIL(BZ_E_INVALID, "engine finish: N = %d above the 512 rows one workgroup serves", N);
  hipLaunchKernelGGL(k_engine_finish, dim3(1), dim3(512), 0, s, rows, next, pos, table, stride, step, logcap, N, status, nlive, gstate, row_lora, bias_cnt, lp_top_n);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------
namespace {
struct EngReq {
  int64_t id = -1; std::vector<int64_t> prompt; bz_request rq{}; int row = -1; bool live = false; int produced = 0; long long first_replay = -1; int shared = 0;
  int top_n = -1; std::vector<uint32_t> bias_ids; std::vector<float> bias_vals;   // bz_request_extras: logprobs (-1: not asked) and the deduplicated bias list
};
// pinned staging for the stream-ordered writes: a slot is reused only after the stream has passed the copies that read it
struct Stage { char* host = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
struct RowMisc { long long next; int pos, lora; EngRow er; uint32_t gram[2]; };   // lora: the row's LoRA slot id (-1: none)
}
struct bz_engine {
  bz_model* m = nullptr; bz_device* dev = nullptr; bz_engine_config cfg{}; bz_model_config mc{};
  bz_grammar_cursor* cursor = nullptr; bz_batch_sampler* sampler = nullptr; bz_paged_kv* kv = nullptr; bz_sched* sched = nullptr; bz_batch_graph* g = nullptr;
  EngRow* d_rows = nullptr; int* status = nullptr; int* nlive = nullptr;
  int max_blocks = 0, max_chunk = 0;
  long long* d_ptok = nullptr; int* d_pslot = nullptr; int* d_ptable = nullptr; int* d_copy = nullptr; bz_tensor* plogits = nullptr;
  std::vector<Stage> stages; size_t off_misc = 0, off_bs = 0, off_ptok = 0, off_pslot = 0, off_copy = 0, off_lp = 0, stage_bytes = 0; int stage_next = 0;
  std::vector<hipEvent_t> rev;               // one event per replay in flight (ring)
  long long read = 0;                        // records harvested; g->replays = enqueued
  std::map<int64_t, EngReq> reqs;            // waiting and admitted
  std::vector<int64_t> row_req;              // host view: the request a row serves, or -1
  std::vector<bz_sched_action> acts;
  std::deque<bz_engine_event> events;
  std::deque<bz_engine_logprobs> lp_events;  // one per token event of a request that asked for logprobs
  long long prompt_tokens = 0, generated = 0; double admit_ms = 0;
  long long skipped = 0, copy_launches = 0, copied_blocks = 0;   // prefix cache
  static const int EVRING = 128;
};

// a request holds its LoRA slot from submit until it leaves e->reqs (finished, cancelled, engine freed): bz_lora_detach looks at the count
static int eng_lora_slot(const EngReq& q) { return q.rq.lora_slot - 1; }
static void eng_lora_release(bz_engine* e, const EngReq& q) {
  BzLoraTable* T = bzi_model_lora(e->m);
  if (T && eng_lora_slot(q) >= 0 && eng_lora_slot(q) < T->n_slots && T->users[eng_lora_slot(q)] > 0) T->users[eng_lora_slot(q)]--;
}

static int eng_stage(bz_engine* e, Stage** out) {
  Stage& s = e->stages[e->stage_next];
  e->stage_next = (e->stage_next + 1) % (int)e->stages.size();
  if (s.pending) { BZ_HIP(hipEventSynchronize(s.ev)); s.pending = false; }
  *out = &s;
  return BZ_OK;
}
static int eng_stage_done(bz_engine* e, Stage* s) { BZ_HIP(hipEventRecord(s->ev, e->dev->stream)); s->pending = true; return BZ_OK; }

extern "C" int bz_engine_free(bz_engine* e) {
  BZ_API_BEGIN
  if (!e) return BZ_OK;
  if (e->dev) { hipSetDevice(e->dev->id); hipStreamSynchronize(e->dev->stream); }
  for (auto& kv : e->reqs) eng_lora_release(e, kv.second);
  if (e->g) bz_decode_batch_graph_free(e->g);
  if (e->sampler) bz_batch_sampler_free(e->sampler);
  if (e->kv) bz_paged_kv_free(e->kv);
  if (e->sched) bz_sched_free(e->sched);
  if (e->plogits) bz_tensor_free(e->plogits);
  for (void* p : {(void*)e->d_rows, (void*)e->d_ptok, (void*)e->d_pslot, (void*)e->d_ptable, (void*)e->d_copy}) if (p) hipFree(p);
  if (e->status) hipHostFree(e->status);
  if (e->nlive) hipHostFree(e->nlive);
  for (Stage& s : e->stages) { if (s.host) hipHostFree(s.host); if (s.ev) hipEventDestroy(s.ev); }
  for (hipEvent_t ev : e->rev) if (ev) hipEventDestroy(ev);
  if (e->dev) bz_dev_release(e->dev);
  delete e;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_create(bz_model* m, const bz_engine_config* cfg, bz_grammar_cursor* cursor, bz_engine** out) {
  BZ_API_BEGIN
  if (!out) BZ_FAIL(BZ_E_INVALID, "engine create: null output pointer");
  *out = nullptr;
  if (!m || !cfg) BZ_FAIL(BZ_E_INVALID, "engine create: null argument");
  bz_model_config mc;
  BZ_TRY(bz_model_get_config(m, &mc));
  if (mc.arch != BZ_ARCH_LLAMA) BZ_FAIL(BZ_E_UNSUPPORTED, "engine create: llama family only (the batched decode graph does not take Mamba2 / DeepSeek-V2)");
  if (cfg->n_rows < 2 || cfg->n_rows > 512) BZ_FAIL(BZ_E_INVALID, "engine create: n_rows = %d out of range (2 <= n_rows <= 512)", cfg->n_rows);
  if (cfg->depth < 1 || cfg->depth > 64) BZ_FAIL(BZ_E_INVALID, "engine create: depth = %d out of range (1 <= depth <= 64)", cfg->depth);
  if (cfg->block_size < 1 || cfg->prefill_chunk < 0) BZ_FAIL(BZ_E_INVALID, "engine create: bad block_size / prefill_chunk (%d / %d)", cfg->block_size, cfg->prefill_chunk);
  if (cfg->max_seq_len < 2 || cfg->max_seq_len > mc.max_seq_len)
    BZ_FAIL(BZ_E_INVALID, "engine create: max_seq_len = %d out of range (2 .. the model's %d)", cfg->max_seq_len, mc.max_seq_len);
  if (cfg->num_blocks <= cfg->n_rows) BZ_FAIL(BZ_E_INVALID, "engine create: num_blocks = %d leaves nothing beside the %d park blocks", cfg->num_blocks, cfg->n_rows);
  if (cfg->prefix_cache != 0 && cfg->prefix_cache != 1) BZ_FAIL(BZ_E_INVALID, "engine create: prefix_cache = %d (0 = off, 1 = on)", cfg->prefix_cache);
  if (cfg->logprobs != 0 && cfg->logprobs != 1) BZ_FAIL(BZ_E_INVALID, "engine create: logprobs = %d (0 = off, 1 = on)", cfg->logprobs);
  if (cfg->logprobs && !cfg->use_sampler) BZ_FAIL(BZ_E_INVALID, "engine create: logprobs = 1 needs use_sampler = 1 (got use_sampler = %d): bias and logprobs live in the batched sampler", cfg->use_sampler);
  const int N = cfg->n_rows;
  bz_device* dev = bzi_model_device(m);
  if (!dev) BZ_FAIL(BZ_E_INVALID, "engine create: model not finalized");
  BZ_HIP(hipSetDevice(dev->id));
  bz_engine* e = new bz_engine();
  bz_dev_retain(dev); e->dev = dev;
  e->m = m; e->cfg = *cfg; e->mc = mc; e->cursor = cursor;
  e->max_blocks = (cfg->max_seq_len + cfg->block_size - 1) / cfg->block_size;
  e->max_chunk = cfg->prefill_chunk > 0 ? std::min(cfg->prefill_chunk, cfg->max_seq_len) : cfg->max_seq_len;
  e->row_req.assign(N, -1);
  e->acts.resize((cfg->prefix_cache ? 4 : 3) * (size_t)N);
  int rc = BZ_OK;
  auto fail = [&](int code) { bz_engine_free(e); return code; };
  if ((rc = bz_sched_create(N, cfg->num_blocks, cfg->block_size, cfg->max_seq_len, cfg->prefill_chunk, &e->sched)) != BZ_OK) return fail(rc);
  if (cfg->prefix_cache && (rc = bz_sched_enable_prefix(e->sched)) != BZ_OK) return fail(rc);
  const int kvdt = mc.act_dtype;
  if ((rc = bz_paged_kv_create(dev, mc.n_layers, cfg->num_blocks, cfg->block_size, mc.n_kv_heads, mc.head_dim, kvdt, &e->kv)) != BZ_OK) return fail(rc);
  if (cfg->use_sampler && (rc = bz_batch_sampler_create(dev, N, mc.vocab, &e->sampler)) != BZ_OK) return fail(rc);
  if (cfg->logprobs && (rc = bz_batch_sampler_enable(e->sampler, BZ_BS_BIAS | BZ_BS_LOGPROBS)) != BZ_OK) return fail(rc);
  // the prompt workspace before the capture, for the largest chunk as well: a later reallocation would synchronise
  if ((rc = bzi_prefill_reserve(m, std::max(N, e->max_chunk))) != BZ_OK) return fail(rc);
  const size_t ring = (size_t)bz_batch_graph::LOGCAP;
  if (hipMalloc(&e->d_rows, (size_t)N * sizeof(EngRow)) != hipSuccess || hipMalloc(&e->d_ptok, (size_t)e->max_chunk * 8) != hipSuccess ||
      hipMalloc(&e->d_pslot, (size_t)e->max_chunk * 4) != hipSuccess || hipMalloc(&e->d_ptable, (size_t)e->max_blocks * 4) != hipSuccess || hipMalloc(&e->d_copy, (size_t)N * 12) != hipSuccess ||
      hipHostMalloc(&e->status, ring * N * 4, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&e->nlive, ring * 4, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError(); bz_set_error("engine create: out of memory"); return fail(BZ_E_OOM);
  }
  memset(e->status, 0, ring * N * 4); memset(e->nlive, 0, ring * 4);
  const int64_t shp[2] = {1, mc.vocab};
  if ((rc = bz_tensor_zeros(dev, BZ_F32, shp, 2, &e->plogits)) != BZ_OK) return fail(rc);
  // staging slots: [table row][RowMisc][sampler row][prompt chunk tokens][prompt chunk slots][copy triples][top_n, bias list (logprobs = 1)]
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  e->off_misc = up((size_t)e->max_blocks * 4);
  e->off_bs = e->off_misc + up(sizeof(RowMisc));
  e->off_ptok = e->off_bs + up(bzk_batch_sampler_row_bytes());
  e->off_pslot = e->off_ptok + up((size_t)e->max_chunk * 8);
  e->off_copy = e->off_pslot + up((size_t)e->max_chunk * 4);
  e->off_lp = e->off_copy + up((size_t)N * 12);
  e->stage_bytes = e->off_lp + (cfg->logprobs ? up(bzk_lp_stage_bytes()) : 0);
  e->stages.resize(std::min(64, std::max(8, 2 * N)));
  for (Stage& s : e->stages)
    if (hipHostMalloc((void**)&s.host, e->stage_bytes, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError(); bz_set_error("engine create: out of pinned memory"); return fail(BZ_E_OOM);
    }
  e->rev.assign(bz_engine::EVRING, nullptr);
  for (hipEvent_t& ev : e->rev) if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { bz_set_error("engine create: hipEventCreate failed"); return fail(BZ_E_HIP); }
  // every row idle: parked at position 0 of its own block
  std::vector<EngRow> rows(N);
  for (int r = 0; r < N; r++) { memset(&rows[r], 0, sizeof(EngRow)); rows[r].park_block = cfg->num_blocks - N + r; }
  if (hipMemcpy(e->d_rows, rows.data(), (size_t)N * sizeof(EngRow), hipMemcpyHostToDevice) != hipSuccess) { bz_set_error("engine create: upload failed"); return fail(BZ_E_HIP); }
  BzEngineRows er{e->d_rows, e->status, e->nlive};
  if ((rc = bzi_engine_capture(m, e->kv, N, e->max_blocks, e->sampler, cursor, &er, &e->g)) != BZ_OK) return fail(rc);
  std::vector<int> table((size_t)N * e->max_blocks, 0);
  for (int r = 0; r < N; r++) table[(size_t)r * e->max_blocks] = rows[r].park_block;
  if (hipMemcpy(e->g->table, table.data(), table.size() * 4, hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    bz_set_error("engine create: upload failed"); return fail(BZ_E_HIP);
  }
  if (cursor) for (int r = 0; r < N; r++) if ((rc = bz_grammar_cursor_set_row(cursor, r, BZ_GRAMMAR_ROW_FREE)) != BZ_OK) return fail(rc);
  *out = e;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_submit(bz_engine* e, const int64_t* prompt, int n_prompt, const bz_request* rq, int64_t* id_out) { return bz_engine_submit_ex(e, prompt, n_prompt, rq, nullptr, id_out); }
extern "C" int bz_engine_submit_ex(bz_engine* e, const int64_t* prompt, int n_prompt, const bz_request* rq, const bz_request_extras* ex, int64_t* id_out) {
  BZ_API_BEGIN
  if (!e || !prompt || !rq || !id_out) BZ_FAIL(BZ_E_INVALID, "engine submit: null argument");
  std::vector<uint32_t> bias_ids; std::vector<float> bias_vals;
  if (ex) {
    if (!e->cfg.logprobs) BZ_FAIL(BZ_E_INVALID, "engine submit: request extras on an engine created with logprobs = %d (bz_engine_config.logprobs = 1 enables bias and logprobs)", e->cfg.logprobs);
    if (ex->top_logprobs < 0 || ex->top_logprobs > BZ_TOP_LOGPROBS_MAX) BZ_FAIL(BZ_E_INVALID, "engine submit: top_logprobs = %d out of range (0 .. %d)", ex->top_logprobs, BZ_TOP_LOGPROBS_MAX);
    BZ_TRY(bzk_lp_check_bias(e->mc.vocab, ex->logit_bias_ids, ex->logit_bias_vals, ex->n_logit_bias, bias_ids, bias_vals, "engine submit"));
  }
  if (n_prompt < 1 || rq->max_tokens < 1) BZ_FAIL(BZ_E_INVALID, "engine submit: n_prompt = %d and max_tokens = %d must both be at least 1", n_prompt, rq->max_tokens);
  if ((long long)n_prompt + rq->max_tokens > e->cfg.max_seq_len)
    BZ_FAIL(BZ_E_INVALID, "engine submit: n_prompt + max_tokens = %lld exceeds max_seq_len = %d", (long long)n_prompt + rq->max_tokens, e->cfg.max_seq_len);
  if (rq->n_stop < 0 || rq->n_stop > BZ_ENGINE_MAX_STOP) BZ_FAIL(BZ_E_INVALID, "engine submit: n_stop = %d stop ids, at most %d", rq->n_stop, BZ_ENGINE_MAX_STOP);
  for (int i = 0; i < n_prompt; i++)
    if (prompt[i] < 0 || prompt[i] >= e->mc.vocab) BZ_FAIL(BZ_E_INVALID, "engine submit: prompt token %d = %lld outside the vocabulary of %d", i, (long long)prompt[i], e->mc.vocab);
  const bz_row_sampling& sp = rq->sampling;
  if (!e->sampler) {
    if (sp.temperature != 0.0f || sp.repeat_penalty != 1.0f || sp.frequency_penalty != 0.0f || sp.presence_penalty != 0.0f)
      BZ_FAIL(BZ_E_INVALID, "engine submit: temperature = %g with penalties %g / %g / %g on an engine without a sampler (greedy without penalties only)", (double)sp.temperature,
              (double)sp.repeat_penalty, (double)sp.frequency_penalty, (double)sp.presence_penalty);
  } else BZ_TRY(bzk_batch_sampler_check_row(&sp, "engine submit"));
  if (rq->grammar_state != BZ_GRAMMAR_ROW_FREE) {
    if (!e->cursor) BZ_FAIL(BZ_E_INVALID, "engine submit: grammar_state = %u on an engine without a grammar cursor", rq->grammar_state);
    if (rq->grammar_state >= (uint32_t)bzk_grammar_cursor_num_states(e->cursor))
      BZ_FAIL(BZ_E_INVALID, "engine submit: grammar_state = %u is not below the grammar's %d states", rq->grammar_state, bzk_grammar_cursor_num_states(e->cursor));
  }
  BzLoraTable* T = bzi_model_lora(e->m);
  if (rq->lora_slot != 0) {
    if (!T) BZ_FAIL(BZ_E_INVALID, "engine submit: lora_slot = %d but the model has no LoRA table", rq->lora_slot);
    if (rq->lora_slot < 0 || rq->lora_slot > T->n_slots || !T->slots[rq->lora_slot - 1])
      BZ_FAIL(BZ_E_INVALID, "engine submit: lora_slot = %d names slot %d, which is empty or outside the table's %d slots", rq->lora_slot, rq->lora_slot - 1, T->n_slots);
  }
  int64_t id = -1;
  // cached KV rows depend on the adapter: a request under one neither looks up nor publishes prefix blocks (submitted without its tokens)
  if (e->cfg.prefix_cache && rq->lora_slot == 0) BZ_TRY(bz_sched_submit_tokens(e->sched, prompt, n_prompt, rq->max_tokens, &id));
  else BZ_TRY(bz_sched_submit(e->sched, n_prompt, rq->max_tokens, &id));  // (names the figure when the request could never fit the pool)
  EngReq& r = e->reqs[id];
  r.id = id; r.prompt.assign(prompt, prompt + n_prompt); r.rq = *rq;
  if (ex) { r.top_n = ex->logprobs ? ex->top_logprobs : -1; r.bias_ids.swap(bias_ids); r.bias_vals.swap(bias_vals); }
  if (rq->lora_slot != 0) T->users[rq->lora_slot - 1]++;
  *id_out = id;
  return BZ_OK;
  BZ_API_END
}

// the stream-ordered write that makes a row idle (cancel): what k_engine_finish does for a row that ends
static int eng_idle_row(bz_engine* e, int row) {
  Stage* s = nullptr;
  BZ_TRY(eng_stage(e, &s));
  hipStream_t st = e->dev->stream;
  RowMisc* mi = (RowMisc*)(s->host + e->off_misc);
  memset(mi, 0, sizeof(*mi));
  mi->er.park_block = e->cfg.num_blocks - e->cfg.n_rows + row;
  mi->lora = -1;
  int* tb = (int*)s->host; tb[0] = mi->er.park_block;
  if (bzi_model_lora(e->m)) BZ_HIP(hipMemcpyAsync(e->g->row_lora + row, &mi->lora, 4, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->d_rows + row, &mi->er, sizeof(EngRow), hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->g->pos + row, &mi->pos, 4, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->g->table + (size_t)row * e->max_blocks, tb, 4, hipMemcpyHostToDevice, st));
  if (e->cursor) BZ_TRY(bzk_grammar_cursor_stage_row(st, e->cursor, row, BZ_GRAMMAR_ROW_FREE, mi->gram));
  if (e->cfg.logprobs) BZ_TRY(bzk_lp_stage_row(st, e->sampler, row, -1, nullptr, nullptr, 0, s->host + e->off_lp));
  return eng_stage_done(e, s);
}

extern "C" int bz_engine_cancel(bz_engine* e, int64_t id) {
  BZ_API_BEGIN
  if (!e) BZ_FAIL(BZ_E_INVALID, "engine cancel: null engine");
  auto it = e->reqs.find(id);
  if (it == e->reqs.end()) BZ_FAIL(BZ_E_INVALID, "engine cancel: request %lld is not waiting or running", (long long)id);
  EngReq& r = it->second;
  BZ_HIP(hipSetDevice(e->dev->id));
  if (r.row >= 0) {
    if (r.live) BZ_TRY(eng_idle_row(e, r.row));
    e->row_req[r.row] = -1;
  }
  BZ_TRY(bz_sched_finish(e->sched, id));
  e->events.push_back(bz_engine_event{id, -1, r.produced, 2, e->g->replays});
  eng_lora_release(e, r);
  e->reqs.erase(it);
  return BZ_OK;
  BZ_API_END
}

// the record of replay number e->read -> events; finished requests give their row and blocks back
static int eng_harvest(bz_engine* e) {
  const long long r = e->read;
  BZ_HIP(hipEventSynchronize(e->rev[r % bz_engine::EVRING]));
  const int N = e->cfg.n_rows;
  const size_t at = (size_t)(r % bz_batch_graph::LOGCAP) * N;
  const volatile int* st = e->status + at;
  const volatile long long* lg = e->g->log + at;
  for (int row = 0; row < N; row++) {
    const int w = st[row];
    if ((w & 3) == ENG_IDLE || e->row_req[row] < 0) continue;
    EngReq& q = e->reqs.at(e->row_req[row]);
    if (!q.live || q.first_replay > r) continue;            // a token of the row's previous (cancelled) request
    const bool fin = (w & 3) == ENG_FINISHED;
    e->events.push_back(bz_engine_event{q.id, lg[row], q.produced, fin ? (w >> 2) : -1, r});
    if (q.top_n >= 0) {                                     // the record k_lp_record wrote in the same replay
      const bz_logprobs_record& rec = bzk_lp_ring(e->sampler)[at + row];
      bz_engine_logprobs lp;
      memset(&lp, 0, sizeof(lp));
      lp.id = q.id; lp.index = q.produced; lp.token = rec.token; lp.logprob = rec.logprob; lp.n_top = rec.n_top;
      for (int k = 0; k < rec.n_top && k < BZ_TOP_LOGPROBS_MAX; k++) { lp.top_ids[k] = rec.top_ids[k]; lp.top_logprobs[k] = rec.top_logprobs[k]; }
      e->lp_events.push_back(lp);
    }
    q.produced++; e->generated++;
    if (fin) {
      const int64_t id = q.id;
      BZ_TRY(bz_sched_finish(e->sched, id));
      e->row_req[row] = -1;
      eng_lora_release(e, q);
      e->reqs.erase(id);
    }
  }
  e->read++;
  return BZ_OK;
}

// one prompt chunk [a, b) of prompt[:-1] through bz_forward_paged; tokens, slots and the table are staged, nothing waits
static int eng_prefill(bz_engine* e, EngReq& q, int a, int b, const int32_t* blocks, int nb) {
  Stage* s = nullptr;
  BZ_TRY(eng_stage(e, &s));
  hipStream_t st = e->dev->stream;
  const int S = b - a, bs = e->cfg.block_size;
  long long* tk = (long long*)(s->host + e->off_ptok); int* sl = (int*)(s->host + e->off_pslot); int* tb = (int*)s->host;
  for (int i = 0; i < S; i++) { tk[i] = q.prompt[a + i]; sl[i] = blocks[(a + i) / bs] * bs + (a + i) % bs; }
  for (int i = 0; i < e->max_blocks; i++) tb[i] = i < nb ? blocks[i] : 0;
  BZ_HIP(hipMemcpyAsync(e->d_ptok, tk, (size_t)S * 8, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->d_pslot, sl, (size_t)S * 4, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->d_ptable, tb, (size_t)e->max_blocks * 4, hipMemcpyHostToDevice, st));
  BZ_TRY(eng_stage_done(e, s));
  bz_tensor t_tok, t_slot, t_tab;
  t_tok.dev = t_slot.dev = t_tab.dev = e->dev; t_tok.owned = t_slot.owned = t_tab.owned = false;
  t_tok.ptr = e->d_ptok; t_tok.dtype = BZ_I64; t_tok.nbytes = (size_t)S * 8; t_tok.shape = {1, S};
  t_slot.ptr = e->d_pslot; t_slot.dtype = BZ_I32; t_slot.nbytes = (size_t)S * 4; t_slot.shape = {S};
  t_tab.ptr = e->d_ptable; t_tab.dtype = BZ_I32; t_tab.nbytes = (size_t)nb * 4; t_tab.shape = {nb};
  BZ_TRY(bzi_forward_paged_lora(e->m, eng_lora_slot(q), &t_tok, S, e->kv, &t_slot, &t_tab, nb, b, a, e->plogits, 0));   // the prompt runs under the request's adapter
  e->prompt_tokens += S;
  return BZ_OK;
}

// the row writes that make a request live: it feeds prompt[-1] at seq_len = n_prompt in the next replay
static int eng_go_live(bz_engine* e, EngReq& q, const int32_t* blocks, int nb) {
  Stage* s = nullptr;
  BZ_TRY(eng_stage(e, &s));
  hipStream_t st = e->dev->stream;
  const int row = q.row, n = (int)q.prompt.size();
  int* tb = (int*)s->host;
  for (int i = 0; i < e->max_blocks; i++) tb[i] = i < nb ? blocks[i] : 0;
  RowMisc* mi = (RowMisc*)(s->host + e->off_misc);
  memset(mi, 0, sizeof(*mi));
  mi->next = q.prompt[n - 1]; mi->pos = n - 2;                     // k_engine_advance adds 1
  mi->lora = eng_lora_slot(q);
  if (bzi_model_lora(e->m)) BZ_HIP(hipMemcpyAsync(e->g->row_lora + row, &mi->lora, 4, hipMemcpyHostToDevice, st));
  mi->er.live = 1; mi->er.left = q.rq.max_tokens; mi->er.n_stop = q.rq.n_stop; mi->er.park_block = e->cfg.num_blocks - e->cfg.n_rows + row;
  for (int k = 0; k < q.rq.n_stop; k++) mi->er.stop[k] = q.rq.stop_ids[k];
  BZ_HIP(hipMemcpyAsync(e->g->table + (size_t)row * e->max_blocks, tb, (size_t)e->max_blocks * 4, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->g->next + row, &mi->next, 8, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(e->g->pos + row, &mi->pos, 4, hipMemcpyHostToDevice, st));
  if (e->sampler) BZ_TRY(bzk_batch_sampler_stage_row(st, e->sampler, row, &q.rq.sampling, q.prompt.data(), n, 0, s->host + e->off_bs));
  if (e->cursor) BZ_TRY(bzk_grammar_cursor_stage_row(st, e->cursor, row, q.rq.grammar_state, mi->gram));
  if (e->cfg.logprobs) BZ_TRY(bzk_lp_stage_row(st, e->sampler, row, q.top_n, q.bias_ids.data(), q.bias_vals.data(), (int)q.bias_ids.size(), s->host + e->off_lp));
  BZ_HIP(hipMemcpyAsync(e->d_rows + row, &mi->er, sizeof(EngRow), hipMemcpyHostToDevice, st));
  BZ_TRY(eng_stage_done(e, s));
  q.live = true; q.first_replay = e->g->replays;
  return BZ_OK;
}

// the step's copy-on-write triples: staged, uploaded and served by one launch, stream-ordered like every other admission write
static int eng_copies(bz_engine* e, Stage* s, int n, int max_j) {
  hipStream_t st = e->dev->stream;
  BZ_HIP(hipMemcpyAsync(e->d_copy, s->host + e->off_copy, (size_t)n * 12, hipMemcpyHostToDevice, st));
  BZ_TRY(eng_stage_done(e, s));
  BZ_TRY(bzk_kv_copy_slots(st, e->kv, e->d_copy, n, max_j));
  e->copy_launches++; e->copied_blocks += n;
  return BZ_OK;
}

extern "C" int bz_engine_step(bz_engine* e, int* busy_out) {
  BZ_API_BEGIN
  if (!e) BZ_FAIL(BZ_E_INVALID, "engine step: null engine");
  BZ_HIP(hipSetDevice(e->dev->id));
  // (1) the oldest unread record, once `depth` are unread
  if (e->g->replays - e->read >= e->cfg.depth) BZ_TRY(eng_harvest(e));
  // (2) admissions, prompt chunks, rows going live
  int na = 0;
  BZ_TRY(bz_sched_step(e->sched, e->acts.data(), (int)e->acts.size(), &na));
  if (na > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> blocks(e->max_blocks);
    Stage* cs = nullptr; int ncopy = 0, max_j = 0;         // this step's copies: one launch, ahead of the step's prompt chunks (admissions come first in the list)
    for (int i = 0; i < na; i++) {
      const bz_sched_action& a = e->acts[i];
      EngReq& q = e->reqs.at(a.id);
      if (a.kind == BZ_SCHED_ADMIT) { q.row = a.row; q.shared = a.b; e->row_req[a.row] = a.id; e->skipped += (long long)a.b * e->cfg.block_size; continue; }
      int64_t rid = -1; int nb = 0;
      BZ_TRY(bz_sched_row(e->sched, a.row, &rid, blocks.data(), e->max_blocks, &nb));
      if (a.kind == BZ_SCHED_COPY) {
        if (ncopy >= e->cfg.n_rows || q.shared >= nb) BZ_FAIL(BZ_E_INVALID, "engine step: copy %d of a step, destination index %d of %d blocks", ncopy, q.shared, nb);
        if (!cs) BZ_TRY(eng_stage(e, &cs));
        int* tr = (int*)(cs->host + e->off_copy) + 3 * ncopy++;
        tr[0] = a.a; tr[1] = blocks[q.shared]; tr[2] = a.b;
        max_j = std::max(max_j, a.b); e->skipped += a.b;
        continue;
      }
      if (cs) { BZ_TRY(eng_copies(e, cs, ncopy, max_j)); cs = nullptr; }
      if (a.kind == BZ_SCHED_PREFILL) {
        for (int c0 = a.a; c0 < a.b; c0 += e->max_chunk) BZ_TRY(eng_prefill(e, q, c0, std::min(a.b, c0 + e->max_chunk), blocks.data(), nb));
      } else BZ_TRY(eng_go_live(e, q, blocks.data(), nb));
    }
    if (cs) BZ_TRY(eng_copies(e, cs, ncopy, max_j));
    e->admit_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  // (3) one replay while any row is live in the host's view; else drain
  bool any = false;
  for (int row = 0; row < e->cfg.n_rows; row++) {
    if (e->row_req[row] < 0) continue;
    const EngReq& q = e->reqs.at(e->row_req[row]);
    if (!q.live) continue;
    any = true;
    // an idle row does not move; a live one is stopped by the device at n_prompt + max_tokens - 1 positions, which submit held within max_seq_len
    const int reach = (int)q.prompt.size() + q.rq.max_tokens - 1;
    if (reach > e->g->capacity) BZ_FAIL(BZ_E_INVALID, "engine step: row %d would reach position %d, beyond the capacity %d the step was captured over", row, reach, e->g->capacity);
  }
  if (any) {
    BZ_TRY(bzi_batch_graph_launch(e->g));
    BZ_HIP(hipEventRecord(e->rev[(e->g->replays - 1) % bz_engine::EVRING], e->dev->stream));
  } else {
    while (e->read < e->g->replays) BZ_TRY(eng_harvest(e));
  }
  if (busy_out) *busy_out = (!e->reqs.empty() || e->read < e->g->replays) ? 1 : 0;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_poll(bz_engine* e, bz_engine_event* out, int max_events, int* n_out) {
  BZ_API_BEGIN
  if (!e || !n_out || (max_events > 0 && !out) || max_events < 0) BZ_FAIL(BZ_E_INVALID, "engine poll: bad argument");
  int n = 0;
  while (n < max_events && !e->events.empty()) { out[n++] = e->events.front(); e->events.pop_front(); }
  *n_out = n;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_poll_logprobs(bz_engine* e, bz_engine_logprobs* out, int max_records, int* n_out) {
  BZ_API_BEGIN
  if (!e || !n_out || (max_records > 0 && !out) || max_records < 0) BZ_FAIL(BZ_E_INVALID, "engine poll_logprobs: bad argument");
  int n = 0;
  while (n < max_records && !e->lp_events.empty()) { out[n++] = e->lp_events.front(); e->lp_events.pop_front(); }
  *n_out = n;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_stats(bz_engine* e, bz_engine_stats_t* out) {
  BZ_API_BEGIN
  if (!e || !out) BZ_FAIL(BZ_E_INVALID, "engine stats: null argument");
  bz_sched_info_t si;
  BZ_TRY(bz_sched_info(e->sched, &si));
  memset(out, 0, sizeof(*out));
  out->replays = e->g->replays; out->free_blocks = si.free_blocks; out->total_blocks = si.num_blocks; out->park_blocks = si.park_blocks;
  out->live_rows = si.live; out->admitted = si.admitted; out->waiting = si.waiting; out->unread = (int)(e->g->replays - e->read);
  out->prompt_tokens = e->prompt_tokens; out->generated_tokens = e->generated; out->admit_host_ms = e->admit_ms;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_prefix_stats(bz_engine* e, bz_engine_prefix_stats_t* out) {
  BZ_API_BEGIN
  if (!e || !out) BZ_FAIL(BZ_E_INVALID, "engine prefix_stats: null argument");
  bz_sched_info_t si; bz_sched_prefix_info_t pi;
  BZ_TRY(bz_sched_info(e->sched, &si));
  BZ_TRY(bz_sched_prefix_info(e->sched, &pi));
  memset(out, 0, sizeof(*out));
  out->enabled = pi.enabled; out->cached_blocks = pi.cached_blocks; out->evictable_blocks = pi.evictable_blocks; out->referenced_blocks = pi.referenced_blocks;
  out->private_blocks = si.owned_blocks; out->hits = pi.hits; out->misses = pi.misses; out->cached_tokens = pi.cached_tokens; out->evictions = pi.evictions;
  out->prompt_tokens_skipped = e->skipped; out->copy_launches = e->copy_launches; out->copied_blocks = e->copied_blocks;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_engine_prefix_flush(bz_engine* e, int* dropped_out) {
  BZ_API_BEGIN
  if (!e) BZ_FAIL(BZ_E_INVALID, "engine prefix_flush: null engine");
  return bz_sched_prefix_flush(e->sched, dropped_out);
  BZ_API_END
}

// ---- the copy kernel on its own ---------------------------------------------------------------------------
extern "C" int bz_paged_kv_copy_slots(bz_paged_kv* kv, int src, int dst, int n_slots) {
  BZ_API_BEGIN
  if (!kv) BZ_FAIL(BZ_E_INVALID, "kv copy_slots: null cache");
  if (src < 0 || src >= kv->num_blocks || dst < 0 || dst >= kv->num_blocks) BZ_FAIL(BZ_E_INVALID, "kv copy_slots: blocks %d -> %d outside the pool's %d", src, dst, kv->num_blocks);
  if (src == dst) BZ_FAIL(BZ_E_INVALID, "kv copy_slots: source and destination are both block %d", src);
  if (n_slots < 1 || n_slots > kv->block_size) BZ_FAIL(BZ_E_INVALID, "kv copy_slots: %d slots outside 1 .. block_size = %d", n_slots, kv->block_size);
  BZ_HIP(hipSetDevice(kv->dev->id));
  const int tr[3] = {src, dst, n_slots};
  int* d = nullptr;
  BZ_HIP(hipMalloc(&d, sizeof(tr)));
  int rc = hipMemcpyAsync(d, tr, sizeof(tr), hipMemcpyHostToDevice, kv->dev->stream) == hipSuccess ? BZ_OK : BZ_E_HIP;
  if (rc == BZ_OK) rc = bzk_kv_copy_slots(kv->dev->stream, kv, d, 1, n_slots);
  if (hipStreamSynchronize(kv->dev->stream) != hipSuccess && rc == BZ_OK) rc = BZ_E_HIP;
  hipFree(d);
  if (rc == BZ_E_HIP) bz_set_error("kv copy_slots: the copy failed on the device");
  return rc;
  BZ_API_END
}

extern "C" int bz_engine_read_status(bz_engine* e, int64_t replay, int32_t* status_out, int32_t* live_after_out) {
  BZ_API_BEGIN
  if (!e || !status_out) BZ_FAIL(BZ_E_INVALID, "engine read_status: null argument");
  if (replay < 0 || replay >= e->g->replays || replay < e->g->replays - bz_batch_graph::LOGCAP) BZ_FAIL(BZ_E_INVALID, "engine read_status: replay %lld out of range", (long long)replay);
  BZ_HIP(hipSetDevice(e->dev->id));
  if (replay >= e->read) BZ_HIP(hipStreamSynchronize(e->dev->stream));
  const size_t at = (size_t)(replay % bz_batch_graph::LOGCAP);
  for (int i = 0; i < e->cfg.n_rows; i++) status_out[i] = ((volatile int*)e->status)[at * e->cfg.n_rows + i];
  if (live_after_out) *live_after_out = ((volatile int*)e->nlive)[at];
  return BZ_OK;
  BZ_API_END
}
