// bz_route.hip -- which path a prompt, a decode batch or a speculative verify takes (DESIGN.md "Which path a prompt takes").  Plain C++: no kernel, no HIP
// call -- a pure function of a model's traits (bz_prompt_traits_t, filled once at finalize), six switches, and the call's kind, rows and context, so that
// tests/prompt_plan_ref.py can restate it and tests/test_prompt_plan.py can sweep it without a device.  The callers in bz_host.hip dispatch on the plan and
// hand it to the prompt functions; bzk_pf_attn launches the attention form it names and refuses one whose preconditions do not hold.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bz_internal.h"

// the six switches the route depends on, read once per process
const bz_prompt_switches_t* bzk_prompt_switches() {
  static const bz_prompt_switches_t sw = [] {
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    bz_prompt_switches_t s;
    s.prefill_min = num("BZ_PREFILL_MIN", 8);
    s.no_mfma_prefill = getenv("BZ_NO_MFMA_PREFILL") != nullptr;
    s.no_gguf_prefill = getenv("BZ_NO_GGUF_PREFILL") != nullptr;
    const char* ex = getenv("BZ_EXACT_PREFILL");     // -1: by prompt length
    s.exact = ex ? atoi(ex) : -1;
    s.exact_max = num("BZ_EXACT_PREFILL_MAX", 16);
    s.exact_i8_max = num("BZ_EXACT_I8_MAX", 0);
    return s;
  }();
  return &sw;
}

namespace {
const size_t LDS_MAX = 160 * 1024;
bool act16(const bz_prompt_traits_t& t) { return t.act_dtype == BZ_F16 || t.act_dtype == BZ_BF16; }
// the most keys any layer's query reads at a context of `len` positions: the window where every layer has one (sliding_window_pattern n > 1 leaves each
// n-th layer, l % n == n - 1, on full attention)
int window_keys(const bz_prompt_traits_t& t, int len) {
  const int n = t.sliding_window_pattern;
  const bool all = t.sliding_window > 0 && !(n > 1 && t.n_layers >= n);
  return all ? std::min(len, t.sliding_window) : len;
}
// Models whose decode sums are exact and whose MFMA sums are not (dense 16-bit projections, DeepSeek-V2, Mamba2): prompts of up to BZ_EXACT_PREFILL_MAX (16)
// rows stay on the decode kernels, token by token, so that their rows are the oracle's bits; BZ_EXACT_PREFILL=0: never, > 0: every prompt
bool short_stays_on_steps(const bz_prompt_switches_t& sw, int S) { return sw.exact != 0 && (sw.exact > 0 || S <= sw.exact_max); }
// EXACT prompt rows (f16 int4 models): the multi-row form of the decode kernels' integer arithmetic for every projection, the exact scalar attention and the
// decode lm_head -- a prompt row is then the same bits as the decode step would produce for it (tests/test_gpu_exact_prefill.py).  One pass over the weights
// serves 8 rows and costs ~3.9 ms at the 8B AWQ shape (13 launches per layer), the MFMA path has a floor of ~4.6 ms: up to BZ_EXACT_PREFILL_MAX rows (default
// 16: two passes) exactness is nearly free (32 rows: 15.8 vs 4.8 ms); longer prompts take the matrix cores, whose f32 accumulation order differs from the exact
// sums: ~1e-6 per GEMM, which the f16 roundings of a deep model amplify to the f16 noise floor (profiles/r03_prefill_parity_depth.txt).
// 0 (MFMA f16 path), 1 (exact rows: BZ_EXACT_PREFILL=1 for every prompt) or 2 (exact integer-MFMA GEMMs: BZ_EXACT_PREFILL=2 for every prompt beyond 16 rows, or
// prompts of up to BZ_EXACT_I8_MAX rows), as far as the model's projections have the form (exact_cap)
int exact_mode(const bz_prompt_traits_t& t, const bz_prompt_switches_t& sw, int n) {
  if (sw.exact == 0 || t.act_dtype != BZ_F16) return 0;
  int mode = 0;
  if (sw.exact == 1) mode = 1; else if (sw.exact >= 2) mode = n <= 16 ? 1 : 2;
  else if (n <= sw.exact_max) mode = 1; else if (n <= sw.exact_i8_max) mode = 2;
  return std::min(mode, t.exact_cap);
}

void plan_llama(const bz_prompt_traits_t& t, const bz_prompt_switches_t& sw, int kind, int rows, int total_len, int min_rows, bz_prompt_plan_t* p) {
  if (!t.shapes_ok) return;
  if (kind == BZ_PLAN_VERIFY) {
    // the multi-row exact rows without the row floor and at any position: f16 int4 model, the exact attention's scores of the whole context in LDS, and a head
    // the multi-row lm_head takes
    if (t.act_dtype != BZ_F16 || rows > 16 || exact_mode(t, sw, rows) != 1 || !t.spec_head) return;
    if (bzk_pf_attn_smem(t.n_heads, t.n_kv_heads, t.head_dim, window_keys(t, total_len), true) > LDS_MAX) return;
    *p = bz_prompt_plan_t{BZ_ROUTE_ROWS, 1, BZ_PF_ATTN_SCALAR_EXACT, BZ_HEAD_SPEC, 2048};
    return;
  }
  const bool batch = kind == BZ_PLAN_DECODE_BATCH;
  const int S = batch ? std::max(rows, min_rows) : rows;     // (a decode batch is never turned away for its row count)
  if (S < min_rows || (!act16(t) && (t.act_dtype != BZ_F32 || sw.no_gguf_prefill))) return;
  const int exact = batch ? 0 : exact_mode(t, sw, S);
  const bool f32 = t.act_dtype == BZ_F32, mfma = bzk_pf_attn_mfma_ok(t.head_dim, t.rep);
  // f32 models: the oracle's double-precision sums cost little next to the f32 cache reads
  const int attn = batch ? BZ_PF_ATTN_ROWS : (exact || f32) ? BZ_PF_ATTN_SCALAR_EXACT : mfma ? BZ_PF_ATTN_MFMA : BZ_PF_ATTN_SCALAR;
  // the scalar kernel keeps a row's scores (its window) in LDS: where the context does not fit, the prompt runs on the decode step, whose attention has no
  // context limit.  ODDITY, kept as found: a decode batch skips this check wherever bzk_pf_attn_mfma_ok holds -- a stand-in for "the split-KV pair exists at
  // this shape" (rows_attn_prepare has the real test and refuses by name) -- so BZ_NO_PF_ATTN_MFMA changes which decode batches are admitted.
  if (attn != BZ_PF_ATTN_MFMA && !(batch && mfma) &&
      bzk_pf_attn_smem(t.n_heads, t.n_kv_heads, t.head_dim, window_keys(t, total_len), attn == BZ_PF_ATTN_SCALAR_EXACT) > LDS_MAX) return;
  int head;
  if (f32) {
    // block formats (GGUF): the split operands go through ONE 16-bit GEMM over 3 K whose element offsets are 32-bit; a quantised head stays the decode step's
    if (!t.gq_all || t.gq_max_n3k >= (1ull << 32) || (unsigned long long)std::min(S, 2048) * 3ull * (unsigned long long)t.gq_max_k >= (1ull << 32)) return;
    head = t.head_rows ? BZ_HEAD_GEMV_ROWS : BZ_HEAD_STEP;
  } else {
    if (!t.proj_16 || (t.any_dense && !batch && short_stays_on_steps(sw, S)) || !t.head_rows) return;
    head = (!exact && t.head_gemm) ? BZ_HEAD_GEMM : BZ_HEAD_GEMV_ROWS;
  }
  *p = bz_prompt_plan_t{BZ_ROUTE_ROWS, exact, attn, head, batch ? 512 : 2048};     // prompts: 2048-row chunks (larger GEMMs: 8B AWQ 2048-token prompt 105 -> 90 ms)
}

void plan_dsv2(const bz_prompt_traits_t& t, const bz_prompt_switches_t& sw, int S, int total_len, int kv_dtype, int min_rows, bz_prompt_plan_t* p) {
  if (S < min_rows || !act16(t) || t.mla_q_lora_rank > 0 || short_stays_on_steps(sw, S)) return;
  if (!t.ds_dims_ok || kv_dtype != t.act_dtype || !t.ds_weights_act) return;
  // the decode kernel's LDS (16 waves, no split) bounds the context
  MlaArgs probe{}; probe.rank = t.mla_kv_lora_rank; probe.rope = t.mla_rope_dim; probe.nope = t.mla_nope_dim; probe.vdim = t.mla_v_dim;
  if (bzk_mla_smem(probe, total_len) > LDS_MAX || !t.head_rows) return;
  *p = bz_prompt_plan_t{BZ_ROUTE_DSV2, 0, BZ_PF_ATTN_NONE, t.head_gemm ? BZ_HEAD_GEMM : BZ_HEAD_GEMV_ROWS, 512};
}

void plan_mamba(const bz_prompt_traits_t& t, const bz_prompt_switches_t& sw, int S, int min_rows, bz_prompt_plan_t* p) {
  if (S < min_rows || !act16(t) || short_stays_on_steps(sw, S)) return;
  if (!t.ssm_scan_ok || !t.ssm_groups_ok || !t.ssm_proj_ok || !t.head_rows) return;
  *p = bz_prompt_plan_t{BZ_ROUTE_MAMBA, 0, BZ_PF_ATTN_NONE, BZ_HEAD_GEMV_ROWS, 512};
}
}  // namespace

extern "C" int bz_prompt_plan(const bz_prompt_traits_t* t, const bz_prompt_switches_t* sw, int kind, int rows, int total_len, int kv_dtype, bz_prompt_plan_t* out) {
  BZ_API_BEGIN
  if (!t || !out || kind < BZ_PLAN_PROMPT || kind > BZ_PLAN_VERIFY || rows <= 0 || total_len <= 0) BZ_FAIL(BZ_E_INVALID, "prompt_plan: bad argument");
  if (!sw) sw = bzk_prompt_switches();
  const int min_rows = sw->no_mfma_prefill ? (1 << 30) : sw->prefill_min;
  *out = bz_prompt_plan_t{BZ_ROUTE_STEPS, 0, BZ_PF_ATTN_NONE, BZ_HEAD_STEP, 0};
  if (t->arch == BZ_ARCH_LLAMA) plan_llama(*t, *sw, kind, rows, total_len, min_rows, out);
  else if (kind != BZ_PLAN_PROMPT) return BZ_OK;     // decode batches and the verify are built for the Llama family
  else if (t->arch == BZ_ARCH_DEEPSEEK2) plan_dsv2(*t, *sw, rows, total_len, kv_dtype, min_rows, out);
  else if (t->arch == BZ_ARCH_MAMBA2) plan_mamba(*t, *sw, rows, min_rows, out);
  return BZ_OK;
  BZ_API_END
}

// ---- packed prompt batches: n_seq inputs laid end to end, one prompt pass for all of them -------------------------------------------------
int bzk_packed_lens(const int32_t* seq_lens, int n_seq, const char* who, std::vector<int>* seg_lo, std::vector<int>* seg_off, int* max_len) {
  if (!seq_lens || n_seq <= 0) BZ_FAIL(BZ_E_INVALID, "%s: n_seq = %d inputs (at least 1, with their lengths)", who, n_seq);
  long long T = 0;
  int ml = 0;
  for (int i = 0; i < n_seq; i++) {
    if (seq_lens[i] <= 0) BZ_FAIL(BZ_E_INVALID, "%s: seq_lens[%d] = %d (every input has at least one token)", who, i, seq_lens[i]);
    T += seq_lens[i]; ml = std::max(ml, (int)seq_lens[i]);
    if (T >= (1ll << 31)) BZ_FAIL(BZ_E_INVALID, "%s: %lld packed rows and more (below 2^31)", who, T);
  }
  if (seg_off) { seg_off->resize((size_t)n_seq + 1); (*seg_off)[0] = 0; for (int i = 0; i < n_seq; i++) (*seg_off)[i + 1] = (*seg_off)[i] + seq_lens[i]; }
  if (seg_lo) {
    seg_lo->resize((size_t)T);
    size_t r = 0;
    for (int i = 0; i < n_seq; i++) { const int lo = (int)r; for (int k = 0; k < seq_lens[i]; k++) (*seg_lo)[r++] = lo; }
  }
  if (max_len) *max_len = ml;
  return BZ_OK;
}

// One packed pass exactly when the prompt plan of T = sum(seq_lens) rows answers ROWS at a context of the LONGEST input: a query reads its own input's keys and
// nothing else, so the longest input is what the scalar attention's score buffer has to hold.  Everything else (odd GQA groups, DeepSeek-V2, Mamba2, T below the
// row floor, models whose plan is STEPS) takes the single-input path once per input inside the library: packed = 0, and `plan` is the plan of the longest input.
extern "C" int bz_packed_plan(const bz_prompt_traits_t* t, const bz_prompt_switches_t* sw, const int32_t* seq_lens, int n_seq, int kv_dtype, bz_packed_plan_t* out) {
  BZ_API_BEGIN
  if (!t || !out) BZ_FAIL(BZ_E_INVALID, "packed_plan: bad argument");
  std::vector<int> off;
  int max_len = 0;
  BZ_TRY(bzk_packed_lens(seq_lens, n_seq, "packed_plan", nullptr, &off, &max_len));
  const int T = off[(size_t)n_seq];
  bz_prompt_plan_t p;
  BZ_TRY(bz_prompt_plan(t, sw, BZ_PLAN_PROMPT, T, max_len, kv_dtype, &p));
  out->packed = p.route == BZ_ROUTE_ROWS ? 1 : 0;
  out->rows = T; out->n_seq = n_seq; out->max_len = max_len;
  if (!out->packed) BZ_TRY(bz_prompt_plan(t, sw, BZ_PLAN_PROMPT, max_len, max_len, kv_dtype, &p));
  out->plan = p;
  return BZ_OK;
  BZ_API_END
}

// the two host-side definitions of bz_score_batch, public as bz_score_row_spec is: a CPU-only test holds them to an independent restatement
extern "C" int bz_packed_targets_spec(const int64_t* tokens, const int32_t* seq_lens, int n_seq, int64_t* targets_out) {
  BZ_API_BEGIN
  std::vector<int> off;
  BZ_TRY(bzk_packed_lens(seq_lens, n_seq, "packed_targets_spec", nullptr, &off, nullptr));
  if (!tokens || !targets_out) BZ_FAIL(BZ_E_INVALID, "packed_targets_spec: null tokens / targets_out");
  for (int i = 0; i < n_seq; i++) {      // every row reads the next token of its own input; an input's last row is not scored
    for (int r = off[i]; r + 1 < off[i + 1]; r++) targets_out[r] = tokens[r + 1];
    targets_out[(size_t)off[i + 1] - 1] = -1;
  }
  return BZ_OK;
  BZ_API_END
}
extern "C" int bz_packed_totals_spec(const bz_score_row* rows, const int32_t* seq_lens, int n_seq, bz_score_total* totals_out) {
  BZ_API_BEGIN
  std::vector<int> off;
  BZ_TRY(bzk_packed_lens(seq_lens, n_seq, "packed_totals_spec", nullptr, &off, nullptr));
  if (!rows || !totals_out) BZ_FAIL(BZ_E_INVALID, "packed_totals_spec: null rows / totals_out");
  for (int i = 0; i < n_seq; i++) {      // per input, in row order, over the scored rows whose logprob is finite -- as a single call's total
    totals_out[i].sum_logprob = 0.0; totals_out[i].n_scored = 0;
    for (int r = off[i]; r < off[i + 1]; r++)
      if (rows[r].n_top >= 0 && std::isfinite(rows[r].logprob)) { totals_out[i].sum_logprob += (double)rows[r].logprob; totals_out[i].n_scored++; }
  }
  return BZ_OK;
  BZ_API_END
}
