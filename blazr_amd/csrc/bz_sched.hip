// bz_sched.hip -- the request scheduler of the continuous-batching engine (engine/request_scheduler.rs:105-205; the chunked prompt of
// engine/batch_engine.rs:172-272).  Plain C++: no HIP call, no clock, no randomness -- a pure function of the calls it receives, so that
// tests/engine_ref.py can restate it and predict every decision.  The policy is in include/blazr_hip.h.
#include <algorithm>
#include <cstdint>
#include <deque>
#include <vector>
#include <map>

#include "bz_internal.h"

namespace {
struct SchedReq { int64_t id; int n_prompt, max_tokens, row, done; bool live; std::vector<int> blocks; };
}
struct bz_sched {
  int n_rows = 0, num_blocks = 0, block_size = 0, max_seq_len = 0, chunk = 0, usable = 0;
  int64_t next_id = 0;
  std::deque<SchedReq> waiting;
  std::map<int64_t, SchedReq> admitted;      // by id
  std::vector<int64_t> row_req;              // [n_rows] id or -1
  std::vector<char> block_used;              // [usable]
  std::vector<int64_t> prefilling;           // admitted and not live yet, in admission order
  int free_blocks = 0;
};

static int blocks_for(const bz_sched* s, int n_prompt, int max_tokens) { return (n_prompt + max_tokens + s->block_size - 1) / s->block_size; }

extern "C" int bz_sched_create(int n_rows, int num_blocks, int block_size, int max_seq_len, int prefill_chunk, bz_sched** out) {
  BZ_API_BEGIN
  if (!out) BZ_FAIL(BZ_E_INVALID, "sched create: null output pointer");
  *out = nullptr;
  if (n_rows < 1 || n_rows > 512) BZ_FAIL(BZ_E_INVALID, "sched create: n_rows = %d out of range (1 <= n_rows <= 512)", n_rows);
  if (block_size < 1 || max_seq_len < 2 || prefill_chunk < 0) BZ_FAIL(BZ_E_INVALID, "sched create: bad block_size / max_seq_len / prefill_chunk (%d / %d / %d)", block_size, max_seq_len, prefill_chunk);
  if (num_blocks <= n_rows) BZ_FAIL(BZ_E_INVALID, "sched create: num_blocks = %d leaves nothing beside the %d park blocks", num_blocks, n_rows);
  bz_sched* s = new bz_sched();
  s->n_rows = n_rows; s->num_blocks = num_blocks; s->block_size = block_size; s->max_seq_len = max_seq_len; s->chunk = prefill_chunk;
  s->usable = num_blocks - n_rows; s->free_blocks = s->usable;
  s->row_req.assign(n_rows, -1);
  s->block_used.assign(s->usable, 0);
  *out = s;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_free(bz_sched* s) { delete s; return BZ_OK; }

extern "C" int bz_sched_submit(bz_sched* s, int n_prompt, int max_tokens, int64_t* id_out) {
  BZ_API_BEGIN
  if (!s || !id_out) BZ_FAIL(BZ_E_INVALID, "sched submit: null argument");
  if (n_prompt < 1 || max_tokens < 1) BZ_FAIL(BZ_E_INVALID, "sched submit: n_prompt = %d and max_tokens = %d must both be at least 1", n_prompt, max_tokens);
  if ((long long)n_prompt + max_tokens > s->max_seq_len)
    BZ_FAIL(BZ_E_INVALID, "sched submit: n_prompt + max_tokens = %lld exceeds max_seq_len = %d", (long long)n_prompt + max_tokens, s->max_seq_len);
  const int need = blocks_for(s, n_prompt, max_tokens);
  if (need > s->usable)
    BZ_FAIL(BZ_E_INVALID, "sched submit: the request needs %d blocks of %d and could never fit the pool's %d (%d minus %d park blocks)", need, s->block_size, s->usable,
            s->num_blocks, s->n_rows);
  SchedReq r{s->next_id++, n_prompt, max_tokens, -1, 0, false, {}};
  s->waiting.push_back(r);
  *id_out = r.id;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_step(bz_sched* s, bz_sched_action* out, int max_out, int* n_out) {
  BZ_API_BEGIN
  if (!s || !out || !n_out) BZ_FAIL(BZ_E_INVALID, "sched step: null argument");
  if (max_out < 3 * s->n_rows) BZ_FAIL(BZ_E_INVALID, "sched step: room for %d actions, a step can take %d", max_out, 3 * s->n_rows);
  int n = 0;
  // admissions: the head of the queue only (no skipping ahead)
  while (!s->waiting.empty()) {
    SchedReq& h = s->waiting.front();
    const int need = blocks_for(s, h.n_prompt, h.max_tokens);
    int row = -1;
    for (int r = 0; r < s->n_rows; r++) if (s->row_req[r] < 0) { row = r; break; }
    if (row < 0 || need > s->free_blocks) break;
    SchedReq a = h;
    s->waiting.pop_front();
    a.row = row;
    for (int b = 0; b < s->usable && (int)a.blocks.size() < need; b++) if (!s->block_used[b]) { s->block_used[b] = 1; a.blocks.push_back(b); }
    s->free_blocks -= need;
    s->row_req[row] = a.id;
    s->prefilling.push_back(a.id);
    out[n++] = bz_sched_action{BZ_SCHED_ADMIT, row, a.id, need, 0};
    s->admitted[a.id] = a;
  }
  // prompt chunks, in admission order, within the step's budget; a request whose prompt[:-1] is complete becomes live
  long long budget = s->chunk > 0 ? s->chunk : (1ll << 40);
  std::vector<int64_t> still;
  for (int64_t id : s->prefilling) {
    SchedReq& a = s->admitted[id];
    const int total = a.n_prompt - 1;
    const int take = (int)std::min<long long>(total - a.done, budget);
    if (take > 0) {
      out[n++] = bz_sched_action{BZ_SCHED_PREFILL, a.row, a.id, a.done, a.done + take};
      a.done += take; budget -= take;
    }
    if (a.done == total) { a.live = true; out[n++] = bz_sched_action{BZ_SCHED_LIVE, a.row, a.id, 0, 0}; }
    else still.push_back(id);
  }
  s->prefilling.swap(still);
  *n_out = n;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_finish(bz_sched* s, int64_t id) {
  BZ_API_BEGIN
  if (!s) BZ_FAIL(BZ_E_INVALID, "sched finish: null scheduler");
  auto it = s->admitted.find(id);
  if (it == s->admitted.end()) {
    for (auto w = s->waiting.begin(); w != s->waiting.end(); ++w) if (w->id == id) { s->waiting.erase(w); return BZ_OK; }
    BZ_FAIL(BZ_E_INVALID, "sched finish: request %lld is neither waiting nor admitted", (long long)id);
  }
  for (int b : it->second.blocks) s->block_used[b] = 0;
  s->free_blocks += (int)it->second.blocks.size();
  s->row_req[it->second.row] = -1;
  for (size_t i = 0; i < s->prefilling.size(); i++) if (s->prefilling[i] == id) { s->prefilling.erase(s->prefilling.begin() + i); break; }
  s->admitted.erase(it);
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_info(const bz_sched* s, bz_sched_info_t* out) {
  BZ_API_BEGIN
  if (!s || !out) BZ_FAIL(BZ_E_INVALID, "sched info: null argument");
  int live = 0, owned = 0;
  for (const auto& kv : s->admitted) { live += kv.second.live; owned += (int)kv.second.blocks.size(); }
  *out = bz_sched_info_t{s->n_rows, s->num_blocks, s->n_rows, s->free_blocks, owned, (int)s->waiting.size(), (int)s->admitted.size(), live};
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_row(const bz_sched* s, int row, int64_t* id_out, int32_t* blocks_out, int max_blocks, int* n_blocks_out) {
  BZ_API_BEGIN
  if (!s || !id_out || row < 0 || row >= s->n_rows) BZ_FAIL(BZ_E_INVALID, "sched row: bad argument (row %d)", row);
  *id_out = s->row_req[row];
  if (n_blocks_out) *n_blocks_out = 0;
  if (*id_out < 0) return BZ_OK;
  const SchedReq& a = s->admitted.at(*id_out);
  if (n_blocks_out) *n_blocks_out = (int)a.blocks.size();
  if (blocks_out) {
    if ((int)a.blocks.size() > max_blocks) BZ_FAIL(BZ_E_INVALID, "sched row: room for %d blocks, the row holds %zu", max_blocks, a.blocks.size());
    for (size_t i = 0; i < a.blocks.size(); i++) blocks_out[i] = a.blocks[i];
  }
  return BZ_OK;
  BZ_API_END
}
