// bz_sched.hip -- the request scheduler of the continuous-batching engine (engine/request_scheduler.rs:105-205; the chunked prompt of
// engine/batch_engine.rs:172-272; the prefix cache of engine/executor_cache.rs:39-131).  Plain C++: no HIP call, no clock, no randomness -- a pure function of
// the calls it receives, so that tests/engine_ref.py and tests/prefix_ref.py can restate it and predict every decision.  The policy is in include/blazr_hip.h.
#include <algorithm>
#include <cstdint>
#include <deque>
#include <vector>
#include <map>

#include "bz_internal.h"

namespace {
struct SchedReq {
  int64_t id; int n_prompt, max_tokens, row, done; bool live; std::vector<int> blocks;
  // prefix cache: the prompt (empty: never matches or publishes), the index entry behind blocks[i] (-1: private), the chain position of the next block to publish
  std::vector<int64_t> tokens; std::vector<int64_t> entry; int pub_next = 0; int64_t pub_parent = -1; bool pub_open = true;
};
// one cached block: the key is (parent entry, the block's tokens), compared token by token
struct PrefixEntry { int64_t parent; int block, refs; long long last_use; long long pin; std::vector<int64_t> tokens; };
enum { BLK_FREE = 0, BLK_PRIVATE = 1, BLK_CACHED = 2 };
struct Match { std::vector<int64_t> chain; int64_t src = -1; int j = 0; };
}
struct bz_sched {
  int n_rows = 0, num_blocks = 0, block_size = 0, max_seq_len = 0, chunk = 0, usable = 0;
  int64_t next_id = 0;
  std::deque<SchedReq> waiting;
  std::map<int64_t, SchedReq> admitted;      // by id
  std::vector<int64_t> row_req;              // [n_rows] id or -1
  std::vector<char> block_used;              // [usable] BLK_*
  std::vector<int64_t> prefilling;           // admitted and not live yet, in admission order
  int free_blocks = 0;
  // prefix cache
  bool prefix = false; bool submitted = false;
  std::map<int64_t, PrefixEntry> entries;                 // by entry id; a child's id is above its parent's
  std::map<int64_t, std::vector<int64_t>> kids;           // parent entry (-1: the root) -> its children, ids ascending
  int64_t next_entry = 0; long long tick = 0, epoch = 0;
  long long hits = 0, misses = 0, cached_tokens = 0, evictions = 0;
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

extern "C" int bz_sched_enable_prefix(bz_sched* s) {
  BZ_API_BEGIN
  if (!s) BZ_FAIL(BZ_E_INVALID, "sched enable_prefix: null scheduler");
  if (s->submitted) BZ_FAIL(BZ_E_INVALID, "sched enable_prefix: called after a submit (%lld requests so far); the switch is set before the first one", (long long)s->next_id);
  s->prefix = true;
  return BZ_OK;
  BZ_API_END
}

static int sched_submit(bz_sched* s, const int64_t* prompt, int n_prompt, int max_tokens, int64_t* id_out) {
  if (!s || !id_out) BZ_FAIL(BZ_E_INVALID, "sched submit: null argument");
  if (n_prompt < 1 || max_tokens < 1) BZ_FAIL(BZ_E_INVALID, "sched submit: n_prompt = %d and max_tokens = %d must both be at least 1", n_prompt, max_tokens);
  if ((long long)n_prompt + max_tokens > s->max_seq_len)
    BZ_FAIL(BZ_E_INVALID, "sched submit: n_prompt + max_tokens = %lld exceeds max_seq_len = %d", (long long)n_prompt + max_tokens, s->max_seq_len);
  const int need = blocks_for(s, n_prompt, max_tokens);
  if (need > s->usable)
    BZ_FAIL(BZ_E_INVALID, "sched submit: the request needs %d blocks of %d and could never fit the pool's %d (%d minus %d park blocks)", need, s->block_size, s->usable,
            s->num_blocks, s->n_rows);
  SchedReq r{s->next_id++, n_prompt, max_tokens, -1, 0, false, {}};
  if (s->prefix && prompt) r.tokens.assign(prompt, prompt + n_prompt);
  s->waiting.push_back(r);
  s->submitted = true;
  *id_out = r.id;
  return BZ_OK;
}

extern "C" int bz_sched_submit(bz_sched* s, int n_prompt, int max_tokens, int64_t* id_out) {
  BZ_API_BEGIN
  return sched_submit(s, nullptr, n_prompt, max_tokens, id_out);
  BZ_API_END
}

extern "C" int bz_sched_submit_tokens(bz_sched* s, const int64_t* prompt, int n_prompt, int max_tokens, int64_t* id_out) {
  BZ_API_BEGIN
  if (!prompt) BZ_FAIL(BZ_E_INVALID, "sched submit_tokens: null prompt");
  return sched_submit(s, prompt, n_prompt, max_tokens, id_out);
  BZ_API_END
}

// ---- the prefix index ------------------------------------------------------------------------------------
// the child of `parent` whose tokens equal t[0 .. bs): the tokens themselves decide, never a hash
static int64_t prefix_child(const bz_sched* s, int64_t parent, const int64_t* t) {
  auto k = s->kids.find(parent);
  if (k == s->kids.end()) return -1;
  for (int64_t c : k->second) if (std::equal(t, t + s->block_size, s->entries.at(c).tokens.begin())) return c;
  return -1;
}

static Match prefix_match(const bz_sched* s, const SchedReq& h) {
  Match mt;
  if (!s->prefix || h.tokens.empty()) return mt;
  const int bs = s->block_size, total = h.n_prompt - 1, F = total / bs;
  int64_t parent = -1;
  while ((int)mt.chain.size() < F) {
    const int64_t c = prefix_child(s, parent, h.tokens.data() + mt.chain.size() * (size_t)bs);
    if (c < 0) break;
    mt.chain.push_back(c); parent = c;
  }
  // copy-on-write: the child with the longest common token prefix with what is left of prompt[:-1]; the lowest entry id wins a tie
  const int at = (int)mt.chain.size() * bs, left = std::min(total - at, bs);
  auto k = s->kids.find(parent);
  if (left > 0 && k != s->kids.end())
    for (int64_t c : k->second) {
      const std::vector<int64_t>& t = s->entries.at(c).tokens;
      int j = 0;
      while (j < left && t[j] == h.tokens[at + j]) j++;
      if (j > mt.j) { mt.j = j; mt.src = c; }
    }
  return mt;
}

// the cached blocks that repeated leaf eviction could free now: unreferenced, not pinned by this step, nothing referenced or pinned below them
static int prefix_evictable(const bz_sched* s, const Match* hold) {
  std::map<int64_t, char> blocked;
  if (hold) { for (int64_t c : hold->chain) blocked[c] = 1; if (hold->src >= 0) blocked[hold->src] = 1; }
  int n = 0;
  for (auto it = s->entries.rbegin(); it != s->entries.rend(); ++it) {
    const PrefixEntry& e = it->second;
    bool b = e.refs > 0 || e.pin == s->epoch || blocked.count(it->first);
    if (b) { if (e.parent >= 0) blocked[e.parent] = 1; }
    else n++;
  }
  return n;
}

static void prefix_drop(bz_sched* s, int64_t id) {
  const PrefixEntry& e = s->entries.at(id);
  std::vector<int64_t>& sib = s->kids[e.parent];
  sib.erase(std::find(sib.begin(), sib.end(), id));
  if (sib.empty()) s->kids.erase(e.parent);
  s->block_used[e.block] = BLK_FREE; s->free_blocks++;
  s->entries.erase(id);
}

// the least recently used unreferenced leaf (ties: the lowest block) leaves the index; false when there is none
static bool prefix_evict_one(bz_sched* s, bool honour_pins) {
  int64_t best = -1;
  for (const auto& kv : s->entries) {
    const PrefixEntry& e = kv.second;
    if (e.refs > 0 || (honour_pins && e.pin == s->epoch) || s->kids.count(kv.first)) continue;
    if (best < 0) { best = kv.first; continue; }
    const PrefixEntry& b = s->entries.at(best);
    if (e.last_use < b.last_use || (e.last_use == b.last_use && e.block < b.block)) best = kv.first;
  }
  if (best < 0) return false;
  prefix_drop(s, best);
  return true;
}

// the request's own full prompt blocks that the prompt chunks have completed enter the index
static void prefix_publish(bz_sched* s, SchedReq& a) {
  if (!s->prefix || a.tokens.empty()) return;
  const int bs = s->block_size, F = (a.n_prompt - 1) / bs;
  while (a.pub_open && a.pub_next < F && (a.pub_next + 1) * bs <= a.done) {
    const int k = a.pub_next++;
    if (a.pub_parent >= 0 && !s->entries.count(a.pub_parent)) { a.pub_open = false; break; }      // the chain's last entry was evicted: nothing to hang on to
    const int64_t* t = a.tokens.data() + (size_t)k * bs;
    const int64_t same = prefix_child(s, a.pub_parent, t);
    if (same >= 0) { a.pub_parent = same; continue; }                                            // an equal entry exists: the block stays a private duplicate
    const int64_t id = s->next_entry++;
    s->entries[id] = PrefixEntry{a.pub_parent, a.blocks[k], 1, ++s->tick, -1, std::vector<int64_t>(t, t + bs)};
    s->kids[a.pub_parent].push_back(id);
    s->block_used[a.blocks[k]] = BLK_CACHED;
    a.entry[k] = id;
    a.pub_parent = id;
  }
}

extern "C" int bz_sched_step(bz_sched* s, bz_sched_action* out, int max_out, int* n_out) {
  BZ_API_BEGIN
  if (!s || !out || !n_out) BZ_FAIL(BZ_E_INVALID, "sched step: null argument");
  const int per_row = s->prefix ? 4 : 3;
  if (max_out < per_row * s->n_rows) BZ_FAIL(BZ_E_INVALID, "sched step: room for %d actions, a step can take %d", max_out, per_row * s->n_rows);
  int n = 0;
  s->epoch++;                                  // copy sources named in this step stay until it is over
  // admissions: the head of the queue only (no skipping ahead)
  while (!s->waiting.empty()) {
    SchedReq& h = s->waiting.front();
    const int need = blocks_for(s, h.n_prompt, h.max_tokens);
    int row = -1;
    for (int r = 0; r < s->n_rows; r++) if (s->row_req[r] < 0) { row = r; break; }
    if (row < 0) break;
    const Match mt = prefix_match(s, h);
    const int m = (int)mt.chain.size();
    if (need - m > s->free_blocks + (s->prefix ? prefix_evictable(s, &mt) : 0)) break;
    SchedReq a = h;
    s->waiting.pop_front();
    a.row = row;
    for (int64_t c : mt.chain) { PrefixEntry& e = s->entries.at(c); e.refs++; e.last_use = ++s->tick; a.blocks.push_back(e.block); a.entry.push_back(c); }
    if (mt.src >= 0) { PrefixEntry& e = s->entries.at(mt.src); e.pin = s->epoch; e.last_use = ++s->tick; }
    int b0 = 0;                                // the lowest free block is at or above b0
    while ((int)a.blocks.size() < need) {
      if (s->free_blocks == 0) {               // eviction only when the free blocks have run out
        if (!prefix_evict_one(s, true)) BZ_FAIL(BZ_E_INVALID, "sched step: no block to evict (the accounting is broken)");
        s->evictions++; b0 = 0;
      }
      for (; b0 < s->usable; b0++) if (s->block_used[b0] == BLK_FREE) { s->block_used[b0] = BLK_PRIVATE; a.blocks.push_back(b0); a.entry.push_back(-1); break; }
      s->free_blocks--;
    }
    a.done = m * s->block_size + mt.j;
    a.pub_next = m; a.pub_parent = m ? mt.chain.back() : -1;
    if (s->prefix && !a.tokens.empty()) { if (a.done > 0) { s->hits++; s->cached_tokens += a.done; } else s->misses++; }
    s->row_req[row] = a.id;
    s->prefilling.push_back(a.id);
    out[n++] = bz_sched_action{BZ_SCHED_ADMIT, row, a.id, need, m};
    if (mt.src >= 0) out[n++] = bz_sched_action{BZ_SCHED_COPY, row, a.id, s->entries.at(mt.src).block, mt.j};
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
      prefix_publish(s, a);
    }
    if (a.done == total) { a.live = true; out[n++] = bz_sched_action{BZ_SCHED_LIVE, a.row, a.id, 0, 0}; }
    else still.push_back(id);
  }
  s->prefilling.swap(still);
  s->epoch++;
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
  const SchedReq& a = it->second;
  for (size_t i = 0; i < a.blocks.size(); i++) {
    if (i < a.entry.size() && a.entry[i] >= 0) s->entries.at(a.entry[i]).refs--;        // a cached block survives its users
    else { s->block_used[a.blocks[i]] = BLK_FREE; s->free_blocks++; }
  }
  s->row_req[a.row] = -1;
  for (size_t i = 0; i < s->prefilling.size(); i++) if (s->prefilling[i] == id) { s->prefilling.erase(s->prefilling.begin() + i); break; }
  s->admitted.erase(it);
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_info(const bz_sched* s, bz_sched_info_t* out) {
  BZ_API_BEGIN
  if (!s || !out) BZ_FAIL(BZ_E_INVALID, "sched info: null argument");
  int live = 0, owned = 0;
  for (const auto& kv : s->admitted) {
    live += kv.second.live;
    for (size_t i = 0; i < kv.second.blocks.size(); i++) owned += !(i < kv.second.entry.size() && kv.second.entry[i] >= 0);
  }
  *out = bz_sched_info_t{s->n_rows, s->num_blocks, s->n_rows, s->free_blocks, owned, (int)s->waiting.size(), (int)s->admitted.size(), live};
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_prefix_info(const bz_sched* s, bz_sched_prefix_info_t* out) {
  BZ_API_BEGIN
  if (!s || !out) BZ_FAIL(BZ_E_INVALID, "sched prefix_info: null argument");
  int referenced = 0;
  for (const auto& kv : s->entries) referenced += kv.second.refs > 0;
  *out = bz_sched_prefix_info_t{s->prefix ? 1 : 0, (int)s->entries.size(), prefix_evictable(s, nullptr), referenced, s->hits, s->misses, s->cached_tokens, s->evictions};
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_sched_prefix_flush(bz_sched* s, int* dropped_out) {
  BZ_API_BEGIN
  if (!s) BZ_FAIL(BZ_E_INVALID, "sched prefix_flush: null scheduler");
  int n = 0;
  while (prefix_evict_one(s, false)) n++;
  if (dropped_out) *dropped_out = n;
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
