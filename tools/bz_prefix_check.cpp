// bz-prefix-check -- a stand-alone driver of the scheduler's prefix cache (blazr_amd/csrc/bz_sched.hip) for a sanitised CPU build: `make -C blazr_amd/csrc sched-check`
// compiles the scheduler's host code and this file with -fsanitize=address,undefined and runs it after bz-sched-check.  Prompts cut from a few shared stems at
// lengths around block_size multiples, small pools, random finishes, cancels and flushes: the index is churned through matching, publishing, eviction and flush.
// After every step: free + private + cached == usable, no private block in two tables, a copy's source and destination are blocks of the pool; at the end a
// flush leaves the whole pool free.  No GPU.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../include/blazr_hip.h"

static char last_error[512];
void bz_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(last_error, sizeof last_error, fmt, ap); va_end(ap); }

static unsigned long long rng_state = 2463534242ull * 977;
static unsigned rnd(unsigned n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state % n); }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "bz-prefix-check: %s failed (line %d, scenario %d; last error: %s)\n", #c, __LINE__, scenario, last_error); return 1; } } while (0)

int main() {
  long long hits = 0, evictions = 0, copies = 0, flushed = 0;
  for (int scenario = 0; scenario < 400; scenario++) {
    const int n_rows = 2 + (int)rnd(5), bs = rnd(2) ? 8 : 4, nreq = 4 + (int)rnd(14), chunks[4] = {0, 3, bs, 2 * bs + 1};
    std::vector<std::vector<int64_t>> stems(3);
    for (auto& st : stems) for (int i = 0; i < 6 * bs + 3; i++) st.push_back(rnd(5));                    // few token values: partial matches are common
    std::vector<std::vector<int64_t>> prompts(nreq);
    std::vector<int> mt(nreq);
    int need_max = 0, need_sum = 0;
    const int off[6] = {-1, 0, 1, 2, bs - 1, bs / 2};
    for (int i = 0; i < nreq; i++) {
      const std::vector<int64_t>& st = stems[rnd(3)];
      int len = (int)rnd(6) * bs + off[rnd(6)];
      len = len < 1 ? 1 : len > (int)st.size() ? (int)st.size() : len;
      prompts[i].assign(st.begin(), st.begin() + len);
      if (rnd(5) < 2) for (int k = 1 + (int)rnd(bs + 1); k > 0; k--) prompts[i].push_back(50 + rnd(10));
      mt[i] = 1 + (int)rnd(2 * bs - 1);
      const int n = ((int)prompts[i].size() + mt[i] + bs - 1) / bs;
      need_max = n > need_max ? n : need_max; need_sum += n;
    }
    const int pool = rnd(3) == 0 ? need_max : rnd(2) ? need_max + (int)rnd(10) : need_sum;
    bz_sched* s = nullptr;
    CHECK(bz_sched_create(n_rows, pool + n_rows, bs, 12 * bs, chunks[rnd(4)], &s) == BZ_OK);
    CHECK(bz_sched_enable_prefix(s) == BZ_OK);
    std::vector<bz_sched_action> acts(4 * (size_t)n_rows);
    int n = 0;
    CHECK(bz_sched_step(s, acts.data(), 3 * n_rows, &n) == BZ_E_INVALID);                                // 4 * n_rows with the switch on
    std::vector<int64_t> live, running;
    int submitted = 0, finished = 0, steps = 0;
    while (finished < nreq) {
      while (submitted < nreq && (rnd(3) == 0 || steps > 14)) {
        int64_t id = -1;
        if (rnd(10)) CHECK(bz_sched_submit_tokens(s, prompts[submitted].data(), (int)prompts[submitted].size(), mt[submitted], &id) == BZ_OK);
        else CHECK(bz_sched_submit(s, (int)prompts[submitted].size(), mt[submitted], &id) == BZ_OK);
        CHECK(id == submitted);
        submitted++;
      }
      if (rnd(20) == 0) { int d = -1; CHECK(bz_sched_prefix_flush(s, &d) == BZ_OK && d >= 0); flushed += d; }
      std::vector<int64_t>& from = rnd(5) ? live : running;                                              // a finish, or a cancel of a request still in its prompt
      if (!from.empty() && (rnd(5) < 2 || (submitted == nreq && !live.empty()))) {
        const int64_t id = from[rnd((unsigned)from.size())];
        CHECK(bz_sched_finish(s, id) == BZ_OK);
        for (auto* v : {&live, &running}) for (size_t k = 0; k < v->size(); k++) if ((*v)[k] == id) { v->erase(v->begin() + (long)k); break; }
        finished++;
      }
      CHECK(bz_sched_step(s, acts.data(), (int)acts.size(), &n) == BZ_OK && n <= (int)acts.size());
      for (int i = 0; i < n; i++) {
        if (acts[i].kind == BZ_SCHED_ADMIT) { running.push_back(acts[i].id); CHECK(acts[i].b >= 0 && acts[i].b <= acts[i].a); }
        if (acts[i].kind == BZ_SCHED_LIVE) live.push_back(acts[i].id);
        if (acts[i].kind == BZ_SCHED_COPY) { copies++; CHECK(acts[i].a >= 0 && acts[i].a < pool && acts[i].b >= 1 && acts[i].b < bs); }
      }
      std::map<int, int> held;
      for (int r = 0; r < n_rows; r++) {
        int64_t id = -1; int nb = 0; std::vector<int32_t> blocks(64);
        CHECK(bz_sched_row(s, r, &id, blocks.data(), 64, &nb) == BZ_OK);
        for (int b = 0; id >= 0 && b < nb; b++) { CHECK(blocks[b] >= 0 && blocks[b] < pool); held[blocks[b]]++; }
      }
      bz_sched_info_t info; bz_sched_prefix_info_t pi;
      CHECK(bz_sched_info(s, &info) == BZ_OK && bz_sched_prefix_info(s, &pi) == BZ_OK);
      CHECK(info.free_blocks + info.owned_blocks + pi.cached_blocks == pool);
      CHECK(pi.evictable_blocks + pi.referenced_blocks <= pi.cached_blocks && (int)held.size() <= info.owned_blocks + pi.referenced_blocks);
      int shared = 0;
      for (const auto& h : held) shared += h.second > 1;
      CHECK(shared <= pi.referenced_blocks);
      CHECK(++steps < 100000);
    }
    bz_sched_prefix_info_t pi; bz_sched_info_t info; int d = -1;
    CHECK(bz_sched_prefix_info(s, &pi) == BZ_OK);
    hits += pi.hits; evictions += pi.evictions;
    CHECK(pi.evictable_blocks == pi.cached_blocks && pi.referenced_blocks == 0);
    CHECK(bz_sched_prefix_flush(s, &d) == BZ_OK && d == pi.cached_blocks);
    CHECK(bz_sched_info(s, &info) == BZ_OK && info.free_blocks == pool && info.owned_blocks == 0);
    int64_t none = -1;
    CHECK(bz_sched_submit_tokens(s, nullptr, 3, 3, &none) == BZ_E_INVALID);
    bz_sched_free(s);
  }
  const int scenario = -1;
  CHECK(hits > 0 && evictions > 0 && copies > 0 && flushed > 0);                                        // the workload reached the cache
  printf("bz-prefix-check: ok (400 scenarios, %lld hits, %lld copies, %lld evictions, %lld flushed)\n", hits, copies, evictions, flushed);
  return 0;
}
