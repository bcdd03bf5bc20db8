// bz-sched-check -- a stand-alone driver of the request scheduler (blazr_amd/csrc/bz_sched.hip) for a sanitised CPU build: `make -C blazr_amd/csrc sched-check`
// compiles the scheduler's host code and this file with -fsanitize=address,undefined and runs it.  Random request streams with random finishes; after every
// step: no block owned twice, no request in two rows, free + owned + park == num_blocks; at the end everything was admitted in submission order.  No GPU.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../include/blazr_hip.h"

static char last_error[512];
void bz_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(last_error, sizeof last_error, fmt, ap); va_end(ap); }

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state % n); }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "bz-sched-check: %s failed (line %d, scenario %d; last error: %s)\n", #c, __LINE__, scenario, last_error); return 1; } } while (0)

int main() {
  for (int scenario = 0; scenario < 400; scenario++) {
    const int n_rows = 2 + (int)rnd(7), bs = rnd(2) ? 16 : 8, nreq = 3 + (int)rnd(12), chunks[3] = {0, 7, 32};
    std::vector<int> np(nreq), mt(nreq);
    int need_max = 0, need_sum = 0;
    for (int i = 0; i < nreq; i++) { np[i] = 1 + (int)rnd(200); mt[i] = 1 + (int)rnd(60); const int n = (np[i] + mt[i] + bs - 1) / bs; need_max = n > need_max ? n : need_max; need_sum += n; }
    const int pool = rnd(3) == 0 ? need_max : rnd(2) ? need_max + (int)rnd(20) : need_sum;
    bz_sched* s = nullptr;
    CHECK(bz_sched_create(n_rows, pool + n_rows, bs, 261, chunks[rnd(3)], &s) == BZ_OK);
    std::vector<bz_sched_action> acts(3 * (size_t)n_rows);
    std::vector<int64_t> live, admitted;
    int submitted = 0, finished = 0, steps = 0;
    while (finished < nreq) {
      while (submitted < nreq && (rnd(3) == 0 || steps > 12)) { int64_t id = -1; CHECK(bz_sched_submit(s, np[submitted], mt[submitted], &id) == BZ_OK && id == submitted); submitted++; }
      if (!live.empty() && (rnd(5) < 2 || submitted == nreq)) { const size_t k = rnd((unsigned)live.size()); CHECK(bz_sched_finish(s, live[k]) == BZ_OK); live.erase(live.begin() + (long)k); finished++; }
      int n = 0;
      CHECK(bz_sched_step(s, acts.data(), (int)acts.size(), &n) == BZ_OK);
      for (int i = 0; i < n; i++) { if (acts[i].kind == BZ_SCHED_ADMIT) admitted.push_back(acts[i].id); if (acts[i].kind == BZ_SCHED_LIVE) live.push_back(acts[i].id); }
      std::set<int> owned; std::set<int64_t> seen;
      for (int r = 0; r < n_rows; r++) {
        int64_t id = -1; int nb = 0; std::vector<int32_t> blocks(64);
        CHECK(bz_sched_row(s, r, &id, blocks.data(), 64, &nb) == BZ_OK);
        if (id < 0) continue;
        CHECK(seen.insert(id).second);
        for (int b = 0; b < nb; b++) CHECK(blocks[b] >= 0 && blocks[b] < pool && owned.insert(blocks[b]).second);
      }
      bz_sched_info_t info;
      CHECK(bz_sched_info(s, &info) == BZ_OK);
      CHECK(info.free_blocks + info.owned_blocks + info.park_blocks == pool + n_rows && info.owned_blocks == (int)owned.size());
      CHECK(++steps < 100000);
    }
    CHECK((int)admitted.size() == nreq);
    for (int i = 0; i < nreq; i++) CHECK(admitted[i] == i);
    int64_t none = -1;
    CHECK(bz_sched_submit(s, 200, 62, &none) == BZ_E_INVALID && bz_sched_finish(s, 9999) == BZ_E_INVALID);
    bz_sched_free(s);
  }
  printf("bz-sched-check: 400 scenarios ok\n");
  return 0;
}
