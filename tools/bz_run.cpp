// bz-run -- the smallest C++ caller of libblazr_hip.so: what blazr's `run` command does around the hot path
// (/root/reference/src/cli/run.rs:60-160 GPU branch: open device -> detect + load the model -> warm up -> Executor::generate), with token ids
// in and out instead of a tokenizer (the tokenizers are out of scope).  It exists to show the C ABI driven from compiled code
// with no Python in the process; tests/test_gpu_loader.py runs it against a checkpoint on disk.
//
//   bz-run <model dir | .safetensors | .gguf> --prompt 1,2,3 [--max-tokens N] [--temperature T] [--top-k K] [--top-p P] [--min-p P]
//          [--repeat-penalty R] [--seed S] [--graphs] [--paged-attention] [--device D] [--stats]
//          [--grammar FILE --vocab-bytes FILE [--grammar-regular]]
//          [--draft <checkpoint> [--spec-tokens k] [--spec-adaptive]]
//          [--lora <PEFT dir | adapter_model.safetensors>]... [--lora-targets q,v,...]
//   bz-run <model> --prompt 1,2,3 --score [--top-logprobs K]
//   bz-run <model> --prompt 1,2,3 --embed mean|cls|last|none [--normalize]
//   bz-run <model> --prompts-file FILE --score [--top-logprobs K]  |  --embed mean|cls|last|none [--normalize]
//   bz-run <model> --requests FILE --rows N [--pool-blocks B] [--prefill-chunk C] [--depth D] [--prefix-cache] [sampling options, --eos]
// --requests: continuous batching (BatchEngine::run, engine/batch_engine.rs:91-169; RequestScheduler::submit, engine/request_scheduler.rs:105-205) over N rows.  The file
// has one request per line, `max_tokens;comma-separated prompt ids`; all are submitted, the engine is stepped until idle, and one line of ids per request is
// printed in submission order; the engine's statistics go to stderr.  --pool-blocks: the paged pool (default: every row can hold a full-length request);
// the sampling options apply to every request (request i draws with seed + i), --eos is its stop id.  --prefix-cache: requests share the cached full blocks of
// earlier prompts (a request admitted in the same step as its donor does not); hits, cached tokens and evictions go to stderr.
// --lora (repeatable): PEFT adapters (Executor::load_lora, executor.rs:397-420; GenerationConfig.lora_adapter, config/generation.rs:142-145) in slots 0, 1, ... of a
// table over --lora-targets (names out of q,k,v,o,gate,up,down; default: the union of what the given adapters hold).  Single-sequence modes generate under the
// first adapter; with --requests, request i uses adapter i mod (n + 1) with 0 = none, so one file exercises a mixed batch.  Not with --draft.
// --draft: speculative decoding (inference.speculative, config/inference.rs:197-208; generate_text.rs:61-136) with that checkpoint as the draft model: greedy only,
// the same ids as without it; iterations / accepted / rejected go to stderr (generate_text.rs:130-135).
// --grammar: a GBNF file (gen_config.grammar, executor_generate.rs:96-121), compiled with the reference's semantics or, with --grammar-regular, as the regular subset of
// GBNF; with --graphs (Llama family, no penalty) the captured step carries the DFA state on the device.  --vocab-bytes: the bytes of every token, which blazr takes from its tokenizer (executor_generate.rs:104-113): u32 V, u32 offsets[V+1], then the bytes.
// --score: one prompt pass, the log-likelihood of every prompt token given its predecessors (bz_score_kv / bz_score_ssm; echo + logprobs, perplexity): one line per
// position from the second on -- `position token logprob rank`, then with --top-logprobs K the K likeliest ids as id:logprob -- then `total <sum> tokens <n> perplexity <p>`.
// --embed: the prompt's contextual embedding (bz_embed_kv / bz_embed_ssm; /v1/embeddings: engine/executor_embed.rs:33-55, server/pooling.rs:4-47), pooled as named
// and L2-normalised with --normalize: the vector on one line, comma separated (`none`: one line per position).
// --prompts-file FILE (one comma-separated id list per line) with --score or --embed: all the inputs in ONE packed call (bz_score_batch / bz_embed_batch; the
// per-text loops of server/embeddings.rs:180 and server/rerank.rs:144); per input what the single-prompt form prints, preceded by `# input i`.
// prints the generated ids, comma separated, on stdout.
#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/blazr_hip.h"

static bool read_file(const std::string& path, std::string& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[65536]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
  fclose(f);
  return true;
}

static int fail(const char* what) { fprintf(stderr, "bz-run: %s: %s\n", what, bz_last_error()); return 1; }

// the LoRA table of `m` and one slot per path; targets: "" = the union of the modules the adapters hold (read from bz_lora_describe's pair keys)
static const char* const kLoraNames[7] = {"q", "k", "v", "o", "gate", "up", "down"};
static int setup_lora(bz_device* dev, bz_model* m, const std::vector<std::string>& paths, const std::string& targets, std::vector<bz_lora*>& out) {
  if (paths.empty()) return 0;
  uint32_t mask = 0;
  if (!targets.empty()) {
    size_t at = 0;
    while (at <= targets.size()) {
      size_t c = targets.find(',', at);
      if (c == std::string::npos) c = targets.size();
      const std::string t = targets.substr(at, c - at);
      bool ok = t.empty();
      for (int i = 0; i < 7; i++) if (t == kLoraNames[i] || t == std::string(kLoraNames[i]) + "_proj") { mask |= 1u << i; ok = true; }
      if (!ok) { fprintf(stderr, "bz-run: --lora-targets: unknown target '%s' (q,k,v,o,gate,up,down)\n", t.c_str()); return 2; }
      at = c + 1;
    }
  } else {
    for (const std::string& p : paths) {
      size_t need = 0;
      if (bz_lora_describe(p.c_str(), nullptr, 0, &need) != BZ_OK) return fail("lora");
      std::string js(need, '\0');
      if (bz_lora_describe(p.c_str(), &js[0], need, nullptr) != BZ_OK) return fail("lora");
      for (int i = 0; i < 7; i++) if (js.find(std::string(".") + kLoraNames[i] + "_proj\"") != std::string::npos) mask |= 1u << i;
    }
  }
  bz_lora_table_config tc;
  memset(&tc, 0, sizeof tc);
  tc.n_slots = (int)paths.size(); tc.max_rank = 128; tc.targets = mask;
  if (bz_lora_table_create(m, &tc) != BZ_OK) return fail("lora table");
  for (size_t i = 0; i < paths.size(); i++) {
    bz_lora* a = nullptr;
    if (bz_lora_load(dev, paths[i].c_str(), &a) != BZ_OK) return fail("lora load");
    if (bz_lora_attach(m, (int)i, a) != BZ_OK) return fail("lora attach");
    out.push_back(a);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: bz-run <model path> --prompt id,id,... [--max-tokens N] [--graphs] [--paged-attention] ...\n"
                            "       bz-run <model path> --requests FILE --rows N [--logprobs K] [--logit-bias id:val,...] ...\n"); return 2; }
  std::string model = argv[1];
  std::vector<int64_t> prompt;
  bz_gen_config gc;
  memset(&gc, 0, sizeof gc);
  gc.max_tokens = 32; gc.temperature = 0.0f; gc.repeat_penalty = 1.0f; gc.repeat_last_n = 64; gc.top_p = 1.0f; gc.eos_id = -1; gc.block_size = 16;
  gc.dry_base = 2; gc.dynatemp_exponent = 1.0f;
  int device_id = 0; bool stats_on = false;
  std::string grammar_path, vocab_path; bool grammar_regular = false;
  std::string draft_path; bz_spec_config sc;
  std::string requests_path; int rows = 0, pool_blocks = 0, prefill_chunk = 0, depth = 2; bool prefix_cache = false;
  std::vector<std::string> lora_paths; std::string lora_targets; std::vector<bz_lora*> loras;
  bool score = false; int top_logprobs = 0; std::string embed; bool normalize = false; std::string prompts_path;
  int logprobs = -1; std::vector<uint32_t> bias_ids; std::vector<float> bias_vals;   // --requests: every request asks for K alternatives / carries this bias
  memset(&sc, 0, sizeof sc);
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&](const char* name) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "bz-run: %s needs a value\n", name); exit(2); } return argv[++i]; };
    if (a == "--prompt") { const char* s = next("--prompt"); char* end; while (*s) { prompt.push_back(strtoll(s, &end, 10)); if (end == s) break; s = *end == ',' ? end + 1 : end; } }
    else if (a == "--max-tokens") gc.max_tokens = atoi(next("--max-tokens"));
    else if (a == "--temperature") gc.temperature = (float)atof(next("--temperature"));
    else if (a == "--top-k") gc.top_k = atoi(next("--top-k"));
    else if (a == "--top-p") gc.top_p = (float)atof(next("--top-p"));
    else if (a == "--min-p") gc.min_p = (float)atof(next("--min-p"));
    else if (a == "--repeat-penalty") gc.repeat_penalty = (float)atof(next("--repeat-penalty"));
    else if (a == "--seed") gc.seed = strtoull(next("--seed"), nullptr, 10);
    else if (a == "--eos") gc.eos_id = strtoll(next("--eos"), nullptr, 10);
    else if (a == "--graphs") gc.use_graph = 1;                    // cli/run.rs:144-157
    else if (a == "--paged-attention") gc.paged = 1;
    else if (a == "--device") device_id = atoi(next("--device"));
    else if (a == "--stats") stats_on = true;
    else if (a == "--grammar") grammar_path = next("--grammar");
    else if (a == "--vocab-bytes") vocab_path = next("--vocab-bytes");
    else if (a == "--grammar-regular") grammar_regular = true;
    else if (a == "--draft") draft_path = next("--draft");
    else if (a == "--spec-tokens") sc.num_speculative_tokens = atoi(next("--spec-tokens"));
    else if (a == "--spec-adaptive") sc.adaptive_depth = 1;
    else if (a == "--requests") requests_path = next("--requests");
    else if (a == "--rows") rows = atoi(next("--rows"));
    else if (a == "--pool-blocks") pool_blocks = atoi(next("--pool-blocks"));
    else if (a == "--prefill-chunk") prefill_chunk = atoi(next("--prefill-chunk"));
    else if (a == "--depth") depth = atoi(next("--depth"));
    else if (a == "--prefix-cache") prefix_cache = true;
    else if (a == "--logprobs") logprobs = atoi(next("--logprobs"));
    else if (a == "--score") score = true;
    else if (a == "--top-logprobs") top_logprobs = atoi(next("--top-logprobs"));
    else if (a == "--embed") embed = next("--embed");
    else if (a == "--normalize") normalize = true;
    else if (a == "--prompts-file") prompts_path = next("--prompts-file");
    else if (a == "--logit-bias") {
      const char* q = next("--logit-bias"); char* end;
      while (*q) {
        const unsigned long id = strtoul(q, &end, 10);
        if (end == q || *end != ':') { fprintf(stderr, "bz-run: --logit-bias takes id:val,id:val,...\n"); return 2; }
        q = end + 1;
        const float v = strtof(q, &end);
        if (end == q) { fprintf(stderr, "bz-run: --logit-bias takes id:val,id:val,...\n"); return 2; }
        bias_ids.push_back((uint32_t)id); bias_vals.push_back(v);
        q = *end == ',' ? end + 1 : end;
      }
    }
    else if (a == "--lora") lora_paths.push_back(next("--lora"));
    else if (a == "--lora-targets") lora_targets = next("--lora-targets");
    else { fprintf(stderr, "bz-run: unknown option %s\n", a.c_str()); return 2; }
  }
  if (lora_paths.size() > 64) { fprintf(stderr, "bz-run: at most 64 --lora adapters\n"); return 2; }
  if (!lora_paths.empty() && !draft_path.empty()) { fprintf(stderr, "bz-run: --lora and --draft do not go together\n"); return 2; }
  if (!requests_path.empty()) {
    if (rows < 2) { fprintf(stderr, "bz-run: --requests needs --rows N (2..512)\n"); return 2; }
    if (!draft_path.empty() || !grammar_path.empty() || !prompt.empty()) { fprintf(stderr, "bz-run: --requests goes without --prompt, --draft and --grammar\n"); return 2; }
    std::string text;
    if (!read_file(requests_path, text)) { fprintf(stderr, "bz-run: cannot read %s\n", requests_path.c_str()); return 2; }
    struct Req { int max_tokens; std::vector<int64_t> prompt; std::vector<int64_t> out; };
    std::vector<Req> reqs;
    size_t at = 0; int longest = 0;
    while (at < text.size()) {
      size_t nl = text.find('\n', at);
      if (nl == std::string::npos) nl = text.size();
      const std::string line = text.substr(at, nl - at);
      at = nl + 1;
      if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
      const size_t semi = line.find(';');
      if (semi == std::string::npos) { fprintf(stderr, "bz-run: %s: line %zu is not `max_tokens;id,id,...`\n", requests_path.c_str(), reqs.size() + 1); return 2; }
      Req r; r.max_tokens = atoi(line.c_str());
      const char* q = line.c_str() + semi + 1; char* end;
      while (*q) { const long long v = strtoll(q, &end, 10); if (end == q) break; r.prompt.push_back(v); q = *end == ',' ? end + 1 : end; }
      if (r.max_tokens < 1 || r.prompt.empty()) { fprintf(stderr, "bz-run: %s: request %zu needs max_tokens >= 1 and a prompt\n", requests_path.c_str(), reqs.size() + 1); return 2; }
      longest = std::max(longest, (int)r.prompt.size() + r.max_tokens);
      reqs.push_back(r);
    }
    if (reqs.empty()) { fprintf(stderr, "bz-run: %s holds no request\n", requests_path.c_str()); return 2; }
    bz_device* dev = nullptr;
    if (bz_device_open(device_id, &dev) != BZ_OK) return fail("device");
    bz_model* m = nullptr; bz_model_config cfg;
    if (bz_load_model(dev, model.c_str(), &m, &cfg) != BZ_OK) return fail("load");
    bz_engine_config ec;
    memset(&ec, 0, sizeof ec);
    ec.n_rows = rows; ec.block_size = gc.block_size; ec.max_seq_len = std::min(longest, cfg.max_seq_len); ec.prefill_chunk = prefill_chunk; ec.depth = depth;
    const int per = (ec.max_seq_len + ec.block_size - 1) / ec.block_size;
    ec.num_blocks = pool_blocks > 0 ? pool_blocks : rows * per + rows;       // one park block per row on top
    const bool greedy = gc.temperature == 0.0f && gc.repeat_penalty == 1.0f && gc.frequency_penalty == 0.0f && gc.presence_penalty == 0.0f;
    const bool extras = logprobs >= 0 || !bias_ids.empty();                  // bias and logprobs live in the batched sampler
    ec.use_sampler = greedy && !extras ? 0 : 1;
    ec.logprobs = extras ? 1 : 0;
    ec.prefix_cache = prefix_cache ? 1 : 0;
    if (int rc = setup_lora(dev, m, lora_paths, lora_targets, loras)) return rc;     // before the engine captures its step
    bz_engine* e = nullptr;
    if (bz_engine_create(m, &ec, nullptr, &e) != BZ_OK) return fail("engine");
    for (size_t i = 0; i < reqs.size(); i++) {
      bz_request rq;
      memset(&rq, 0, sizeof rq);
      rq.max_tokens = reqs[i].max_tokens; rq.grammar_state = BZ_GRAMMAR_ROW_FREE;
      rq.lora_slot = (int32_t)(i % (loras.size() + 1));                        // 0 = none, k = adapter k - 1
      if (gc.eos_id >= 0) { rq.n_stop = 1; rq.stop_ids[0] = gc.eos_id; }
      rq.sampling.temperature = gc.temperature; rq.sampling.top_k = gc.top_k; rq.sampling.top_p = gc.top_p; rq.sampling.min_p = gc.min_p;
      rq.sampling.repeat_penalty = gc.repeat_penalty; rq.sampling.frequency_penalty = gc.frequency_penalty; rq.sampling.presence_penalty = gc.presence_penalty;
      rq.sampling.repeat_last_n = gc.repeat_last_n; rq.sampling.seed = gc.seed + i;
      int64_t id = -1;
      bz_request_extras ex;
      memset(&ex, 0, sizeof ex);
      ex.logprobs = logprobs >= 0; ex.top_logprobs = logprobs >= 0 ? logprobs : 0;
      ex.n_logit_bias = (int32_t)bias_ids.size(); ex.logit_bias_ids = bias_ids.data(); ex.logit_bias_vals = bias_vals.data();
      if (bz_engine_submit_ex(e, reqs[i].prompt.data(), (int)reqs[i].prompt.size(), &rq, extras ? &ex : nullptr, &id) != BZ_OK) return fail("submit");
      if (id != (int64_t)i) { fprintf(stderr, "bz-run: request %zu got id %lld\n", i, (long long)id); return 1; }
    }
    int busy = 1;
    bz_engine_event ev[256];
    while (busy) {
      if (bz_engine_step(e, &busy) != BZ_OK) return fail("step");
      int n = 0;
      do {
        if (bz_engine_poll(e, ev, 256, &n) != BZ_OK) return fail("poll");
        for (int k = 0; k < n; k++) if (ev[k].token >= 0) reqs[(size_t)ev[k].id].out.push_back(ev[k].token);
      } while (n == 256);
      if (logprobs >= 0) {
        static bz_engine_logprobs lp[64];
        do {
          if (bz_engine_poll_logprobs(e, lp, 64, &n) != BZ_OK) return fail("poll logprobs");
          for (int k = 0; k < n; k++) {
            fprintf(stderr, "logprobs: request %lld token %d = %lld %.6f", (long long)lp[k].id, lp[k].index, (long long)lp[k].token, (double)lp[k].logprob);
            for (int j = 0; j < lp[k].n_top; j++) fprintf(stderr, "%s%u:%.6f", j ? "," : " top ", lp[k].top_ids[j], (double)lp[k].top_logprobs[j]);
            fprintf(stderr, "\n");
          }
        } while (n == 64);
      }
    }
    for (const Req& r : reqs) {
      for (size_t k = 0; k < r.out.size(); k++) printf(k ? ",%lld" : "%lld", (long long)r.out[k]);
      printf("\n");
    }
    bz_engine_stats_t es;
    if (bz_engine_stats(e, &es) != BZ_OK) return fail("stats");
    fprintf(stderr, "engine: %lld replays, %d / %d blocks free (%d park), %d live rows, %d waiting, %lld prompt tokens, %lld generated tokens, %.2f ms host time in admissions\n",
            (long long)es.replays, es.free_blocks, es.total_blocks, es.park_blocks, es.live_rows, es.waiting, (long long)es.prompt_tokens, (long long)es.generated_tokens,
            es.admit_host_ms);
    if (prefix_cache) {
      bz_engine_prefix_stats_t ps;
      if (bz_engine_prefix_stats(e, &ps) != BZ_OK) return fail("prefix stats");
      fprintf(stderr, "prefix cache: %lld hits, %lld misses, %lld cached tokens, %lld evictions, %d blocks cached, %lld prompt tokens skipped, %lld blocks copied in %lld launches\n",
              (long long)ps.hits, (long long)ps.misses, (long long)ps.cached_tokens, (long long)ps.evictions, ps.cached_blocks, (long long)ps.prompt_tokens_skipped,
              (long long)ps.copied_blocks, (long long)ps.copy_launches);
    }
    bz_engine_free(e);
    bz_model_free(m);
    for (bz_lora* a : loras) bz_lora_free(a);
    bz_device_close(dev);
    return 0;
  }
  if (!prompts_path.empty() && !score && embed.empty()) { fprintf(stderr, "bz-run: --prompts-file goes with --score or --embed\n"); return 2; }
  if (prompt.empty() && prompts_path.empty()) { fprintf(stderr, "bz-run: --prompt id,id,... is required\n"); return 2; }
  if (!draft_path.empty() && !grammar_path.empty()) { fprintf(stderr, "bz-run: --draft and --grammar do not go together\n"); return 2; }
  if (grammar_path.empty() != vocab_path.empty()) { fprintf(stderr, "bz-run: --grammar and --vocab-bytes go together\n"); return 2; }
  bz_grammar* grammar = nullptr;
  std::vector<uint8_t> vbytes; std::vector<int64_t> voff;
  if (!grammar_path.empty()) {
    std::string text;
    if (!read_file(grammar_path, text)) { fprintf(stderr, "bz-run: cannot read %s\n", grammar_path.c_str()); return 2; }
    if (text.find('\0') != std::string::npos) { fprintf(stderr, "bz-run: %s holds a NUL byte\n", grammar_path.c_str()); return 2; }
    if (bz_grammar_compile(text.c_str(), grammar_regular ? BZ_GRAMMAR_REGULAR : 0u, &grammar) != BZ_OK) return fail("grammar");
    std::string raw;
    if (!read_file(vocab_path, raw) || raw.size() < 8) { fprintf(stderr, "bz-run: cannot read %s\n", vocab_path.c_str()); return 2; }
    uint32_t V = 0;
    memcpy(&V, raw.data(), 4);
    const size_t head = 4 + ((size_t)V + 1) * 4;
    if (V == 0 || raw.size() < head) { fprintf(stderr, "bz-run: %s is shorter than its offset table\n", vocab_path.c_str()); return 2; }
    voff.resize((size_t)V + 1);
    for (size_t i = 0; i <= V; i++) { uint32_t o; memcpy(&o, raw.data() + 4 + 4 * i, 4); voff[i] = o; }
    if ((size_t)voff[V] != raw.size() - head) { fprintf(stderr, "bz-run: %s: the last offset does not match the number of bytes\n", vocab_path.c_str()); return 2; }
    vbytes.assign(raw.begin() + head, raw.end());
  }
  bz_device* dev = nullptr;
  if (bz_device_open(device_id, &dev) != BZ_OK) return fail("device");                    // CudaDevice::new + CudaClient::new (run.rs:70-81)
  bz_model* m = nullptr; bz_model_config cfg;
  if (bz_load_model(dev, model.c_str(), &m, &cfg) != BZ_OK) return fail("load");          // detect_model_source + load_model (run.rs:88-118)
  if (int rc = setup_lora(dev, m, lora_paths, lora_targets, loras)) return rc;
  if (!loras.empty() && bz_model_set_lora(m, 0) != BZ_OK) return fail("set lora");          // single-sequence modes: the first adapter
  if (score || !embed.empty()) {
    if (score && !embed.empty()) { fprintf(stderr, "bz-run: --score and --embed do not go together\n"); return 2; }
    static const char* const kPool[4] = {"none", "mean", "cls", "last"};      // BZ_POOL_*
    bz_embed_config ecfg;
    memset(&ecfg, 0, sizeof ecfg);
    ecfg.pooling = -1; ecfg.normalize = normalize ? 1 : 0;
    for (int i = 0; i < 4; i++) if (embed == kPool[i]) ecfg.pooling = i;
    if (!score && ecfg.pooling < 0) { fprintf(stderr, "bz-run: --embed takes mean, cls, last or none\n"); return 2; }
    if (bz_model_get_config(m, &cfg) != BZ_OK) return fail("config");            // the cache's shape as the library keeps it (MLA: one latent 'head')
    auto print_score = [&](const bz_score_row* rows, int S, const bz_score_total& tot) {
      for (int i = 0; i + 1 < S; i++) {
        printf("%d %lld %.6f %d", i + 1, (long long)rows[i].target, (double)rows[i].logprob, rows[i].rank);
        for (int j = 0; j < rows[i].n_top; j++) printf(" %u:%.6f", rows[i].top_ids[j], (double)rows[i].top_logprobs[j]);
        printf("\n");
      }
      printf("total %.6f tokens %lld perplexity %.6f\n", tot.sum_logprob, (long long)tot.n_scored, tot.n_scored ? exp(-tot.sum_logprob / (double)tot.n_scored) : 0.0);
    };
    auto print_vecs = [&](const float* v, int nvec) {
      for (int r = 0; r < nvec; r++) {
        for (int j = 0; j < cfg.hidden; j++) printf(j ? ",%.9g" : "%.9g", (double)v[(size_t)r * cfg.hidden + j]);
        printf("\n");
      }
    };
    if (!prompts_path.empty()) {      // many inputs, one packed call
      std::string text;
      if (!read_file(prompts_path, text)) { fprintf(stderr, "bz-run: cannot read %s\n", prompts_path.c_str()); return 2; }
      std::vector<int64_t> flat; std::vector<int32_t> lens;
      {
        std::string line;
        size_t at = 0;
        while (at <= text.size()) {
          const size_t nl = text.find('\n', at);
          line = text.substr(at, nl == std::string::npos ? std::string::npos : nl - at);
          at = nl == std::string::npos ? text.size() + 1 : nl + 1;
          const char* q = line.c_str(); char* end; int n = 0;
          while (*q) { const long long id = strtoll(q, &end, 10); if (end == q) break; flat.push_back(id); n++; q = *end == ',' ? end + 1 : end; }
          if (n) lens.push_back(n);
        }
      }
      if (lens.empty()) { fprintf(stderr, "bz-run: %s holds no input\n", prompts_path.c_str()); return 2; }
      if (cfg.arch == BZ_ARCH_MAMBA2) { fprintf(stderr, "bz-run: --prompts-file takes models with a KV cache\n"); return 2; }
      const int T = (int)flat.size(), n_seq = (int)lens.size();
      const int64_t shp[1] = {T};
      bz_tensor* tok = nullptr; bz_kv* kv = nullptr;
      if (bz_tensor_from_host(dev, BZ_I64, shp, 1, flat.data(), &tok) != BZ_OK) return fail("tokens");
      if (bz_kv_create(dev, cfg.n_layers, 1, cfg.n_kv_heads, T, T > cfg.max_seq_len ? T : cfg.max_seq_len, cfg.head_dim, cfg.act_dtype, &kv) != BZ_OK) return fail("cache");
      if (score) {
        std::vector<bz_score_row> rows((size_t)T); std::vector<bz_score_total> tots((size_t)n_seq);
        bz_score_config scfg;
        memset(&scfg, 0, sizeof scfg);
        scfg.top_n = top_logprobs;
        if (bz_score_batch(m, tok, lens.data(), n_seq, kv, nullptr, &scfg, rows.data(), tots.data()) != BZ_OK) return fail("score");
        for (int i = 0, o = 0; i < n_seq; o += lens[i], i++) { printf("# input %d\n", i); print_score(rows.data() + o, lens[i], tots[i]); }
      } else {
        const bool none = ecfg.pooling == BZ_POOL_NONE;
        const int64_t oshp[2] = {none ? T : n_seq, cfg.hidden};
        bz_tensor* out = nullptr;
        if (bz_tensor_zeros(dev, BZ_F32, oshp, 2, &out) != BZ_OK) return fail("out");
        if (bz_embed_batch(m, tok, lens.data(), n_seq, kv, &ecfg, out) != BZ_OK) return fail("embed");
        std::vector<float> v((size_t)oshp[0] * cfg.hidden);
        if (bz_tensor_to_host(out, v.data(), v.size() * 4) != BZ_OK) return fail("read");
        for (int i = 0, o = 0; i < n_seq; o += lens[i], i++) { printf("# input %d\n", i); print_vecs(v.data() + (size_t)(none ? o : i) * cfg.hidden, none ? lens[i] : 1); }
        bz_tensor_free(out);
      }
      bz_tensor_free(tok); bz_kv_free(kv); bz_model_free(m);
      for (bz_lora* a : loras) bz_lora_free(a);
      bz_device_close(dev);
      return 0;
    }
    const int S = (int)prompt.size();
    const int64_t shp[1] = {S};
    bz_tensor* tok = nullptr;
    if (bz_tensor_from_host(dev, BZ_I64, shp, 1, prompt.data(), &tok) != BZ_OK) return fail("tokens");
    bz_kv* kv = nullptr; bz_ssm_state* ssm = nullptr;
    const bool is_ssm = cfg.arch == BZ_ARCH_MAMBA2;
    if (is_ssm ? bz_ssm_state_create(m, 1, cfg.act_dtype, &ssm) != BZ_OK
               : bz_kv_create(dev, cfg.n_layers, 1, cfg.n_kv_heads, S, cfg.max_seq_len, cfg.head_dim, cfg.act_dtype, &kv) != BZ_OK) return fail("cache");
    if (score) {
      std::vector<int64_t> targets(prompt.begin() + 1, prompt.end());
      targets.push_back(-1);
      std::vector<bz_score_row> rows((size_t)S);
      bz_score_config scfg; bz_score_total tot;
      memset(&scfg, 0, sizeof scfg);
      scfg.top_n = top_logprobs;
      if ((is_ssm ? bz_score_ssm(m, tok, S, ssm, targets.data(), &scfg, rows.data(), &tot) : bz_score_kv(m, tok, S, kv, 0, targets.data(), &scfg, rows.data(), &tot)) != BZ_OK)
        return fail("score");
      print_score(rows.data(), S, tot);
    } else {
      const int nvec = ecfg.pooling == BZ_POOL_NONE ? S : 1;
      const int64_t oshp[2] = {nvec, cfg.hidden};
      bz_tensor* out = nullptr;
      if (bz_tensor_zeros(dev, BZ_F32, oshp, 2, &out) != BZ_OK) return fail("out");
      if ((is_ssm ? bz_embed_ssm(m, tok, S, ssm, &ecfg, out) : bz_embed_kv(m, tok, S, kv, 0, &ecfg, out)) != BZ_OK) return fail("embed");
      std::vector<float> v((size_t)nvec * cfg.hidden);
      if (bz_tensor_to_host(out, v.data(), v.size() * 4) != BZ_OK) return fail("read");
      print_vecs(v.data(), nvec);
      bz_tensor_free(out);
    }
    bz_tensor_free(tok);
    if (kv) bz_kv_free(kv);
    if (ssm) bz_ssm_state_free(ssm);
    bz_model_free(m);
    for (bz_lora* a : loras) bz_lora_free(a);
    bz_device_close(dev);
    return 0;
  }
  std::vector<int64_t> out((size_t)(gc.max_tokens > 0 ? gc.max_tokens : 1));
  bz_gen_stats st;
  if (!draft_path.empty()) {
    bz_model* dm = nullptr; bz_model_config dcfg; bz_speculative* sp = nullptr; bz_spec_stats ss;
    if (bz_load_model(dev, draft_path.c_str(), &dm, &dcfg) != BZ_OK) return fail("load draft");
    if (bz_speculative_create(m, dm, &sc, &sp) != BZ_OK) return fail("speculative");
    if (bz_generate_speculative(sp, prompt.data(), (int)prompt.size(), &gc, out.data(), &st, &ss) != BZ_OK) return fail("generate");
    fprintf(stderr, "speculative: iterations %lld, accepted %lld, rejected %lld, verify path %d, final depth %d\n", (long long)ss.iterations, (long long)ss.accepted_tokens,
            (long long)ss.rejected_tokens, ss.verify_path, ss.final_depth);
    bz_speculative_free(sp);
    bz_model_free(dm);
  } else
  if (bz_generate_grammar(m, prompt.data(), (int)prompt.size(), &gc, grammar, vbytes.data(), grammar ? voff.data() : nullptr, (int64_t)voff.size() - (grammar ? 1 : 0), out.data(), &st) != BZ_OK)
    return fail("generate");
  for (int i = 0; i < st.n_generated; i++) printf(i ? ",%lld" : "%lld", (long long)out[i]);
  printf("\n");
  if (stats_on)   // cli/bench.rs:299-306 decode tok/s = (tokens - 1) / (total - TTFT)
    fprintf(stderr, "prefill %.2f ms, decode %.2f ms, %d tokens, %.1f tok/s decode, finish=%s\n", st.prefill_ms, st.decode_ms, st.n_generated,
            st.n_generated > 1 ? (st.n_generated - 1) / (st.decode_ms / 1e3) : 0.0, st.finish_reason ? "eos" : "length");
  bz_grammar_free(grammar);
  bz_model_free(m);
  for (bz_lora* a : loras) bz_lora_free(a);
  bz_device_close(dev);
  return 0;
}
