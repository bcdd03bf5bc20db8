"""A Python restatement of the scheduler with the prefix cache on (include/blazr_hip.h, "The prefix cache"): shared blocks with reference counts, an index
keyed by (parent entry, the block's tokens), copy-on-write of a partly shared block, deterministic LRU eviction of unreferenced leaves.  It predicts every
action and every table of bz_sched_* from the calls alone.  engine_ref.RefSched restates the switch-off policy and stays as it is."""

ADMIT, PREFILL, LIVE, COPY = 0, 1, 2, 3


class RefPrefixSched:
    def __init__(self, n_rows, num_blocks, block_size, max_seq_len, chunk=0):
        self.n_rows, self.num_blocks, self.bs, self.max_seq_len, self.chunk = n_rows, num_blocks, block_size, max_seq_len, chunk
        self.usable = num_blocks - n_rows
        self.free = set(range(self.usable))
        self.rows = [-1] * n_rows
        self.waiting, self.admitted, self.prefilling = [], {}, []
        self.next_id = 0
        # the index: entry id -> dict(parent, block, refs, use, tokens); ids count up, so a child's id is above its parent's
        self.entries = {}
        self.next_entry = 0
        self.tick = 0
        self.sources = set()                      # the copy sources this step has named
        self.hits = self.misses = self.cached_tokens = self.evictions = 0
        self.evicted_log = []                     # (block, entry) in eviction order, flush included

    def need(self, n_prompt, max_tokens):
        return -(-(n_prompt + max_tokens) // self.bs)

    def submit(self, prompt, max_tokens, n_prompt=None):
        """prompt None (with n_prompt): a request without tokens, which never matches or publishes"""
        n_prompt = len(prompt) if prompt is not None else n_prompt
        assert n_prompt >= 1 and max_tokens >= 1 and n_prompt + max_tokens <= self.max_seq_len and self.need(n_prompt, max_tokens) <= self.usable
        rid = self.next_id
        self.next_id += 1
        self.waiting.append(dict(id=rid, n_prompt=n_prompt, max_tokens=max_tokens, row=-1, done=0, live=False, blocks=[], entry=[],
                                 tokens=None if prompt is None else [int(t) for t in prompt], pub_next=0, pub_parent=-1, pub_open=True))
        return rid

    # ---- the index ----
    def children(self, parent):
        return [e for e in sorted(self.entries) if self.entries[e]["parent"] == parent]

    def child(self, parent, toks):
        for e in self.children(parent):
            if self.entries[e]["tokens"] == toks:         # the tokens themselves
                return e
        return -1

    def match(self, r):
        if r["tokens"] is None:
            return [], -1, 0
        bs, total = self.bs, r["n_prompt"] - 1
        chain, parent = [], -1
        while len(chain) < total // bs:
            c = self.child(parent, r["tokens"][len(chain) * bs:(len(chain) + 1) * bs])
            if c < 0:
                break
            chain.append(c)
            parent = c
        rest = r["tokens"][len(chain) * bs:total][:bs]
        src, best = -1, 0
        for e in self.children(parent):
            j = 0
            while j < len(rest) and self.entries[e]["tokens"][j] == rest[j]:
                j += 1
            if j > best:
                src, best = e, j
        return chain, src, best

    def evictable(self, hold=()):
        blocked, n = set(hold), 0
        for e in sorted(self.entries, reverse=True):
            ent = self.entries[e]
            if ent["refs"] > 0 or e in self.sources or e in blocked:
                blocked.add(ent["parent"])
            else:
                n += 1
        return n

    def evict_one(self, honour_sources=True):
        parents = {ent["parent"] for ent in self.entries.values()}
        cand = [(ent["use"], ent["block"], e) for e, ent in self.entries.items()
                if ent["refs"] == 0 and e not in parents and not (honour_sources and e in self.sources)]
        if not cand:
            return False
        _, block, e = min(cand)
        del self.entries[e]
        self.free.add(block)
        self.evicted_log.append((block, e))
        return True

    def touch(self, e):
        self.tick += 1
        self.entries[e]["use"] = self.tick

    def publish(self, r):
        if r["tokens"] is None:
            return
        bs, F = self.bs, (r["n_prompt"] - 1) // self.bs
        while r["pub_open"] and r["pub_next"] < F and (r["pub_next"] + 1) * bs <= r["done"]:
            k = r["pub_next"]
            r["pub_next"] += 1
            if r["pub_parent"] >= 0 and r["pub_parent"] not in self.entries:
                r["pub_open"] = False
                break
            toks = r["tokens"][k * bs:(k + 1) * bs]
            same = self.child(r["pub_parent"], toks)
            if same >= 0:
                r["pub_parent"] = same
                continue
            e = self.next_entry
            self.next_entry += 1
            self.entries[e] = dict(parent=r["pub_parent"], block=r["blocks"][k], refs=1, use=0, tokens=toks)
            self.touch(e)
            r["entry"][k] = e
            r["pub_parent"] = e

    # ---- the calls ----
    def step(self):
        acts = []
        self.sources = set()
        while self.waiting and -1 in self.rows:
            h = self.waiting[0]
            need = self.need(h["n_prompt"], h["max_tokens"])
            chain, src, j = self.match(h)
            m = len(chain)
            if need - m > len(self.free) + self.evictable(chain + ([src] if src >= 0 else [])):
                break
            r = self.waiting.pop(0)
            r["row"] = self.rows.index(-1)
            for e in chain:
                self.entries[e]["refs"] += 1
                self.touch(e)
                r["blocks"].append(self.entries[e]["block"])
                r["entry"].append(e)
            if src >= 0:
                self.sources.add(src)
                self.touch(src)
            while len(r["blocks"]) < need:
                if not self.free:
                    assert self.evict_one()
                    self.evictions += 1
                b = min(self.free)
                self.free.remove(b)
                r["blocks"].append(b)
                r["entry"].append(-1)
            r["done"] = m * self.bs + j
            r["pub_next"], r["pub_parent"] = m, (chain[-1] if m else -1)
            if r["tokens"] is not None:
                if r["done"] > 0:
                    self.hits += 1
                    self.cached_tokens += r["done"]
                else:
                    self.misses += 1
            self.rows[r["row"]] = r["id"]
            self.admitted[r["id"]] = r
            self.prefilling.append(r["id"])
            acts.append((ADMIT, r["row"], r["id"], need, m))
            if src >= 0:
                acts.append((COPY, r["row"], r["id"], self.entries[src]["block"], j))
        budget = self.chunk if self.chunk > 0 else 1 << 40
        still = []
        for rid in self.prefilling:
            r = self.admitted[rid]
            take = min(r["n_prompt"] - 1 - r["done"], budget)
            if take > 0:
                acts.append((PREFILL, r["row"], rid, r["done"], r["done"] + take))
                r["done"] += take
                budget -= take
                self.publish(r)
            if r["done"] == r["n_prompt"] - 1:
                r["live"] = True
                acts.append((LIVE, r["row"], rid, 0, 0))
            else:
                still.append(rid)
        self.prefilling = still
        self.sources_of_last_step, self.sources = self.sources, set()
        return acts

    def finish(self, rid):
        if rid not in self.admitted:
            self.waiting = [w for w in self.waiting if w["id"] != rid]
            return
        r = self.admitted.pop(rid)
        for b, e in zip(r["blocks"], r["entry"]):
            if e >= 0:
                self.entries[e]["refs"] -= 1
            else:
                self.free.add(b)
        self.rows[r["row"]] = -1
        self.prefilling = [p for p in self.prefilling if p != rid]

    def flush(self):
        n = 0
        while self.evict_one(honour_sources=False):
            n += 1
        return n

    def info(self):
        return dict(n_rows=self.n_rows, num_blocks=self.num_blocks, park_blocks=self.n_rows, free_blocks=len(self.free),
                    owned_blocks=sum(e < 0 for r in self.admitted.values() for e in r["entry"]), waiting=len(self.waiting), admitted=len(self.admitted),
                    live=sum(r["live"] for r in self.admitted.values()))

    def prefix_info(self):
        return dict(enabled=1, cached_blocks=len(self.entries), evictable_blocks=self.evictable(), referenced_blocks=sum(e["refs"] > 0 for e in self.entries.values()),
                    hits=self.hits, misses=self.misses, cached_tokens=self.cached_tokens, evictions=self.evictions)

    def row(self, row):
        rid = self.rows[row]
        return rid, (list(self.admitted[rid]["blocks"]) if rid >= 0 else [])
