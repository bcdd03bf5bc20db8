"""The scheduler's prefix cache (bz_sched_enable_prefix, bz_sched_submit_tokens, BZ_SCHED_COPY; plain C++) against its Python restatement
(tests/prefix_ref.py), action by action and table by table, with the accounting invariants after every step.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_ref as R0  # noqa: E402
import prefix_ref as R  # noqa: E402
from blazr_amd import _lib as L, runtime  # noqa: E402


class CheckedRef(R.RefPrefixSched):
    def evict_one(self, honour_sources=True):
        before = len(self.evicted_log)
        ok = super().evict_one(honour_sources)
        if ok:
            block, _ = self.evicted_log[before]
            assert all(block not in r["blocks"] for r in self.admitted.values()), block      # an evicted block is in no live table
        return ok


class Pair:
    """The C scheduler and the restatement side by side, the prefix switch on."""

    def __init__(self, n_rows, num_blocks, bs, max_seq_len, chunk):
        self.c = runtime.Scheduler(n_rows, num_blocks, bs, max_seq_len, chunk)
        self.c.enable_prefix()
        self.r = CheckedRef(n_rows, num_blocks, bs, max_seq_len, chunk)
        self.n_rows, self.num_blocks, self.bs, self.usable = n_rows, num_blocks, bs, num_blocks - n_rows
        self.live, self.admitted, self.finished, self.log = [], [], 0, []

    def submit(self, prompt, max_tokens, tokens=True):
        if tokens:
            a, b = self.c.submit_tokens(prompt, max_tokens), self.r.submit(prompt, max_tokens)
        else:
            a, b = self.c.submit(len(prompt), max_tokens), self.r.submit(None, max_tokens, n_prompt=len(prompt))
        assert a == b
        return a

    def finish(self, rid):
        self.c.finish(rid)
        self.r.finish(rid)
        for lst in (self.live, self.admitted):
            if rid in lst:
                lst.remove(rid)
        self.finished += 1

    def flush(self):
        a, b = self.c.prefix_flush(), self.r.flush()
        assert a == b
        self.check()
        return a

    def check(self):
        assert self.c.info() == self.r.info()
        assert self.c.prefix_info() == self.r.prefix_info()
        tables = {}
        for row in range(self.n_rows):
            got, want = self.c.row(row), self.r.row(row)
            assert got == want, (row, got, want)
            if got[0] >= 0:
                tables[got[0]] = got[1]
        i, p = self.c.info(), self.c.prefix_info()
        # free + private + cached == usable, and no block in two states
        assert i["free_blocks"] + i["owned_blocks"] + p["cached_blocks"] == self.usable
        cached = {e["block"]: e for e in self.r.entries.values()}
        assert len(cached) == len(self.r.entries)                                  # no block behind two entries
        private = [b for rid, tb in tables.items() for b, e in zip(tb, self.r.admitted[rid]["entry"]) if e < 0]
        assert len(private) == len(set(private)) == i["owned_blocks"]
        assert not (set(private) & set(cached)) and not (self.r.free & set(cached)) and not (self.r.free & set(private))
        assert len(self.r.free) == i["free_blocks"] and all(0 <= b < self.usable for tb in tables.values() for b in tb)
        # reference count == the number of admitted requests whose table holds the block
        for b, e in cached.items():
            assert e["refs"] == sum(b in tb for tb in tables.values()), (b, e, tables)
        assert p["referenced_blocks"] == sum(e["refs"] > 0 for e in cached.values())

    def step(self):
        mark = len(self.r.evicted_log)
        got, want = self.c.step(), self.r.step()
        assert got == want, (got, want)
        self.check()
        gone = {b for b, _ in self.r.evicted_log[mark:]}
        for kind, row, rid, a, b in got:
            if kind == R.ADMIT:
                self.admitted.append(rid)
            elif kind == R.LIVE:
                self.live.append(rid)
            elif kind == R.COPY:
                assert a not in gone                                               # a copy source outlives the step that names it
                assert any(e["block"] == a for e in self.r.entries.values())
                assert 1 <= b < self.bs
        self.log.append(got)
        return got


def _stems(rng, bs, vocab=50):
    return [rng.integers(0, vocab, size=6 * bs + 3).tolist() for _ in range(3)]


def _prompt(rng, stems, bs):
    """a stem cut around a block_size multiple +-1, now and then with a private tail"""
    stem = stems[int(rng.integers(0, len(stems)))]
    n = int(rng.integers(0, 6)) * bs + int(rng.choice([-1, 0, 1, 2, bs - 1, bs // 2]))
    n = min(max(n, 1), len(stem))
    p = stem[:n]
    if rng.random() < 0.4:
        p = p + rng.integers(50, 60, size=int(rng.integers(1, bs + 2))).tolist()
    return p


@pytest.mark.parametrize("seed", range(8))
def test_random_workloads_follow_the_restatement(seed):
    rng = np.random.default_rng(4000 + seed)
    copies = hits = evictions = zero = 0
    for _ in range(25):
        n_rows, bs = int(rng.integers(2, 6)), int(rng.choice([4, 8]))
        stems = _stems(rng, bs)
        nreq = int(rng.integers(4, 16))
        reqs = [(_prompt(rng, stems, bs), int(rng.integers(1, 2 * bs))) for _ in range(nreq)]
        need = [-(-(len(p) + t) // bs) for p, t in reqs]
        pool = int(rng.choice([max(need), max(need) + int(rng.integers(0, 10)), sum(need)]))     # pool pressure .. everything fits
        p = Pair(n_rows, pool + n_rows, bs, 8 * bs + 3 + 2 * bs + bs + 2, int(rng.choice([0, 3, bs, 2 * bs + 1])))
        arrive = sorted(int(rng.integers(0, 14)) for _ in range(nreq))
        ids, step = [], 0
        while p.finished < nreq:
            while len(ids) < nreq and arrive[len(ids)] <= step:
                ids.append(p.submit(*reqs[len(ids)], tokens=rng.random() < 0.9))
            if rng.random() < 0.05:
                p.flush()
            pick = p.live if rng.random() < 0.8 else p.admitted + [w["id"] for w in p.r.waiting]          # finishes, and cancels in any state
            if pick and (rng.random() < 0.4 or (len(ids) == nreq and p.live)):
                p.finish(pick[int(rng.integers(0, len(pick)))])
            got = p.step()
            copies += sum(a[0] == R.COPY for a in got)
            for k, _, rid, a, b in got:
                if k == R.LIVE and not any(x[0] == R.PREFILL and x[2] == rid for acts in p.log for x in acts) and len(reqs[ids.index(rid)][0]) > 1:
                    zero += 1
            step += 1
            assert step < 3000
        pi = p.c.prefix_info()
        hits += pi["hits"]; evictions += pi["evictions"]
        p.flush()
        i = p.c.info()
        assert i["free_blocks"] == pool and i["admitted"] == 0 and p.c.prefix_info()["cached_blocks"] == 0
    assert copies > 0 and hits > 0 and evictions > 0 and zero > 0           # the workload reaches what it is for


def test_full_blocks_copy_on_write_and_zero_prefill():
    bs = 16
    p = Pair(4, 20 + 4, bs, 128, 0)
    stem = list(range(100, 160))
    a = p.submit(stem[:53], 4)                                              # F = 52 // 16 = 3 blocks cacheable; need = 4
    assert p.step() == [(R.ADMIT, 0, a, 4, 0), (R.PREFILL, 0, a, 0, 52), (R.LIVE, 0, a, 0, 0)]
    assert p.c.prefix_info()["cached_blocks"] == 3 and p.c.prefix_info()["misses"] == 1
    b = p.submit(stem[:40] + [7] * 13, 4)                                   # shares 40 tokens: m = 2, j = 8 from a's third block (block 2)
    assert p.step() == [(R.ADMIT, 1, b, 4, 2), (R.COPY, 1, b, 2, 8), (R.PREFILL, 1, b, 40, 52), (R.LIVE, 1, b, 0, 0)]
    assert p.c.row(1) == (b, [0, 1, 4, 5])
    assert p.c.prefix_info()["cached_tokens"] == 40 and p.c.prefix_info()["cached_blocks"] == 4        # b published its own third block
    p.finish(a)
    assert p.c.info()["free_blocks"] == 20 - 4 - 1                          # a's private block came back; four blocks are cached, b holds one private block
    c = p.submit(stem[:49], 3)                                              # n_prompt - 1 = 48 = three whole cached blocks: nothing to prefill
    assert p.step() == [(R.ADMIT, 0, c, 4, 3), (R.LIVE, 0, c, 0, 0)]
    assert p.c.row(0) == (c, [0, 1, 2, 3])
    d = p.submit(stem[:48], 3)                                              # n_prompt - 1 = 47: two blocks and j = 15 = block_size - 1
    assert p.step() == [(R.ADMIT, 2, d, 4, 2), (R.COPY, 2, d, 2, 15), (R.LIVE, 2, d, 0, 0)]
    e = p.submit(stem[:17], 3)                                              # F = 1: one block, and position 16 is its own
    assert p.step() == [(R.ADMIT, 3, e, 2, 1), (R.LIVE, 3, e, 0, 0)]
    for rid in (b, c, d, e):
        p.finish(rid)
    p.step()
    assert p.c.prefix_info()["evictable_blocks"] == 4 == p.flush()
    assert p.c.info()["free_blocks"] == 20


def test_a_request_admitted_before_the_donors_chunk_does_not_match():
    p = Pair(3, 12 + 3, 8, 64, 8)
    stem = list(range(30))
    a, b = p.submit(stem[:25], 2), p.submit(stem[:25], 2)
    assert p.step() == [(R.ADMIT, 0, a, 4, 0), (R.ADMIT, 1, b, 4, 0), (R.PREFILL, 0, a, 0, 8)]
    c = p.submit(stem[:25], 2)                                              # a's first block is in the index now
    assert p.step() == [(R.ADMIT, 2, c, 4, 1), (R.PREFILL, 0, a, 8, 16)]
    p.step()
    got = p.step()
    assert (R.PREFILL, 1, b, 0, 8) in got                                   # b prefills everything and keeps private duplicates
    for _ in range(6):
        p.step()
    assert p.c.prefix_info()["cached_blocks"] == 3 and p.c.info()["owned_blocks"] == 1 + 4 + 3


def test_eviction_takes_the_least_recently_used_leaf():
    p = Pair(2, 6 + 2, 4, 32, 0)
    x, y = [1] * 9, [2] * 9                                                 # two cacheable blocks each, three blocks with the new token
    a = p.submit(x, 1); p.step(); p.finish(a)                               # x in blocks 0, 1
    b = p.submit(y, 1); p.step(); p.finish(b)                               # y in blocks 2, 3
    assert p.c.prefix_info()["cached_blocks"] == 4 and p.c.info()["free_blocks"] == 2
    c = p.submit(x, 1)                                                      # touches x's chain; it holds it, too
    assert p.step() == [(R.ADMIT, 0, c, 3, 2), (R.LIVE, 0, c, 0, 0)] and p.c.row(0) == (c, [0, 1, 4])
    big = p.submit([3] * 12, 4)                                             # 4 blocks > 1 free + 2 evictable: waits, and evicts nothing
    assert p.step() == [] and p.c.prefix_info()["evictions"] == 0
    p.finish(big)
    d = p.submit([3] * 8, 4)                                                # 3 blocks: the free one, then y's leaf, then y's first block
    assert p.step() == [(R.ADMIT, 1, d, 3, 0), (R.PREFILL, 1, d, 0, 7), (R.LIVE, 1, d, 0, 0)]
    assert p.c.row(1) == (d, [5, 3, 2]) and p.c.prefix_info()["evictions"] == 2
    assert p.c.prefix_info()["cached_blocks"] == 2 + 1                      # x's two, and d's own first block


def test_switch_off_submit_tokens_is_submit():
    rng = np.random.default_rng(7)
    c = runtime.Scheduler(3, 10 + 3, 8, 64, 5)
    r = R0.RefSched(3, 10 + 3, 8, 64, 5)
    stem = list(range(40))
    live = []
    for step in range(60):
        if step < 20:
            n, t = int(rng.integers(1, 40)), int(rng.integers(1, 20))
            assert c.submit_tokens(stem[:n], t) == r.submit(n, t)
        if live and rng.random() < 0.5:
            rid = live.pop(0)
            c.finish(rid); r.finish(rid)
        got = c.step()
        assert got == r.step() and all(a[0] != R.COPY for a in got)
        live += [a[2] for a in got if a[0] == R.LIVE]
        assert c.info() == r.info() and all(c.row(i) == r.row(i) for i in range(3))
    assert c.prefix_info() == dict(enabled=0, cached_blocks=0, evictable_blocks=0, referenced_blocks=0, hits=0, misses=0, cached_tokens=0, evictions=0)


def test_refusals():
    s = runtime.Scheduler(2, 6, 8, 64)
    s.submit(3, 3)
    with pytest.raises(L.BlazrHipError) as e:
        s.enable_prefix()
    assert e.value.code == L.E_INVALID and "after a submit" in str(e.value)
    s = runtime.Scheduler(2, 6, 8, 64)
    s.enable_prefix()
    acts = (L.SchedAction * 6)()
    n = C.c_int()
    assert L.lib().bz_sched_step(s.h, acts, 6, C.byref(n)) == L.E_INVALID   # 4 * n_rows with the switch on
    assert "8" in L.lib().bz_last_error().decode()
