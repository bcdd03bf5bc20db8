"""The engine's host scheduler (bz_sched_*, plain C++) against its Python restatement (tests/engine_ref.py), decision by decision.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_ref as R  # noqa: E402
from blazr_amd import _lib as L, runtime  # noqa: E402


class Pair:
    """The C scheduler and the restatement side by side: every call goes to both, every answer is compared, the invariants are checked after every step."""

    def __init__(self, n_rows, num_blocks, bs, max_seq_len, chunk):
        self.c = runtime.Scheduler(n_rows, num_blocks, bs, max_seq_len, chunk)
        self.r = R.RefSched(n_rows, num_blocks, bs, max_seq_len, chunk)
        self.n_rows, self.num_blocks, self.bs = n_rows, num_blocks, bs
        self.live, self.admitted_ever, self.prompts, self.finished = [], [], {}, 0
        self.log = []

    def submit(self, n_prompt, max_tokens):
        a, b = self.c.submit(n_prompt, max_tokens), self.r.submit(n_prompt, max_tokens)
        assert a == b
        self.prompts[a] = (n_prompt, max_tokens)
        return a

    def finish(self, rid):
        self.c.finish(rid)
        self.r.finish(rid)
        if rid in self.live:
            self.live.remove(rid)
        self.finished += 1

    def step(self):
        got, want = self.c.step(), self.r.step()
        assert got == want, (got, want)
        assert self.c.info() == self.r.info()
        owner, seen_req = {}, set()
        for row in range(self.n_rows):
            (rid, blocks), (rid2, blocks2) = self.c.row(row), self.r.row(row)
            assert rid == rid2 and blocks == blocks2
            if rid < 0:
                continue
            assert rid not in seen_req                                    # no request in two rows (so no row holds two)
            seen_req.add(rid)
            n_prompt, max_tokens = self.prompts[rid]
            assert len(blocks) == -(-(n_prompt + max_tokens) // self.bs)
            for b in blocks:
                assert 0 <= b < self.num_blocks - self.n_rows and b not in owner, (b, owner)   # no block owned twice, none of them a park block
                owner[b] = rid
        i = self.c.info()
        assert i["free_blocks"] + i["owned_blocks"] + i["park_blocks"] == self.num_blocks and i["owned_blocks"] == len(owner)
        for kind, row, rid, a, b in got:
            if kind == R.ADMIT:
                self.admitted_ever.append(rid)
            if kind == R.LIVE:
                self.live.append(rid)
        self.log.append(got)
        return got


def _prefill_ranges(log, rid):
    return [(a, b) for acts in log for k, _, i, a, b in acts if k == R.PREFILL and i == rid]


@pytest.mark.parametrize("seed", range(8))
def test_random_scenarios_follow_the_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    for _ in range(40):                                                   # 8 x 40 scenarios
        n_rows, bs = int(rng.integers(2, 9)), int(rng.choice([8, 16]))
        nreq = int(rng.integers(3, 14))
        reqs = [(int(rng.integers(1, 201)), int(rng.integers(1, 61))) for _ in range(nreq)]
        need = [-(-(p + t) // bs) for p, t in reqs]
        pool = int(rng.choice([max(need), max(need) + int(rng.integers(0, 20)), sum(need)]))   # one at a time .. everything fits
        p = Pair(n_rows, pool + n_rows, bs, 261, int(rng.choice([0, 7, 32])))
        arrive = sorted(int(rng.integers(0, 12)) for _ in range(nreq))
        ids, step = [], 0
        while p.finished < nreq:
            while len(ids) < nreq and arrive[len(ids)] <= step:
                ids.append(p.submit(*reqs[len(ids)]))
            if p.live and (rng.random() < 0.4 or len(ids) == nreq):       # finishes arrive at random steps (always, once everything is submitted)
                p.finish(p.live[int(rng.integers(0, len(p.live)))])
            p.step()
            step += 1
            assert step < 4000
        assert p.admitted_ever == ids                                     # FIFO: admitted in submission order, everything eventually
        for rid, (n_prompt, _) in zip(ids, reqs):
            rg = _prefill_ranges(p.log, rid)
            assert [a for a, _ in rg] == [0] + [b for _, b in rg[:-1]] if rg else n_prompt == 1
            assert (rg[-1][1] if rg else 0) == n_prompt - 1
        i = p.c.info()
        assert i["free_blocks"] == pool and i["waiting"] == 0 and i["admitted"] == 0


def test_a_request_that_exactly_fills_the_pool():
    p = Pair(2, 5 + 2, 16, 128, 0)
    a = p.submit(40, 40)                                                  # 80 positions = 5 blocks = the whole pool
    b = p.submit(1, 1)
    assert p.step() == [(R.ADMIT, 0, a, 5, 0), (R.PREFILL, 0, a, 0, 39), (R.LIVE, 0, a, 0, 0)]
    assert p.c.info()["free_blocks"] == 0 and p.c.row(0) == (a, [0, 1, 2, 3, 4])
    assert p.step() == []                                                 # b has a free row but no block
    p.finish(a)
    assert p.step() == [(R.ADMIT, 0, b, 1, 0), (R.LIVE, 0, b, 0, 0)]
    with pytest.raises(L.BlazrHipError) as e:
        p.c.submit(41, 40)                                                # 6 blocks: could never fit
    assert e.value.code == L.E_INVALID and "6 blocks" in str(e.value)
    with pytest.raises(L.BlazrHipError) as e:
        p.c.submit(100, 29)
    assert e.value.code == L.E_INVALID and "129" in str(e.value) and "max_seq_len" in str(e.value)


def test_head_of_line_blocking():
    p = Pair(4, 6 + 4, 16, 128, 0)
    a = p.submit(30, 30)                                                  # 4 blocks
    big = p.submit(50, 14)                                                # 4 blocks: waits for a
    small = p.submit(3, 2)                                                # 1 block, would fit -- and waits behind `big`
    assert [x[:3] for x in p.step() if x[0] == R.ADMIT] == [(R.ADMIT, 0, a)]
    assert p.step() == [] and p.c.info()["waiting"] == 2 and p.c.info()["free_blocks"] == 2
    p.finish(a)
    got = p.step()
    assert [x[:3] for x in got if x[0] == R.ADMIT] == [(R.ADMIT, 0, big), (R.ADMIT, 1, small)]
    assert p.c.row(0) == (big, [0, 1, 2, 3]) and p.c.row(1) == (small, [4])


def test_one_token_prompt_and_one_token_output():
    p = Pair(2, 4 + 2, 16, 64, 7)
    a = p.submit(1, 1)
    b = p.submit(1, 20)
    assert p.step() == [(R.ADMIT, 0, a, 1, 0), (R.ADMIT, 1, b, 2, 0), (R.LIVE, 0, a, 0, 0), (R.LIVE, 1, b, 0, 0)]   # nothing to prefill: live at once
    c = p.submit(9, 1)                                                    # prompt[:-1] = 8 tokens over a budget of 7
    p.finish(a)
    assert p.step() == [(R.ADMIT, 0, c, 1, 0), (R.PREFILL, 0, c, 0, 7)]
    assert p.step() == [(R.PREFILL, 0, c, 7, 8), (R.LIVE, 0, c, 0, 0)]


def test_chunk_boundary_on_the_last_prompt_token():
    p = Pair(3, 12 + 3, 16, 128, 32)
    a = p.submit(33, 5)                                                   # prompt[:-1] = 32 tokens = exactly one chunk: live in the admission step
    b = p.submit(65, 5)                                                   # 64 = two whole chunks; a has used this step's budget
    c = p.submit(34, 5)                                                   # 33 = a chunk and one token
    assert p.step() == [(R.ADMIT, 0, a, 3, 0), (R.ADMIT, 1, b, 5, 0), (R.ADMIT, 2, c, 3, 0), (R.PREFILL, 0, a, 0, 32), (R.LIVE, 0, a, 0, 0)]
    assert p.step() == [(R.PREFILL, 1, b, 0, 32)]
    assert p.step() == [(R.PREFILL, 1, b, 32, 64), (R.LIVE, 1, b, 0, 0)]
    assert p.step() == [(R.PREFILL, 2, c, 0, 32)]
    assert p.step() == [(R.PREFILL, 2, c, 32, 33), (R.LIVE, 2, c, 0, 0)]
    assert p.step() == []


def test_chunk_budget_is_shared_in_admission_order():
    p = Pair(3, 12 + 3, 16, 128, 32)
    a, b = p.submit(11, 5), p.submit(41, 5)
    assert p.step() == [(R.ADMIT, 0, a, 1, 0), (R.ADMIT, 1, b, 3, 0), (R.PREFILL, 0, a, 0, 10), (R.LIVE, 0, a, 0, 0), (R.PREFILL, 1, b, 0, 22)]
    assert p.step() == [(R.PREFILL, 1, b, 22, 40), (R.LIVE, 1, b, 0, 0)]


def test_finish_rule():
    live = np.array([True, True, True, False, True])
    left = np.array([5, 1, 1, 3, 9])
    toks = np.array([7, 7, 8, 7, 3])
    stop = np.zeros((5, 8), dtype=np.int64)
    stop[:, 0], stop[:, 1] = 7, 3
    n_stop = np.array([1, 0, 1, 1, 1])                                    # row 4: its second id is not counted
    left2, ended, reason = R.finish_rule(live, left, toks, stop, n_stop)
    assert left2.tolist() == [4, 0, 0, 3, 8]
    assert ended.tolist() == [True, True, True, False, False]
    assert reason[:3].tolist() == [1, 0, 0]                               # stop before length; row 1 has no stop ids


def test_simulated_engine_counts_replays():
    # one request of 3 tokens alone: live at replay 0, replays 0..2 produce its tokens; the host learns of the end `depth` steps late
    for depth, want in ((1, 3), (4, 6)):
        sim = R.simulate_engine(2, 6, 16, 64, 0, depth, [(0, 5, 3, 3)])
        assert sim["first_replay"] == {0: 0} and sim["replays"] == want, (depth, sim)
    # the second request waits for the first one's row: its first replay follows the harvest of the first one's end
    sim = R.simulate_engine(2, 2 + 2, 16, 32, 0, 1, [(0, 5, 20, 2), (0, 5, 20, 2)])
    assert sim["admitted"] == [0, 1] and sim["first_replay"][1] > sim["first_replay"][0] + 1
