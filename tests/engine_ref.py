"""A Python restatement of the request engine's host policy (include/blazr_hip.h, "continuous batching"): the scheduler, the finish rule of
k_engine_finish, and the order of one bz_engine_step -- enough to predict every decision of the C code from the requests alone."""
import numpy as np

ADMIT, PREFILL, LIVE = 0, 1, 2


class RefSched:
    """bz_sched_*: FIFO admission without skipping ahead, all blocks reserved at admission, lowest free row and lowest free blocks, the last n_rows blocks
    are the rows' park blocks, prefill_chunk prompt tokens per step over the admitted requests that are not live yet, in admission order."""

    def __init__(self, n_rows, num_blocks, block_size, max_seq_len, chunk=0):
        self.n_rows, self.num_blocks, self.bs, self.max_seq_len, self.chunk = n_rows, num_blocks, block_size, max_seq_len, chunk
        self.usable = num_blocks - n_rows
        self.free = list(range(self.usable))          # kept sorted
        self.rows = [-1] * n_rows
        self.waiting, self.admitted, self.prefilling = [], {}, []
        self.next_id = 0

    def need(self, n_prompt, max_tokens):
        return -(-(n_prompt + max_tokens) // self.bs)

    def submit(self, n_prompt, max_tokens):
        assert n_prompt >= 1 and max_tokens >= 1 and n_prompt + max_tokens <= self.max_seq_len and self.need(n_prompt, max_tokens) <= self.usable
        rid = self.next_id
        self.next_id += 1
        self.waiting.append(dict(id=rid, n_prompt=n_prompt, max_tokens=max_tokens, row=-1, done=0, live=False, blocks=[]))
        return rid

    def step(self):
        acts = []
        while self.waiting and -1 in self.rows and self.need(self.waiting[0]["n_prompt"], self.waiting[0]["max_tokens"]) <= len(self.free):
            r = self.waiting.pop(0)
            n = self.need(r["n_prompt"], r["max_tokens"])
            r["row"] = self.rows.index(-1)
            r["blocks"], self.free = self.free[:n], self.free[n:]
            self.rows[r["row"]] = r["id"]
            self.admitted[r["id"]] = r
            self.prefilling.append(r["id"])
            acts.append((ADMIT, r["row"], r["id"], n, 0))
        budget = self.chunk if self.chunk > 0 else 1 << 40
        still = []
        for rid in self.prefilling:
            r = self.admitted[rid]
            take = min(r["n_prompt"] - 1 - r["done"], budget)
            if take > 0:
                acts.append((PREFILL, r["row"], rid, r["done"], r["done"] + take))
                r["done"] += take
                budget -= take
            if r["done"] == r["n_prompt"] - 1:
                r["live"] = True
                acts.append((LIVE, r["row"], rid, 0, 0))
            else:
                still.append(rid)
        self.prefilling = still
        return acts

    def finish(self, rid):
        if rid not in self.admitted:
            self.waiting = [w for w in self.waiting if w["id"] != rid]
            return
        r = self.admitted.pop(rid)
        self.free = sorted(self.free + r["blocks"])
        self.rows[r["row"]] = -1
        self.prefilling = [p for p in self.prefilling if p != rid]

    def info(self):
        return dict(n_rows=self.n_rows, num_blocks=self.num_blocks, park_blocks=self.n_rows, free_blocks=len(self.free),
                    owned_blocks=sum(len(r["blocks"]) for r in self.admitted.values()), waiting=len(self.waiting), admitted=len(self.admitted),
                    live=sum(r["live"] for r in self.admitted.values()))

    def row(self, row):
        rid = self.rows[row]
        return rid, (list(self.admitted[rid]["blocks"]) if rid >= 0 else [])


def finish_rule(live, left, tokens, stop_ids, n_stop):
    """k_engine_finish for all rows at once: (left after, ended, reason) -- a live row ends on a stop id (reason 1), else when left reaches 0 (reason 0)."""
    left = np.where(live, left - 1, left)
    stop = live & ((np.arange(stop_ids.shape[1])[None, :] < n_stop[:, None]) & (stop_ids == tokens[:, None])).any(axis=1)
    return left, stop | (live & (left <= 0)), np.where(stop, 1, 0)


def simulate_engine(n_rows, num_blocks, block_size, max_seq_len, chunk, depth, requests):
    """The order of bz_engine_step.  requests: [(arrival step, n_prompt, max_tokens, tokens the request really produces)] in submission order (arrival steps
    ascending; a request arriving at step s is submitted before that step).  Returns dict(replays, steps, first_replay {id}, admitted [ids in order])."""
    s = RefSched(n_rows, num_blocks, block_size, max_seq_len, chunk)
    pending = list(requests)
    meta, first, order = {}, {}, []
    rows = [-1] * n_rows                      # the host's view
    live = {}
    replays = read = step = 0

    def harvest(r):
        for row in range(n_rows):
            rid = rows[row]
            if rid < 0 or rid not in live or first[rid] > r:
                continue
            if r == first[rid] + meta[rid] - 1:   # the device ended the row in this replay
                s.finish(rid)
                rows[row] = -1
                del live[rid]

    while True:
        while pending and pending[0][0] <= step:
            _, n_prompt, max_tokens, n_gen = pending.pop(0)
            meta[s.submit(n_prompt, max_tokens)] = n_gen
        if replays - read >= depth:
            harvest(read)
            read += 1
        for kind, row, rid, _, _ in s.step():
            if kind == ADMIT:
                rows[row] = rid
                order.append(rid)
            elif kind == LIVE:
                live[rid] = True
                first[rid] = replays
        if live:
            replays += 1
        else:
            while read < replays:
                harvest(read)
                read += 1
        step += 1
        busy = bool(s.waiting or s.admitted or read < replays)
        if not busy and not pending:
            return dict(replays=replays, steps=step, first_replay=first, admitted=order)
