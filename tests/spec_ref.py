"""numpy restatement of the speculative accept rule (include/blazr_hip.h: bz_spec_accept): per-row argmax with the lowest index on ties, the longest
prefix on which the draft agrees with it, and the record layout {n_accept, tokens[0 .. n_accept], -1 ...}."""
import numpy as np


def row_argmax(logits):
    """first maximum of every row of [R, V] (np.argmax returns the first occurrence; an all -inf row gives 0)"""
    return np.argmax(np.asarray(logits, dtype=np.float32), axis=1).astype(np.int64)


def accept(argmax, draft):
    """(n_accept, tokens[0 .. n_accept]): tokens[i] = draft[i] while the draft agrees, then the target's own token (correction or bonus)"""
    argmax, draft = np.asarray(argmax, dtype=np.int64), np.asarray(draft, dtype=np.int64)
    assert len(draft) == len(argmax) - 1
    n = 0
    while n < len(draft) and draft[n] == argmax[n]:
        n += 1
    return n, np.concatenate([draft[:n], argmax[n:n + 1]])


def record(logits, draft):
    """the device record I64 [R + 1]"""
    am = row_argmax(logits)
    n, toks = accept(am, draft)
    rec = np.full(len(am) + 1, -1, dtype=np.int64)
    rec[0] = n
    rec[1:2 + n] = toks
    return rec
