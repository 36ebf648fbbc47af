"""A numpy model of constrained word selection (odic_topk_rows_constrained), written from the semantics in
include/odic_hip.h and DESIGN.md §4.14, not from the kernel.

Row n's prefix is p = tokens[n][0 .. pos] (slot 0 = SOS).  For a growing row, word w is inadmissible if

  * w is in `banned`, or
  * w == eos and pos < min_words, or
  * no_repeat_ngram = g > 0 and some j in [0, pos - g + 1] has p[j .. j+g-2] == p[pos-g+2 .. pos] and p[j+g-1] == w
    (g = 1: every word of the prefix).

Banned ids and prefix words outside [0, V) are ignored.  A finished row (row_valid == 0) is unconstrained.  The k best
admissible words come back by value descending, then word ascending; the values are the row's own, untouched.

Not a conftest and not a test module: import it (`import search_constraints_model as SC`).
"""
from __future__ import annotations

import numpy as np


def inadmissible(prefix, pos: int, V: int, banned=(), no_repeat_ngram: int = 0, min_words: int = 0, eos: int = -1):
    """Boolean [V]: the words a growing row with this prefix may not take at step `pos`."""
    p = [int(w) for w in prefix[:pos + 1]]
    bad = np.zeros(V, bool)
    for w in banned:
        if 0 <= int(w) < V:
            bad[int(w)] = True
    if pos < min_words and 0 <= eos < V:
        bad[eos] = True
    g = int(no_repeat_ngram)
    if g > 0:
        tail = p[pos - g + 2:pos + 1] if g > 1 else []
        for j in range(0, pos - g + 2):
            if p[j:j + g - 1] == tail and 0 <= p[j + g - 1] < V:
                bad[p[j + g - 1]] = True
    return bad


def topk_rows_constrained(logp, k: int, tokens, pos: int, row_valid=None, banned=(), no_repeat_ngram: int = 0,
                          min_words: int = 0, eos: int = -1):
    """logp [N, V] float32, tokens [N, T] → (top_val float32 [N, k], top_idx int32 [N, k])."""
    logp = np.asarray(logp, np.float32)
    N, V = logp.shape
    top_val = np.empty((N, k), np.float32)
    top_idx = np.empty((N, k), np.int32)
    for n in range(N):
        if row_valid is not None and int(row_valid[n]) == 0:
            bad = np.zeros(V, bool)
        else:
            bad = inadmissible(tokens[n], pos, V, banned, no_repeat_ngram, min_words, eos)
        words = np.flatnonzero(~bad)
        order = words[np.lexsort((words, -logp[n, words].astype(np.float64)))][:k]
        assert order.size == k, "fewer than k admissible words: the caller's n_banned + T + k <= V bound was not kept"
        top_idx[n] = order
        top_val[n] = logp[n, order]
    return top_val, top_idx


def repeats_ngram(caption, g: int) -> bool:
    """True if the token list holds some g-gram twice (the whole list as given: pass it with SOS, as the prefix is)."""
    seen = set()
    for j in range(len(caption) - g + 1):
        key = tuple(caption[j:j + g])
        if key in seen:
            return True
        seen.add(key)
    return False
