"""A plain Python restatement of what csrc/caption_metrics.hip and metrics.py compute (include/odic_hip.h has the contracts):
the BLEU components from collections.Counter, the LCS by the textbook dynamic programme (NOT the bit-parallel form the kernel
uses), and the score formulas of the reference's bleu_scorer.compute_score and rouge.Rouge.calc_score.  The host tests
compare it with the reference's recorded values (tests/golden/caption_metrics.json, tools/make_golden_metrics.py), the GPU
tests compare the kernels with it.  Not a test module and not a conftest: import it.

The integers must be equal.  The scores are at most 1 and come from a handful of fp64 operations on integers: they are held to
cider_device_model.TOL = 1e-10 absolute, the project's figure for fp64 scores against the reference.
"""
from __future__ import annotations

import math
from collections import Counter

import numpy as np

STAT_WORDS, MAX_LEN = 12, 128
TINY, SMALL, BETA = 1e-15, 1e-9, 1.2


def ngrams(ids):
    ids = [int(t) for t in ids]
    return Counter(tuple(ids[i:i + k]) for k in range(1, 5) for i in range(len(ids) - k + 1))


def bleu_stats(hyp, refs, max_len=MAX_LEN):
    """The 12 words odic_bleu_stats writes for one query: correct_1..4, guess_1..4, testlen, the closest, the shortest and the
    summed reference length."""
    hyp, refs = list(hyp)[:max_len], [list(r)[:max_len] for r in refs]
    most = Counter()
    for r in refs:
        for g, c in ngrams(r).items():
            most[g] = max(most[g], c)
    correct = [0] * 4
    for g, c in ngrams(hyp).items():
        correct[len(g) - 1] += min(c, most[g])
    L, lens = len(hyp), [len(r) for r in refs]
    closest = min((abs(l - L), l) for l in lens)[1] if lens else 0
    return correct + [max(0, L - k) for k in range(4)] + [L, closest, min(lens) if lens else 0, sum(lens)]


def lcs(a, b):
    a, b = list(a), list(b)
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def bleu_from_stats(s):
    """Four scores from one row of stats (a sentence's, or the corpus sums): bleu_scorer.compute_score's expressions."""
    out, prod = [], 1.0
    for k in range(4):
        prod *= (float(s[k]) + TINY) / (float(s[4 + k]) + SMALL)
        out.append(prod ** (1.0 / (k + 1)))
    ratio = (s[8] + TINY) / (s[9] + SMALL)
    if ratio < 1:
        out = [v * math.exp(1 - 1 / ratio) for v in out]
    return out


def bleu(cands, refs):
    """→ (corpus scores [4], per-sentence scores [4][H], stats [H][12])"""
    stats = [bleu_stats(c, r) for c, r in zip(cands, refs)]
    per = [bleu_from_stats(s) for s in stats]
    return bleu_from_stats(np.sum(np.array(stats, dtype=np.int64), axis=0).tolist()), [list(v) for v in zip(*per)], stats


def rouge_from_lcs(lcs_len, len_c, len_r):
    """rouge.Rouge.calc_score for one candidate: the LCS with each reference, the candidate's and the references' lengths."""
    if len_c == 0:
        return 0.0
    prec, rec = max(l / float(len_c) for l in lcs_len), max(l / float(n) for l, n in zip(lcs_len, len_r))
    if prec == 0 or rec == 0:
        return 0.0
    return ((1 + BETA ** 2) * prec * rec) / float(rec + BETA ** 2 * prec)


def rouge_l(cand, refs):
    return rouge_from_lcs([lcs(r, cand) for r in refs], len(cand), [len(r) for r in refs])


def consensus_rows(cands, eos_idx):
    return [list(c[1:]) + ([] if len(c) > 1 and c[-1] == eos_idx else [eos_idx]) for c in cands]


def pairwise(cands, eos_idx, metric):
    """The utility matrix of one image: entry (i, j) scores candidate i against candidate j as its single reference."""
    rows = consensus_rows(cands, eos_idx)
    if metric == "bleu4":
        return np.array([[bleu_from_stats(bleu_stats(a, [b]))[3] for b in rows] for a in rows])
    return np.array([[rouge_l(a, [b]) for b in rows] for a in rows])


def consensus_from_matrix(m):
    """→ (best index, scores [N]): the off-diagonal row means, summed in ascending order, ties to the lower index."""
    m = np.asarray(m, dtype=np.float64)
    N = m.shape[0]
    if N == 1:
        return 0, np.zeros(1)
    s = np.array([np.sum(np.sort([m[i, j] for j in range(N) if j != i])) / (N - 1) for i in range(N)])
    return int(np.argmax(s)), s


def consensus(cands, eos_idx, metric):
    return consensus_from_matrix(pairwise(cands, eos_idx, metric))
