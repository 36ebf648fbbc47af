"""A numpy restatement of exactly what csrc/cider.hip computes (include/odic_hip.h has the contract): packed uint64 n-gram
keys, sorted unique keys with their term frequency, IDF by searchsorted in a sorted table, per-order sums.  The GPU tests
compare the kernels with it entry by entry; the host tests compare it with the reference's recorded scores
(tests/golden/reinforce_cider.json) and with cider.CiderD.  Not a test module and not a conftest: import it.

Tolerance shared by every comparison (device against model, device against golden, model against golden): a score is a sum
of at most 512 non-negative fp64 terms per order, two square roots, one division and one exp, scaled to [0, 10] — an error
of about 512 · 2^-52 · 10 ≈ 1e-12.  TOL = 1e-10 absolute.
"""
from __future__ import annotations

import math

import numpy as np

TOL = 1e-10
MAX_LEN, MAX_KEYS, MAX_ID, SIGMA = 128, 512, 65533, 6.0


def pack_keys(ids):
    """All n-grams of orders 1..4 of a caption as uint64 keys Σ_j (id_j + 1) << (16·j), order after order."""
    keys = []
    for k in range(1, 5):
        for i in range(len(ids) - k + 1):
            key = 0
            for j in range(k):
                assert 0 <= ids[i + j] <= MAX_ID
                key |= (int(ids[i + j]) + 1) << (16 * j)
            keys.append(key)
    return np.array(keys, dtype=np.uint64)


def key_order(keys):
    """0..3: the index of the highest non-zero 16-bit field."""
    k = np.asarray(keys, dtype=np.uint64)
    return ((k >> np.uint64(16)) != 0).astype(int) + ((k >> np.uint64(32)) != 0) + ((k >> np.uint64(48)) != 0)


class Table:
    """The document-frequency table of a corpus: list[n_images][n_refs] of id lists (EOS already appended)."""

    def __init__(self, corpus):
        per_image = [np.unique(np.concatenate([pack_keys(r) for r in refs])) for refs in corpus]
        self.keys, df = np.unique(np.concatenate(per_image), return_counts=True)
        self.n_images = len(corpus)
        self.default_idf = math.log(float(self.n_images))
        self.idf = self.default_idf - np.log(np.maximum(1.0, df.astype(np.float64)))


def vectorize(ids, table=None, default_idf=1.0, max_len=MAX_LEN):
    """→ dict(keys uint64 [U] ascending, tf int [U], w fp64 [U], norms fp64 [4], length int): one workspace row."""
    ids = list(ids)[:max_len]
    keys, tf = np.unique(pack_keys(ids), return_counts=True)            # (np.unique sorts uint64 as unsigned)
    idf = np.full(keys.size, float(default_idf))
    if table is not None and table.keys.size and keys.size:
        at = np.searchsorted(table.keys, keys)
        hit = (at < table.keys.size) & (table.keys[np.minimum(at, table.keys.size - 1)] == keys)
        idf[hit] = table.idf[at[hit]]
    w = tf.astype(np.float64) * idf
    order = key_order(keys)
    norms = np.array([math.sqrt(float(np.sum(w[order == o] ** 2))) for o in range(4)])
    return dict(keys=keys, tf=tf, w=w, norms=norms, length=max(len(ids) - 1, 0))


def pair(h, r):
    """CIDEr-D of one vectorised hypothesis against one vectorised reference (× 10, mean of the four orders)."""
    val = np.zeros(4)
    if h["keys"].size and r["keys"].size:
        at = np.searchsorted(r["keys"], h["keys"])
        hit = (at < r["keys"].size) & (r["keys"][np.minimum(at, r["keys"].size - 1)] == h["keys"])
        wr = r["w"][at[hit]]
        term = np.minimum(h["w"][hit], wr) * wr
        order = key_order(h["keys"][hit])
        for o in range(4):
            val[o] = float(np.sum(term[order == o]))
    for o in range(4):
        if h["norms"][o] != 0 and r["norms"][o] != 0:
            val[o] /= h["norms"][o] * r["norms"][o]
    delta = float(h["length"] - r["length"])
    return float(np.sum(val * math.exp(-(delta ** 2) / (2 * SIGMA ** 2))) / 4.0 * 10.0)


def score(hyp, refs, table=None, default_idf=1.0):
    """The score of one hypothesis against its references: the mean of its pair similarities."""
    h = vectorize(hyp, table, default_idf)
    return sum(pair(h, vectorize(r, table, default_idf)) for r in refs) / len(refs)


def reward(pred, logprob, image_idx, corpus, table, base=None):
    """ReinforceCiderReward.compute_reward on id lists: pred list[B][S] with SOS and EOS, corpus with EOS appended."""
    def scores(caps):
        return np.array([[score(c[1:], corpus[i], table, table.default_idf) for c in per]
                         for per, i in zip(caps, image_idx)])
    r = scores(pred)
    b = (r.sum(-1, keepdims=True) - r) / (r.shape[1] - 1) if base is None else scores(base)
    loss = float(np.mean((r - b) * np.sum(-np.asarray(logprob, dtype=np.float64), axis=-1)))
    return loss, r, b


def consensus(cands, eos_idx, table=None, default_idf=1.0):
    """consensus_rerank for one image: → (best index, scores [N])."""
    rows = [list(c[1:]) + ([] if len(c) > 1 and c[-1] == eos_idx else [eos_idx]) for c in cands]
    N = len(rows)
    if N == 1:
        return 0, np.zeros(1)
    v = [vectorize(r, table, default_idf) for r in rows]
    # the similarities are summed in ascending order: equal candidates then get equal scores to the bit, whatever their
    # positions, and the tie goes to the lower index
    s = np.array([np.sum(np.sort([pair(v[i], v[j]) for j in range(N) if j != i])) / (N - 1) for i in range(N)])
    return int(np.argmax(s)), s
