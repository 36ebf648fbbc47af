"""A numpy model of odic_contrast_topk (include/odic_hip.h): the float64 reference, an fp32 restatement
of rules 1-5, the error bound of a score, the seeded row families and `clear`.  Plain data, no GPU:
test_contrast_host.py checks this module, test_contrast_rows_gpu.py uses it.  Not a conftest: `import contrast_model`.

The bound.  With u23 = 2^-23 (one fp32 rounding, taken with the factor 2 of vocab_rows_refs for the binade edges) and
B(lp, lse) = E0 + u23·(|lse| + |lp|) the documented bound of a log-prob in the x − (max + log Σ exp(x − max)) form
(vocab_rows_refs.bound_lse_form), the kernel's out[v] = lp_t − w·max(s, floor) errs by at most

    B(lp_t, lse_t) + w·err(s) + u23·(|w·s'| + |out|)                      (the rounded product, the rounded difference)

with err(s) for the suppressor s of c active distractors:
  c == 1:  s = lp_1, err(s) = B(lp_1, lse_1).
  c  > 1:  s = (m + logf(Σ_d expf(lp_d − m))) − logf(c), m = max_d lp_d.
    * log Σ_d exp(lp_d) moves by at most max_d |δ lp_d| when its arguments move (its gradient is a probability vector):
      max_d B(lp_d, lse_d) over the distractors that do not mask the word (a masked one is exactly -inf);
    * the sum Σ lies in [1, c] (the largest term is exp(0) = 1 exactly).  Each term carries the rounding of its exponent,
      u24·|lp_d − m|·exp(lp_d − m) <= u24/e absolutely, and expf's few ulp, 4·u24 relative; the c − 1 additions add
      (c − 1)·u24 relative: together at most (7/e + 4 + 7)·u24 < 14·u24 = 8.4e-7 relative on Σ, so absolute on log Σ;
    * logf(Σ) and logf(c) are good to a few ulp of a number <= log 8 = 2.08: 2 ulp of the binade [2, 4) is 4.8e-7 each;
    together EMIX = 2.5e-6 > 8.4e-7 + 2·4.8e-7;
    * the two roundings of m + log Σ (a number of size <= |s| + log c) and of the difference (size |s|):
      u23·(2·|s| + log c).
    err(s) = max_d B(lp_d, lse_d) + EMIX + u23·(2·|s| + log c).
  max(·, floor) moves by no more than its argument; a word every active distractor masks has s' = floor exactly.
Where the model says -inf (a word the target masks, an inadmissible word) the kernel must say exactly -inf: bound 0.
Admissibility itself is exact: it is decided on the fp32 logits by one fp32 subtraction and integer ranks, which numpy
restates bit for bit.
"""
from __future__ import annotations

import functools
import math

import numpy as np

E0 = 6e-6                       # vocab_rows_refs.E0: the error of log Σ exp as the row kernels form it
U23 = 2.0 ** -23
EMIX = 2.5e-6
NINF = -np.inf

VS = (17, 259, 10001)
KS = (1, 3, 16)
MS = (1, 2, 8)
EXTRA_SHAPES = ((10241, 3, 2), (10241, 16, 8))       # rows above 10240 words take the kernel's streaming path
STRUCTURED = ("ties", "tie_cut", "target_masked", "masked_all", "masked_some", "identical", "offset", "dominant",
              "below_floor", "short")
N_DENSE = 6
#: the two settings every shape runs under: (weight, plausibility, floor, extra), min_keep = min(k + extra, V)
SETTINGS = ((0.7, 0.1, -20.0, 2), (1.25, 0.0, -12.0, 0))
MAX_UNCLEAR_DENSE = 0.02


def min_keep_of(k: int, extra: int, V: int) -> int:
    return min(k + extra, V)


def shapes():
    return [(V, k, M) for V in VS for k in KS for M in MS if k <= V] + list(EXTRA_SHAPES)


def log_alpha_of(plausibility: float) -> np.float32:
    return np.float32(math.log(plausibility)) if plausibility > 0 else np.float32(NINF)


# ---------------------------------------------------------------------------------------------------------- the rows
def _rng(*key):
    return np.random.default_rng([7919] + [int(v) for v in key])


def _head(V: int, n: int, rng) -> np.ndarray:
    """n distinct word ids, spread over the row (both ends included when there is room)."""
    n = min(n, V)
    ids = rng.choice(V, size=n, replace=False)
    if V > n + 2:
        ids[0], ids[-1] = V - 1, 0
        ids = np.array(list(dict.fromkeys(ids.tolist())))
    return ids.astype(np.int64)


def family_row(family: str, V: int, k: int, M: int, salt: int = 0) -> np.ndarray:
    """fp32 [M, V]: the target's logits and those of M - 1 distractors for one row of `family`."""
    rng = _rng(STRUCTURED.index(family) if family in STRUCTURED else 99, V, k, M, salt)
    x = rng.standard_normal((M, V)).astype(np.float32)
    if family == "dense":
        return (x * np.float32(3.0)).astype(np.float32)
    h = _head(V, k + 4, rng)                          # the words the row is about, best first
    n = len(h)
    x[0, h] = (8.0 - 0.5 * np.arange(n)).astype(np.float32)
    for d in range(1, M):                             # the distractors like them too, each in its own order
        x[d, h] = (6.0 - 0.375 * rng.permutation(n)).astype(np.float32)
    if family == "ties":                              # equal in every row: exact ties, decided by the index
        x[:, h] = x[:, h[:1]]
    elif family == "tie_cut":                         # one plausible word, then a level the min_keep cut falls into
        x[0, h[1:]] = np.float32(5.0)
        x[1:, h[1:]] = x[1:, h[1:2]]
    elif family == "target_masked":
        x[0, h[1::2]] = NINF
        x[0, rng.choice(V, size=max(1, V // 7), replace=False)] = NINF
        x[0, h[0]] = np.float32(8.0)
    elif family == "masked_all":
        x[1:, h[::2]] = NINF
    elif family == "masked_some":
        x[1::2, h[::2]] = NINF
    elif family == "identical":
        x[1:2] = x[0:1]
    elif family == "offset":
        x[0] += np.float32(80.0)
        x[1::2] -= np.float32(80.0)
        x[2::2] += np.float32(80.0)
    elif family == "dominant":
        x[0, h[0]] = np.float32(38.0)
    elif family == "below_floor":
        x[1:, h[::2]] = np.float32(-60.0)
    elif family == "short":                           # fewer than k finite words (one at least: the contract)
        keep = h[:max(1, min(k - 1, n))]
        v = x[0, keep].copy()
        x[0] = NINF
        x[0, keep] = v
    else:
        raise KeyError(family)
    return x.astype(np.float32)


MAX_SALTS = 16


@functools.lru_cache(maxsize=None)
def batch(V: int, k: int, M: int):
    """The rows of one launch: every structured family twice — with all M - 1 distractors, and with a ragged count — and
    N_DENSE dense rows.  A structured row is the first of its family's seeded rows (salts 0, 1, ...) that is `clear`
    under every one of SETTINGS: where a family leaves the order of two words to chance (random words it does not
    shape), the model alone — never the kernel — decides which row is used; the dense rows are taken as they come.
    → (names, x fp32 [M, N, V], count int32 [N], refs: per setting the `reference` of every row)."""
    names, rows, count = [], [], []
    D = M - 1
    for rep in range(2):
        for f, fam in enumerate(STRUCTURED):
            c = D if rep == 0 else (f * 3 + 1) % (D + 1)
            for salt in range(MAX_SALTS):
                x = family_row(fam, V, k, M, rep * MAX_SALTS + salt)
                if all(reference(x, c, w, log_alpha_of(pl), fl, min_keep_of(k, extra, V), k)["clear"] for w, pl, fl, extra in SETTINGS):
                    break
            names.append(fam)
            rows.append(x)
            count.append(c)
    for j in range(N_DENSE):
        names.append("dense")
        rows.append(family_row("dense", V, k, M, j))
        count.append(D if j % 2 == 0 else j % (D + 1))
    refs = [[reference(x, c, w, log_alpha_of(pl), fl, min_keep_of(k, extra, V), k) for x, c in zip(rows, count)]
            for w, pl, fl, extra in SETTINGS]
    return names, np.stack(rows, axis=1), np.array(count, dtype=np.int32), refs


# ------------------------------------------------------------------------------------------------- rule 4, bit for bit
def admissible(xt: np.ndarray, log_alpha, min_keep: int):
    """(mask bool [V], m): the admissible words of a target row and the number of plausible ones, as the kernel decides
    them: one fp32 subtraction, then the first max(m, min_keep) words by (value descending, index ascending)."""
    xt = xt.astype(np.float32)
    with np.errstate(invalid="ignore"):
        plaus = (xt - xt.max()).astype(np.float32) >= np.float32(log_alpha)
    m = int(plaus.sum())
    order = np.argsort(-xt.astype(np.float64), kind="stable")
    mask = np.zeros(xt.shape[0], dtype=bool)
    mask[order[:max(m, int(min_keep))]] = True
    return mask, m


def _logsoftmax64(x):
    x = x.astype(np.float64)
    mx = x.max()
    lse = mx + math.log(np.exp(x - mx).sum())
    with np.errstate(invalid="ignore"):
        return x - lse, lse


# ------------------------------------------------------------------------------------------------ float64 reference
def reference(x: np.ndarray, c: int, w: float, log_alpha, floor: float, min_keep: int, k: int) -> dict:
    """One row, x fp32 [M, V].  out float64 [V] (rules 1-4), bound float64 [V] (0 where out is -inf), kept, mask, top
    int64 [k] (rule 5 on the float64 scores), clear (see `clear`)."""
    V = x.shape[1]
    w = float(np.float32(w))
    floor = float(np.float32(floor))
    lp_t, lse_t = _logsoftmax64(x[0])
    mask, m = admissible(x[0], log_alpha, min_keep)
    b_t = E0 + U23 * (abs(lse_t) + np.abs(np.where(np.isfinite(lp_t), lp_t, 0.0)))
    if c > 0 and w != 0.0:
        lps, lses = zip(*[_logsoftmax64(x[d]) for d in range(1, c + 1)])
        lps = np.stack(lps)
        fin = np.isfinite(lps)
        b_d = np.where(fin, E0 + U23 * (np.abs(np.array(lses))[:, None] + np.abs(np.where(fin, lps, 0.0))), 0.0).max(0)
        if c == 1:
            s, err_s = lps[0], b_d
        else:
            mm = lps.max(0)
            with np.errstate(invalid="ignore", divide="ignore"):
                s = np.where(np.isfinite(mm), mm + np.log(np.exp(lps - np.where(np.isfinite(mm), mm, 0.0)).sum(0)) - math.log(c),
                             NINF)
            err_s = b_d + EMIX + U23 * (2.0 * np.abs(np.where(np.isfinite(s), s, 0.0)) + math.log(c))
        err_s = np.where(np.isfinite(s), err_s, 0.0)                  # masked by every active distractor: floor exactly
        sp = np.maximum(s, floor)
        out = lp_t - w * sp
        bound = b_t + w * err_s + U23 * (np.abs(w * sp) + np.abs(np.where(np.isfinite(out), out, 0.0)))
    else:
        out, bound = lp_t.copy(), b_t
    out = np.where(mask, out, NINF)
    bound = np.where(np.isfinite(out), bound, 0.0)
    top = np.argsort(-out, kind="stable")[:k]
    return dict(out=out, bound=bound, kept=m, mask=mask, top=top, clear=clear(x[:c + 1] if w != 0.0 else x[:1], out, bound, k))


def clear(x_used: np.ndarray, out: np.ndarray, bound: np.ndarray, k: int) -> bool:
    """Can the kernel's top-k be asked for exactly?  In float64, every gap among ranks 1 .. k+1 exceeds twice the bound
    (the sum of the two neighbours' bounds).  Two neighbours that are both -inf, or whose logits agree in every row that
    is read (the kernel then computes one number twice), are an exact tie, decided by the index: clear as well."""
    order = np.argsort(-out, kind="stable")[:k + 1]
    for a, b in zip(order[:-1], order[1:]):
        if out[a] == NINF and out[b] == NINF:
            continue
        if np.array_equal(x_used[:, a], x_used[:, b]):
            continue
        if not (out[a] - out[b] > bound[a] + bound[b]):
            return False
    return True


# ------------------------------------------------------------------------------------------------- fp32 restatement
def f32_form(x: np.ndarray, c: int, w: float, log_alpha, floor: float, min_keep: int, k: int, *, clamp: bool = True):
    """Rules 1-5 with every operation rounded to fp32 (numpy's expf / logf, not the device's) → (out fp32 [V], top
    int64 [k]).  clamp=False restates a mutation: no floor."""
    f = np.float32
    w, floor = f(w), f(floor)

    def lsm(r):
        with np.errstate(invalid="ignore", divide="ignore"):
            mx = r.max()
            return (r - f(mx + np.log(np.exp((r - mx).astype(f)).sum(dtype=f)))).astype(f)

    lp_t = lsm(x[0].astype(f))
    mask, _ = admissible(x[0], log_alpha, min_keep)
    out = lp_t
    if c > 0 and w != 0:
        lps = np.stack([lsm(x[d].astype(f)) for d in range(1, c + 1)])
        if c == 1:
            s = lps[0]
        else:
            mm = lps.max(0)
            with np.errstate(invalid="ignore", divide="ignore"):
                acc = np.zeros_like(mm)
                for d in range(c):
                    acc = (acc + np.exp((lps[d] - mm).astype(f)).astype(f)).astype(f)
                s = ((mm + np.log(acc).astype(f)).astype(f) - f(math.log(c))).astype(f)
            s = np.where(np.isfinite(mm), s, f(NINF)).astype(f)
        sp = np.maximum(s, floor) if clamp else s
        with np.errstate(invalid="ignore"):
            out = (lp_t - (w * sp).astype(f)).astype(f)
    out = np.where(mask, out, f(NINF)).astype(f)
    return out, np.argsort(-out.astype(np.float64), kind="stable")[:k]
