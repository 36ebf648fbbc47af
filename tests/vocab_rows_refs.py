"""Hard vocabulary rows for the six per-row kernels over the vocabulary (odic_logsoftmax_topk, odic_logsoftmax_sample,
odic_topk_rows, odic_topk_rows_constrained, odic_ensemble_logprobs, odic_token_stats): seeded fp32 rows, float64
references and error bounds.  Plain data, no GPU: test_vocab_rows_host.py checks this module, test_vocab_rows_gpu.py
uses it.  Not a conftest: import it (`import vocab_rows_refs`).

Row families (FAMILIES), each a function of (V, k) alone: see `row`.  A family that cannot be built at a (V, k) is left out
of the plan (`constructible`), never skipped at run time; no row of the plan is without a finite word.

Bounds.  They come from what the kernels compute, not from what they were seen to give.  With m = max_v x_v, d_v = x_v - m,
S = Σ_v exp(d_v), lse = m + log S, logp_v = x_v - lse, u = 2^-24 (half an fp32 ulp, relative):

  E0 = 6e-6 is the error of log S as every one of the kernels forms it:
    * d_v is one rounding, |δd_v| <= u·|d_v|; through exp it moves S by at most Σ_v exp(d_v)·u·|d_v|, i.e. log S by u
      times the softmax average of |d_v|.  With d_v = logp_v + log S that average is H - log S <= H <= log V (H the
      entropy of the row): 5.5e-7 at V = 10241;
    * expf is good to a few ulp: relative 4u = 2.4e-7 on every term, so on S;
    * the terms are >= 0 and are added 34 deep at most (10 or 40 per thread at V = 10241, 6 shuffle levels, 8 or 16 wave
      sums — fewer per thread where there are more waves): relative (1 + u)^34 - 1 <= 2.1e-6 on S, so on log S;
    * logf is good to a few ulp of log S <= 9.3: 2 ulp of the binade [8, 16) is 1.9e-6.
    Sum <= 4.8e-6 < E0.
  The x - (m + log S) form (odic_logsoftmax_topk, odic_logsoftmax_sample): lse = fl(m + log S) is one rounding, at most
    2^-24·|lse|, shared by the whole row; x - lse is another, at most 2^-24·|logp|.  Taken with a factor 2 for the binade
    edges (half an ulp is up to 2^-24 RELATIVE only at a power of two):
        |err| <= E0 + 2^-23·(|lse| + |logp|).
  The (x - m) - log S form (odic_token_stats, and torch): the rounding of d_v is at most 2^-24·|d_v| <= 2^-24·(|logp| + log S)
    and the final subtraction's at most 2^-24·|logp|; the log S part (<= 5.6e-7) is inside E0's margin:
        |err| <= E0 + 2^-23·|logp|          (logp_target, max_logp; max_logp = -log S has d = 0 exactly).
  sum_logp = Σ_v d_v - V·log S, Σ_v d_v in fp64 of fp32-rounded d_v, one final rounding to fp32:
        |err| <= V·(E0 + 2^-24·max_v |d_v|) + 2^-24·|Σ|.
  odic_ensemble_logprobs, out_v = log((1/M) Σ_m exp(x_m,v - m_m)/S_m): per member the exponent's rounding u·|d_m,v| and
    the E0 of its S_m; logf of a number in (0, 1] is a few ulp of |out|:
        |err| <= E0 + 2^-23·(max_m |x_m,v - m_m| + |out_v|).
    That holds while the averaged probability is a normal fp32 number.  Below 2^-126 fp32 is spaced 2^-149 apart whatever
    the magnitude: expf's result (<= 1.5 spacings), its product with 1/S_m (<= 1), the sum over m and the product with 1/M
    together move the probability by at most A = 2^-147 absolutely, which moves the logarithm by |log(1 ± A/p)|
    (`ensemble_bounds`); a probability below half the smallest denormal rounds to 0 and gives exactly -inf.
  Whatever the reference says is -inf must be exactly -inf, a reference 0 (V = 1) exactly 0, and no output is ever NaN.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
NINF = float("-inf")

VS = (1, 37, 513, 10240, 10241)
KS = (1, 5, 9, 16)
FAMILIES = ("plain", "offset+30", "offset-30", "offset+1000", "offset-1000", "peaked", "two_level", "ramp", "near_tie",
            "zeros", "masked_30", "masked_k_one_wave", "masked_k_spread", "masked_short")
MASKED = ("masked_30", "masked_k_one_wave", "masked_k_spread", "masked_short")
K_FAMILIES = ("masked_k_one_wave", "masked_k_spread", "masked_short")      # the row depends on k too

BLOCK, WAVE, NWAVES = 512, 64, 8          # row_logsoftmax_topk: element i belongs to wave (i % 512) / 64
E0 = 6e-6
U23, U24 = 2.0 ** -23, 2.0 ** -24
DENORM_A = 2.0 ** -147                    # absolute error of an averaged probability below 2^-126


def wave_of(i):
    return (np.asarray(i) % BLOCK) // WAVE


def _gen(*key) -> torch.Generator:
    seed = 0x5EED
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _plain(V: int, salt: int = 0) -> torch.Tensor:
    return torch.randn(V, generator=_gen(1, V, salt)) * 3.0


def short_m(k: int) -> int:
    return max(1, k - 2)


def _slices(V: int) -> int:
    """Wave slices that hold at least one word of a V-word row."""
    return min(NWAVES, -(-min(V, BLOCK) // WAVE))


def constructible(family: str, V: int, k: int) -> bool:
    if k > V:
        return False
    if family in ("peaked", "two_level", "near_tie"):
        return V >= 2
    if family == "masked_30":
        return int(0.3 * V) >= 1 and V - int(0.3 * V) >= k
    if family == "masked_k_one_wave":
        return V > k and int((wave_of(np.arange(V)) == 0).sum()) >= k
    if family == "masked_k_spread":
        return V > k and k <= _slices(V) * (1 if k <= NWAVES else 2)
    if family == "masked_short":
        return V > short_m(k)
    return True


def plan():
    """Every (family, V, k) of the suite."""
    return [(f, V, k) for V in VS for k in KS for f in FAMILIES if constructible(f, V, k)]


def families_at(V: int, k: int):
    return [f for f in FAMILIES if constructible(f, V, k)]


def finite_words(family: str, V: int, k: int) -> np.ndarray:
    """The positions a masked family keeps finite (ascending)."""
    if family == "masked_30":
        perm = torch.randperm(V, generator=_gen(2, V)).numpy()
        return np.sort(perm[int(0.3 * V):])
    if family == "masked_k_one_wave":
        pool = np.flatnonzero(wave_of(np.arange(V)) == 0)
        return np.sort(pool[torch.randperm(len(pool), generator=_gen(3, V, k)).numpy()[:k]])
    if family == "masked_k_spread":
        # word j goes to slice j % ns: one per slice while k <= ns, at most two beyond
        ns, g, out = _slices(V), _gen(4, V, k), []
        for j in range(k):
            pool = np.setdiff1d(np.flatnonzero(wave_of(np.arange(V)) == j % ns), out)
            out.append(int(pool[int(torch.randint(len(pool), (1,), generator=g))]))
        return np.sort(np.array(out))
    if family == "masked_short":
        return np.sort(torch.randperm(V, generator=_gen(5, V, k)).numpy()[:short_m(k)])
    raise ValueError(family)


def peak_word(V: int) -> int:
    return int(torch.randint(V, (1,), generator=_gen(6, V)))


def row(family: str, V: int, k: int) -> torch.Tensor:
    """One fp32 row of `family`."""
    if not constructible(family, V, k):
        raise ValueError(f"{family} cannot be built at V={V}, k={k}")
    if family == "plain":
        return _plain(V)
    if family.startswith("offset"):
        return _plain(V) + float(family[len("offset"):])
    if family == "peaked":
        x, p = _plain(V), peak_word(V)
        x[p] = NINF
        x[p] = x.max() + 60.0
        return x
    if family == "two_level":
        x = torch.zeros(V)
        x[1::2] = -200.0
        return x
    if family == "ramp":
        return torch.linspace(-80.0, 80.0, V) if V > 1 else torch.zeros(1)
    if family == "near_tie":
        j = torch.randperm(V, generator=_gen(7, V)).double()
        return (5.0 + j * 2.0 ** -21).float()              # exact: ulp(5) = 2^-21
    if family == "zeros":
        return torch.zeros(V)
    x = torch.full((V,), NINF)
    keep = torch.from_numpy(finite_words(family, V, k))
    x[keep] = _plain(V)[keep]
    return x


def stack(V: int, k: int):
    """(names, X): every family of the plan at (V, k) as the rows of one fp32 [R, V] tensor."""
    names = families_at(V, k)
    return names, torch.stack([row(f, V, k) for f in names])


# ------------------------------------------------------------------------------------------------ float64 references
def log_softmax_ref(x: torch.Tensor):
    """(logp, lse) in float64 of fp32 rows [R, V]; a -inf entry gives -inf.  Shifted by the row maximum in float64, where
    the shift is exact to 2^-53."""
    x = x.to(F64)
    m = x.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    logp = x - lse
    logp[x == NINF] = NINF
    return logp, lse.squeeze(-1)


def topk_ref(x: torch.Tensor, k: int) -> torch.Tensor:
    """The first k indices of every row by (value descending, index ascending) on the raw inputs: int64 [R, k]."""
    return torch.sort(x.to(F64), dim=-1, descending=True, stable=True).indices[..., :k]


def argmax_ref(x: torch.Tensor) -> torch.Tensor:
    return topk_ref(x, 1)[..., 0]


def sum_logp_ref(x: torch.Tensor) -> torch.Tensor:
    return log_softmax_ref(x)[0].sum(-1)


def ensemble_ref(members):
    """log(mean_m softmax_m) in float64 and the mean probability itself."""
    p = torch.stack([torch.exp(log_softmax_ref(x)[0]) for x in members]).mean(0)
    return torch.log(p), p


# ------------------------------------------------------------------------------------------------------------ bounds
def bound_lse_form(logp: torch.Tensor, lse: torch.Tensor) -> torch.Tensor:
    """odic_logsoftmax_topk / _sample: logp_out [R, V] (lse [R]) or gathered top_val; -inf entries get bound 0."""
    b = E0 + U23 * (lse.abs().unsqueeze(-1) + logp.abs())
    return torch.where(torch.isfinite(logp), b, torch.zeros_like(b))


def bound_shifted_form(logp: torch.Tensor) -> torch.Tensor:
    """odic_token_stats logp_target / max_logp."""
    b = E0 + U23 * logp.abs()
    return torch.where(torch.isfinite(logp), b, torch.zeros_like(b))


def bound_sum_logp(x: torch.Tensor) -> torch.Tensor:
    """odic_token_stats sum_logp of rows without -inf (a masked row: exactly -inf, bound 0)."""
    x = x.to(F64)
    V = x.shape[-1]
    d = (x - x.max(-1, keepdim=True).values).abs().max(-1).values
    s = sum_logp_ref(x)
    b = V * (E0 + U24 * d) + U24 * s.abs()
    return torch.where(torch.isfinite(s), b, torch.zeros_like(b))


def ensemble_bounds(members, out_ref: torch.Tensor, p_ref: torch.Tensor):
    """(lower, upper) allowed deviation of odic_ensemble_logprobs from out_ref, element-wise, both >= 0; lower = +inf
    where the kernel may round the probability to 0 (p_ref <= DENORM_A)."""
    d = torch.stack([(x.to(F64) - x.to(F64).max(-1, keepdim=True).values).abs() for x in members]).max(0).values
    b = E0 + U23 * (d + out_ref.abs())
    sub = p_ref < 2.0 ** -126 * (1.0 + 2.0 ** -20)
    up = torch.where(sub, b + torch.log1p(DENORM_A / p_ref), b)
    lo = torch.where(sub & (p_ref > DENORM_A), b - torch.log1p(-(DENORM_A / p_ref).clamp(max=1 - 1e-16)), b)
    lo = torch.where(sub & (p_ref <= DENORM_A), torch.full_like(b, float("inf")), lo)
    return lo, up


def ratios(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """err / bound element-wise; where the reference is -inf or the bound is 0 (an exact value is asked for): 0 when the
    output has exactly the reference's value, +inf otherwise.  A NaN output gives +inf."""
    got, want = got.to(F64), want.to(F64)
    exact = (bound == 0) | ~torch.isfinite(want)
    err = (got - want).abs()
    r = torch.where(exact, torch.where(got == want, 0.0, float("inf")), err / bound.clamp(min=1e-300))
    return torch.where(torch.isnan(got) | torch.isnan(r), torch.full_like(r, float("inf")), r)


# ------------------------------------------------------------------------------------- fp32 restatements of the kernels
def f32_lse_form(x: torch.Tensor, drop_max=False, extra_term=False) -> torch.Tensor:
    """x - (max + log Σ exp(x - max)) with every operation rounded to fp32 (numpy): the form of odic_logsoftmax_topk.
    drop_max and extra_term restate two mutations: no maximum subtraction, and a sum that runs one element past the row
    (the element behind a row is the next logit, taken here as the row's last word again)."""
    a = x.numpy().astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = np.zeros((a.shape[0], 1), np.float32) if drop_max else a.max(-1, keepdims=True)
        e = np.exp((a - m).astype(np.float32)).astype(np.float32)
        s = e.sum(-1, keepdims=True, dtype=np.float32)
        if extra_term:
            s = (s + e[:, -1:]).astype(np.float32)
        lse = (m + np.log(s).astype(np.float32)).astype(np.float32)
        return torch.from_numpy((a - lse).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- ensemble cases
ENSEMBLE_VS = (37, 513, 10241)
ENSEMBLE_MS = (2, 3)
UNDERFLOW_DEPTHS = (200.0, 215.0, 230.0)


def ens_own_words(members):
    return [int(argmax_ref(-x[None])[0]) for x in members]


def ens_disagree(M: int, V: int):
    """Member m: randn·3 with +40 on its own word a_m, a_m the member's lowest word.  (Anywhere else the other words
    could fall more than 40 + 24 below it — randn·3 spans ±12 at V = 10241 — and the 2^-60 floor of the issue would not
    hold; with the lowest word raised every other word of the member is at most 40 + 1e-3 below the new maximum.)
    Returns (members, own words)."""
    base = [_plain(V, salt=10 + m) for m in range(M)]
    own = ens_own_words(base)
    members = []
    for x, a in zip(base, own):
        x = x.clone()
        x[a] += 40.0
        members.append(x[None])
    return members, own


def ens_offsets(M: int, V: int):
    """(shifted, unshifted): members randn·3 rounded to multiples of 2^-14 = ulp(1000), shifted by +1000, -1000, 0 (the
    first M of them).  On that grid x + c is exact in fp32, so the shifted rows ARE the unshifted ones moved: the two
    references agree to float64 rounding and the kernel's whole deviation is its own."""
    base = [(torch.round(_plain(V, salt=20 + m) * 2.0 ** 14) * 2.0 ** -14)[None] for m in range(M)]
    return [x + c for x, c in zip(base, (1000.0, -1000.0, 0.0))], base


def ens_underflow(M: int, V: int):
    """Every member a ramp whose low end sits UNDERFLOW_DEPTHS[m] below its maximum."""
    return [torch.linspace(-UNDERFLOW_DEPTHS[m], 0.0, V)[None] for m in range(M)]


def ens_masked_member(M: int, V: int):
    """(members, word): member 0 has -inf at a word the others keep."""
    members = [_plain(V, salt=30 + m)[None].clone() for m in range(M)]
    w = int(torch.randint(V, (1,), generator=_gen(8, V, M)))
    members[0][0, w] = NINF
    return members, w


UNDERFLOW_P = 2.0 ** -149 * 0.5           # below it the fp32 probability rounds to 0
UNDERFLOW_OUT_MAX = math.log(2.0 ** -140)


# --------------------------------------------------------------------------------------------------------- sampling
SAMPLE_REPS = 64                          # rows = seeds: the noise is keyed by the row
SAMPLE_SEED, SAMPLE_POS = 20231, 3
GOLDEN_ROWS = 4                           # `plain` rows recorded from the parent build (tests/golden/vocab_rows_sample.npz)


def sample_stack(V: int, k: int):
    """(names, X [R·SAMPLE_REPS, V]): row r·SAMPLE_REPS + s is family r under noise stream s."""
    names, X = stack(V, k)
    return names, X.repeat_interleave(SAMPLE_REPS, 0)


def sample_shapes():
    return [(V, k) for V in VS for k in KS if k <= V] + [(16, 16)]
