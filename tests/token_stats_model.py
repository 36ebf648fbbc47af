"""odic_token_stats and odic_dec_embed_seq (csrc/decoder_seq.hip) restated without a GPU: a float64 reference, a float32
numpy model that follows token_stats_kernel operation by operation, named row families, and the error bound of every output
as a function of the row.  Plain data: test_token_stats_host.py checks this module, test_token_stats_gpu.py uses it.  Not a
conftest: import it (`import token_stats_model`).

The kernel (one 256-thread block = 4 waves of 64 per row; thread t owns elements t, t + 256, ...):
  pass 1  per thread (m, mi) = (-inf, INT_MAX); an element replaces it when it is LARGER or when the thread has none yet
          (so a thread's first element is always taken, a NaN too; later NaNs are skipped since NaN > m is false).
          wave_argmax: 6 butterfly steps (lane ^ 32, 16, ... 1), a lane adopts its partner's pair when that pair
          ranks_before its own: larger value, or equal value and lower index.  A NaN ranks neither before nor after
          anything: a lane that holds one keeps it and no lane ever adopts it, so whatever had to travel THROUGH that lane
          is lost.  Lane 0 of each wave stores the wave's pair; the block's pair is wave 0's, replaced in ascending wave
          order by a pair that ranks_before it.  A thread (or a whole wave, V < 64·w) without an element carries
          (-inf, INT_MAX), which loses against a real -inf by its index.
  pass 2  per thread se += expf(x - m) in fp32 and sx += (double)(x - m), elements in ascending order; wave_sum is the
          same butterfly with +, the block sum adds the four wave sums to 0 in ascending order.
  tail    lg = logf(e); sum_logp = (float)(dsum - (double)V·lg); max_logp = -lg; argmax = mi;
          target in [0, V): logp_target = (x[target] - m) - lg, otherwise logp_target = 0 and bit 0 is OR-ed into *status.

What that pins (kernel_model computes all of it; NONFINITE is the table):
  * arg-max = the lowest index of the maximum, for every row without a NaN (a -inf row included: index 0);
  * a flagged row gets exactly 0.0, and *status is only ever OR-ed: 0 -> 1, 4 -> 5, untouched without a flagged row;
  * -inf words: log-prob and sum_logp exactly -inf, arg-max / max_logp unaffected (as torch.log_softmax);
  * one +inf, or no finite word at all: x - m is inf - inf = NaN for the maximum itself, so the three float outputs are
    NaN (as torch.log_softmax gives) while the arg-max is still the lowest index of the maximum;
  * a NaN anywhere makes the three float outputs NaN (as torch).  The arg-max is NOT torch's (torch ranks NaN highest):
    a NaN that is not its thread's first element (index >= 256) is skipped and the arg-max is that of the other words; a
    NaN at index 0 keeps lane 0 of wave 0 and gives index 0; any other NaN in the first 256 words hides from the arg-max
    the words whose butterfly path to lane 0 runs through its lane (lanes_hidden_by).

Bounds.  u = 2^-24.  d_v = x_v - m is one fp32 rounding (|δ| <= u·|d_v|; exact for close values), S = Σ_v exp(d_v) >= 1,
lg = log S, p_v = exp(d_v)/S.  The error of the kernel's lg, absolute:
    A1 = u·Σ_v p_v·|d_v|                        the rounding of d_v, through exp, weighted as S weights it
    A2 = EXPF_ULP·2^-23                         expf, relative on every term and so on S
    A3 = (ceil(V/256) + 6 + 4)·u                the additions on the longest path of the sum of non-negative terms: the
                                                thread's own, 6 butterfly levels, 4 wave sums
    A4 = LOGF_ULP·2^-23·|lg|                    logf (an ulp of y is at most 2^-23·|y|)
    A5 = V·2^-126                               terms flushed or rounded below the normal range, S >= 1
    E_lg = (A1 + A2 + A3 + A5)·(1 + 1e-6) + A4
  max_logp = -lg:                               E_lg
  logp_target = fl(fl(x_t - m) - lg):           u·|d_t| + E_lg + u·(|logp_t| + E_lg)              (a -inf target: exact)
  sum_logp = fl32(Σ_v d_v - V·lg), Σ in fp64:   u·Σ_v|d_v| + V·E_lg + 2^-50·(Σ_v|d_v| + V·|lg|) + u·(|sum| + the rest)
                                                                                        (a row with a -inf: exactly -inf)
EXPF_ULP = LOGF_ULP = 2 covers the device's expf / logf (documented at 1 ulp) with a factor 2.  kernel_model rounds a
float64 exp / log to fp32 (half an ulp) and otherwise has the kernel's operation order, so it must sit well inside:
test_token_stats_host.py asserts ratio <= EMU_ROOM = 0.5 for every (family, V).
    Measured worst ratio of the model over all (family, V):  logp_target 0.41, sum_logp 0.40, max_logp 0.17
    (EMU_WORST below; the host test prints them).
The GPU is held to the bound itself, GPU_FACTOR = 1.0: a factor 1/0.41 = 2.4 over the model's worst case, which is the room
for the device's expf / logf being 1 to 2 ulp where the model's are half an ulp.  The `randn3` family is held to the
2e-6·scale of test_token_stats as well.
"""
from __future__ import annotations

import math

import numpy as np

F32, F64 = np.float32, np.float64
NT, WAVE, NWAVES = 256, 64, 4
INT_MAX = 0x7FFFFFFF
INT64_MIN = -(2 ** 63)
NINF = float("-inf")
U24 = 2.0 ** -24
EXPF_ULP, LOGF_ULP = 2.0, 2.0
EMU_ROOM = 0.5
EMU_WORST = {"logp_target": 0.41, "sum_logp": 0.40, "max_logp": 0.17}
GPU_FACTOR = 1.0

V_EDGES = (1, 2, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 10000, 10003)
TARGET_EDGES = ("0", "V-1", "V", "-1", "2^40", "INT64_MIN")
_LANE = np.arange(WAVE)


def target_edges(V: int):
    return [0, V - 1, V, -1, 2 ** 40, INT64_MIN]


# ------------------------------------------------------------------------------------------------------- row families
def _rng(name: str, V: int, seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[sum(ord(c) * (i + 1) for i, c in enumerate(name)) * 100003 + V, seed]))


def _randn(V, g, scale=1.0):
    return (g.standard_normal(V) * scale).astype(F32)


def _tie(V, g, a, b):
    x = _randn(V, g, 3.0)
    x[a] = x[b] = x.max() + F32(1.0)
    return x


def _masked(V, g):
    x = _randn(V, g, 3.0)
    x[g.permutation(V)[:V // 3]] = NINF
    return x


def _dominant(V, g):
    x = _randn(V, g)
    x[int(g.integers(V))] += F32(1e3)
    return x


def _two_level(V, g):
    x = np.zeros(V, F32)
    x[g.permutation(V)[:V // 2]] = -200.0
    return x


#: name -> (smallest V the family can be built at, (V, rng) -> fp32 row).  Every row here has a finite maximum and no NaN.
FAMILIES = {
    "randn3": (1, lambda V, g: _randn(V, g, 3.0)),
    "offset+1e4": (1, lambda V, g: _randn(V, g, 3.0) + F32(1e4)),
    "offset-1e4": (1, lambda V, g: _randn(V, g, 3.0) - F32(1e4)),
    "offset+1e30": (1, lambda V, g: _randn(V, g, 3.0) + F32(1e30)),
    "offset-1e30": (1, lambda V, g: _randn(V, g, 3.0) - F32(1e30)),
    "dominant": (2, _dominant),
    "uniform": (1, lambda V, g: np.full(V, 0.25, F32)),
    "uniform_negzero": (1, lambda V, g: np.full(V, -0.0, F32)),
    "two_level": (2, _two_level),
    "underflow": (2, lambda V, g: _randn(V, g, 40.0)),
    "masked": (3, _masked),
    "tie_63_64": (65, lambda V, g: _tie(V, g, 63, 64)),               # last lane of wave 0, first lane of wave 1
    "tie_191_192": (193, lambda V, g: _tie(V, g, 191, 192)),           # the seam in front of the wave reduced last
    "tie_255_256": (257, lambda V, g: _tie(V, g, 255, 256)),           # last thread's first, thread 0's second element
    "tie_i_i256": (257, lambda V, g: (lambda i: _tie(V, g, i, i + NT))(int(g.integers(V - NT)))),   # one thread's 1st and 2nd
    "tie_last_wave": (262, lambda V, g: _tie(V, g, 200, 261)),         # wave 3 (reduced last) holds the LOWER index
    "tie_last_first": (2, lambda V, g: _tie(V, g, V - 1, 0)),
}
TIES = {"tie_63_64": lambda V: (63, 64), "tie_191_192": lambda V: (191, 192), "tie_255_256": lambda V: (255, 256),
        "tie_last_wave": lambda V: (200, 261), "tie_last_first": lambda V: (0, V - 1)}


def families_at(V: int):
    """The generator leaves out what a V is too short for; nothing is skipped at run time."""
    return [f for f, (vmin, _) in FAMILIES.items() if V >= vmin]


def row(family: str, V: int, seed: int = 0) -> np.ndarray:
    vmin, fn = FAMILIES[family]
    if V < vmin:
        raise ValueError(f"{family} needs V >= {vmin}")
    return np.ascontiguousarray(fn(V, _rng(family, V, seed)), dtype=F32)


def cases():
    return [(f, V) for V in V_EDGES for f in families_at(V)]


def stack(V: int, seed: int = 0):
    names = families_at(V)
    return names, np.stack([row(f, V, seed) for f in names])


def default_target(family: str, x: np.ndarray, seed: int = 0) -> int:
    """An in-range target: a masked word where the row has one (its log-prob is exactly -inf), else a seeded one."""
    if np.isneginf(x).any():
        return int(np.flatnonzero(np.isneginf(x))[0])
    return int(_rng(family + ".tg", len(x), seed).integers(len(x)))


# -------------------------------------------------------------------------------------------------- float64 reference
def reference(x: np.ndarray, target=None):
    """(logp_target or None, sum_logp, argmax, max_logp) of a row with a finite maximum and no NaN, in float64."""
    x = np.asarray(x, F64)
    m = x.max()
    am = int(np.flatnonzero(x == m)[0])                    # lowest index of the maximum
    with np.errstate(invalid="ignore"):
        d = x - m
    lg = math.log(math.fsum(np.exp(d)))
    s = NINF if np.isneginf(d).any() else math.fsum(d) - len(x) * lg
    lt = None if target is None else (NINF if np.isneginf(d[target]) else float(d[target]) - lg)
    return lt, s, am, -lg


def bounds(x: np.ndarray, target=None) -> dict:
    """The module docstring's bounds for this row; 0 where an exact value (-inf) is asked for."""
    x = np.asarray(x, F64)
    V = len(x)
    d = x - x.max()
    fin = np.isfinite(d)
    ad = np.abs(d[fin])
    e = np.exp(d[fin])
    S = math.fsum(e)
    lg = math.log(S)
    a1 = U24 * math.fsum(e * ad) / S
    a2 = EXPF_ULP * 2.0 ** -23
    a3 = (-(-V // NT) + 6 + NWAVES) * U24
    a4 = LOGF_ULP * 2.0 ** -23 * abs(lg)
    a5 = V * 2.0 ** -126
    e_lg = (a1 + a2 + a3 + a5) * (1 + 1e-6) + a4
    out = {"max_logp": e_lg}
    if fin.all():
        sd = math.fsum(ad)
        rest = U24 * sd + V * e_lg + 2.0 ** -50 * (sd + V * abs(lg))
        out["sum_logp"] = rest + U24 * (abs(-sd - V * lg) + rest)
    else:
        out["sum_logp"] = 0.0
    if target is not None:
        if np.isfinite(d[target]):
            out["logp_target"] = U24 * abs(d[target]) + e_lg + U24 * (abs(d[target] - lg) + e_lg)
        else:
            out["logp_target"] = 0.0
    return out


def ratio(got: float, want: float, bound: float) -> float:
    """err / bound; where an exact value is asked for (bound 0 or a reference -inf): 0 if equal, else inf.  NaN -> inf."""
    got, want = float(got), float(want)
    if math.isnan(got):
        return math.inf
    if bound == 0 or not math.isfinite(want):
        return 0.0 if got == want else math.inf
    return abs(got - want) / bound


# ------------------------------------------------------------------------------------------- the kernel, in numpy fp32
def ranks_before(v, i, bv, bi):
    """row_select.h: larger value first, ties to the LOWER index; false whenever a NaN is involved."""
    with np.errstate(invalid="ignore"):
        return (v > bv) | ((v == bv) & (i < bi))


def _thread_scan(x):
    m, mi = np.full(NT, NINF, F32), np.full(NT, INT_MAX, np.int64)
    for t0 in range(0, len(x), NT):
        v = x[t0:t0 + NT]
        n = len(v)
        with np.errstate(invalid="ignore"):
            take = (v > m[:n]) | (mi[:n] == INT_MAX)
        m[:n] = np.where(take, v, m[:n])
        mi[:n] = np.where(take, np.arange(t0, t0 + n), mi[:n])
    return m, mi


def block_argmax(x: np.ndarray):
    """(m, mi) as every thread of token_stats_kernel holds them after block_argmax."""
    m, mi = (a.reshape(NWAVES, WAVE) for a in _thread_scan(np.asarray(x, F32)))
    for o in (32, 16, 8, 4, 2, 1):
        ov, oi = m[:, _LANE ^ o], mi[:, _LANE ^ o]
        take = ranks_before(ov, oi, m, mi)
        m, mi = np.where(take, ov, m), np.where(take, oi, mi)
    best, besti = m[0, 0], mi[0, 0]
    for w in range(1, NWAVES):
        if ranks_before(m[w, 0], mi[w, 0], best, besti):
            best, besti = m[w, 0], mi[w, 0]
    return F32(best), int(besti)


def _block_sum(per_thread: np.ndarray):
    v = per_thread.reshape(NWAVES, WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, _LANE ^ o]
    t = per_thread.dtype.type(0)
    for w in range(NWAVES):
        t = t + v[w, 0]
    return t


def kernel_model(x: np.ndarray, target=None):
    """(logp_target or None, sum_logp, argmax, max_logp, flagged) of one row as token_stats_kernel computes them: fp32
    arithmetic in the kernel's order, exp and log as the correctly rounded fp32 value."""
    x = np.asarray(x, F32)
    V = len(x)
    m, mi = block_argmax(x)
    se, sx = np.zeros(NT, F32), np.zeros(NT, F64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t0 in range(0, V, NT):
            dv = (x[t0:t0 + NT] - m).astype(F32)
            n = len(dv)
            se[:n] = se[:n] + np.exp(dv.astype(F64)).astype(F32)
            sx[:n] = sx[:n] + dv.astype(F64)
        e, dsum = _block_sum(se), _block_sum(sx)
        lg = F32(np.log(F64(e)))
        sum_logp = F32(dsum - F64(V) * F64(lg))
        max_logp = F32(-lg)
        lt, flagged = None, False
        if target is not None:
            if 0 <= target < V:
                lt = F32(F32(x[target] - m) - lg)
            else:
                lt, flagged = F32(0.0), True                  # the flagged-target rule
    return lt, sum_logp, mi, max_logp, flagged


def launch_model(X, targets, status_in: int = 0):
    """A whole launch: per-row outputs and the status word afterwards (OR-ed, never cleared)."""
    rows = [kernel_model(x, None if targets is None else int(t)) for x, t in
            zip(X, targets if targets is not None else [None] * len(X))]
    status = status_in
    if any(r[4] for r in rows):
        status = status | 1
    return rows, status


# ------------------------------------------------------------------------------------------------- non-finite rows
def lanes_hidden_by(lane: int):
    """The lanes of a wave whose pair can reach lane 0 only through `lane` (1..63): a pair travels from lane l to lane 0 by
    clearing l's bits from the top (lane ^ 32 first), and passes `lane` when `lane` is l with some of its top bits cleared
    and all bits below that kept."""
    return [l for l in range(WAVE) if l != lane and any((l & ((1 << b) - 1)) == lane for b in range(1, 7))]


def _with(x, idx, val):
    x = x.copy()
    x[idx] = val
    return x


def _base(V, g):
    return _randn(V, g, 3.0)


#: The non-finite table: what token_stats_kernel gives today, per output.  "nan" / "-inf" are exact classes; arg-max rules:
#:   lowest_max     lowest index of the maximum of the row (a +inf, or -inf everywhere, included)
#:   finite_max     lowest index of the maximum of the words that are not NaN
#:   zero           index 0
#:   emulated       block_argmax(row): the words lanes_hidden_by hides are out of the race
NONFINITE = {
    "masked_target": dict(vmin=3, build=_masked,
                          logp_target="-inf", sum_logp="-inf", max_logp="finite", argmax="lowest_max"),
    "pos_inf_one": dict(vmin=2, build=lambda V, g: _with(_base(V, g), int(g.integers(V)), np.inf),
                        logp_target="nan", sum_logp="nan", max_logp="nan", argmax="lowest_max"),
    "all_neg_inf": dict(vmin=1, build=lambda V, g: np.full(V, NINF, F32),
                        logp_target="nan", sum_logp="nan", max_logp="nan", argmax="zero"),
    "nan_at_0": dict(vmin=2, build=lambda V, g: _with(_base(V, g), 0, np.nan),
                     logp_target="nan", sum_logp="nan", max_logp="nan", argmax="zero"),
    "nan_at_max": dict(vmin=2, build=lambda V, g: (lambda x: _with(x, int(np.argmax(x)), np.nan))(_base(V, g)),
                       logp_target="nan", sum_logp="nan", max_logp="nan", argmax="emulated"),
    "nan_elsewhere": dict(vmin=3, build=lambda V, g: (lambda x: _with(x, int(np.argsort(x[:NT])[0]), np.nan))(_base(V, g)),
                          logp_target="nan", sum_logp="nan", max_logp="nan", argmax="emulated"),
    "nan_second_trip": dict(vmin=257, build=lambda V, g: _with(_base(V, g), NT + int(g.integers(V - NT)), np.nan),
                            logp_target="nan", sum_logp="nan", max_logp="nan", argmax="finite_max"),
}
OUTPUTS = ("logp_target", "sum_logp", "argmax", "max_logp")


def nonfinite_at(V: int):
    return [n for n, c in NONFINITE.items() if V >= c["vmin"]]


def nonfinite_row(name: str, V: int, seed: int = 0) -> np.ndarray:
    return np.ascontiguousarray(NONFINITE[name]["build"](V, _rng(name, V, seed)), dtype=F32)


def nonfinite_argmax(name: str, x: np.ndarray) -> int:
    rule = NONFINITE[name]["argmax"]
    if rule == "zero":
        return 0
    if rule == "lowest_max":
        return int(np.flatnonzero(x == x.max())[0])
    if rule == "finite_max":
        return int(np.flatnonzero(x == np.nanmax(x))[0])
    return block_argmax(x)[1]


def in_class(v: float, cls: str) -> bool:
    v = float(v)
    return {"nan": math.isnan(v), "-inf": v == NINF, "finite": math.isfinite(v)}[cls]


# ------------------------------------------------------------------------------------------------- odic_dec_embed_seq
def dec_embed_ref(tokens, embed, pos_table, scale, dec_len):
    """float64: y [N, T, d] = embed[tok]·scale + pos_table[t], an id outside [0, vocab) embeds as exactly pos_table[t];
    prod [N, T, d] the product alone (its magnitude sets the rounding of a multiply-then-add); row_valid [N, T]."""
    tok = np.asarray(tokens, dtype=object)                     # (ids beyond int64 arithmetic stay what they are)
    N, T = tok.shape
    vocab, d = embed.shape
    e, p = np.asarray(embed, F64), np.asarray(pos_table, F64)
    prod = np.zeros((N, T, d), F64)
    for n in range(N):
        for t in range(T):
            if 0 <= tok[n, t] < vocab:
                prod[n, t] = e[int(tok[n, t])] * float(scale)
    y = prod + p[None, :T]
    valid = (np.arange(T)[None, :] < np.asarray(dec_len)[:, None]).astype(np.int32)
    return y, prod, valid


def ulp32(a):
    """The spacing of fp32 at magnitude |a| (float64 array in, float64 out); the smallest normal's below it."""
    a = np.maximum(np.abs(np.asarray(a, F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)
