"""References, inputs and case lists for two decoder kernels on hard rows: the fp32 skinny GEMM with the LayerNorm of its A
operand folded in (csrc/gemm_f32.hip, odic_gemm with ln_colsum) and the cross-attention step (csrc/decoder_ops.hip,
odic_cross_attn_step), shared by test_decoder_refs_host.py (no GPU: the references agree with independent formulations, every
recorded float32 error reproduces, every bound is met by a float32 evaluation of the same formula) and
test_decoder_hard_rows_gpu.py (the HIP kernels against the references).

The references are plain torch, float64 by default; `dtype=torch.float32` evaluates the same formula in float32 on the CPU.
The error of that evaluation, relative to the case's output scale, stands beside every case (`hard_err`, `f32_err`): the GPU
bound of a hard row is max(project bound, 4 x that figure), the rule of frontend_refs.layernorm_offset_bound (the factor covers
another summation order, not a one-pass variance).  Nothing here is derived from a kernel's output.

Not a conftest: import it (`import decoder_refs as DR`), like frontend_refs.py.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from frontend_refs import F32, F64, _randn, assert_within, max_err  # noqa: F401  (re-exported for the two test files)

ACT_RELU = 2

# =====================================================================================================================
# folded-LayerNorm GEMM
# =====================================================================================================================
#: the project's bound for the folded form (test_gemm_f32_folded_layernorm), relative to the output's largest magnitude
FOLD_BOUND = 3e-5
FOLD_EPS = 1e-5
FOLD_TILE_CFGS = (-1, 0, 1, 2)
FOLD_CONST = 3.0
FOLD_OUTLIER = 1e4

#: the hard rows of every case, in the order of FoldCase.hard_err.  Rows 1..7 and the last row (in the ragged last row tile
#: when M is no multiple of 16); every other row is randn at scale 3.
HARD_KINDS = ("const", "zero", "plus30", "minus30", "outlier_first", "outlier_last", "tiny", "tail_plus30")


class FoldCase(NamedTuple):
    M: int
    N: int
    K: int
    act: int
    residual: bool
    hard_err: Tuple[float, ...]     # float32 CPU layer_norm + matmul against float64 on each hard row (HARD_KINDS order), relative
                                    # to the case's scale, as test_fold_hard_row_errors_are_recorded measured it

    @property
    def name(self):
        return f"M{self.M}_N{self.N}_K{self.K}" + ("_relu_residual" if self.act or self.residual else "")


#: measured on x86-64 (torch's CPU layer_norm and sgemm): 1e-8 to 1.1e-6, so four times the figure stays under 3e-5 and every hard
#: row's bound is the project's 3e-5
FOLD_CASES = [
    FoldCase(17, 100, 64, 0, False, (1.463e-08, 1.463e-08, 2.563e-07, 1.679e-07, 1.981e-07, 4.992e-08, 3.639e-08, 1.940e-07)),
    FoldCase(48, 200, 512, 0, False, (1.779e-08, 1.779e-08, 7.855e-07, 7.435e-07, 4.749e-07, 4.723e-08, 5.955e-08, 2.386e-07)),
    FoldCase(144, 512, 512, 0, False, (2.037e-08, 2.037e-08, 8.995e-07, 8.559e-07, 6.547e-07, 6.008e-08, 7.190e-08, 2.943e-07)),
    FoldCase(100, 1000, 512, 0, False, (2.984e-08, 2.984e-08, 9.484e-07, 9.025e-07, 5.562e-07, 1.214e-07, 9.174e-08, 4.976e-07)),
    FoldCase(192, 64, 512, 0, False, (2.143e-08, 2.143e-08, 9.879e-07, 1.061e-06, 5.204e-07, 1.004e-07, 4.724e-08, 3.379e-07)),
    FoldCase(48, 200, 512, ACT_RELU, True, (2.050e-08, 2.332e-08, 7.574e-07, 8.185e-07, 2.557e-07, 4.038e-08, 6.307e-08, 2.593e-07)),
]


def fold_hard_rows(M):
    """kind -> row index."""
    rows = {k: i + 1 for i, k in enumerate(HARD_KINDS[:-1])}
    rows[HARD_KINDS[-1]] = M - 1
    return rows


def fold_inputs(c: FoldCase):
    """buf [M, 3K] (NaN outside columns K..2K, which hold the rows: the engine's residual-stream layout, lda = 3K), W [N, K],
    bias [N], gamma, beta [K], residual [M, N] or None (float32, CPU)."""
    x = _randn(c.M, c.K, seed=300 + c.M) * 3.0
    r = fold_hard_rows(c.M)
    x[r["const"]] = FOLD_CONST
    x[r["zero"]] = 0.0
    x[r["plus30"]] = _randn(c.K, seed=301) + 30.0
    x[r["minus30"]] = _randn(c.K, seed=302) - 30.0
    x[r["outlier_first"], 0] = FOLD_OUTLIER
    x[r["outlier_last"], c.K - 1] = FOLD_OUTLIER
    x[r["tiny"]] = _randn(c.K, seed=303) * 1e-3            # variance 1e-6 against eps = 1e-5
    x[r["tail_plus30"]] = _randn(c.K, seed=304) + 30.0
    buf = torch.full((c.M, 3 * c.K), float("nan"))
    buf[:, c.K:2 * c.K] = x
    W, b = _randn(c.N, c.K, seed=310) * 0.1, _randn(c.N, seed=311)
    gamma, beta = 1 + 0.1 * _randn(c.K, seed=312), 0.1 * _randn(c.K, seed=313)
    res = _randn(c.M, c.N, seed=314) if c.residual else None
    return buf, W, b, gamma, beta, res


def fold_rows(buf, K):
    return buf[:, K:2 * K]


def fold_ref(c: FoldCase, buf, W, b, gamma, beta, res, dtype=F64):
    """act(LayerNorm(x)·Wᵀ + b) + residual: the unfused pair."""
    x = fold_rows(buf, c.K).to(dtype)
    y = F.layer_norm(x, (c.K,), gamma.to(dtype), beta.to(dtype), FOLD_EPS) @ W.to(dtype).T + b.to(dtype)
    if c.act == ACT_RELU:
        y = torch.relu(y)
    return y + res.to(dtype) if res is not None else y


FOLD_ALPHA = 0.5


def fold_alpha_ref(c: FoldCase, buf, W, b, gamma, beta, res, alpha=FOLD_ALPHA):
    """The header's formula for alpha != 1, float64: rstd·(alpha·a·W'ᵀ − mean·colsum) + bias' (no activation, no residual)."""
    x = fold_rows(buf, c.K).double()
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(1, keepdim=True) + FOLD_EPS)
    Wg = W.double() * gamma.double()[None, :]
    return rstd * (alpha * (x @ Wg.T) - mean * Wg.sum(1)[None, :]) + fold_bias_prime(W, b, beta)


def fold_bias_prime(W, b, beta):
    """bias' = b + W·beta (float64): what a constant row must give before the activation."""
    return b.double() + W.double() @ beta.double()


def fold_row_bound(c: FoldCase, kind: str) -> float:
    return max(FOLD_BOUND, 4.0 * c.hard_err[HARD_KINDS.index(kind)])


def fold_emulate(c: FoldCase, buf, W, b, gamma, beta, res, form: str, slices: int = 8):
    """A float32 CPU evaluation of the folded product rstd·(…) + bias' with W' = W·diag(gamma), colsum = Σ_k W', in one of three
    forms (the arithmetic of each, not a kernel's summation order):
      "one_pass"  mean = Σa/K, var = Σa²/K − mean², (a·W'ᵀ − mean·colsum)·rstd
      "pairwise"  per K-slice moments about the slice's own mean, merged with the pairwise update; the product as above
      "centred"   the kernel's: every slice centred on c_s = the mean of its first round of loads (its first 64 elements at
                  the most); slice moments from Σ(a − c_s) and Σ(a − c_s)², merged with the pairwise update; the product on
                  a − c_s plus (c_s − mean)·(the slice's column sums)
    """
    x = fold_rows(buf, c.K).contiguous()
    K = c.K
    Wg = (W.double() * gamma.double()[None, :]).float()
    bp = fold_bias_prime(W, b, beta).float()
    colsum = Wg.double().sum(1).float()
    slices = max(1, min(slices, K // 16))
    xs, ws = x.view(c.M, slices, K // slices), Wg.view(c.N, slices, K // slices)
    if form == "one_pass":
        mean = x.sum(1) / K
        var = torch.clamp((x * x).sum(1) / K - mean * mean, min=0.0)
    else:
        n_s = float(K // slices)
        if form == "centred":
            cs = xs[:, :, :64].mean(2)                                # [M, slices]
            d = xs - cs[:, :, None]
            sd = d.sum(2)
            ms, m2s = cs + sd / n_s, torch.clamp((d * d).sum(2) - sd * sd / n_s, min=0.0)
        else:
            ms = xs.mean(2)
            m2s = ((xs - ms[:, :, None]) ** 2).sum(2)
        n, mean, m2 = 0.0, torch.zeros(c.M), torch.zeros(c.M)
        for s in range(slices):
            tot, dm = n + n_s, ms[:, s] - mean
            mean = mean + dm * (n_s / tot)
            m2 = m2 + m2s[:, s] + dm * dm * (n * n_s / tot)
            n = tot
        var = m2 / K
    rstd = torch.rsqrt(var + FOLD_EPS)
    if form == "centred":
        prod = torch.einsum("msk,nsk->mn", d, ws) + (cs - mean[:, None]) @ ws.sum(2).T
    else:
        prod = x @ Wg.T - mean[:, None] * colsum[None, :]
    y = prod * rstd[:, None] + bp
    if c.act == ACT_RELU:
        y = torch.relu(y)
    return y + res if res is not None else y


# =====================================================================================================================
# cross-attention step
# =====================================================================================================================
XATTN_BOUND = 2e-5              # test_cross_attn_step
XATTN_F32_CAP = 1e-3            # a planted case whose float32 CPU evaluation errs by more than this measures expf, not the kernel
XATTN_N_IMG = 3
XATTN_GAP = 20.0                # score gap between a planted key and the best other valid key: e^-20 · 2048 keys = 4e-6 of mass
XATTN_MASKED_Q = 2.0            # the q multiple of a plant on a masked key (position >= len)


class XCase(NamedTuple):
    name: str
    beams: int
    S: int
    d: int
    heads: int
    lens: Tuple[int, int, int]
    plants: Tuple[Tuple[int, int, int, int], ...]      # (image, beam, head, key): q of that (row, head) = a multiple of that key
    f32_err: float                                     # the float32 CPU evaluation against float64, relative to the case's scale

    @property
    def dk(self):
        return self.d // self.heads

    @property
    def N(self):
        return XATTN_N_IMG * self.beams


def xattn_keys_per_sweep(dk):
    """cross_attn_step_kernel: dk/16 lanes per key, so a wave sweeps 64/(dk/16) keys; a wave's loop covers 12 sweeps a trip."""
    return 64 // (dk // 16)


def xattn_nb(beams):
    """Beams per block (the NB of the instantiation the entry point picks)."""
    return beams if beams <= 3 else (5 if beams == 5 or beams > 8 else 4)


def _long(S, d, f32_err, beams=3):
    """A key range that reaches the second 12-sweep trip.  lens = (S, S//2 + 1, S − 4); every head of a planted row has its own
    key: key 0, key S − 1, the first key of the 13th sweep (image 0), key len − 1 and a masked key behind it (images 1, 2)."""
    dk = d // 2
    k13 = 12 * xattn_keys_per_sweep(dk)
    assert k13 < S
    l1, l2 = S // 2 + 1, S - 4
    plants = ((0, 0, 0, 0), (0, 0, 1, S - 1), (0, 1, 0, k13), (0, 1, 1, S // 3),
              (1, 0, 0, l1 - 1), (1, 0, 1, l1), (2, 2 % beams, 0, S - 1), (2, 2 % beams, 1, l2 - 1))
    return XCase(f"S{S}_dk{dk}_beams{beams}", beams, S, d, 2, (S, l1, l2), plants, f32_err)


def _beams(beams, f32_err):
    """S = 50, dk = 16: chunk remainders of NB = 4 (beams 4, 6, 8) and NB = 5 (9, 10); plants in image 2's last chunk (key 0,
    key len − 1, a masked key) and in image 0's first."""
    S = 50
    plants = ((2, beams - 1, 0, 0), (2, beams - 1, 1, 45), (2, beams - 2, 0, 47), (2, beams - 2, 1, 23),
              (0, 0, 0, S - 1), (0, 0, 1, 0))
    return XCase(f"S{S}_dk16_beams{beams}", beams, S, 32, 2, (S, 26, 46), plants, f32_err)


#: f32_err as measured (x86-64): 1e-7 to 5e-7 — the planted rows are one-hot to e^-20, so the size of their scores does not
#: reach the output — and every case's bound is the project's 2e-5
XATTN_CASES = [
    _long(193, 128, 3.073e-07), _long(200, 128, 3.193e-07), _long(777, 128, 4.354e-07), _long(385, 64, 1.846e-07),
    _long(769, 32, 2.530e-07),
    _long(2048, 128, 4.198e-07, beams=5),
    _beams(4, 2.248e-07), _beams(6, 2.248e-07), _beams(8, 2.248e-07), _beams(9, 2.248e-07), _beams(10, 2.248e-07),
    # enc_len 0, 1 and S: image 0 averages all S value rows, image 1 returns value row 0
    XCase("S50_dk16_len_0_1_S", 3, 50, 32, 2, (0, 1, 50), ((2, 0, 0, 49), (2, 0, 1, 0), (1, 1, 0, 7)), 1.090e-07),
    XCase("S200_dk64_len_0_1_S", 2, 200, 128, 2, (0, 1, 200), ((2, 0, 0, 199), (2, 0, 1, 192), (0, 0, 1, 3)), 2.170e-07),
]
XATTN_PROBS_CROSS_CHECK = ("S193_dk64_beams3", "S777_dk64_beams3")
XATTN_REFUSED_S = 2049


def xattn_invalid_rows(c: XCase):
    """Rows with row_valid = 0: the last slot of image 0's first chunk and the last slot of image 1's last chunk (never a
    planted row)."""
    return (min(xattn_nb(c.beams), c.beams) - 1, 2 * c.beams - 1)


def xattn_inputs(c: XCase):
    """q [N, d], kv [3, S, 3d] (K at column d, V at 2d, as test_cross_attn_step), enc_len [3], row_valid [N] (CPU).
    V[s, c] = randn + s/8: every key's value row has its own level.  A planted key's K slice is doubled (no other key can then
    out-score it) and q of the (row, head) is the multiple of it that puts it XATTN_GAP above the best other valid key; a plant
    on a masked key takes the multiple XATTN_MASKED_Q, and the softmax over the valid keys is what must come out."""
    S, d, dk = c.S, c.d, c.dk
    q = _randn(c.N, d, seed=400 + c.S)
    kv = _randn(XATTN_N_IMG, S, 3 * d, seed=401 + c.S)
    kv[:, :, 2 * d:] += (torch.arange(S, dtype=torch.float32) / 8.0)[None, :, None]
    lens = torch.tensor(c.lens, dtype=torch.int32)
    valid = torch.ones(c.N, dtype=torch.int32)
    for n in xattn_invalid_rows(c):
        valid[n] = 0
    for img, beam, h, key in c.plants:
        assert 0 <= key < S and 0 <= beam < c.beams and valid[img * c.beams + beam]
        kv[img, key, d + h * dk:d + (h + 1) * dk] *= 2.0
    for img, beam, h, key in c.plants:
        K = kv[img, :, d + h * dk:d + (h + 1) * dk].double()
        if key < c.lens[img]:
            sc = K @ K[key] / math.sqrt(dk)
            other = sc.clone()
            other[key] = -math.inf
            other[c.lens[img]:] = -math.inf
            gap = float(sc[key] - other.max()) if c.lens[img] > 1 else float(sc[key])
            assert gap > 0.25 * float(sc[key]), (c.name, img, h, key)
            mult = XATTN_GAP / gap
        else:
            mult = XATTN_MASKED_Q
        q[img * c.beams + beam, h * dk:(h + 1) * dk] = (mult * K[key]).float()
    return q, kv, lens, valid


def xattn_ref(c: XCase, q, kv, lens, valid, dtype=F64, return_probs=False):
    """The formula of test_cross_attn_step: softmax over all S keys of q·k/sqrt(dk) with the keys behind enc_len and every key of
    an invalid row set to −1e4 (masked_fill), times V.  [N, d]; with return_probs also the probabilities [N, heads, S]."""
    S, d, dk, h = c.S, c.d, c.dk, c.heads
    img = torch.arange(c.N) // c.beams
    K = kv[:, :, d:2 * d].to(dtype).view(XATTN_N_IMG, S, h, dk)
    V = kv[:, :, 2 * d:3 * d].to(dtype).view(XATTN_N_IMG, S, h, dk)
    out = torch.empty(c.N, d, dtype=dtype)
    probs = torch.empty(c.N, h, S, dtype=dtype) if return_probs else None
    allow = (torch.arange(S)[None, :] < lens[img][:, None]) & (valid[:, None] != 0)            # [N, S]
    for i in range(XATTN_N_IMG):
        rows = img == i
        s = torch.einsum("nhc,shc->nhs", q[rows].to(dtype).view(-1, h, dk), K[i]) / math.sqrt(dk)
        p = torch.softmax(s.masked_fill(~allow[rows][:, None, :], -1e4), -1)
        out[rows] = torch.einsum("nhs,shc->nhc", p, V[i]).reshape(-1, d)
        if return_probs:
            probs[rows] = p
    return (out, probs) if return_probs else out


def xattn_bound(c: XCase) -> float:
    return max(XATTN_BOUND, 4.0 * c.f32_err)
