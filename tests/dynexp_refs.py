"""Reference, input families and per-entry bounds for the decoder's dynamic expansion on hard rows: odic_dynexp_step
(csrc/decoder_ops.hip), odic_dynexp_seq (csrc/decoder_seq.hip) and odic_dynexp_fill_caches (csrc/decoder_prefill.hip), shared by
test_dynexp_refs_host.py (no GPU: the reference equals the oracle, every family has the properties it is there for, every bound
is met by a float32 evaluation with the factor below) and test_dynexp_hard_rows_gpu.py (the three kernels against the reference).

The reference restates oracle/expansionnet_ref.py::dynamic_expansion on the five column blocks of `lin` (the families need control
of `lin` that a weight matrix cannot give) and also returns the weight tables.  float64 by default; `dtype=torch.float32` evaluates
the same formula in float32 with every sum taken in REVERSED order, one IEEE addition at a time (elementwise torch operations
only: the figure does not depend on a BLAS or on the vector width of the machine).  A bound is 8 x the largest error of that
evaluation over the family's cases (FACTOR: the kernels group the (t+1)·E-term sums differently and fuse their multiply-adds).
Nothing here is derived from a kernel's output.

Re-ordered searches take their plans from dynexp_step_model.ancestry_plan and materialise histories with
dynexp_step_model.history; there is no second model of the caches here.

Not a conftest and not a test module: import it (`import dynexp_refs as DX`).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

import dynexp_step_model as M

F64, F32 = torch.float64, torch.float32
EPS = 1e-9
N_SEQ = 3                                    # three sequences; a re-ordered search is one image with three beams
SHAPES = {"T20": (20, 128, 4), "T40": (40, 192, 16)}        # (T, d, E): t + 1 crosses 16 / 17 (and 32 / 33 at T = 40)
FAMILIES = ("gauss", "one_sided", "eps_regime", "peaked", "cancel", "probe")
PLANS = ("identity", "reorder")
KEY_CH = 64                                  # the structured families keep keys and qexp on the last 64 channels
MARGIN = 2.0 ** -10                          # every |z| >= MARGIN x its row's largest |z| (sign_margin)
PEAK = 2.0 ** 12
FACTOR = 8.0
CAP = 0.05                                   # share of a case's entries the atol term may take out of the relative comparison
REL_FLOOR = 2.0 ** -8                        # measuring: entries below REL_FLOOR x rowscale are measured against the rowscale

#: Largest error of the float32 reversed-order evaluation over the family's cases (both shapes, identity and re-ordered plan),
#: as test_dynexp_refs_host.py::test_float32_evaluation_meets_every_bound re-measures it: (relative error of the entries at or
#: above REL_FLOOR x rowscale, error of the others as a fraction of the rowscale).  The probe's figures are those of its
#: coefficients (sums of non-negative terms), the others' those of the output rows.  `cancel` is evaluated with the split dot
#: product (qexp·key and cond·key summed separately, as the kernels cache them).
MEASURED = {                         # measured (rel, abs)          -> bound (rtol, atol) = 8 x
    "gauss":      (5.3e-05, 2.7e-07),   # 5.262e-05, 2.687e-07          4.24e-04, 2.16e-06
    "one_sided":  (5.6e-05, 3.9e-07),   # 5.568e-05, 3.863e-07          4.48e-04, 3.12e-06
    "eps_regime": (3.3e-05, 2.9e-07),   # 3.237e-05, 2.808e-07          2.64e-04, 2.32e-06
    "peaked":     (4.3e-05, 3.1e-07),   # 4.243e-05, 3.007e-07          3.44e-04, 2.48e-06
    "cancel":     (1.9e-04, 1.6e-06),   # 1.801e-04, 1.575e-06          1.52e-03, 1.28e-05   (split dot product)
    "probe":      (1.9e-06, 2.0e-09),   # 1.866e-06, 1.956e-09          1.52e-05, 1.60e-08   (per coefficient)
}
#: (rtol, atol) = FACTOR x MEASURED:  |got − want| <= rtol·|want| + atol·rowscale, rowscale = the row's largest |want|
BOUNDS = {f: (FACTOR * r, FACTOR * a) for f, (r, a) in MEASURED.items()}


# =====================================================================================================================
# the reference
# =====================================================================================================================
def _rdot(a, b):
    """Σ_c a[..., c]·b[..., c] (broadcast), channels in descending order, one rounding per product and per addition."""
    acc = None
    for c in range(a.shape[-1] - 1, -1, -1):
        p = a[..., c] * b[..., c]
        acc = p if acc is None else acc + p
    return acc


def _rsum(x):
    """Σ over the last axis in descending order, one rounding per addition."""
    acc = x[..., -1]
    for i in range(x.shape[-1] - 2, -1, -1):
        acc = acc + x[..., i]
    return acc


def _normalise(x, s, eps, norm):
    """x / (s + eps) as the reference has it; the other forms are the wrong kernels test_dynexp_refs_host.py must see fail."""
    if norm == "plus":
        return x / (s + eps)
    if norm == "max":
        return x / torch.clamp(s, min=eps)
    if norm in ("none", "guard"):                         # eps dropped; `guard` is s > 0 ? 1/s : 0 (0/0 taken as 0 in both)
        return torch.where(s > 0, x / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(x))
    raise ValueError(norm)


def dynexp_ref(cond, key, va, vb, sel, qexp, bexp, lens, eps=EPS, dtype=F64, split=False, norm="plus", last_only=False):
    """oracle/expansionnet_ref.py::dynamic_expansion on the column blocks of lin.  cond, key, va, vb, sel [N, T, d]; qexp, bexp
    [E, d]; lens [N] (positions >= lens[n] are padded: masked as rows and as columns).
    Returns (out [N, T, d], tables): out is what the block adds to y (0 on padded rows); tables holds
      z [N, T, E, T]   z[n, a, e, b] = (qexp[e] + cond_a)·key_b / sqrt(d), unmasked
      wfa, wfb [N, T, E, T]   forward weights of position t's query e over the keys i <= t
      wba, wbb [N, T, T, E]   backward weights of output position t over (j <= t, e)
      qk [N, T, E]     qexp[e]·key_t;  sfa, sfb [N, T, E] and sba, sbb [N, T] the normalisers before eps.
    dtype float32: the same formula in float32, sums in reversed order (split: qexp·key and cond·key summed separately, the
    form the kernels cache).  last_only: out and wba / wbb for the last position only ([N, 1, ...]): a step of a search."""
    N, T, d = cond.shape
    E = qexp.shape[0]
    c, k, a, b, s, qe, be = (v.to(dtype) for v in (cond, key, va, vb, sel, qexp, bexp))
    f32 = dtype == F32
    if f32:
        qk = _rdot(qe[None, None, :, :], k[:, :, None, :])                               # [N, Tb, E]
        if split:
            ck = _rdot(c[:, :, None, :], k[:, None, :, :])                               # [N, Ta, Tb]
            z = qk.transpose(1, 2)[:, None, :, :] + ck[:, :, None, :]
        else:
            z = _rdot((qe[None, None] + c[:, :, None])[:, :, :, None, :], k[:, None, None, :, :])
    else:
        qk = torch.einsum("ed,ntd->nte", qe, k)
        z = torch.einsum("naed,nbd->naeb", qe[None, None] + c[:, :, None], k)
    z = z / math.sqrt(d)
    t_idx = torch.arange(T)
    valid = t_idx[None, :] < torch.as_tensor(lens)[:, None]                              # [N, T]
    causal = (t_idx[:, None] >= t_idx[None, :])[None] & valid[:, :, None] & valid[:, None, :]     # [N, t, i<=t]
    m1 = causal[:, :, None, :].to(dtype)
    pos, neg = torch.relu(z) * m1, torch.relu(-z) * m1
    sfa, sfb = (_rsum(pos), _rsum(neg)) if f32 else (pos.sum(-1), neg.sum(-1))
    wfa, wfb = _normalise(pos, sfa[..., None], eps, norm), _normalise(neg, sfb[..., None], eps, norm)
    rows = slice(T - 1, T) if last_only else slice(0, T)
    zt = z.permute(0, 3, 1, 2)[:, rows]                                                  # [N, t, j, e]
    m2 = causal[:, rows, :, None].to(dtype)
    pb, nb = torch.relu(zt) * m2, torch.relu(-zt) * m2
    R = pb.shape[1]
    if f32:
        sba, sbb = _rsum(pb.reshape(N, R, T * E)), _rsum(nb.reshape(N, R, T * E))
    else:
        sba, sbb = pb.sum((-1, -2)), nb.sum((-1, -2))
    wba, wbb = _normalise(pb, sba[..., None, None], eps, norm), _normalise(nb, sbb[..., None, None], eps, norm)
    Bv = be[None, None] + c[:, :, None, :]                                               # [N, T, E, d]
    if f32:
        A = Bm = None
        for i in range(T - 1, -1, -1):
            pa, pm = wfa[..., i, None] * a[:, None, None, i, :], wfb[..., i, None] * b[:, None, None, i, :]
            A, Bm = (pa, pm) if A is None else (A + pa, Bm + pm)
        A, Bm = (A + Bv).reshape(N, T * E, d), (Bm + Bv).reshape(N, T * E, d)
        fa, fb = wba.reshape(N, R, T * E), wbb.reshape(N, R, T * E)
        A2 = B2 = None
        for q in range(T * E - 1, -1, -1):
            pa, pm = fa[:, :, q, None] * A[:, None, q, :], fb[:, :, q, None] * Bm[:, None, q, :]
            A2, B2 = (pa, pm) if A2 is None else (A2 + pa, B2 + pm)
    else:
        A = torch.einsum("njei,nid->njed", wfa, a) + Bv
        Bm = torch.einsum("njei,nid->njed", wfb, b) + Bv
        A2 = torch.einsum("ntje,njed->ntd", wba, A)
        B2 = torch.einsum("ntje,njed->ntd", wbb, Bm)
    sg = torch.sigmoid(s[:, rows])
    sg = torch.where(s[:, rows] <= -100.0, torch.zeros_like(sg), sg)      # float32 sigma is exactly 0 there (e^100 overflows): the
                                                                          # probe rests on it, and 4e-44 of a row is no reference
    out = sg * A2 + (1 - sg) * B2
    return out, dict(z=z, wfa=wfa, wfb=wfb, wba=wba, wbb=wbb, qk=qk, sfa=sfa, sfb=sfb, sba=sba, sbb=sbb)


def coefficients(tabs):
    """The coefficients of the re-associated sum (csrc/decoder_ops.hip), from the reference's tables alone:
    ca[n, t, i] = Σ_{j, e} wba[t, j, e]·wfa[j, e, i] (cb), wja[n, t, j] = Σ_e wba (wjb), wea[n, t, e] = Σ_j wba (web).
    With last_only tables t is the last position only."""
    out = {}
    for x in "ab":
        wb, wf = tabs["wb" + x], tabs["wf" + x]
        out["c" + x] = torch.einsum("ntje,njei->nti", wb, wf)
        out["wj" + x] = wb.sum(-1)
        out["we" + x] = wb.sum(2)
    return out


# =====================================================================================================================
# plans and cases
# =====================================================================================================================
def identity_plan(T, N=N_SEQ) -> M.Plan:
    """Every slot descends from itself, nobody finishes; entries of anc at positions >= t hold the sentinel."""
    par = np.tile(np.arange(N, dtype=np.int32), (T - 1, 1))
    anc = np.full((T, N, T), M.SENTINEL, np.int32)
    for t in range(T):
        anc[t, :, :t] = np.arange(N, dtype=np.int32)[:, None]
    return M.Plan(1, N, T, par, anc, np.ones((T, N), np.int32))


_PLANS = {}


def plan_of(shape: str, kind: str) -> M.Plan:
    if (shape, kind) not in _PLANS:
        T = SHAPES[shape][0]
        _PLANS[shape, kind] = identity_plan(T) if kind == "identity" else M.ancestry_plan(1, N_SEQ, T, seed=40 + T)
    return _PLANS[shape, kind]


class Data(NamedTuple):
    family: str
    shape: str
    plan: str
    lin: torch.Tensor            # [N, T, 5d] float32, indexed [slot][position]
    qexp: torch.Tensor           # [E, d]
    bexp: torch.Tensor           # [E, d]
    plant_key: torch.Tensor      # [N, T] the scale a key row was multiplied by (peaked: 2^12 on the planted row; eps_regime: the level), float64
    plant_cond: torch.Tensor     # [N, T] the same for a planted cond row
    extra: dict                  # gauss: sd (the weights) and x

    @property
    def dims(self):
        return SHAPES[self.shape]

    def blocks(self, lin=None):
        lin = self.lin if lin is None else lin
        d = self.dims[1]
        return tuple(lin[..., i * d:(i + 1) * d] for i in range(5))


def _gen(*key):
    """A generator seeded by the key's text (not by hash(): that differs from process to process)."""
    return torch.Generator().manual_seed(sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key)))


def _structured(family, shape):
    """The structured families.  With kb = d − 64: qexp[e] = alpha·e_{kb+e}; key rows live on channels kb..kb+E:
    key[kb+e] = f·u[e] (|u| in [1, 2]), key[kb+E] = f·kappa, |kappa| in [1/16, 1/8]; cond[kb+E] = gamma, |gamma| in [1, 2] (not in the probe).  Then
        z[a, e, b]·sqrt(d) = f_b·(alpha·u_b[e] + gamma_a·kappa_b)
    for ANY slot a slot b is paired with: the families' properties hold in every history a re-ordered search can form."""
    T, d, E = SHAPES[shape]
    N, kb = N_SEQ, d - KEY_CH
    g = _gen(family, shape)

    def rnd(*s):
        return torch.randn(*s, generator=g)

    def uni(*s):
        return torch.rand(*s, generator=g)

    sign = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
    alpha = 8.0 if family == "cancel" else 1.0
    u = (1 + uni(N, T, E)) * sign(N, T, E)
    kappa = (1 + uni(N, T)) / 16 * sign(N, T)
    gamma = (1 + uni(N, T)) * sign(N, T)
    f = torch.ones(N, T)
    pk, pc = torch.ones(N, T, dtype=F64), torch.ones(N, T, dtype=F64)
    cond, va, vb, sel = rnd(N, T, d), rnd(N, T, d), rnd(N, T, d), rnd(N, T, d)
    cond[:, :, kb:] = 0
    key = torch.zeros(N, T, d)
    qexp, bexp = torch.zeros(E, d), 0.3 * rnd(E, d)
    qexp[torch.arange(E), kb + torch.arange(E)] = alpha

    if family == "one_sided":
        # slot 0: query 0 scores negative and query 1 positive on every key; slot 2: query 2 negative on every key
        u[0, :, 0], u[0, :, 1], u[2, :, 2] = -u[0, :, 0].abs(), u[0, :, 1].abs(), -u[2, :, 2].abs()
        # slot 1: every query scores positive on the keys of positions 0, T//2 and T-1, so every backward score of those
        # positions is positive (nb all zeros, B2 = 0): the key sits in the first, a middle and the last slot of the history
        for t in (0, T // 2, T - 1):
            u[1, t] = u[1, t].abs()
    elif family == "eps_regime":
        # five levels of the key scale: slot 0 holds 1e-11 on its first half and 1e-10 on its second, slot 1 holds 1e-9, slot 2
        # 1e-7 then 1e-8.  A score is level·(8/T)·(alpha·u + gamma·kappa)/1: a forward normaliser (1 to T/4 terms) lies between
        # 0.3 and 3 times the level, a backward one (up to (t+1)·E/2 terms) above it by up to that count
        half = (torch.arange(T) >= T // 2).long()
        level = torch.stack([torch.tensor([1e-11, 1e-10])[half], torch.tensor([1e-9, 1e-9])[half], torch.tensor([1e-7, 1e-8])[half]])
        f = level * (math.sqrt(d) * 8.0 / T)
        pk = f.double()                                       # (a key row's level is its scale: divided out by sign_margin)
    elif family == "peaked":
        f[:, T // 3] = PEAK                                   # every forward row from T//3 on peaks on that key
        pk[:, T // 3] = PEAK
        gamma[:, T // 2] *= 16 * PEAK                         # gamma·kappa = 2^12·(1..4): every backward row from T//2 on peaks
        pc[:, T // 2] = 16 * PEAK                             # on that cond row
        # that cond row is also an output term: the other terms are raised to 2^15 so that its channel does not set the rowscale
        cond[:, :, :kb] *= 2.0 ** 15
        va, vb, bexp = va * 2.0 ** 15, vb * 2.0 ** 15, bexp * 2.0 ** 15
    elif family == "probe":
        amp = 0.5
        cond.zero_(), va.zero_(), vb.zero_(), bexp.zero_()
        ar = torch.arange(T)
        va[:, ar, ar] = 1.0
        vb[:, ar, ar] = 1.0
        cond[:, ar, T + ar] = amp
        bexp[torch.arange(E), 2 * T + torch.arange(E)] = 1.0
        sel = torch.where((torch.arange(N)[:, None] + ar[None, :]) % 2 == 0, 100.0, -100.0)[:, :, None].expand(N, T, d).contiguous()
        kappa.zero_()
    key[:, :, kb:kb + E] = f[:, :, None] * u
    if family != "probe":
        key[:, :, kb + E] = f * kappa
        cond[:, :, kb + E] = gamma
    if family == "cancel":
        # cond rows carry the common component −Q0 and qexp rows +Q0 on the dense channels; the dense part of every key is
        # ±2^10·Q0/|Q0|² plus noise orthogonal to Q0: qexp[e]·key = ±2^10 + alpha·u, cond·key = ∓2^10 + gamma·kappa
        q0 = rnd(kb)
        qexp[:, :kb] = q0
        cond[:, :, :kb] = -q0
        noise = rnd(N, T, kb).double()
        noise = noise - (noise @ q0.double())[..., None] * q0.double() / (q0.double() @ q0.double())
        dense = sign(N, T).double()[..., None] * 2.0 ** 10 * q0.double() / (q0.double() @ q0.double()) + noise
        key[:, :, :kb] = dense.float()
    lin = torch.cat([cond, key, va, vb, sel], -1).contiguous()
    return lin, qexp, bexp, pk, pc


def _gauss(shape, plan: M.Plan):
    """Today's data: lin = x·Wᵀ + b in float64, rounded once, x and the weights standard normal (dynexp_step_model.weights).
    A row of x is re-drawn until none of the scores it completes (its forward rows and its backward row, against the rows
    of its own ancestors in the plan) lies within 1.5·2^-10 of that row's largest: normal data, conditioned on the margin."""
    T, d, E = SHAPES[shape]
    N = plan.N
    sd = M.weights(d, E, 7000 + T)
    sd64 = {k: v.double() for k, v in sd.items()}
    qe = sd64["p.query_exp_vectors.weight"]
    g = _gen("gauss", shape)
    x = torch.zeros(N, T, d)
    lin = torch.zeros(N, T, 5 * d)
    thr = 1.5 * MARGIN
    for t in range(T):
        for n in range(N):
            hist = torch.stack([lin[int(plan.anc[t][n][j]), j] for j in range(t)]).double() if t else torch.zeros(0, 5 * d, dtype=F64)
            hc, hk = hist[:, :d], hist[:, d:2 * d]
            while True:
                cand = torch.randn(128, d, generator=g)
                cl = M.linear_rows(sd64, cand.double()).float()
                c, k = cl[:, :d].double(), cl[:, d:2 * d].double()
                own = torch.einsum("ced,cd->ce", qe[None] + c[:, None], k)                       # [C, E]
                fw = torch.cat([torch.einsum("ced,id->cei", qe[None] + c[:, None], hk), own[:, :, None]], 2).abs()
                bw = torch.cat([torch.einsum("jed,cd->cje", qe[None] + hc[:, None], k), own[:, None, :]], 1).abs().reshape(128, -1)
                ok = ((fw.amin(2) >= thr * fw.amax(2)).all(1)) & (bw.amin(1) >= thr * bw.amax(1))
                if bool(ok.any()):
                    i = int(torch.nonzero(ok)[0])
                    x[n, t], lin[n, t] = cand[i], cl[i]
                    break
    ones = torch.ones(N, T, dtype=F64)
    return lin, sd["p.query_exp_vectors.weight"], sd["p.bias_exp_vectors.weight"], ones, ones, dict(sd=sd, x=x)


_DATA = {}


def data(family: str, shape: str, plan: str = "identity") -> Data:
    """The inputs of a family at a shape (cached; never modified by a test).  The structured families are the same data under
    both plans; gauss is drawn against the plan's ancestry."""
    k = (family, shape, plan if family == "gauss" else "any")
    if k not in _DATA:
        if family == "gauss":
            lin, qe, be, pk, pc, extra = _gauss(shape, plan_of(shape, plan))
        else:
            lin, qe, be, pk, pc = _structured(family, shape)
            extra = {}
        _DATA[k] = (lin, qe, be, pk, pc, extra)
    lin, qe, be, pk, pc, extra = _DATA[k]
    return Data(family, shape, plan, lin, qe, be, pk, pc, extra)


def y_in_of(dt: Data, valid) -> torch.Tensor:
    """y_in [..., d] float32 for rows with the given validity mask: zeros on valid rows — the comparison then sees what the
    block adds, not that sum rounded at the size of y_in — and normal data on padded rows, which must come back bit-equal."""
    T, d, E = dt.dims
    valid = torch.as_tensor(valid).bool()
    r = torch.randn(*valid.shape, d, generator=_gen("y_in", dt.family, dt.shape))
    return torch.where(valid[..., None], torch.zeros(()), r)


# =====================================================================================================================
# reference of a whole search / a whole sequence
# =====================================================================================================================
def sign_margin(z, pk, pc):
    """The smallest |z| / (its row's largest |z|) over the forward rows (t, e) — keys i <= t — and the backward rows t — (j <= t,
    e) — of every sequence, all positions valid.  z [N, T, E, T]; a planted row's power-of-two factor (pk [N, T] by key,
    pc [N, T] by cond row) is divided out first: a score is compared with the scores of its own scale."""
    N, T, E, _ = z.shape
    zn = (z.abs() / (pc[:, :, None, None] * pk[:, None, None, :]))
    tri = torch.tril(torch.ones(T, T, dtype=torch.bool))                                 # [a, b]: b <= a
    inf = torch.tensor(float("inf"), dtype=zn.dtype)
    fw = torch.where(tri[None, :, None, :], zn, inf).amin(3) / torch.where(tri[None, :, None, :], zn, -inf).amax(3)
    zb = zn.permute(0, 3, 1, 2)                                                           # [n, t, j, e]
    bw = torch.where(tri[None, :, :, None], zb, inf).amin((2, 3)) / torch.where(tri[None, :, :, None], zb, -inf).amax((2, 3))
    return float(min(fw.min(), bw.min()))


def _history_blocks(dt: Data, plan: M.Plan, t: int):
    """The five blocks [N, t+1, d] and the plant factors [N, t+1] of the histories the N slots hold at step t."""
    lin = torch.stack([M.history(dt.lin, plan.anc[t], n, t) for n in range(plan.N)])
    pk = torch.stack([M.history(dt.plant_key, plan.anc[t], n, t) for n in range(plan.N)])
    pc = torch.stack([M.history(dt.plant_cond, plan.anc[t], n, t) for n in range(plan.N)])
    return dt.blocks(lin), pk, pc


class SearchRef(NamedTuple):
    out: torch.Tensor        # [T, N, d]    what step t adds to y in slot n (0 where row_valid = 0)
    fw: dict                 # wfa, wfb [T, N, E, T]: the forward weights step t caches (0 at i > t); qk [T, N, E]
    coef: dict               # ca, cb, wja, wjb [T, N, T]; wea, web [T, N, E]: the step's coefficients (0 at i > t)
    margin: float            # sign_margin over every history


_REFS = {}


def search_ref(dt: Data, plan_kind: str, dtype=F64, **kw) -> SearchRef:
    """The reference of a T-step search under the plan: every step's histories are materialised and run through dynexp_ref,
    all positions valid; the last row is the step's.  (Identity plan: the histories are prefixes of one sequence and the
    reference is causal, so one call over the whole sequence gives every step.)  float64 results are cached."""
    k = (dt.family, dt.shape, plan_kind)
    cacheable = dtype == F64 and not kw
    if cacheable and k in _REFS:
        return _REFS[k]
    T, d, E = dt.dims
    plan = plan_of(dt.shape, plan_kind)
    N = plan.N
    out = torch.zeros(T, N, d, dtype=dtype)
    fw = dict(wfa=torch.zeros(T, N, E, T, dtype=dtype), wfb=torch.zeros(T, N, E, T, dtype=dtype), qk=torch.zeros(T, N, E, dtype=dtype))
    coef = {k_: torch.zeros(T, N, T, dtype=dtype) for k_ in ("ca", "cb", "wja", "wjb")}
    coef.update(wea=torch.zeros(T, N, E, dtype=dtype), web=torch.zeros(T, N, E, dtype=dtype))
    margin = float("inf")
    if plan_kind == "identity":
        o, tabs = dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * N, dtype=dtype, **kw)
        out = o.transpose(0, 1).contiguous()
        for n_ in ("wfa", "wfb", "qk"):
            fw[n_] = tabs[n_].transpose(0, 1).contiguous()
        for n_, v in coefficients(tabs).items():
            coef[n_] = v.transpose(0, 1).contiguous()
        margin = sign_margin(tabs["z"].double(), dt.plant_key, dt.plant_cond)
    else:
        for t in range(T):
            blocks, pk, pc = _history_blocks(dt, plan, t)
            o, tabs = dynexp_ref(*blocks, dt.qexp, dt.bexp, [t + 1] * N, dtype=dtype, last_only=True, **kw)
            out[t] = o[:, 0] * torch.from_numpy(plan.valid[t]).to(dtype)[:, None]
            fw["wfa"][t, :, :, :t + 1], fw["wfb"][t, :, :, :t + 1] = tabs["wfa"][:, t], tabs["wfb"][:, t]
            fw["qk"][t] = tabs["qk"][:, t]
            for n_, v in coefficients(tabs).items():
                coef[n_][t, :, :v.shape[-1]] = v[:, 0]
            margin = min(margin, sign_margin(tabs["z"].double(), pk, pc))
    ref = SearchRef(out, fw, coef, margin)
    if cacheable:
        _REFS[k] = ref
    return ref


def seq_ref(dt: Data, lens):
    """float64 reference of the whole-sequence pass with the given lengths: out [N, T, d], 0 on padded rows."""
    return dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, list(lens))[0]


def seq_lens(T):
    return ((T, 1, 0), (T, T // 2, 7))


# =====================================================================================================================
# the comparison
# =====================================================================================================================
def measure(got, want, floor=REL_FLOOR):
    """(largest relative error over the entries with |want| >= floor·rowscale, largest error / rowscale over the others);
    rowscale = the largest |want| of the last axis."""
    got, want = got.double(), want.double()
    rs = want.abs().amax(-1, keepdim=True).expand_as(want)
    err = (got - want).abs()
    big = (want.abs() >= floor * rs) & (want != 0)
    small = ~big & (rs > 0)
    rel = float((err[big] / want.abs()[big]).max()) if bool(big.any()) else 0.0
    ab = float((err[small] / rs[small]).max()) if bool(small.any()) else 0.0
    return rel, ab


def excess(got, want, rtol, atol):
    """|got − want| / (rtol·|want| + atol·rowscale) per entry (float64); 0 where both are exactly 0, inf where got is not
    finite or where want is exactly 0 in a row of zeros and got is not."""
    got, want = got.double(), want.double()
    rs = want.abs().amax(-1, keepdim=True).expand_as(want)
    lim = rtol * want.abs() + atol * rs
    err = (got - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / lim)                           # (x / 0 = inf for x > 0)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))


def assert_entries(got, want, family, what, names, bounds=None):
    """Every entry within the family's bound; the failure names the worst entry through names(index tuple).  Prints the
    largest excess ratio (1 = at the bound).  Returns it."""
    rtol, atol = BOUNDS[family] if bounds is None else bounds
    r = excess(got, want, rtol, atol)
    worst = float(r.max()) if r.numel() else 0.0
    print(f"{what}: worst entry at {worst:.3f} of its bound (rtol {rtol:.2e}, atol {atol:.2e})")
    if worst > 1.0:
        idx = tuple(int(v) for v in np.unravel_index(int(r.argmax()), r.shape))
        nbad = int((r > 1.0).sum())
        raise AssertionError(f"{what}: {nbad} entries beyond the bound; worst at {names(idx)}: got {float(got[idx]):.9e}, want "
                             f"{float(want[idx]):.9e}, {worst:.3g} x the bound (rtol {rtol:.2e}, atol {atol:.2e})")
    return worst


def atol_share(want, rtol, atol):
    """Share of the non-zero entries whose bound is mostly the atol term (atol·rowscale > rtol·|want|): the entries the atol
    term takes out of the relative comparison."""
    want = want.double()
    rs = want.abs().amax(-1, keepdim=True).expand_as(want)
    nz = want != 0
    return float(((atol * rs > rtol * want.abs()) & nz).sum()) / max(1, int(nz.sum()))


def compared(dt: Data, plan_kind: str, out, ref: SearchRef, live=None):
    """(got, want) of a search's outputs [T, N, d] as the family is compared: the output rows themselves, or for the probe the
    decoded coefficients against the reference's (concatenated c | wj | we).  live [T, N]: the rows that are compared (default:
    the plan's row_valid); the reference is zero on the others and `out` must be."""
    T, d, E = dt.dims
    live = torch.from_numpy(plan_of(dt.shape, plan_kind).valid) if live is None else torch.as_tensor(live)
    live = live.bool()[..., None]
    if dt.family != "probe":
        return out, torch.where(live, ref.out, torch.zeros((), dtype=ref.out.dtype))
    got = probe_decode(out, T, E)
    want = probe_want(ref.coef, probe_branch(dt).T)
    return (torch.cat([got[k] for k in PROBE_KINDS], -1),
            torch.cat([torch.where(live, want[k], torch.zeros((), dtype=want[k].dtype)) for k in PROBE_KINDS], -1))


def measure_case(family, shape, plan_kind, **kw):
    """measure() of the float32 reversed-order evaluation of one case against the float64 reference."""
    dt = data(family, shape, plan_kind)
    ref = search_ref(dt, plan_kind)
    f32 = search_ref(dt, plan_kind, dtype=F32, split=(family == "cancel"), **kw)
    return measure(*compared(dt, plan_kind, f32.out, ref))


# =====================================================================================================================
# the probe
# =====================================================================================================================
PROBE_KINDS = ("c", "wj", "we")


def probe_decode(y, T, E):
    """Output rows [..., d] of a probe input → {c: [..., T], wj: [..., T], we: [..., E]}: channel i is ca[i] (cb[i] on a
    B-branch row), channel T + j is amp·wja[j], channel 2T + e is wea[e]."""
    amp = 0.5
    return dict(c=y[..., :T], wj=y[..., T:2 * T] / amp, we=y[..., 2 * T:2 * T + E])


def probe_branch(dt: Data):
    """[N, T] bool: True where the selector is +100 (sigma rounds to 1: the A branch)."""
    d = dt.dims[1]
    return dt.lin[:, :, 4 * d] > 0


def probe_want(coef, branch_a):
    """The coefficient tables of the branch each row takes.  coef values and branch_a share their leading axes."""
    return {k: torch.where(branch_a[..., None], coef[k + "a"], coef[k + "b"]) for k in PROBE_KINDS}


def entry_name(dt: Data, idx) -> str:
    """(step, slot, column) of a compared search → the words a failure carries."""
    t, n, c = idx
    if dt.family != "probe":
        return f"sequence {n}, step {t}, channel {c}"
    T, d, E = dt.dims
    x = "a" if bool(probe_branch(dt)[n, t]) else "b"
    kind, i = (f"c{x}", c) if c < T else ((f"wj{x}", c - T) if c < 2 * T else (f"we{x}", c - 2 * T))
    return f"sequence {n}, step {t}, {kind}[{i}]"


def assert_search(dt: Data, plan_kind: str, out, ref: SearchRef, what: str, live=None):
    """A search's outputs [T, N, d] (what each step added to y) against the reference, entry by entry, with the family's bound;
    the probe is compared coefficient by coefficient, and where the reference's coefficient is exactly 0 so must the channel be."""
    got, want = compared(dt, plan_kind, out, ref, live)
    if dt.family == "probe":
        stray = (want == 0) & (got != 0)
        if bool(stray.any()):
            idx = tuple(int(v) for v in torch.nonzero(stray)[0])
            raise AssertionError(f"{what}: {entry_name(dt, idx)} is {float(got[idx]):.3e} where the reference weight is exactly 0")
    return assert_entries(got, want, dt.family, what, lambda idx: entry_name(dt, idx))


assert_probe = assert_search
