"""The six per-row kernels over the vocabulary on hard rows (`-m gpu`): offsets of +-30 and +-1000, a peaked row, rows whose
exp terms underflow, near ties, all-equal rows and rows with masked (-inf) words placed by wave slice — down to fewer finite
words than k.  Rows, float64 references and the derived bounds come from vocab_rows_refs.py (test_vocab_rows_host.py checks
them without a GPU).  One launch per (V, k) with every family stacked as rows.

Every figure is printed before it is asserted, as `vocab-rows <kernel> V=.. k=..: family err/bound, ...`; the worst of them
per kernel and family are kept in profiles/r23_vocab_rows.txt.
"""
import math
import os

import numpy as np
import pytest
import torch

import vocab_rows_refs as VR
from guards import guarded
from vocab_rows_refs import F32, F64, NINF

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_rows_sample.npz")

SHAPES = [(V, k) for V in VR.VS for k in VR.KS if k <= V]
IDS = [f"V{V}-k{k}" for V, k in SHAPES]
T_CONS = 2                                                   # the shortest prefix buffer odic_topk_rows_constrained takes
CONS_SHAPES = [(V, k) for V, k in SHAPES if T_CONS + k <= V]   # it refuses n_banned + T + k > V: V = 1 is not in its plan


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()          # fail loudly if the extension is missing
    return o


_DATA = {}


def data(V, k):
    """Per (V, k), once: the stacked rows, their float64 log-probs and log-sum-exp, on the CPU and the rows on the device."""
    if (V, k) not in _DATA:
        names, X = VR.stack(V, k)
        logp, lse = VR.log_softmax_ref(X)
        _DATA[(V, k)] = dict(names=names, X=X, Xd=X.to(DEV), logp=logp, lse=lse)
    return _DATA[(V, k)]


def report(kernel, V, k, names, r):
    """Prints the worst err / bound per family (r: one figure per row, rows in the order of `names`, any number of
    repetitions per family) and returns the families over 1."""
    r = r.reshape(len(names), -1).max(-1).values.tolist()
    print(f"vocab-rows {kernel} V={V} k={k}: " + ", ".join(f"{f} {v:.3f}" for f, v in zip(names, r)))
    return [(f, v) for f, v in zip(names, r) if not v <= 1.0]


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- odic_logsoftmax_topk
@pytest.mark.parametrize("V,k", SHAPES, ids=IDS)
def test_logsoftmax_topk_hard_rows(ops, V, k):
    D = data(V, k)
    R = len(D["names"])
    lp = torch.full((R, V), float("nan"), device=DEV)
    tv = torch.full((R, k), float("nan"), device=DEV)
    ti = torch.full((R, k), -1, dtype=torch.int32, device=DEV)
    ops.logsoftmax_topk(D["Xd"], V, lp, V, tv, ti, R, V, k)
    lp, tv, ti = lp.cpu(), tv.cpu(), ti.cpu().long()
    want_i = VR.topk_ref(D["X"], k)
    over = report("logsoftmax_topk.logp_out", V, k, D["names"],
                  VR.ratios(lp, D["logp"], VR.bound_lse_form(D["logp"], D["lse"])).max(-1).values)
    assert torch.equal(ti, want_i), [(f, a.tolist(), b.tolist()) for f, a, b in zip(D["names"], ti, want_i)
                                     if not torch.equal(a, b)]
    want_v = torch.gather(D["logp"], 1, want_i)
    over += report("logsoftmax_topk.top_val", V, k, D["names"],
                   VR.ratios(tv, want_v, VR.bound_lse_form(want_v, D["lse"])).max(-1).values)
    assert not bool(torch.isnan(lp).any()) and not bool(torch.isnan(tv).any())
    assert torch.equal(lp == NINF, D["logp"] == NINF) and torch.equal(tv == NINF, want_v == NINF)
    if V == 1:
        assert bool((lp == 0).all()) and bool((tv == 0).all())
    assert not over, over


# ------------------------------------------------------------------------- odic_topk_rows, odic_topk_rows_constrained
def _topk_rows(ops, V, k):
    D = data(V, k)
    L = D["logp"].to(F32)                                     # log-prob rows as a search hands them on, -inf included
    R = L.shape[0]
    tv = torch.full((R, k), float("nan"), device=DEV)
    ti = torch.full((R, k), -1, dtype=torch.int32, device=DEV)
    Ld = L.to(DEV)
    ops.topk_rows(Ld, tv, ti, k)
    return D, L, Ld, tv.cpu(), ti.cpu()


@pytest.mark.parametrize("V,k", SHAPES, ids=IDS)
def test_topk_rows_on_masked_logprob_rows(ops, V, k):
    D, L, _, tv, ti = _topk_rows(ops, V, k)
    want_i = VR.topk_ref(L, k)                                # ranked on the fp32 values the kernel sees
    assert torch.equal(ti.long(), want_i), [(f, a.tolist(), b.tolist()) for f, a, b in zip(D["names"], ti, want_i)
                                            if not torch.equal(a.long(), b)]
    assert torch.equal(bits(tv), bits(torch.gather(L, 1, want_i)))


@pytest.mark.parametrize("V,k", CONS_SHAPES, ids=[f"V{V}-k{k}" for V, k in CONS_SHAPES])
def test_topk_rows_constrained_without_constraint_is_topk_rows(ops, V, k):
    D, L, Ld, tv, ti = _topk_rows(ops, V, k)
    R = L.shape[0]
    tok = torch.zeros(R, T_CONS, dtype=torch.int64, device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    cv = torch.full((R, k), float("nan"), device=DEV)
    ci = torch.full((R, k), -1, dtype=torch.int32, device=DEV)
    ops.topk_rows_constrained(Ld, ops.search_constraints(tok, pos, T_CONS, 0), cv, ci, k)
    assert torch.equal(ci.cpu(), ti) and torch.equal(bits(cv.cpu()), bits(tv))
    assert torch.equal(ci.cpu().long(), VR.topk_ref(L, k))


# -------------------------------------------------------------------------------------------------- odic_token_stats
@pytest.mark.parametrize("V,k", SHAPES, ids=IDS)
def test_token_stats_hard_rows(ops, V, k):
    D = data(V, k)
    X, logp, names = D["X"], D["logp"], D["names"]
    R = len(names)
    am = VR.argmax_ref(X)
    first_masked = torch.where((X == NINF).any(-1), (X == NINF).int().argmax(-1), am)
    targets = dict(peak=am, masked=first_masked, first=torch.zeros(R, dtype=torch.int64),
                   last=torch.full((R,), V - 1, dtype=torch.int64))
    over = []
    for what, tg in targets.items():
        lt, sl, ml = (torch.full((R,), float("nan"), device=DEV) for _ in range(3))
        ax = torch.full((R,), -1, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.token_stats(D["Xd"], V, tg.to(DEV), lt, sl, ax, ml, status, R, V)
        lt, sl, ml, ax = lt.cpu(), sl.cpu(), ml.cpu(), ax.cpu().long()
        assert int(status) == 0
        want_t = torch.gather(logp, 1, tg[:, None])[:, 0]
        over += report(f"token_stats.logp_target[{what}]", V, k, names, VR.ratios(lt, want_t, VR.bound_shifted_form(want_t)))
        assert torch.equal(lt == NINF, want_t == NINF) and not bool(torch.isnan(lt).any())
        if what == "masked":
            has = (X == NINF).any(-1)
            assert bool((lt[has] == NINF).all()) and bool(has.any()) == any(f in VR.MASKED for f in names)
        if what != "peak":
            continue                                          # the other three outputs do not depend on the target
        assert torch.equal(ax, am), (ax.tolist(), am.tolist())
        want_m = torch.gather(logp, 1, am[:, None])[:, 0]
        over += report("token_stats.max_logp", V, k, names, VR.ratios(ml, want_m, VR.bound_shifted_form(want_m)))
        want_s = VR.sum_logp_ref(X)
        over += report("token_stats.sum_logp", V, k, names, VR.ratios(sl, want_s, VR.bound_sum_logp(X)))
        masked = (X == NINF).any(-1)
        assert torch.equal(sl == NINF, masked) and not bool(torch.isnan(sl).any()) and not bool(torch.isnan(ml).any())
        if V == 1:
            assert bool((lt == 0).all()) and bool((ml == 0).all()) and bool((sl == 0).all())
    assert not over, over


# -------------------------------------------------------------------------------------------- odic_ensemble_logprobs
def _ensemble(ops, members):
    out = torch.full(tuple(members[0].shape), float("nan"), device=DEV)
    ops.ensemble_logprobs([m.contiguous().to(DEV) for m in members], out)
    return out.cpu()


def _ens_report(what, M, V, got, members, ref_members=None):
    """got against the float64 ensemble of ref_members (default: members) with the bounds of `members`; prints the worst
    figures of the normal and of the subnormal probabilities and returns (out_ref, p_ref, lower, upper, inside)."""
    out, p = VR.ensemble_ref(ref_members if ref_members is not None else members)
    lo, up = VR.ensemble_bounds(members, out, p)
    d = got.double() - out
    inside = (d <= up) & (-d <= lo) & ~torch.isnan(got)
    rr = torch.where(d >= 0, d / up, torch.where(torch.isinf(lo), torch.zeros_like(d), -d / lo))
    normal = p >= 2.0 ** -120
    print(f"vocab-rows ensemble_logprobs.{what} M={M} V={V}: normal {float(rr[normal].max()):.3f}"
          + (f", below 2^-120 {float(rr[~normal].max()):.3f} ({int((~normal).sum())} words)" if bool((~normal).any()) else ""))
    return out, p, lo, up, inside


@pytest.mark.parametrize("V", VR.ENSEMBLE_VS)
@pytest.mark.parametrize("M", VR.ENSEMBLE_MS)
def test_ensemble_logprobs_hard_rows(ops, M, V):
    # members that disagree: every probability is a normal number
    members, own = VR.ens_disagree(M, V)
    got = _ensemble(ops, members)
    out, p, lo, up, inside = _ens_report("disagree", M, V, got, members)
    assert bool(inside.all()), int((~inside).sum())
    for a in own:
        assert abs(float(got[0, a]) - math.log(1.0 / M)) <= float(up[0, a]), (a, float(got[0, a]))
    # offsets: the shifted members (x + c is exact in fp32 on their grid) give the unshifted ensemble
    shifted, base = VR.ens_offsets(M, V)
    got = _ensemble(ops, shifted)
    _, _, _, _, inside = _ens_report("offsets", M, V, got, base)
    assert bool(inside.all()), int((~inside).sum())
    # underflow: every entry is in one of the three sets
    members = VR.ens_underflow(M, V)
    got = _ensemble(ops, members)
    out, p, lo, up, inside = _ens_report("underflow", M, V, got, members)
    named = p < VR.UNDERFLOW_P
    assert int(named.sum()) >= 1
    assert not bool(torch.isnan(got).any())
    assert bool(((got[named] == NINF) | (got[named] <= VR.UNDERFLOW_OUT_MAX)).all())
    assert bool(((got.double() - out) <= up)[~named].all())                     # never above the reference plus the bound
    assert bool(inside[~named].all()), int((~inside[~named]).sum())              # (lower side: free only where p <= 2^-147)
    # one member masks a word the others keep
    members, w = VR.ens_masked_member(M, V)
    got = _ensemble(ops, members)
    _, _, _, _, inside = _ens_report("masked-member", M, V, got, members)
    assert math.isfinite(float(got[0, w])) and bool(inside.all()), int((~inside).sum())


# -------------------------------------------------------------------------------------------- odic_logsoftmax_sample
SAMPLE_SHAPES = VR.sample_shapes()


@pytest.mark.parametrize("V,k", SAMPLE_SHAPES, ids=[f"V{V}-k{k}" for V, k in SAMPLE_SHAPES])
def test_logsoftmax_sample_hard_rows(ops, V, k):
    names, Xs = VR.sample_stack(V, k)
    X = Xs[::VR.SAMPLE_REPS]
    logp1, lse1 = VR.log_softmax_ref(X)
    S, F, N = VR.SAMPLE_REPS, len(names), Xs.shape[0]
    Xd = Xs.to(DEV)
    pos = torch.full((1,), VR.SAMPLE_POS, dtype=torch.int32, device=DEV)
    runs = []
    for _ in range(2):
        lp, tv, ti = guarded(N, V, V + 1, F32, DEV), guarded(N, k, k, F32, DEV), guarded(N, k, k, torch.int32, DEV)
        ops.logsoftmax_sample(Xd, V, lp.t, V + 1, tv.t, ti.t, N, V, k, VR.SAMPLE_SEED, pos)
        torch.cuda.synchronize()
        for g_, nm in ((lp, "logp_out"), (tv, "top_val"), (ti, "top_idx")):
            g_.assert_untouched(what=f"logsoftmax_sample V={V} k={k} {nm}")
        runs.append((lp.t[:, :V].cpu(), tv.t.cpu(), ti.t.cpu()))
    (lp, tv, ti), (lp2, tv2, ti2) = runs
    assert torch.equal(bits(lp), bits(lp2)) and torch.equal(bits(tv), bits(tv2)) and torch.equal(ti, ti2)
    I = ti.long()
    assert bool((I >= 0).all()) and bool((I < V).all()), (int(I.min()), int(I.max()))      # before anything gathers with it
    srt = I.sort(-1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "a word drawn twice"
    rep = lambda t: t.repeat_interleave(S, 0)                                               # noqa: E731
    logp, lse = rep(logp1), rep(lse1)
    over = report("logsoftmax_sample.logp_out", V, k, names, VR.ratios(lp, logp, VR.bound_lse_form(logp, lse)).max(-1).values)
    want_v = torch.gather(logp, 1, I)
    over += report("logsoftmax_sample.top_val", V, k, names,
                   VR.ratios(tv, want_v, VR.bound_lse_form(want_v, lse)).max(-1).values)
    assert not bool(torch.isnan(lp).any()) and not bool(torch.isnan(tv).any())
    assert torch.equal(lp == NINF, logp == NINF) and torch.equal(tv == NINF, want_v == NINF)
    if V == k:
        assert torch.equal(srt, torch.arange(V).expand(N, V)), "V = k: every word is drawn"
    I3, tv3 = I.reshape(F, S, k), tv.reshape(F, S, k)
    for r, f in enumerate(names):
        x = X[r]
        finite = torch.isfinite(x)
        if f in ("masked_30", "masked_k_one_wave", "masked_k_spread"):
            assert bool(finite[I3[r]].all()), f"{f}: a masked word was drawn"
        if f == "peaked":
            assert bool((I3[r, :, 0] == VR.peak_word(V)).all()), f"{f}: first draws {I3[r, :, 0].tolist()}"
        if f == "masked_short":
            m = VR.short_m(k)
            words = torch.from_numpy(VR.finite_words(f, V, k))
            assert torch.equal(I3[r, :, :m].sort(-1).values, words.expand(S, m)), "the finite words come first"
            fill = torch.nonzero(~finite)[:k - m, 0]
            assert torch.equal(I3[r, :, m:], fill.expand(S, k - m)), "then the masked words by ascending index"
            assert bool((tv3[r, :, m:] == NINF).all()) and bool(torch.isfinite(tv3[r, :, :m]).all())
    # rows with at least k finite words keep the draws of the build before the short-row rule, bit for bit
    G = np.load(GOLDEN)
    p0 = names.index("plain") * S
    assert np.array_equal(ti[p0:p0 + VR.GOLDEN_ROWS].numpy(), G[f"idx_V{V}_k{k}"])
    assert np.array_equal(bits(tv[p0:p0 + VR.GOLDEN_ROWS]).numpy(), G[f"val_V{V}_k{k}"].view(np.int32))
    assert not over, over
