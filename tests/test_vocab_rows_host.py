"""vocab_rows_refs.py checked without a GPU: the float64 references against torch, every row family against the property its
name claims, the ensemble constructions, the plan, and the bounds against a float32 evaluation on the CPU — in both
log-prob forms, and against four mutated restatements that must fall outside them."""
import math

import numpy as np
import pytest
import torch

import vocab_rows_refs as VR
from vocab_rows_refs import F32, F64, NINF

torch.set_grad_enabled(False)

SHAPES = [(V, k) for V in VR.VS for k in VR.KS if k <= V]
IDS = [f"V{V}-k{k}" for V, k in SHAPES]


def test_plan_is_constructible_and_complete():
    P = VR.plan()
    assert len(set(P)) == len(P)
    for f, V, k in P:
        x = VR.row(f, V, k)                                      # raises where the plan lists what cannot be built
        assert x.dtype == F32 and x.shape == (V,) and not bool(torch.isnan(x).any())
        assert bool(torch.isfinite(x).any()), (f, V, k)          # a row without a finite word is outside the contract
    for V, k in SHAPES:
        assert "plain" in VR.families_at(V, k) and "zeros" in VR.families_at(V, k)
    # every family appears, the k-dependent ones on both sides of the k <= 8 threshold path and at a streamed length
    for f in VR.FAMILIES:
        ks = {k for g, V, k in P if g == f}
        assert ks & {1, 5} and ks & {9, 16}, (f, ks)
        assert {V for g, V, k in P if g == f} >= {513, 10240, 10241}, f
    assert set(VR.families_at(1, 1)) == {"plain", "offset+30", "offset-30", "offset+1000", "offset-1000", "ramp", "zeros"}


def test_rows_are_seeded():
    for f, V, k in VR.plan()[::7]:
        a, b = VR.row(f, V, k), VR.row(f, V, k)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("V", VR.VS)
def test_references_against_torch_on_plain(V):
    x = VR.row("plain", V, 1)[None]
    logp, lse = VR.log_softmax_ref(x)
    assert torch.allclose(logp, torch.log_softmax(x.double(), -1), rtol=0, atol=1e-12)
    assert torch.allclose(lse, torch.logsumexp(x.double(), -1), rtol=0, atol=1e-12)
    for k in (1, min(V, 16)):
        assert torch.equal(VR.topk_ref(x, k), torch.topk(x, k, dim=-1).indices)      # no ties in a randn row
    assert int(VR.argmax_ref(x)) == int(x.argmax())
    assert abs(float(VR.sum_logp_ref(x)) - float(torch.log_softmax(x.double(), -1).sum())) < 1e-9 * V


def test_reference_order_breaks_ties_by_index_and_puts_masked_words_last():
    x = torch.tensor([[1.0, NINF, 3.0, 3.0, NINF, 1.0, 3.0]])
    assert VR.topk_ref(x, 7).tolist() == [[2, 3, 6, 0, 5, 1, 4]]
    logp, _ = VR.log_softmax_ref(x)
    assert logp[0, 1] == NINF and logp[0, 4] == NINF and not bool(torch.isnan(logp).any())
    assert abs(float(torch.exp(logp).sum()) - 1) < 1e-14
    # an offset the float64 exp could not take unshifted
    big, _ = VR.log_softmax_ref(torch.tensor([[1000.0, 999.0]]))
    assert torch.allclose(big, torch.log_softmax(torch.tensor([[1.0, 0.0]], dtype=F64), -1), atol=1e-13)


def test_ensemble_reference():
    g = torch.Generator().manual_seed(3)
    ms = [torch.randn(2, 50, generator=g) * 3 for _ in range(3)]
    out, p = VR.ensemble_ref(ms)
    want = torch.stack([torch.softmax(m.double(), -1) for m in ms]).mean(0)
    assert torch.allclose(p, want, rtol=1e-13, atol=0) and torch.allclose(out, want.log(), atol=1e-12)


@pytest.mark.parametrize("V,k", SHAPES, ids=IDS)
def test_families_have_the_property_their_name_claims(V, k):
    names = VR.families_at(V, k)
    R = {f: VR.row(f, V, k) for f in names}
    fin = {f: np.flatnonzero(torch.isfinite(R[f]).numpy()) for f in names}
    for f in names:
        if f not in VR.MASKED:
            assert len(fin[f]) == V, f
    for f in ("offset+30", "offset-30", "offset+1000", "offset-1000"):
        c = float(f[len("offset"):])
        assert torch.equal(R[f], R["plain"] + c) and abs(float(R[f].double().mean()) - c) < 3 * 5.0 / math.sqrt(V)
    if "peaked" in names:
        x, p = R["peaked"], VR.peak_word(V)
        rest = torch.cat([x[:p], x[p + 1:]])
        assert float(x[p]) == float(rest.max() + 60.0)                           # (an fp32 sum)
        logp, _ = VR.log_softmax_ref(x[None])
        assert -1e-22 < float(logp[0, p]) <= 0 and float(logp[0].topk(2).values[1]) < -59.9
        assert int(VR.argmax_ref(x[None])) == p
    if "two_level" in names:
        x = R["two_level"]
        assert bool((x[0::2] == 0).all()) and bool((x[1::2] == -200).all())
        assert bool((torch.exp(x[1::2]) == 0).all())                             # the lower half underflows in fp32 ...
        assert bool((torch.exp(x[1::2].double()) > 0).all())                     # ... and not in float64
    x = R["ramp"]
    if V > 1:
        assert float(x[0]) == -80 and float(x[-1]) == 80 and bool((x[1:] > x[:-1]).all())
    if "near_tie" in names:
        x = R["near_tie"]
        s = torch.sort(x).values
        assert float(s[0]) == 5.0 and bool((s[1:] == torch.nextafter(s[:-1], torch.tensor(9.0))).all())
        assert not bool((x[1:] > x[:-1]).all())                                  # permuted, not a ramp
    assert bool((R["zeros"] == 0).all())
    assert abs(float(VR.log_softmax_ref(R["zeros"][None])[0][0, 0]) + math.log(V)) < 1e-12
    if "masked_30" in names:
        assert V - len(fin["masked_30"]) == int(0.3 * V) and len(fin["masked_30"]) >= k
        keep = fin["masked_30"]
        assert torch.equal(R["masked_30"][keep], R["plain"][keep])
    if "masked_k_one_wave" in names:
        w = fin["masked_k_one_wave"]
        assert len(w) == k and bool((w % 512 < 64).all()) and len(w) < V
        assert bool((VR.wave_of(w) == 0).all())
    if "masked_k_spread" in names:
        w = fin["masked_k_spread"]
        per = np.bincount(VR.wave_of(w), minlength=8)
        assert len(w) == k and len(w) < V and per.max() <= (1 if k <= 8 else 2)
        if V >= 512:
            assert (per > 0).sum() == min(k, 8)
    if "masked_short" in names:
        m = len(fin["masked_short"])
        assert m == VR.short_m(k) and m >= 1 and m < V and (m < k or k == 1)
    for f in VR.K_FAMILIES:
        if f in names:
            assert np.array_equal(fin[f], VR.finite_words(f, V, k))


def _restated(fn, **kw):
    """Worst err / bound of an fp32 restatement over every (V, k) stack, per family, against the x - lse form's bound."""
    worst = {}
    for V, k in SHAPES:
        names, X = VR.stack(V, k)
        logp, lse = VR.log_softmax_ref(X)
        r = VR.ratios(fn(X, **kw), logp, VR.bound_lse_form(logp, lse)).max(-1).values
        for f, v in zip(names, r.tolist()):
            worst[f] = max(worst.get(f, 0.0), v)
    return worst


def test_float32_evaluations_stay_inside_the_bounds():
    """torch.log_softmax in fp32, which is the (x - max) - log Σ form, inside the tighter bound; the x - (max + log Σ)
    form restated in fp32 inside its own.  A figure over 1 here means the derivation is wrong, not the GPU."""
    worst_t, worst_s = {}, {}
    for V, k in SHAPES:
        names, X = VR.stack(V, k)
        logp, lse = VR.log_softmax_ref(X)
        got = torch.log_softmax(X, -1)
        rt = VR.ratios(got, logp, VR.bound_shifted_form(logp)).max(-1).values
        rs = VR.ratios(got, logp, VR.bound_lse_form(logp, lse)).max(-1).values
        for f, a, b in zip(names, rt.tolist(), rs.tolist()):
            worst_t[f], worst_s[f] = max(worst_t.get(f, 0.0), a), max(worst_s.get(f, 0.0), b)
        # Σ_v logp of the fp32 rows, summed in float64 as the kernel sums it
        s = got.double().sum(-1)
        rsum = VR.ratios(s, VR.sum_logp_ref(X), VR.bound_sum_logp(X))
        assert float(rsum.max()) <= 1.0, (V, k, dict(zip(names, rsum.tolist())))
    worst_l = _restated(VR.f32_lse_form)
    print("torch fp32 / shifted bound:", {f: f"{v:.3f}" for f, v in worst_t.items()})
    print("x - lse restated / its bound:", {f: f"{v:.3f}" for f, v in worst_l.items()})
    assert max(worst_t.values()) <= 1.0, worst_t
    assert max(worst_s.values()) <= 1.0, worst_s
    assert max(worst_l.values()) <= 1.0, worst_l


def test_the_two_forms_differ_where_the_bounds_say():
    """The x - lse form loses ulp(|lse|) on an offset row, the shifted form does not: the difference between the two bounds
    is real, and the tighter one may not be asked of odic_logsoftmax_topk."""
    for f in ("offset+1000", "offset-1000"):
        X = VR.row(f, 10241, 1)[None]
        logp, lse = VR.log_softmax_ref(X)
        r = VR.ratios(VR.f32_lse_form(X), logp, VR.bound_shifted_form(logp))
        assert float(r.max()) > 3.0, float(r.max())


def test_mutated_restatements_fall_outside_the_bounds():
    """Two of the mutations the GPU tests must catch, on the CPU restatement: without the maximum subtraction the rows at
    +-1000 overflow or vanish (exp(x) of every other family stays inside fp32, and the result inside its bound: only the
    offset rows notice); a sum over V + 1 elements moves every log-prob by log(1 + p_last)."""
    w = _restated(VR.f32_lse_form, drop_max=True)
    assert w["plain"] <= 1.0                                   # the old regime does not notice
    for f in ("offset+1000", "offset-1000"):
        assert w[f] == float("inf"), (f, w[f])
    w = _restated(VR.f32_lse_form, extra_term=True)
    for f in ("zeros", "ramp", "plain"):
        assert w[f] > 1.0, (f, w[f])


def test_mutated_orders_differ_from_the_reference():
    """The other two, on the reference order: ties to the HIGHER index change zeros / two_level / masked_short; a -inf that
    counts as a finite candidate (here: as 0) changes the masked families that keep k words or fewer."""
    for V, k in [(37, 5), (513, 9), (10241, 16)]:
        names, X = VR.stack(V, k)
        want = VR.topk_ref(X, k)
        flipped = (V - 1) - VR.topk_ref(X.flip(-1), k)          # (value descending, index DEScending)
        as_zero = VR.topk_ref(torch.where(torch.isinf(X), torch.zeros_like(X), X), k)
        for r, f in enumerate(names):
            if f in ("zeros", "two_level", "masked_short") and (f != "masked_short" or k > 1):
                assert not torch.equal(flipped[r], want[r]), (f, V, k)
            if f in ("masked_short", "masked_k_one_wave", "masked_k_spread") and k > 1:      # some kept word is below 0
                assert not torch.equal(as_zero[r], want[r]), (f, V, k)


@pytest.mark.parametrize("V", VR.ENSEMBLE_VS)
@pytest.mark.parametrize("M", VR.ENSEMBLE_MS)
def test_ensemble_constructions(M, V):
    members, own = VR.ens_disagree(M, V)
    out, p = VR.ensemble_ref(members)
    assert len(set(own)) == M
    assert float(p.min()) >= 2.0 ** -60, float(p.min())
    for a in own:
        assert abs(float(out[0, a]) - math.log(1.0 / M)) < VR.E0 / 3            # the rest of the row weighs 2e-6 at most
    shifted, base = VR.ens_offsets(M, V)
    for x, y, c in zip(shifted, base, (1000.0, -1000.0, 0.0)):
        assert torch.equal(x.double(), y.double() + c)                                     # the shift is exact in fp32
    assert torch.allclose(VR.ensemble_ref(shifted)[0], VR.ensemble_ref(base)[0], rtol=0, atol=1e-11)
    members = VR.ens_underflow(M, V)
    out, p = VR.ensemble_ref(members)
    named = p[0] < VR.UNDERFLOW_P
    assert int(named.sum()) >= 1 and bool((p > 0).all()) and float(p[0, -1]) > 1e-4
    assert all(float(x.max() - x.min()) >= 200 for x in members)
    lo, up = VR.ensemble_bounds(members, out, p)
    assert bool((lo[0, named] == float("inf")).all()) and bool((up >= VR.E0).all())
    normal = p[0] >= 2.0 ** -120
    assert bool((lo[0, normal] == up[0, normal]).all()) and float(up[0, normal].max()) < 6e-5
    members, w = VR.ens_masked_member(M, V)
    out, p = VR.ensemble_ref(members)
    assert members[0][0, w] == NINF and all(torch.isfinite(x[0, w]) for x in members[1:])
    assert bool(torch.isfinite(out).all()) and float(p[0, w]) > 2.0 ** -60


def test_ensemble_bounds_hold_for_a_float32_evaluation():
    for M in VR.ENSEMBLE_MS:
        for V in VR.ENSEMBLE_VS:
            for members in (VR.ens_disagree(M, V)[0], VR.ens_offsets(M, V)[0], VR.ens_masked_member(M, V)[0]):
                out, p = VR.ensemble_ref(members)
                got = torch.log(torch.stack([torch.softmax(x, -1) for x in members]).sum(0) * (1.0 / M))
                lo, up = VR.ensemble_bounds(members, out, p)
                assert bool(((got.double() - out) <= up).all()) and bool(((out - got.double()) <= lo).all()), (M, V)


def test_sampling_plan():
    assert (16, 16) in VR.sample_shapes() and all(k <= V for V, k in VR.sample_shapes())
    names, X = VR.sample_stack(37, 5)
    assert X.shape == (len(names) * VR.SAMPLE_REPS, 37)
    assert torch.equal(X[VR.SAMPLE_REPS * 2 + 5].view(torch.int32), VR.row(names[2], 37, 5).view(torch.int32))
