"""tests/dynexp_refs.py without a GPU: the float64 reference equals the oracle, the families have the properties they are there
for, the recorded float32 errors reproduce (so every bound is 8 x a figure measured here, not a kernel's), the wrong forms of
the normaliser miss the bounds, the probe decodes to the coefficients, and the atol term stays a small share of every case."""
import math

import pytest
import torch

import dynexp_refs as DX
import dynexp_step_model as M
from oracle import expansionnet_ref as R

torch.set_grad_enabled(False)
F64 = torch.float64
CASES = [(f, s, p) for f in DX.FAMILIES for s in DX.SHAPES for p in DX.PLANS]
ids = lambda c: "-".join(c)


@pytest.mark.parametrize("shape", list(DX.SHAPES))
@pytest.mark.parametrize("lens_i", [0, 1])
def test_reference_equals_the_oracle(shape, lens_i):
    """On lin = x·Wᵀ + b (float64, unrounded) with padded sequences; 1e-12 of the output scale.  The oracle's own eps is its
    default: a changed DX.EPS fails here (gauss normalisers are O(1): 1e-9 of them is 1e3 x this tolerance)."""
    T, d, E = DX.SHAPES[shape]
    dt = DX.data("gauss", shape, "identity")
    sd64 = {k: v.double() for k, v in dt.extra["sd"].items()}
    x64 = dt.extra["x"].double()
    lens = DX.seq_lens(T)[lens_i]
    ok = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    causal = (torch.tril(torch.ones(T, T, dtype=torch.bool))[None] & ok[:, :, None] & ok[:, None, :]).double()
    want = R.dynamic_expansion(sd64, "p", x64, E, causal)
    lin = M.linear_rows(sd64, x64)
    got, _ = DX.dynexp_ref(*(lin[..., i * d:(i + 1) * d] for i in range(5)), sd64["p.query_exp_vectors.weight"],
                           sd64["p.bias_exp_vectors.weight"], lens, eps=DX.EPS)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"{shape} lens {lens}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= 1e-12 * scale
    assert bool((got[~ok] == 0).all())


def test_bounds_are_eight_times_the_recorded_figures():
    assert DX.EPS == 1e-9 and DX.FACTOR == 8.0
    for f in DX.FAMILIES:
        assert DX.BOUNDS[f] == (8.0 * DX.MEASURED[f][0], 8.0 * DX.MEASURED[f][1])


_SEEN = {}


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_float32_evaluation_meets_every_bound(case):
    """The reversed-order float32 evaluation stays within one eighth of the family's bound, entry by entry; the recorded figure
    is not more than 10 % above the largest one measured (checked by the last case of the family)."""
    f, s, p = case
    rel, ab = DX.measure_case(f, s, p)
    print(f"{ids(case)}: relative {rel:.3e}, absolute / rowscale {ab:.3e}; recorded {DX.MEASURED[f]}")
    assert rel <= DX.MEASURED[f][0] and ab <= DX.MEASURED[f][1]
    dt = DX.data(f, s, p)
    f32 = DX.search_ref(dt, p, dtype=torch.float32, split=(f == "cancel"))
    got, want = DX.compared(dt, p, f32.out, DX.search_ref(dt, p))
    rtol, atol = DX.BOUNDS[f]
    assert float(DX.excess(got, want, rtol, atol).max()) <= 1.0 / DX.FACTOR
    _SEEN.setdefault(f, []).append((rel, ab))
    if len(_SEEN[f]) == len(DX.SHAPES) * len(DX.PLANS):
        assert max(r for r, _ in _SEEN[f]) >= 0.9 * DX.MEASURED[f][0], "the recorded relative figure is stale"
        assert max(a for _, a in _SEEN[f]) >= 0.9 * DX.MEASURED[f][1], "the recorded absolute figure is stale"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_no_score_lies_near_zero(case):
    """Every |z| is at least 2^-10 of its row's largest (forward rows and backward rows of every history; a planted row's
    scale divided out): the sign of every relu argument is the same in float32 and float64."""
    f, s, p = case
    m = DX.search_ref(DX.data(f, s, p), p).margin
    print(f"{ids(case)}: smallest |z| / row max = {m:.3e}")
    assert m >= DX.MARGIN


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_atol_term_takes_at_most_five_percent(case):
    f, s, p = case
    dt = DX.data(f, s, p)
    ref = DX.search_ref(dt, p)
    _, want = DX.compared(dt, p, ref.out, ref)
    share = DX.atol_share(want, *DX.BOUNDS[f])
    print(f"{ids(case)}: {100 * share:.2f} % of the non-zero entries are bounded mostly by the atol term")
    assert share <= DX.CAP


@pytest.mark.parametrize("shape", list(DX.SHAPES))
def test_one_sided_rows(shape):
    T, d, E = DX.SHAPES[shape]
    dt = DX.data("one_sided", shape)
    out, tabs = DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * DX.N_SEQ)
    # slot 0: query 0 has no positive forward score at any position (so from t = 3 on), query 1 no negative one
    assert bool((tabs["sfa"][0, :, 0] == 0).all()) and bool((tabs["wfa"][0, :, 0] == 0).all())
    assert bool((tabs["sfb"][0, :, 1] == 0).all()) and bool((tabs["sfa"][0, 3:, 1] > 0).all())
    # class A of that query is bexp + cond alone: the reference's A row with zero weights
    assert bool((tabs["sfb"][0, 3:, 0] > 0).all())
    # slot 1: the backward scores of positions 0, T//2 and T-1 are all positive: nb all zeros, the B branch adds nothing
    for t in (0, T // 2, T - 1):
        assert float(tabs["sbb"][1, t]) == 0 and bool((tabs["wbb"][1, t] == 0).all()) and float(tabs["sba"][1, t]) > 0
    coef = DX.coefficients(tabs)
    assert bool((coef["cb"][1, T - 1] == 0).all()) and bool((coef["web"][1, T // 2] == 0).all())
    # re-ordered: exact zeros survive the mixing of slots (reference weights that are 0 at later steps than t = 0)
    ref = DX.search_ref(dt, "reorder")
    assert int((ref.coef["web"][3:] == 0).sum()) > 0


@pytest.mark.parametrize("shape", list(DX.SHAPES))
def test_eps_regime_spread_and_wrong_normalisers(shape):
    T, d, E = DX.SHAPES[shape]
    dt = DX.data("eps_regime", shape)
    N = DX.N_SEQ
    out, tabs = DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * N)
    assert float(dt.lin.abs()[dt.lin != 0].min()) >= 2.0 ** -126, "a subnormal input"
    sums = torch.cat([tabs[k].reshape(-1) for k in ("sfa", "sfb", "sba", "sbb")])
    sums = sums[sums > 0]
    fw = torch.cat([tabs["sfa"].reshape(-1), tabs["sfb"].reshape(-1)])
    for level in (1e-11, 1e-10, 1e-9, 1e-8, 1e-7):                       # forward normalisers within half a decade of each level
        n = int(((fw > level / math.sqrt(10)) & (fw < level * math.sqrt(10))).sum())
        assert n > 0, f"no forward normaliser near {level:g}"
    share = sums / (sums + 1e-9)                                           # what 1/(s + eps) keeps of 1/s
    print(f"{shape}: normalisers {float(sums.min()):.2e} .. {float(sums.max()):.2e}; s/(s+eps) {float(share.min()):.3f} .. {float(share.max()):.3f}")
    assert float(share.min()) <= 0.05 and float(share.max()) >= 0.95
    # the reference result differs by 1 % to 99 % from the eps-free one: per row, the norm of the difference
    free, _ = DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * N, norm="none")
    rel = (free - out).norm(dim=-1) / free.norm(dim=-1)
    print(f"{shape}: rows differ from the eps-free result by {100 * float(rel.min()):.1f} % .. {100 * float(rel.max()):.1f} %")
    assert float(rel.min()) <= 0.05 and float(rel.max()) >= 0.95 and int(((rel > 0.2) & (rel < 0.8)).sum()) > 0
    rtol, atol = DX.BOUNDS["eps_regime"]
    worst = {v: float(DX.excess(DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * N, norm=v)[0], out, rtol, atol).max())
             for v in ("none", "max", "guard")}
    print(f"{shape}: wrong normalisers miss the bound by {worst}")
    assert worst["none"] >= 100 and worst["guard"] >= 100 and worst["max"] > 1
    other_eps, _ = DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * N, eps=2e-9)
    assert float(DX.excess(other_eps, out, rtol, atol).max()) >= 100


@pytest.mark.parametrize("shape", list(DX.SHAPES))
def test_peaked_and_cancel_rows(shape):
    T, d, E = DX.SHAPES[shape]
    dt = DX.data("peaked", shape)
    assert float(dt.lin.abs().max()) < 2.0 ** 60
    _, tabs = DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * DX.N_SEQ)
    for k in ("wf", "wb"):          # a row's two classes together: the peak is in one of them, beside 2^-12-sized weights
        w = (tabs[k + "a"] + tabs[k + "b"])[:, T - 1]
        w = w if k == "wf" else w.reshape(DX.N_SEQ, 1, -1)
        span = w.amax(-1) / torch.where(w > 0, w, torch.ones_like(w)).amin(-1)
        print(f"peaked {shape} {k}[t = {T - 1}]: weights span {float(span.min()):.1e} .. {float(span.max()):.1e}")
        assert bool((span > 1e3).all())
    # the planted key scores 2^12 times the others of its forward row (up to the spread of the unplanted scores, < 2^4)
    z = tabs["z"][:, T - 1].abs()                                          # [N, E, T]
    ratio = z[:, :, T // 3] / z[:, :, T // 3 + 1]
    assert bool((ratio > DX.PEAK / 16).all()) and bool((ratio < DX.PEAK * 16).all())
    dt = DX.data("cancel", shape)
    cond, key = dt.blocks()[0].double(), dt.blocks()[1].double()
    qk = torch.einsum("ed,ntd->nte", dt.qexp.double(), key)
    ck = torch.einsum("nad,nbd->nab", cond, key)
    z = DX.dynexp_ref(*dt.blocks(), dt.qexp, dt.bexp, [T] * DX.N_SEQ)[1]["z"]
    print(f"cancel {shape}: |qexp·key| {float(qk.abs().min()):.1f} .. {float(qk.abs().max()):.1f}, |cond·key| "
          f"{float(ck.abs().min()):.1f} .. {float(ck.abs().max()):.1f}, |z| {float(z.abs().min()):.3f} .. {float(z.abs().max()):.3f}")
    assert float(qk.abs().min()) > 900 and float(qk.abs().max()) < 1150 and float(ck.abs().min()) > 900 and float(ck.abs().max()) < 1150
    assert bool((torch.sign(qk)[:, None, :, :].transpose(2, 3) == -torch.sign(ck)[:, :, None, :]).all())
    assert float(z.abs().max()) < 4.0 and float(z.abs().min()) > 0.25
    common = cond[:, :, :d - DX.KEY_CH]
    assert bool((common == common[0, 0]).all()) and float(common[0, 0].norm()) > 5.0


@pytest.mark.parametrize("shape", list(DX.SHAPES))
@pytest.mark.parametrize("plan", DX.PLANS)
def test_probe_channels_decode_to_the_coefficients(shape, plan):
    """With the reference itself as the kernel: channel i is ca[i] (cb[i]), T + j is amp·wja[j], 2T + e is wea[e], to the last
    bits of float64, and every other channel is zero."""
    T, d, E = DX.SHAPES[shape]
    assert d >= 2 * T + E + 64
    dt = DX.data("probe", shape, plan)
    ref = DX.search_ref(dt, plan)
    got, want = DX.compared(dt, plan, ref.out, ref)
    assert float((got - want).abs().max()) <= 1e-15
    assert bool((ref.out[..., 2 * T + E:] == 0).all())
    br = DX.probe_branch(dt)
    assert 0.4 < float(br.float().mean()) < 0.6
    assert int((want == 0).sum()) > 0 and int((want > 0).sum()) > 0
    with pytest.raises(AssertionError, match=r"sequence 1, step 5, wea\[2\]"):          # a failure names the entry
        bad = ref.out.clone()
        bad[5, 1, 2 * T + 2] *= 1.01
        DX.assert_probe(dt, plan, bad, ref, "mutated")
