"""The window-attention probe (tests/window_probe.py) proves itself on the CPU:

  * run through the oracle's fp64 window_attention_core, the one-hot-V launches give back the fp64 reference to 1e-12 at
    every geometry the GPU tests use;
  * mutants of the REFERENCE (not of the kernels) — a bias index off by one, an un-reversed x axis, a region boundary off by
    one, a -inf mask, a swapped key order — each move pairs beyond the bf16 bound (the widest) in the family meant to catch
    them;
  * the reference evaluated in float32 stays inside the fp32 bound: the bound is reachable.
"""
import pytest
import torch

import window_probe as wp
from on_device_image_captioning_amd import weights as W

torch.set_grad_enabled(False)

WS12 = [(1, 12, 12, 0), (1, 12, 12, 1), (1, 12, 12, 11), (2, 24, 12, 5), (1, 24, 12, 6), (3, 36, 12, 7)]
SMALL = [(2, 14, 7, 3), (2, 21, 7, 0), (2, 8, 4, 1), (2, 6, 2, 1), (2, 3, 1, 0), (2, 22, 11, 10)]


def _geo(t):
    return wp.Geometry(*t)


@pytest.mark.parametrize("name", wp.FAMILIES)
@pytest.mark.parametrize("g", WS12 + SMALL, ids=lambda t: "B%d-res%d-ws%d-shift%d" % t)
def test_probe_recovers_the_reference_through_the_oracle(g, name):
    geo = _geo(g)
    fam = wp.family(name, geo)
    P = wp.probe(geo, fam, wp.oracle_attend(geo, fam))
    want = wp.p_want(name, geo)
    assert bool(torch.isfinite(P).all()), "a pair was never filled"
    assert float((P - want).abs().max()) <= 1e-12
    assert float((want.sum(-1) - 1.0).abs().max()) <= 1e-12


def test_inputs_are_exact_in_both_16_bit_formats():
    geo = _geo((2, 24, 12, 5))
    for name in wp.FAMILIES:
        fam = wp.family(name, geo)
        for t in (fam.q, fam.k):
            assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t), name
        # the packed bias divides by the scale: still the same fp32 numbers times 8
        assert torch.equal((fam.table.double() / wp.SCALE).float().double() * wp.SCALE, fam.table.double()), name
    per_slot = wp.family("score", geo, False)
    assert torch.equal(per_slot.k[0, 0], per_slot.k[1, 3])
    assert not torch.equal(wp.family("score", geo).k[0, 0], wp.family("score", geo).k[1, 3])


def test_families_reach_the_softmax_edges():
    geo = _geo((3, 36, 12, 7))
    m = wp.masked_pairs(geo)
    # peaked: scores tens of units apart, and rows whose largest raw (unmasked) score sits on a masked key
    fam = wp.family("peaked", geo)
    s = wp.scores(geo, fam)
    raw = wp.scores(geo, fam, mask=torch.zeros(geo.nW, geo.N, geo.N, dtype=torch.float64))
    assert float((s.max(-1).values - s.masked_fill(m.expand_as(s), float("inf")).min(-1).values).max()) >= 60.0
    top = raw.argmax(-1, keepdim=True)
    assert int(torch.gather(m.expand_as(s), -1, top).sum()) >= 1000
    # mask: masked keys only 20 below the row maximum: e^-20 = 2e-9 shared among the <= 144 keys at the maximum
    P = wp.p_want("mask", geo)
    vis = P[m.expand_as(P)]
    assert float(vis.max()) > 1e-11 and int((vis > 1e-12).sum()) >= 1000
    # bias: masked pairs are zero to working precision (the -100 leaves nothing above e^-94)
    P = wp.p_want("bias", geo)
    assert float(P[m.expand_as(P)].max()) < 1e-37


# ------------------------------------------------------------------------------------------------- reference mutants
def _moved(name, geo, **kw):
    """Pairs a mutated reference moves beyond the bf16 bound (the widest of the four) in family `name`."""
    got = kw.pop("P", None)
    if got is None:
        got = wp.p_reference(geo, wp.family(name, geo), **kw)
    return wp.compare(got, wp.p_want(name, geo), *wp.BOUNDS["bf16"]).bad


def _rel_index(ws, dx=0, reverse_x=True):
    r = torch.arange(ws)
    hh, ww = r.repeat_interleave(ws), r.repeat(ws)
    dh = hh[:, None] - hh[None, :] + (ws - 1)
    dw = (ww[:, None] - ww[None, :]) if reverse_x else (ww[None, :] - ww[:, None])
    dw = (dw + (ws - 1) + dx).clamp(0, 2 * ws - 2)
    return dh * (2 * ws - 1) + dw


def _mask(geo, boundary_off=0, value=-100.0):
    n = geo.res // geo.ws
    edges = torch.zeros(geo.res, dtype=torch.int64)
    edges[geo.res - geo.ws:geo.res - geo.shift - boundary_off] = 1
    edges[geo.res - geo.shift - boundary_off:] = 2
    rid = edges[:, None] * 3 + edges[None, :]
    win = rid.view(n, geo.ws, n, geo.ws).permute(0, 2, 1, 3).reshape(n * n, geo.N)
    diff = win[:, None, :] != win[:, :, None]
    return torch.where(diff, torch.tensor(value, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))


GEO = (2, 24, 12, 5)          # 2 x 4 windows x 6 heads x 144² = 995,328 pairs


def test_mutant_helpers_restate_the_true_reference():
    geo = _geo(GEO)
    assert torch.equal(_rel_index(12), W.relative_position_index(12))
    assert torch.equal(_mask(geo), wp.attn_mask(geo))


def test_mutant_relative_index_off_by_one_in_x():
    # moves 568,048 of 995,328 pairs (bias), 565,032 (peaked); the score and mask families (table = 0) see nothing
    geo = _geo(GEO)
    assert _moved("bias", geo, rel_index=_rel_index(12, dx=1)) >= 1
    assert _moved("peaked", geo, rel_index=_rel_index(12, dx=1)) >= 1
    assert _moved("score", geo, rel_index=_rel_index(12, dx=1)) == 0


def test_mutant_x_axis_not_reversed():
    # moves 560,692 of 995,328 pairs (bias), 532,486 (peaked)
    geo = _geo(GEO)
    assert _moved("bias", geo, rel_index=_rel_index(12, reverse_x=False)) >= 1
    assert _moved("peaked", geo, rel_index=_rel_index(12, reverse_x=False)) >= 1


def test_mutant_region_boundary_one_early():
    # boundary at res - shift - 1: moves 370,694 of 995,328 pairs (bias), 458,496 (mask)
    geo = _geo(GEO)
    assert _moved("bias", geo, mask=_mask(geo, boundary_off=1)) >= 1
    assert _moved("mask", geo, mask=_mask(geo, boundary_off=1)) >= 1
    # with one window and shift = 1 the whole seam is one row and one column of slots: 91,776 of 124,416 pairs
    one = _geo((1, 12, 12, 1))
    assert _moved("bias", one, mask=_mask(one, boundary_off=1)) >= 1


def test_mutant_mask_minus_infinity():
    # moves 197,820 of 995,328 pairs, in the mask family only: everywhere else a masked pair is below the smallest step either way
    geo = _geo(GEO)
    assert _moved("mask", geo, mask=_mask(geo, value=float("-inf"))) >= 1
    assert _moved("bias", geo, mask=_mask(geo, value=float("-inf"))) == 0
    P = wp.p_reference(geo, wp.family("mask", geo), mask=_mask(geo, value=float("-inf")))
    with pytest.raises(AssertionError):
        wp.assert_mask_is_additive(P, wp.p_want("mask", geo), geo, "bf16", "mutant")
    assert wp.assert_mask_is_additive(wp.p_want("mask", geo), wp.p_want("mask", geo), geo, "bf16", "reference") >= 1000
    # fp16 / h2: the floor atol / (1 - rtol) = 1.2e-7 lies above every masked probability (<= 2e-9): nothing to ask there
    assert wp.assert_mask_is_additive(wp.p_want("mask", geo), wp.p_want("mask", geo), geo, "fp16", "reference") == 0


def test_mutant_key_order_of_one_step_swapped():
    # keys 64..79 <-> 80..95 (the two halves of the third 32-key step) on the P side only: moves 172,368 of
    # 995,328 pairs (score), 179,940 (peaked)
    geo = _geo(GEO)
    perm = torch.arange(geo.N)
    perm[64:80], perm[80:96] = torch.arange(80, 96), torch.arange(64, 80)
    assert _moved("score", geo, P=wp.p_want("score", geo)[..., perm]) >= 1
    assert _moved("peaked", geo, P=wp.p_want("peaked", geo)[..., perm]) >= 1


# ------------------------------------------------------------------------------------------------- the bound is reachable
@pytest.mark.parametrize("name", wp.FAMILIES)
@pytest.mark.parametrize("g", [(3, 36, 12, 7), (2, 22, 11, 10)], ids=lambda t: "B%d-res%d-ws%d-shift%d" % t)
def test_float32_evaluation_is_inside_the_fp32_bound(g, name):
    geo = _geo(g)
    got = wp.p_reference(geo, wp.family(name, geo), dtype=torch.float32).double()
    v = wp.compare(got, wp.p_want(name, geo), *wp.BOUNDS["fp32"])
    assert v.bad == 0, v
    assert v.used < 0.5, v          # and with room: the rounding argument gives ~1e-5
