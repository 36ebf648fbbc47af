"""The data behind test_frontend_shapes_gpu.py, checked without a GPU.

  * Every reference of frontend_refs.py equals the oracle (oracle/expansionnet_ref.py) on a TINY-sized input, float64 both,
    to 1e-12 of the output scale: the new references hang off the oracle the rest of the suite trusts.
  * Every bound the GPU test applies is met by a float32 CPU evaluation of the same formula, case by case: each bound is
    reachable by an fp32 implementation that sums in another order.  No bound comes from a kernel's output.
  * The error float32 CPU layer_norm itself makes on the randn + 30 row of every LayerNorm case is measured here and stands
    beside the case (LayerNormCase.off_err).
"""
import math

import pytest
import torch

import frontend_refs as FR
from frontend_refs import F32, F64

from on_device_image_captioning_amd import weights as W

torch.set_grad_enabled(False)


def _ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------------------------------------------- references vs oracle
def test_patch_embed_ref_equals_the_oracle():
    from oracle import expansionnet_ref as R
    g = W.TINY
    sd = {k: W.synth_tensor(k, s, kind, g).double() for k, s, kind in W.state_dict_spec(g) if "patch_embed" in k}
    img = W.synth_images(2, g).double()
    P = "swin_transf.patch_embed"
    want = R.patch_embed(sd, g, img)
    got = FR.patch_embed_ref(img, sd[P + ".proj.weight"].reshape(g.swin_embed_dim, -1), sd[P + ".proj.bias"],
                             sd[P + ".norm.weight"], sd[P + ".norm.bias"], g.swin_patch_size, 1e-5)
    assert got.dtype == F64 and want.dtype == F64
    FR.assert_within(got, want, 1e-12, "patch_embed_ref vs oracle")


def test_patch_merge_ln_ref_equals_the_oracle():
    from oracle import expansionnet_ref as R
    g = W.TINY
    B, res, C = 2, g.stage_res(0), g.swin_embed_dim
    x = FR._randn(B, res * res, C, seed=5).double()
    gm, bt = (1 + 0.1 * FR._randn(4 * C, seed=2)).double(), (0.1 * FR._randn(4 * C, seed=3)).double()
    sd = {"m.norm.weight": gm, "m.norm.bias": bt, "m.reduction.weight": torch.eye(4 * C, dtype=F64)}
    want = R.patch_merging(sd, "m", x, res)             # identity reduction: the gather and the LayerNorm, nothing else
    FR.assert_within(FR.patch_merge_ln_ref(x, gm, bt, B, res, C, 1e-5), want, 1e-12, "patch_merge_ln_ref vs oracle")


def test_stcexp_and_selector_refs_equal_the_oracle():
    """R.static_expansion returns only the block's output, so the block is rebuilt here around stcexp_ref's four tables and
    selector_mix_ref (the products between them are plain matmuls) and compared with it: a table that differed from the
    oracle's normalisation steps would change the output."""
    from oracle import expansionnet_ref as R
    g = W.TINY
    groups, d, B, S = g.num_exp_enc_list, g.d_model, 3, 20
    nq = sum(groups)
    p = "e"
    sd = {p + ".query_exp_vectors.weight": FR._randn(nq, d, seed=1).double(),
          p + ".bias_exp_vectors.weight": FR._randn(nq, d, seed=2).double() * 0.1}
    for i, n in enumerate(("key_embed", "class_a_embed", "class_b_embed", "selector_embed")):
        sd[f"{p}.{n}.weight"] = FR._randn(d, d, seed=10 + i).double() / math.sqrt(d)
        sd[f"{p}.{n}.bias"] = FR._randn(d, seed=20 + i).double() * 0.1
    x = FR._randn(B, S, d, seed=3).double()
    lens = torch.tensor([20, 13, 1])
    valid = torch.arange(S)[None, :] < lens[:, None]
    want = R.static_expansion(sd, p, x, groups, valid)

    lin = lambda n: torch.nn.functional.linear(x, sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"])
    Q, Bv = sd[p + ".query_exp_vectors.weight"], sd[p + ".bias_exp_vectors.weight"]
    z = torch.matmul(Q, lin("key_embed").transpose(-1, -2)) / math.sqrt(d)
    pf, nf, pb, nb = FR.stcexp_ref(z, lens, groups, 1e-9)
    A, Bm = torch.matmul(pf, lin("class_a_embed")) + Bv, torch.matmul(nf, lin("class_b_embed")) + Bv
    got = FR.selector_mix_ref(torch.zeros_like(x), lin("selector_embed"), torch.matmul(pb, A), torch.matmul(nb, Bm))
    FR.assert_within(got, want, 1e-12, "stcexp_ref + selector_mix_ref vs oracle")
    # and the tables are not trivially equal: masking matters for the forward ones only
    full = FR.stcexp_ref(z, torch.tensor([S] * B), groups, 1e-9)
    assert not torch.equal(full[0], pf) and torch.equal(full[2], pb) and torch.equal(full[3], nb)


# ---------------------------------------------------------------------------------------------------- bounds are reachable
@pytest.mark.parametrize("case", FR.PATCH_EMBED_CASES, ids=_ids(FR.PATCH_EMBED_CASES))
def test_patch_embed_bound_is_reachable_in_float32(case):
    ins = FR.patch_embed_inputs(case)
    want = FR.patch_embed_ref(*ins, 4, 1e-5)
    assert want.shape == (case.B, (case.H // 4) * (case.W // 4), case.C)
    FR.assert_within(FR.patch_embed_ref(*ins, 4, 1e-5, dtype=F32), want, FR.BOUND_F32, f"patch_embed {case.name} in float32")


def test_patch_embed_images_differ():
    """Every image's tokens are far from every other image's (and from its own other tokens): a token read from the wrong
    place misses the bound by orders of magnitude."""
    for case in FR.PATCH_EMBED_CASES:
        want = FR.patch_embed_ref(*FR.patch_embed_inputs(case), 4, 1e-5).reshape(-1, case.C)
        if want.shape[0] == 1:
            continue
        dist = torch.cdist(want, want, p=float("inf")) + torch.eye(want.shape[0], dtype=F64) * 1e9
        assert float(dist.min()) > 1e3 * FR.BOUND_F32 * float(want.abs().max()), case.name


def test_patch_embed_unfixed_index_arithmetic_reads_other_tokens():
    """The load loop once corrected the image index a single time (`if (r >= per_img) { r -= per_img; ++b; }`).  Replayed on
    the host for every case: with fewer than 64 tokens per image that arithmetic names another (image, row, column) than the
    flat token index does, for the two cases that exist to show it and for no other."""
    wrong = {}
    for case in FR.PATCH_EMBED_CASES:
        gh, gw = case.H // 4, case.W // 4
        per_img, bad = gh * gw, 0
        for tok in range(case.B * per_img):
            tok0 = tok // 64 * 64
            b, r = tok0 // per_img, tok0 % per_img + tok - tok0
            if r >= per_img:
                r, b = r - per_img, b + 1
            bad += (b, r // gw, r % gw) != (tok // per_img, tok % per_img // gw, tok % per_img % gw)
        wrong[case.name] = bad
    assert {k for k, v in wrong.items() if v} == {"B5_c3_16x16_C64", "B4_c3_20x24_C96"}, wrong
    assert wrong["B5_c3_16x16_C64"] == 32        # block 0: all of images 2 and 3 (image 4 is block 1's first)
    assert wrong["B4_c3_20x24_C96"] == 4         # block 0: the head of image 2
    # 60 tokens per image: block starts are multiples of 4 (64 mod 60), a block reaches a third image only from an offset
    # above 56, so the single correction is right there whatever B is
    assert wrong["B3_c3_40x24_C96"] == 0


@pytest.mark.parametrize("case", FR.LAYERNORM_CASES, ids=_ids(FR.LAYERNORM_CASES))
def test_layernorm_bounds_are_reachable_in_float32(case):
    x, gm, bt = FR.layernorm_inputs(case)
    want = FR.layernorm_ref(x, gm, bt, 1e-5)
    got = FR.layernorm_ref(x, gm, bt, 1e-5, dtype=F32)
    scale = float(want.abs().max())
    rc, rz, ro = FR.layernorm_rows(case.M)
    for odt in case.odts:
        o = got.to(odt)
        FR.assert_within(o, want, FR.bound_of(odt), f"layernorm {case.name} {odt} in float32")
        if rc is not None:
            for r in (rc, rz):
                FR.assert_within(o[r], bt.double(), FR.bound_of(odt), f"layernorm {case.name} {odt} row {r} = beta", scale=scale)
    if ro is not None:
        FR.assert_within(got[ro], want[ro], FR.layernorm_offset_bound(case), f"layernorm {case.name} offset row", scale=scale)


@pytest.mark.parametrize("case", FR.LAYERNORM_CASES, ids=_ids(FR.LAYERNORM_CASES))
def test_layernorm_offset_row_error_is_recorded(case):
    """off_err is what torch's float32 CPU layer_norm loses against float64 on the randn + 30 row, relative to the case's
    scale.  The recorded figure is the measurement itself; another CPU's vector width may sum in another order, so the
    measurement may differ from the record by the factor the bound itself allows (4), not more."""
    x, gm, bt = FR.layernorm_inputs(case)
    ro = FR.layernorm_rows(case.M)[2]
    if ro is None:
        assert case.off_err == 0.0
        return
    want = FR.layernorm_ref(x, gm, bt, 1e-5)
    err, _ = FR.max_err(torch.nn.functional.layer_norm(x[ro], (case.C,), gm, bt, 1e-5), want[ro])
    measured = err / float(want.abs().max())
    print(f"layernorm {case.name}: float32 CPU error on the offset row / scale = {measured:.3e} (recorded {case.off_err:.3e})")
    assert case.off_err > 0.0 and measured <= 4.0 * case.off_err and case.off_err <= 4.0 * max(measured, 1e-8)
    assert 4.0 * measured <= FR.layernorm_offset_bound(case)


@pytest.mark.parametrize("case", FR.PATCH_MERGE_CASES, ids=_ids(FR.PATCH_MERGE_CASES))
def test_patch_merge_bounds_are_reachable_in_float32(case):
    x, gm, bt = FR.patch_merge_inputs(case)
    want = FR.patch_merge_ln_ref(x, gm, bt, case.B, case.res, case.C, 1e-5)
    assert want.shape == (case.B, (case.res // 2) ** 2, 4 * case.C)
    got = FR.patch_merge_ln_ref(x, gm, bt, case.B, case.res, case.C, 1e-5, dtype=F32)
    for odt in case.odts:
        FR.assert_within(got.to(odt), want, FR.bound_of(odt), f"patch_merge_ln {case.name} {odt} in float32")
    # a swapped pair of neighbours is not within the bound
    g = x.double().reshape(case.B, case.res // 2, 2, case.res // 2, 2, case.C)
    swapped = torch.cat([g[:, :, 0, :, 0], g[:, :, 0, :, 1], g[:, :, 1, :, 0], g[:, :, 1, :, 1]], -1)
    swapped = torch.nn.functional.layer_norm(swapped.reshape(want.shape), (4 * case.C,), gm.double(), bt.double(), 1e-5)
    assert FR.max_err(swapped, want)[0] > 1e3 * FR.BOUND_F32 * float(want.abs().max())


@pytest.mark.parametrize("S", FR.STCEXP_S)
@pytest.mark.parametrize("groups", FR.STCEXP_GROUPS, ids=lambda g: f"nq{sum(g)}")
def test_stcexp_bounds_are_reachable_in_float32(groups, S):
    z, lens = FR.stcexp_inputs(groups, S)
    want = FR.stcexp_ref(z, lens, groups, 1e-9)
    got = FR.stcexp_ref(z, lens, groups, 1e-9, dtype=F32)
    FR.assert_stcexp_tables(got, want, groups, FR.BOUND_F32, f"stcexp nq={sum(groups)} S={S} float32")
    FR.assert_stcexp_tables([t.bfloat16() for t in got], want, groups, FR.BOUND_BF16, f"stcexp nq={sum(groups)} S={S} bf16")
    # the properties of z the GPU test relies on
    assert int((z == 0).sum()) > 10 and bool(torch.signbit(z[z == 0]).any()) and not bool(torch.signbit(z[z == 0]).all())
    q0, n = FR.stcexp_widest(groups)
    assert bool((z[0, FR.STCEXP_NEG_ROW] < 0).all()) and bool((z[0, q0:q0 + n, FR.stcexp_pos_col(S)] > 0).all())
    assert float(want[0][0, FR.STCEXP_NEG_ROW].abs().max()) == 0.0 and float(want[1][0, FR.STCEXP_NEG_ROW].sum()) > 0.99
    assert float(want[3][0, FR.stcexp_pos_col(S), q0:q0 + n].abs().max()) == 0.0
    assert float(want[0][2].abs().max()) == 0.0 and float(want[1][2].abs().max()) == 0.0        # enc_len = 0
    assert float(want[2][2].abs().max()) > 0.0                                                  # backward: not masked


def test_stcexp_groups_reach_every_branch_of_the_column_sum():
    """MIRRORS stcexp_colsum_kernel (csrc/encoder_ops.hip): slice y of 16 starts at query y of its group, takes eight queries
    16 apart per trip while y + 112 < n, then one query per trip.  If the kernel changes its split, change this with it and
    look at the group lists again."""
    SL = 16

    def trips(n, y):
        q, unrolled = y, 0
        while q + 7 * SL < n:
            q, unrolled = q + 8 * SL, unrolled + 1
        return unrolled, len(range(q, n, SL))

    seen = {trips(n, y) for n in FR.STCEXP_GROUPS[1] for y in range(SL)}
    assert {(0, 0), (0, 1), (0, 2), (0, 7), (1, 0), (1, 1), (1, 7), (2, 0)} <= seen, seen
    assert max(r for _, r in seen) == 7                                              # (an eighth remainder trip is an unrolled one)
    assert {trips(n, y)[0] for n in FR.STCEXP_GROUPS[0] for y in range(SL)} == {0, 1, 2, 4}
    assert all(trips(n, y)[0] == 0 for n in (8, 16, 24) for y in range(SL))         # the groups of every older kernel test
    nq = sum(FR.STCEXP_GROUPS[1])
    assert nq == 772 and nq % 32 == 4 and all(S % 32 for S in FR.STCEXP_S)


def test_selector_mix_bound_is_reachable_in_float32():
    x, sel, a, b = FR.selector_inputs()
    want = FR.selector_mix_ref(x, sel, a, b)
    got = FR.selector_mix_ref(x, sel, a, b, dtype=F32)
    FR.assert_within(got, want, FR.BOUND_F32, "selector_mix in float32")
    scale = float(want.abs().max())
    FR.assert_within(got[:, [0, 2]], (x.double() + a.double())[:, [0, 2]], FR.BOUND_F32, "selector +100, +20: x + a", scale=scale)
    FR.assert_within(got[:, [1, 3]], (x.double() + b.double())[:, [1, 3]], FR.BOUND_F32, "selector -100, -20: x + b", scale=scale)


def test_cast_rows_hold_what_they_claim():
    x = FR.cast_finite_row()
    assert x.shape == (1, 32) and bool(torch.isfinite(x).all())
    bits = x.view(torch.int32) & 0x7FFFFFFF
    assert int(((bits > 0) & (bits < 0x00800000)).sum()) == 6                       # subnormals
    assert int(((x.view(torch.int32) & 0xFFFF) == 0x8000).sum()) >= 4               # exact bf16 ties
    r = x.bfloat16().view(torch.int16)[0]
    assert int(r[8]) == 0x3F80 and int(r[9]) == 0x3F82                              # ties go to the even neighbour: down, up
    assert bool(torch.isinf(x.bfloat16()[0, 28]))                                   # the largest float rounds to inf
    y, nan = FR.cast_special_rows()
    assert y.shape == (2, 40) and int(nan.sum()) == 4 and int(torch.isinf(y).sum()) == 2
