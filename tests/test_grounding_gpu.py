"""Word grounding on the GPU (`-m gpu`): odic_cross_attn_probs against fp64, its accumulate mode and containment,
word_attention against the maps recorded from the reference (tests/golden/tiny_attention.npz), and the exact invariances.

Bounds are the project's own for the same arithmetic: the kernel 2e-5 of scale as test_cross_attn_step, the model
2e-4 of scale as LP_BOUND["xavier"] of test_scoring_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

import guards
from conftest import GOLDEN, cached_state_dict
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
TSOS, TEOS = 3, 2
KERNEL_BOUND = 2e-5
MODEL_BOUND = 2e-4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, want, rtol, name):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = want.abs().max().item() + 1e-12
    err = (got - want).abs().max().item()
    print(f"{name}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e} (bound {rtol:.0e})")
    assert err <= rtol * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e} (rtol {rtol})"


_MODELS = {}


def build_model(variant):
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    if variant not in _MODELS:
        g = W.TINY
        m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                                output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=DEV)
        m.load_state_dict(cached_state_dict("TINY", variant), strict=True)
        _MODELS[variant] = m.to(DEV).eval()
    return _MODELS[variant].set_precision("fp32")


def fixture_set(name):
    fx = np.load(os.path.join(GOLDEN, "tiny_attention.npz"))
    y = torch.from_numpy(fx[name + ".tokens"]).long()
    pads = [int(p) for p in fx[name + ".pads"]]
    caps = [y[i, :y.shape[1] - p].tolist() for i, p in enumerate(pads)]
    real = torch.arange(y.shape[1] - 1)[None, :] < (y.shape[1] - 1 - torch.tensor(pads))[:, None]
    return fx, y, pads, caps, real


# ------------------------------------------------------------------------------------------------- 1. the kernel
SHAPES = [(1, 1, 64, 4), (7, 5, 128, 4), (23, 144, 128, 4), (6, 145, 128, 2), (3, 144, 512, 8), (2, 576, 64, 1)]
N_IMG = 3


def probs_case(rows, S, d, heads, seed=0):
    """q, kv (K at column d of a 3d-wide kv), enc_len = [S, max(1, S//2 + 1), 0], one row_valid = 0 row per image, and the
    fp64 probabilities [N, heads, S]."""
    N = N_IMG * rows
    q, kv = rnd(N, d, seed=seed + 1), rnd(N_IMG, S, 3 * d, seed=seed + 2)
    lens = torch.tensor([S, max(1, S // 2 + 1), 0], dtype=torch.int32)
    valid = torch.ones(N, dtype=torch.int32)
    for i in range(N_IMG):
        valid[i * rows + (i % rows)] = 0
    dk = d // heads
    img = torch.arange(N) // rows
    K = kv[:, :, d:2 * d].double().view(N_IMG, S, heads, dk)[img]                          # [N, S, heads, dk]
    sc = torch.einsum("nhc,nshc->nhs", q.double().view(N, heads, dk), K) / math.sqrt(dk)
    allow = (torch.arange(S)[None, :] < lens[img][:, None]) & (valid[:, None] != 0)         # [N, S]
    want = torch.softmax(sc.masked_fill(~allow[:, None, :], -1e4), -1)
    return q, kv, lens, valid, allow, want


@pytest.mark.parametrize("per_head", [0, 1])
@pytest.mark.parametrize("rows,S,d,heads", SHAPES)
def test_cross_attn_probs_matches_fp64(ops, rows, S, d, heads, per_head):
    N = N_IMG * rows
    q, kv, lens, valid, allow, want = probs_case(rows, S, d, heads)
    width = heads * S if per_head else S
    scale = 1.0 if per_head else 1.0 / heads
    out = torch.full((N, width), float("nan"), device=DEV)
    ops.cross_attn_probs(q.to(DEV), d, kv.to(DEV), 3 * d, d, lens.to(DEV), valid.to(DEV), out, width, N, N_IMG, S, d, heads,
                         per_head=per_head, scale=scale)
    got = out.cpu()
    ref = want.reshape(N, heads * S) if per_head else want.mean(1)
    close(got, ref, KERNEL_BOUND, f"cross_attn_probs rows={rows} S={S} d={d} heads={heads} per_head={per_head}")
    # exact: 0 at the masked keys of a valid row with a key left; 1/S in a row_valid = 0 row and in the enc_len = 0 image
    g3 = got.view(N, heads if per_head else 1, S)
    live = allow.any(-1)                                                                    # rows with a key to look at
    masked = (~allow & live[:, None])[:, None, :].expand_as(g3)
    assert rows == 1 or (live.any() and (S == 1 or masked.any()))         # (rows = 1: the only row of every image is the invalid one)
    assert torch.equal(g3[masked], torch.zeros_like(g3[masked]))
    assert (~live).sum() >= rows + 2                                                        # the third image and two rows
    uniform = torch.tensor(1.0, dtype=torch.float32) / S                                    # fl(1/S); heads are powers of 2
    assert torch.equal(g3[~live], uniform.expand_as(g3[~live]))
    sums = g3.double().sum(-1)
    print(f"  row sums deviate from 1 by at most {float((sums - 1).abs().max()):.3e}")
    assert float((sums - 1).abs().max()) <= 1e-5              # scale·heads = 1 (head mean), scale = 1 per head


def test_cross_attn_probs_accumulate_adds_what_overwrite_stores(ops):
    rows, S, d, heads = 7, 37, 128, 4
    N = N_IMG * rows
    for per_head in (0, 1):
        width = heads * S if per_head else S
        outs = []
        for seed, scale in ((0, 0.125), (10, 1.0 / 3)):
            q, kv, lens, valid, _, _ = probs_case(rows, S, d, heads, seed=seed)
            args = (q.to(DEV), d, kv.to(DEV), 3 * d, d, lens.to(DEV), valid.to(DEV))
            o = torch.full((N, width), float("nan"), device=DEV)
            ops.cross_attn_probs(*args, o, width, N, N_IMG, S, d, heads, per_head=per_head, scale=scale)
            outs.append((args, scale, o))
        both = torch.full((N, width), float("nan"), device=DEV)
        ops.cross_attn_probs(*outs[0][0], both, width, N, N_IMG, S, d, heads, per_head=per_head, scale=outs[0][1])
        assert torch.equal(both, outs[0][2])
        ops.cross_attn_probs(*outs[1][0], both, width, N, N_IMG, S, d, heads, per_head=per_head, scale=outs[1][1],
                             accumulate=True)
        assert torch.equal(both, outs[0][2] + outs[1][2]), per_head
        assert not torch.equal(both, outs[0][2])


@pytest.mark.parametrize("per_head", [0, 1])
@pytest.mark.parametrize("rows,S,d,heads", [(23, 144, 128, 4), (7, 5, 128, 4)])
def test_cross_attn_probs_containment(ops, rows, S, d, heads, per_head):
    """ldo above the row width, ldq above d, ldkv above the kv width: the bands and padding columns of the output keep their
    poison, every owned element is written, and no input padding is read (it is NaN)."""
    N = N_IMG * rows
    q, kv, lens, valid, _, _ = probs_case(rows, S, d, heads)
    width = heads * S if per_head else S
    ref = torch.full((N, width), float("nan"), device=DEV)
    ops.cross_attn_probs(q.to(DEV), d, kv.to(DEV), 3 * d, d, lens.to(DEV), valid.to(DEV), ref, width, N, N_IMG, S, d, heads,
                         per_head=per_head, scale=0.25)
    ldq, ldkv, ldo = d + 4, 3 * d + 8, width + 3
    gq = guards.poisoned_input(q, N, d, ldq, device=DEV)
    gkv = guards.poisoned_input(kv, S, 3 * d, ldkv, batch=N_IMG, stride=S * ldkv, device=DEV)
    gl = guards.poisoned_input(lens, 1, N_IMG, N_IMG, device=DEV)
    gv = guards.poisoned_input(valid, 1, N, N, device=DEV)
    o = guards.guarded(N, width, ldo, torch.float32, DEV)
    ops.cross_attn_probs(gq.t, ldq, gkv.t, ldkv, d, gl.t, gv.t, o.t, ldo, N, N_IMG, S, d, heads, per_head=per_head,
                         scale=0.25)
    torch.cuda.synchronize()
    o.assert_untouched(what="cross_attn_probs")
    for gi in (gq, gkv, gl, gv):
        gi.assert_untouched(what="cross_attn_probs input")
    owned = o.t[:, :width]
    assert bool(torch.isfinite(owned).all())                  # every owned element was written (poison is NaN)
    assert torch.equal(owned, ref)
    # accumulate reads and writes the same elements and nothing else
    ops.cross_attn_probs(gq.t, ldq, gkv.t, ldkv, d, gl.t, gv.t, o.t, ldo, N, N_IMG, S, d, heads, per_head=per_head,
                         accumulate=True, scale=0.25)
    torch.cuda.synchronize()
    o.assert_untouched(what="cross_attn_probs accumulate")
    assert torch.equal(o.t[:, :width], ref + ref)
    o2 = guards.guarded(N, width, ldo, torch.float32, DEV)
    for bad in (dict(ldq=d + 3), dict(ldo=width - 1)):        # refused before any launch: nothing is written
        kw = dict(ldq=ldq, ldo=ldo)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.cross_attn_probs(gq.t, kw["ldq"], gkv.t, ldkv, d, gl.t, gv.t, o2.t, kw["ldo"], N, N_IMG, S, d, heads,
                                 per_head=per_head)
    torch.cuda.synchronize()
    o2.assert_all_poison("refused cross_attn_probs")


# ------------------------------------------------------------------------------------------------- 2. the model
@pytest.fixture(scope="module")
def e2e_all():
    """word_attention(layers="all", heads="mean") on the e2e set, computed once."""
    fx, y, pads, caps, real = fixture_set("e2e")
    m = build_model("xavier")
    img = W.synth_images(3, W.TINY).to(DEV)
    return m, img, m.word_attention(img, caps, captions_per_image=2, layers="all", heads="mean")


def test_word_attention_matches_the_reference_fixture(e2e_all):
    fx, y, pads, caps, real = fixture_set("e2e")
    m, img, wa = e2e_all
    g = W.TINY
    want = torch.from_numpy(fx["e2e.head_mean"])                                    # [6, L, 23, 144]
    got = wa.maps.cpu()
    assert tuple(got.shape) == tuple(want.shape) == (6, g.N_dec, 23, 144) and got.dtype == torch.float32
    sel = real[:, None, :, None].expand_as(got)
    close(got[sel], want[sel], MODEL_BOUND, "word_attention e2e, head mean per layer")
    assert torch.equal(got[~sel], torch.zeros_like(got[~sel]))                      # padded rows are exactly 0
    assert wa.tokens == caps and wa.grid == (12, 12)
    assert torch.equal(wa.lengths.cpu(), real.sum(-1)) and wa.lengths.dtype == torch.int64
    assert torch.equal(wa.enc_lengths.cpu(), torch.full((6,), 144)) and wa.enc_lengths.dtype == torch.int64
    for n in range(6):
        assert tuple(wa.word_maps(n).shape) == (g.N_dec, int(real[n].sum()), 144)
    # per head, captions 0 and 2
    rows = fx["e2e.per_head_rows"].tolist()
    ph = m.word_attention(img, caps, captions_per_image=2, layers="all", heads="all").maps.cpu()
    assert tuple(ph.shape) == (6, g.N_dec, g.num_heads, 23, 144)
    want_ph = torch.from_numpy(fx["e2e.per_head"])
    sel_ph = real[rows][:, None, None, :, None].expand_as(want_ph)
    close(ph[rows][sel_ph], want_ph[sel_ph], MODEL_BOUND, "word_attention e2e, per head")
    close(ph.mean(2), got, 1e-6, "head mean of heads='all' vs heads='mean'")
    # layers="mean" is the mean of layers="all"
    mean = m.word_attention(img, caps, captions_per_image=2).maps.cpu()
    assert tuple(mean.shape) == (6, 23, 144)
    d = float((mean.double() - got.double().mean(1)).abs().max())
    print(f"layers='mean' vs the mean of layers='all': {d:.3e}")
    assert d <= 1e-7
    # a list of layers, negative indices: the same maps in the order asked for
    pick = m.word_attention(img, caps, captions_per_image=2, layers=[-1, 0]).maps.cpu()
    assert torch.equal(pick[:, 0], got[:, g.N_dec - 1]) and torch.equal(pick[:, 1], got[:, 0])
    one = m.word_attention(img, caps, captions_per_image=2, layers=1).maps.cpu()
    assert torch.equal(one[:, 0], got[:, 1])
    mh = m.word_attention(img, caps, captions_per_image=2, heads="all").maps.cpu()   # layers="mean" with heads="all"
    assert tuple(mh.shape) == (6, g.num_heads, 23, 144)
    assert float((mh.double() - ph.double().mean(1)).abs().max()) <= 1e-7


def test_peak_cells_match_the_reference_fixture(e2e_all):
    fx, y, pads, caps, real = fixture_set("e2e")
    m, img, wa = e2e_all
    want_mean = torch.from_numpy(fx["e2e.head_mean"]).mean(1)
    sure = real & (torch.from_numpy(fx["e2e.margin"]) > 2 * MODEL_BOUND * float(want_mean[real].max()))
    excluded = float((real & ~sure).sum()) / float(real.sum())
    print(f"peak cells: {100 * excluded:.2f} % of the real positions excluded by the margin rule")
    assert excluded <= 0.01
    peaks = wa.peak_cells().cpu()
    assert torch.equal(peaks[sure], torch.from_numpy(fx["e2e.peak"]).long()[sure])
    assert bool((peaks[~real] == -1).all())
    assert torch.equal(m.word_attention(img, caps, captions_per_image=2).peak_cells().cpu()[sure], peaks[sure])
    assert tuple(wa.heatmaps(24).shape) == (6, 23, 24, 24)
    assert wa.cell_box(int(peaks[1, 0]), 384) == tuple(32 * v for v in (int(peaks[1, 0]) % 12, int(peaks[1, 0]) // 12,
                                                                        int(peaks[1, 0]) % 12 + 1, int(peaks[1, 0]) // 12 + 1))


def test_word_attention_on_the_features_only_model():
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import make_drop_args
    from on_device_image_captioning_amd.ExpansionNet_v2 import ExpansionNet_v2
    fx, y, pads, caps, real = fixture_set("feat")
    g, fd = W.TINY, 64
    sd = cached_state_dict("TINY", "eos", end_to_end=False, img_feature_dim=fd)
    m = ExpansionNet_v2(d_model=g.d_model, N_enc=g.N_enc, N_dec=g.N_dec, ff=g.ff, num_heads=g.num_heads,
                        num_exp_enc_list=list(g.num_exp_enc_list), num_exp_dec=g.num_exp_dec,
                        output_word2idx={i: i for i in range(g.vocab_size)}, output_idx2word=list(range(g.vocab_size)),
                        max_seq_len=g.max_seq_len, drop_args=make_drop_args(), img_feature_dim=fd, rank=DEV)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    epads = fx["feat.enc_pads"].tolist()
    assert epads == [0, 3, 7, 1]
    feats = W.synth_features(4, 20, fd)
    wa = m.word_attention(feats.to(DEV), caps, epads, layers="all")
    want = torch.from_numpy(fx["feat.head_mean"])                                   # [4, L, 23, 20]
    got = wa.maps.cpu()
    sel = real[:, None, :, None].expand_as(got)
    close(got[sel], want[sel], MODEL_BOUND, "word_attention features-only, head mean per layer")
    assert torch.equal(got[~sel], torch.zeros_like(got[~sel]))
    for n, p in enumerate(epads):                                                   # keys at or past the valid length
        assert torch.equal(got[n, :, :, 20 - p:], torch.zeros_like(got[n, :, :, 20 - p:])), n
    assert wa.grid is None and torch.equal(wa.enc_lengths.cpu(), torch.tensor([20, 17, 13, 19]))
    with pytest.raises(ValueError, match="grid"):
        wa.heatmaps(24)
    sure = real & (torch.from_numpy(fx["feat.margin"]) > 2 * MODEL_BOUND * float(want.mean(1)[real].max()))
    assert float((real & ~sure).sum()) <= 0.01 * float(real.sum())
    assert torch.equal(wa.peak_cells().cpu()[sure], torch.from_numpy(fx["feat.peak"]).long()[sure])


# ------------------------------------------------------------------------------------------------- 3. nothing else moved
def test_attn_leaves_the_statistics_bit_identical(ops):
    fx, y, pads, caps, real = fixture_set("e2e")
    m = build_model("xavier")
    eng = m._captioner_engine()
    img = W.synth_images(3, W.TINY).to(DEV)
    mem = m.forward_enc(img, [0] * 3)
    kv, enc_len = eng.project_kv(mem), m._enc_lens(3, mem.shape[1], None)
    dec, tgt = y[:, :-1].contiguous().to(DEV), y[:, 1:].contiguous().to(DEV)
    dec_len = torch.tensor([y.shape[1] - 1 - p for p in pads], dtype=torch.int32, device=DEV)
    counts = []
    res = []
    for attn in (None, {"layers": [0, 1], "per_head": False, "reduce_layers": True},
                 {"layers": [1], "per_head": True, "reduce_layers": False}):
        with ops.profile() as recs:
            res.append(eng.decode_sequence(dec, dec_len, kv, enc_len, 3, targets=tgt, attn=attn))
            counts.append([r[0] for r in recs])
    base = res[0]
    assert "attn" not in base and "cross_attn_probs" not in counts[0]
    for r, names, extra in zip(res[1:], counts[1:], (2, 1)):
        for k in ("logp", "sum_logp", "argmax", "max_logp"):
            assert torch.equal(r[k], base[k]), k
        assert names.count("cross_attn_probs") == extra and len(names) == len(counts[0]) + extra
        assert [n for n in names if n != "cross_attn_probs"] == counts[0]
    assert tuple(res[1]["attn"].shape) == (6, 23, 144) and tuple(res[2]["attn"].shape) == (6, 1, W.TINY.num_heads, 23, 144)
    # padded rows hold the masked row's uniform 1/S (the API zeroes them)
    pad_rows = res[1]["attn"].cpu()[~real]
    assert torch.equal(pad_rows, (torch.tensor(1.0) / 144).expand_as(pad_rows))
    # score_captions on the same set still meets its fixture
    sfx = np.load(os.path.join(GOLDEN, "tiny_scoring.npz"))
    sc = m.score_captions(img, caps, captions_per_image=2)
    err = float((sc.logprobs.cpu() - torch.from_numpy(sfx["xavier.fresh.logp_target"]))[real].abs().max())
    print(f"score_captions xavier/fresh after the attn passes: log-prob max err {err:.3e}")
    assert err <= MODEL_BOUND


# ------------------------------------------------------------------------------------------------- 4. invariances
def test_word_attention_invariances(e2e_all):
    fx, y, pads, caps, real = fixture_set("e2e")
    m, img, wa = e2e_all
    # captions_per_image = 2 against the same captions with each image repeated
    one = m.word_attention(img.repeat_interleave(2, 0), caps, layers="all")
    assert torch.equal(one.maps, wa.maps)
    # the padded-tensor form of the captions
    t = m.word_attention(img, y, captions_per_image=2, dec_x_num_pads=pads, layers="all")
    assert torch.equal(t.maps, wa.maps) and t.tokens == caps
    # causality: other tokens behind position t (same lengths) leave the rows <= t alone
    t0 = 4
    caps2 = [c[:t0 + 1] + [4 + (v + 17) % (W.TINY.vocab_size - 4) for v in c[t0 + 1:-1]] + c[-1:] if len(c) > t0 + 2 else c
             for c in caps]
    assert caps2 != caps and [len(c) for c in caps2] == [len(c) for c in caps]
    other = m.word_attention(img, caps2, captions_per_image=2, layers="all")
    a, b = wa.maps[:, :, :t0 + 1].cpu(), other.maps[:, :, :t0 + 1].cpu()
    print(f"rows <= {t0} after changing the tokens behind them: bitwise equal = {torch.equal(a, b)}, "
          f"max diff {float((a - b).abs().max()):.3e}")
    assert float((a - b).abs().max()) <= MODEL_BOUND * float(a.abs().max())
    assert not torch.equal(wa.maps[:, :, t0 + 1:], other.maps[:, :, t0 + 1:])


def test_word_attention_of_generated_captions():
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import E2E_ExpansionNet_Captioner
    m = build_model("eos")
    img = W.synth_images(3, W.TINY).to(DEV)
    wa = m.word_attention(img, None, sos_idx=TSOS, eos_idx=TEOS, beam_size=3, max_seq_len=12)
    best, _ = m.beam_search(img, [0] * 3, sos_idx=TSOS, eos_idx=TEOS, beam_size=3, how_many_outputs=1, max_seq_len=12)
    assert wa.tokens == [per[0] for per in best]
    again = m.word_attention(img, wa.tokens)
    assert torch.equal(again.maps, wa.maps) and torch.equal(again.lengths, wa.lengths)
    sums = wa.maps.sum(-1).cpu()
    real = torch.arange(wa.maps.shape[1])[None, :] < wa.lengths.cpu()[:, None]
    assert float((sums[real] - 1).abs().max()) <= 1e-5 and bool((sums[~real] == 0).all())
    cap = E2E_ExpansionNet_Captioner({"sos_idx": TSOS, "eos_idx": TEOS, "beam_size": 3, "beam_max_seq_len": 12}, model=m)
    c = cap.word_attention(img)
    assert c.tokens == wa.tokens and torch.equal(c.maps, wa.maps)
    assert torch.equal(cap.word_attention(img, wa.tokens, layers="all").maps, m.word_attention(img, wa.tokens, layers="all").maps)
