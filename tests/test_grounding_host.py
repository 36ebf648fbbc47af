"""Word grounding without a GPU: argument validation of odic_cross_attn_probs, the WordAttention helpers on synthetic
tensors, the argument errors of word_attention, and the recorded reference maps (tests/golden/tiny_attention.npz,
tools/make_golden_attention.py) against an fp64 restatement from the oracle's pieces."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, cached_state_dict
from on_device_image_captioning_amd import weights as W

torch.set_grad_enabled(False)
FIX = os.path.join(GOLDEN, "tiny_attention.npz")


@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


# ------------------------------------------------------------------------------------------------- 1. the C entry
def test_cross_attn_probs_is_declared_exported_and_bound(lib):
    from on_device_image_captioning_amd import _hip
    assert "odic_cross_attn_probs" in _hip.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "odic_hip.h")).read()
    assert "int odic_cross_attn_probs(" in header
    fn = lib.odic_cross_attn_probs
    assert len(fn.argtypes) == 18 and lib.odic_abi_version() == _hip.ABI_VERSION >= 20


def test_cross_attn_probs_validates_without_a_gpu(lib):
    P = 4096                                       # any non-NULL, 16-byte aligned value: nothing is dereferenced

    def call(q=P, ldq=128, kv=P, ldkv=256, koff=128, enc_len=P, row_valid=P, out=P, ldo=None, N=6, n_img=3, S=144, d=128,
             heads=4, per_head=0):
        ldo = (heads * S if per_head else S) if ldo is None else ldo
        return lib.odic_cross_attn_probs(q, ldq, kv, ldkv, koff, enc_len, row_valid, out, ldo, N, n_img, S, d, heads,
                                         per_head, 0, 1.0, None)
    for name in ("q", "kv", "enc_len", "row_valid", "out"):
        assert call(**{name: None}) == -2, name
    assert call(heads=3) == -1                                  # d % heads
    assert call(heads=1) == -1 and call(d=32, ldq=32, heads=4) == -1      # d / heads = 128, 8: not in {16, 32, 64}
    assert call(S=0) == -1 and call(N=0) == -1 and call(N=7) == -1        # N % n_img
    assert call(ldq=130) == -1 and call(ldkv=258) == -1 and call(koff=126) == -1
    assert call(ldo=143) == -1 and call(per_head=1, ldo=4 * 144 - 1) == -1
    assert call(S=8160, d=64, ldq=64, heads=1, N=3) == -1        # one row of scores and sums no longer fits the block's LDS
    # (the valid shapes — S = 576 among them — launch, and are run on the GPU: tests/test_grounding_gpu.py)


# ------------------------------------------------------------------------------------------------- 2. WordAttention
def _synthetic(grid=(12, 12), layers=None, heads=None):
    from on_device_image_captioning_amd.grounding import WordAttention
    N, T, S = 3, 5, 144
    lead = [n for n in (layers, heads) if n]
    g = torch.Generator().manual_seed(4)
    maps = torch.softmax(torch.randn(N, *lead, T, S, generator=g) * 2, -1)
    lengths = torch.tensor([5, 1, 3])
    real = (torch.arange(T)[None, :] < lengths[:, None]).view([N] + [1] * len(lead) + [T, 1])
    maps = maps * real
    toks = [[3] + [7] * (int(n) - 1) + [2] for n in lengths]
    return WordAttention(tokens=toks, maps=maps, lengths=lengths, enc_lengths=torch.full((N,), S), grid=grid)


@pytest.mark.parametrize("layers,heads", [(None, None), (2, None), (2, 4), (None, 4)])
def test_word_attention_helpers(layers, heads):
    wa = _synthetic(layers=layers, heads=heads)
    lead = [n for n in (layers, heads) if n]
    for n, want in enumerate([5, 1, 3]):
        wm = wa.word_maps(n)
        assert list(wm.shape) == lead + [want, 144]
        assert torch.equal(wm, wa.maps[n][..., :want, :]) and bool((wm.sum(-1) - 1).abs().max() < 1e-5)
    mean = wa.maps
    for _ in lead:
        mean = mean.mean(1)
    peaks = wa.peak_cells()
    assert peaks.dtype == torch.int64 and tuple(peaks.shape) == (3, 5)
    real = torch.arange(5)[None, :] < wa.lengths[:, None]
    assert torch.equal(peaks[real], mean.argmax(-1)[real]) and bool((peaks[~real] == -1).all())
    hm = wa.heatmaps(48)
    assert tuple(hm.shape) == (3, 5, 48, 48) and tuple(wa.heatmaps((24, 36)).shape) == (3, 5, 24, 36)
    want = torch.nn.functional.interpolate(mean.view(3, 5, 12, 12), size=(48, 48), mode="bilinear", align_corners=False)
    assert torch.equal(hm, want)


def test_peak_cells_takes_the_first_of_equal_maxima():
    wa = _synthetic()
    wa.maps[0, 0] = 0
    wa.maps[0, 0, 17] = wa.maps[0, 0, 90] = 0.5
    assert int(wa.peak_cells()[0, 0]) == 17


def test_cell_box():
    wa = _synthetic()
    assert wa.cell_box(13, 384) == (32, 32, 64, 64)
    assert wa.cell_box(0, 384) == (0, 0, 32, 32) and wa.cell_box(143, 384) == (352, 352, 384, 384)
    assert wa.cell_box(11, (384, 768)) == (704, 0, 768, 32)          # row-major: position 11 is the last cell of row 0
    assert wa.cell_box(12, (100, 50)) == (0, 8, 4, 16)               # sizes that are no multiple of the grid: floor
    with pytest.raises(ValueError):
        wa.cell_box(144, 384)
    flat = _synthetic(grid=None)
    with pytest.raises(ValueError, match="grid"):
        flat.cell_box(13, 384)
    with pytest.raises(ValueError, match="grid"):
        flat.heatmaps(48)
    assert tuple(flat.peak_cells().shape) == (3, 5)                  # needs no grid


# ------------------------------------------------------------------------------------------------- 3. word_attention
def _host_model():
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    return End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                               output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank="cpu")


def test_word_attention_rejects_bad_arguments_before_any_gpu_work():
    g = W.TINY
    m = _host_model()
    img = W.synth_images(2, g)
    caps = [[3, 5, 2], [3, 2]]
    for bad in ("sum", g.N_dec, -g.N_dec - 1, [0, g.N_dec], [], [0, 0], 1.5, None, True):
        with pytest.raises(ValueError, match="layer"):
            m.word_attention(img, caps, layers=bad)
    for bad in ("max", 0, None, ["mean"]):
        with pytest.raises(ValueError, match="heads"):
            m.word_attention(img, caps, heads=bad)
    with pytest.raises(ValueError, match="captions for 2 inputs"):
        m.word_attention(img, caps + [[3, 9, 2]])
    with pytest.raises(ValueError, match="captions for 2 inputs"):
        m.word_attention(img, caps, captions_per_image=2)
    with pytest.raises(ValueError, match="token ids"):
        m.word_attention(img, [[3, g.vocab_size, 2], [3, 2]])
    with pytest.raises(ValueError, match="at least"):
        m.word_attention(img, [[3], [3, 2]])
    with pytest.raises(ValueError, match="max_seq_len"):
        m.word_attention(img, [[3] + [5] * g.max_seq_len, [3, 2]])
    for kw in ({}, {"sos_idx": 3}, {"eos_idx": 2}):
        with pytest.raises(ValueError, match="sos_idx and eos_idx"):
            m.word_attention(img, None, **kw)
    from on_device_image_captioning_amd.captioning_model import Captioner
    with pytest.raises(ValueError, match="layer"):
        Captioner({"sos_idx": 3, "eos_idx": 2}, model=m).word_attention(img, caps, layers="sum")
    if not torch.cuda.is_available():              # valid arguments reach the engine, and there is no CPU fallback
        with pytest.raises(RuntimeError, match="no CPU"):
            m.word_attention(img, caps, layers=[-1, 0], heads="all")


def test_parse_layers():
    from on_device_image_captioning_amd.grounding import parse_heads, parse_layers
    assert parse_layers("mean", 3) == ([0, 1, 2], True) and parse_layers("all", 3) == ([0, 1, 2], False)
    assert parse_layers(-1, 3) == ([2], False) and parse_layers([2, -3], 3) == ([2, 0], False)
    assert parse_heads("mean") is False and parse_heads("all") is True


def test_the_ensemble_has_no_word_attention():
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    ens = EsembleCaptioningModel([_host_model(), _host_model()], rank="cpu")
    with pytest.raises(NotImplementedError, match="member"):
        ens.word_attention(W.synth_images(2, W.TINY), [[3, 5, 2], [3, 2]])


# ------------------------------------------------------------------------------------------------- 4. the fixture
def oracle_maps(sd, g, mem, tokens, dec_pads, enc_pads):
    """The cross-attention probabilities of every decoder layer in fp64, from the oracle's pieces (decoder_forward with the
    softmax kept): [N, L, H, T, S]."""
    from oracle import expansionnet_ref as R
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    mem = mem.double()
    N, T = tokens.shape
    S, H = mem.shape[1], g.num_heads
    dk = g.d_model // H
    causal, allow = R._dec_masks(N, T, S, dec_pads, enc_pads)
    y = sd["out_embedder.embed.weight"][tokens] * math.sqrt(g.d_model) + sd["pos_encoder.weight"][:T]
    maps = []
    for i in range(g.N_dec):
        p = f"decoders.{i}"
        y = y + R.dynamic_expansion(sd, p + ".dyn_exp", R._ln(sd, p + ".norm_1", y), g.num_exp_dec, causal.double())
        x2 = R._ln(sd, p + ".norm_2", y)
        q = R._linear(sd, p + ".mha.Wq", x2).view(N, T, H, dk).transpose(1, 2)
        k = R._linear(sd, p + ".mha.Wk", mem).view(N, S, H, dk).transpose(1, 2)
        s = (torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dk)).masked_fill(allow[:, None] == 0, -1e4)
        maps.append(torch.softmax(s, -1))
        y = y + R.cross_attention(sd, p + ".mha", x2, mem, H, allow)
        y = y + R.feed_forward(sd, p + ".ff", R._ln(sd, p + ".norm_3", y))
    return torch.stack(maps, 1)


def test_the_attention_fixture_matches_the_fp64_restatement():
    """Measured: 1.25e-7 (e2e), the fp32 softmax rounding of the reference; the bound is 1e-6 absolute."""
    from oracle import expansionnet_ref as R
    fx = np.load(FIX)
    g = W.TINY
    y = torch.from_numpy(fx["e2e.tokens"]).long()
    pads = fx["e2e.pads"].tolist()
    sc = np.load(os.path.join(GOLDEN, "tiny_scoring.npz"))
    assert np.array_equal(fx["e2e.tokens"], sc["xavier.fresh.tokens"]) and np.array_equal(fx["e2e.pads"], sc["xavier.fresh.pads"])
    N, Ty = y.shape
    sd = cached_state_dict("TINY", "xavier")
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    mem = R.forward_enc(sd64, g, W.synth_images(3, g).double(), [0] * 3).repeat_interleave(N // 3, 0)
    want = oracle_maps(sd, g, mem, y[:, :-1], pads, [0] * N)                        # [N, L, H, T, S]
    real = torch.arange(Ty - 1)[None, :] < (Ty - 1 - torch.tensor(pads))[:, None]
    hm = torch.from_numpy(fx["e2e.head_mean"])
    assert tuple(hm.shape) == (6, g.N_dec, 23, 144) and hm.dtype == torch.float32
    sel = real[:, None, :, None].expand_as(hm)
    err = float((hm.double() - want.mean(2))[sel].abs().max())
    assert torch.equal(hm[~sel], torch.zeros_like(hm[~sel]))                        # rows behind a caption's end: zeros
    rows = fx["e2e.per_head_rows"].tolist()
    assert rows == [0, 2]
    ph = torch.from_numpy(fx["e2e.per_head"])
    sel = real[rows][:, None, None, :, None].expand_as(ph)
    err_ph = float((ph.double() - want[rows])[sel].abs().max())
    print(f"fixture vs fp64 restatement: head-mean {err:.3e}, per head {err_ph:.3e}")
    assert err <= 1e-6 and err_ph <= 1e-6
    mean = want.mean((1, 2))
    top2 = mean.topk(2, -1).values
    assert float((torch.from_numpy(fx["e2e.margin"]).double() - (top2[..., 0] - top2[..., 1]))[real].abs().max()) <= 1e-6
    sure = real & (torch.from_numpy(fx["e2e.margin"]) > 2 * 2e-4 * float(hm.mean(1)[real].max()))
    assert float((real & ~sure).sum()) <= 0.01 * float(real.sum())
    assert torch.equal(mean.argmax(-1)[sure], torch.from_numpy(fx["e2e.peak"]).long()[sure])
