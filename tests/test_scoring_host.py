"""Caption scoring without a GPU: the closed-form label-smoothing loss against nn.KLDivLoss and against the recorded
results of the reference's LabelSmoothingLoss (tests/golden/tiny_scoring.npz, tools/make_golden_scoring.py), the oracle
against that fixture, argument validation of the whole-sequence entry points, and caption packing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, cached_state_dict
from on_device_image_captioning_amd import weights as W

torch.set_grad_enabled(False)
FIX = os.path.join(GOLDEN, "tiny_scoring.npz")
LP_BOUND = {"xavier": 2e-4, "eos": 1e-3}
SETS = [(v, s) for v in ("xavier", "eos") for s in ("teacher", "fresh")]


def kl_loss(logits, target, ignore_index, smoothing, divide):
    """losses/loss.py:15-39 written out with nn.KLDivLoss, on the CPU."""
    pred = torch.log_softmax(logits, -1)
    N, T, V = pred.shape
    prob = torch.full((N, T, V), smoothing / (V - 1), dtype=pred.dtype)
    prob.scatter_(2, target.clamp(0, V - 1).unsqueeze(2), 1 - smoothing)
    ign = target == ignore_index
    prob.masked_fill_(ign.unsqueeze(2), 0)
    tot = torch.nn.KLDivLoss(reduction="none")(pred, prob).masked_fill(ign.unsqueeze(2), 0.0).sum()
    return tot / (~ign).sum() if divide else tot


def oracle_logp(variant, name):
    from oracle import expansionnet_ref as R
    fx = np.load(FIX)
    g = W.TINY
    k = f"{variant}.{name}."
    y = torch.from_numpy(fx[k + "tokens"]).long()
    pads = fx[k + "pads"].tolist()
    per = int(fx[k + "per_image"])
    img = W.synth_images(3, g).repeat_interleave(per, 0)
    sd = cached_state_dict("TINY", variant)
    lp = R.forward_teacher(sd, g, img, y[:, :-1], [0] * y.shape[0], pads, log_softmax=True)
    return fx, k, y, pads, lp


@pytest.mark.parametrize("variant,name", SETS)
def test_oracle_reproduces_the_scoring_fixture(variant, name):
    fx, k, y, pads, lp = oracle_logp(variant, name)
    tgt = y[:, 1:]
    Ty = y.shape[1]
    real = torch.arange(Ty - 1)[None, :] < (Ty - 1 - torch.tensor(pads))[:, None]
    got = lp.gather(-1, tgt[..., None])[..., 0]
    want = torch.from_numpy(fx[k + "logp_target"])
    assert float((got - want).abs().max()) <= 0.25 * LP_BOUND[variant]
    ssum = torch.from_numpy(fx[k + "sum_logp"])
    assert float(((lp.double().sum(-1).float() - ssum).abs() / ssum.abs()).max()) <= 1e-5
    sure = real & (torch.from_numpy(fx[k + "margin"]) > 2 * LP_BOUND[variant])
    assert float((real & ~sure).sum()) <= 0.01 * float(real.sum())
    assert torch.equal(lp.argmax(-1)[sure], torch.from_numpy(fx[k + "argmax"]).long()[sure])


@pytest.mark.parametrize("variant,name", SETS)
def test_closed_form_loss_matches_kldiv_and_the_reference(variant, name):
    from on_device_image_captioning_amd.scoring import label_smoothing_loss
    fx, k, y, pads, lp = oracle_logp(variant, name)
    V = lp.shape[-1]
    tgt = y[:, 1:]
    lpt = lp.gather(-1, tgt[..., None])[..., 0]
    ssum = lp.double().sum(-1).float()
    for tag, ign in (("pad", 0), ("none", -1)):
        ignored = tgt == ign
        n_keep = int((~ignored).sum())                                 # the positions that enter the loss
        rec = fx[k + f"loss_ignore_{tag}"]
        for si, s in enumerate(fx["smoothings"].tolist()):
            for di, divide in enumerate((False, True)):
                got = float(label_smoothing_loss(lpt, ssum, ignored, V, s, divide))
                kl = float(kl_loss(lp.double(), tgt, ign, s, divide))
                # fp32 statistics against an fp64 KLDivLoss on the same log-probs: 6e-6 per position of value ~20
                scale = 1 if divide else n_keep
                assert abs(got - kl) <= 6e-6 * scale + 1e-6 * abs(kl), (tag, s, divide, got, kl)
                # against the reference's own module on the reference's logits: the oracle's log-prob error per position
                want = float(rec[si, di])
                bound = (0.25 * LP_BOUND[variant] + 6e-6) * scale + 1e-5 * abs(want)
                assert abs(got - want) <= bound, (tag, s, divide, got, want)
    assert bool((tgt == 0).any()) and not bool((tgt == -1).any())          # both cases are what they claim to be


def test_closed_form_loss_edge_cases():
    from on_device_image_captioning_amd.scoring import label_smoothing_loss
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 5, 37, generator=g, dtype=torch.float64) * 3
    tgt = torch.randint(0, 37, (2, 5), generator=g)
    tgt[1, 3:] = 7
    lp = torch.log_softmax(logits, -1)
    for s in (0.0, 0.1, 1.0):
        for divide in (False, True):
            got = label_smoothing_loss(lp.gather(-1, tgt[..., None])[..., 0].float(), lp.sum(-1).float(), tgt == 7, 37, s,
                                       divide)
            assert abs(float(got) - float(kl_loss(logits, tgt, 7, s, divide))) <= 1e-4
    with pytest.raises(ValueError):
        label_smoothing_loss(torch.zeros(1), torch.zeros(1), torch.zeros(1, dtype=torch.bool), 37, 1.5)


@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_sequence_entry_points_validate_without_a_gpu(lib):
    P = 4096                                       # any non-NULL, 16-byte aligned value: nothing is dereferenced
    # odic_dynexp_seq(lin, ldlin, qexp, bexp, dec_len, y_in, ldy_in, y, ldy, N, T, d, E, eps, stream)

    def dyn(lin=P, ldlin=None, N=2, T=9, d=128, E=4, y=P):
        return lib.odic_dynexp_seq(lin, 5 * d if ldlin is None else ldlin, P, P, P, P, d, y, d, N, T, d, E, 1e-9, None)
    assert dyn(lin=None) == -2 and dyn(y=None) == -2
    assert dyn(T=129) == -1 and dyn(E=5) == -1 and dyn(d=96) == -1 and dyn(N=0) == -1 and dyn(T=0) == -1
    assert dyn(ldlin=5 * 128 - 4) == -1 and dyn(ldlin=5 * 128 + 2) == -1 and dyn(lin=P + 4) == -1
    # odic_token_stats(logits, ldl, target, logp_target, sum_logp, argmax, max_logp, status, R, V, stream)
    assert lib.odic_token_stats(None, 10, P, P, P, P, P, P, 3, 10, None) == -2
    assert lib.odic_token_stats(P, 10, P, None, P, P, P, P, 3, 10, None) == -2      # a target needs its output ...
    assert lib.odic_token_stats(P, 10, P, P, P, P, P, None, 3, 10, None) == -2      # ... and the status word
    assert lib.odic_token_stats(P, 10, P, P, P, P, P, P, 3, 0, None) == -1          # V = 0
    assert lib.odic_token_stats(P, 9, P, P, P, P, P, P, 3, 10, None) == -1          # ldl < V
    assert lib.odic_token_stats(P, 10, P, P, P, P, P, P, 0, 10, None) == -1
    # odic_dec_embed_seq(tokens, embed, pos_table, dec_len, row_valid, y, ldy, N, T, d, vocab, pos_rows, scale, stream)
    assert lib.odic_dec_embed_seq(None, P, P, None, None, P, 128, 2, 9, 128, 500, 24, 1.0, None) == -2
    assert lib.odic_dec_embed_seq(P, P, P, None, P, P, 128, 2, 9, 128, 500, 24, 1.0, None) == -2    # row_valid without dec_len
    assert lib.odic_dec_embed_seq(P, P, P, None, None, P, 128, 2, 25, 128, 500, 24, 1.0, None) == -1  # T > pos_rows
    assert lib.odic_dec_embed_seq(P, P, P, None, None, P, 128, 2, 9, 128, 0, 24, 1.0, None) == -1    # vocab = 0
    assert lib.odic_dec_embed_seq(P, P, P, None, None, P, 64, 2, 9, 128, 500, 24, 1.0, None) == -1   # ldy < d


def test_caption_packing():
    from on_device_image_captioning_amd.scoring import pack_captions
    caps = [[3, 9, 8, 2], [3, 2], [3, 5, 6, 7, 8, 9, 2]]
    toks, lens = pack_captions(caps, max_seq_len=24)
    assert lens == [4, 2, 7] and tuple(toks.shape) == (3, 7) and toks.dtype == torch.int64
    assert toks[1].tolist() == [3, 2, 0, 0, 0, 0, 0]
    assert [toks[i, :n].tolist() for i, n in enumerate(lens)] == caps
    # padded tensor + pad counts, and trailing pads measured with pad_idx: the same packing
    padded = torch.full((3, 9), 499, dtype=torch.int64)
    for i, c in enumerate(caps):
        padded[i, :len(c)] = torch.tensor(c)
    t2, l2 = pack_captions(padded, [5, 7, 2])
    assert l2 == lens and torch.equal(t2, toks)
    t3, l3 = pack_captions(padded, pad_idx=499)
    assert l3 == lens and torch.equal(t3, toks)
    with pytest.raises(ValueError, match="at least"):
        pack_captions([[3, 4, 2], [3]])
    with pytest.raises(ValueError, match="max_seq_len"):
        pack_captions([[3] + [5] * 23 + [2]], max_seq_len=24)
    pack_captions([[3] + [5] * 22 + [2]], max_seq_len=24)               # exactly max_seq_len tokens is fine
    with pytest.raises(ValueError):
        pack_captions(padded, [5, 7])                                   # one pad count short
    with pytest.raises(ValueError):
        pack_captions(caps, [0, 0, 0])                                  # pad counts with ragged lists


def _host_model():
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    return End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                               output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank="cpu")


def test_scoring_rejects_bad_arguments_before_any_gpu_work():
    """Every ValueError of score_captions / caption_loss is raised from the host-side checks: they need neither an engine
    nor a GPU (the model here lives on the CPU)."""
    g = W.TINY
    m = _host_model()
    img = W.synth_images(2, g)
    with pytest.raises(ValueError, match="captions for 2 inputs"):
        m.score_captions(img, [[3, 5, 2], [3, 2], [3, 9, 2]])                      # 3 captions, 2 images x 1
    with pytest.raises(ValueError, match="captions for 2 inputs"):
        m.score_captions(img, [[3, 5, 2], [3, 2]], captions_per_image=2)           # 2 captions, 2 images x 2
    with pytest.raises(ValueError, match="captions for 2 inputs"):
        m.score_captions(img, [[3, 5, 2], [3, 2]], captions_per_image=0)
    with pytest.raises(ValueError, match="token ids"):
        m.score_captions(img, [[3, g.vocab_size, 2], [3, 2]])
    with pytest.raises(ValueError, match="token ids"):
        m.score_captions(img, [[3, -1, 2], [3, 2]])
    with pytest.raises(ValueError, match="at least"):
        m.score_captions(img, [[3], [3, 2]])
    with pytest.raises(ValueError, match="max_seq_len"):
        m.score_captions(img, [[3] + [5] * g.max_seq_len, [3, 2]])
    y = torch.tensor([[3, 5, 6, 2], [3, 7, 2, 0]])
    with pytest.raises(ValueError, match="two columns"):
        m.caption_loss(img, y[:, :1], [0, 0], [0, 0], 0)
    with pytest.raises(ValueError, match="token ids"):
        m.caption_loss(img, torch.tensor([[3, 5, g.vocab_size, 2], [3, 7, 2, 0]]), [0, 0], [0, 1], 0)
    with pytest.raises(ValueError, match="target rows"):
        m.caption_loss(img, y[:1], [0, 0], [0], 0)
    with pytest.raises(RuntimeError, match="expected 2 pad counts"):
        m.caption_loss(img, y, [0, 0], [0], 0)
    # an ignored target may lie outside the vocabulary (ignore_index = -100): only then does the call reach the engine
    y2 = torch.tensor([[3, 5, 6, 2], [3, 7, 2, -100]])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU"):
            m.caption_loss(img, y2.clamp(min=0), [0, 0], [0, 1], 0)


def test_scoring_has_no_cpu_fallback():
    m = _host_model()
    if not torch.cuda.is_available():          # (with a GPU a host-resident model runs on it: tests/test_scoring_gpu.py)
        with pytest.raises(RuntimeError, match="no CPU"):
            m.score_captions(W.synth_images(2, W.TINY), [[3, 5, 2], [3, 2]])
