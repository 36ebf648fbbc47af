"""Stochastic beam search end to end on the GPU (`-m gpu`): TINY geometry, the synthetic "eos" checkpoint,
four synthetic images, fp32, max_seq_len 12, num_samples 1 and 4.

The search is replayed in the numpy model of tests/stochastic_beam_model.py from the candidates the device produced at
every step (the `_cand_log` hook, which carries cand_pert here), which takes the decoder's rounding out of the comparison.
The other tests pin what the search means: distinct captions in sampling order, the model's own log-probs (score_captions,
the 2e-3 of test_sample_filter_gpu.agree_with_score_captions), the three ways in (method, forward mode, Captioner), consensus
over its candidates, the refusals, and that the existing searches launch what they launched before.
"""
import numpy as np
import pytest
import torch

import stochastic_beam_model as SM
from conftest import cached_state_dict
from on_device_image_captioning_amd import weights as W
from test_sample_filter_gpu import agree_with_score_captions

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
SOS, EOS = 3, 2
N_IMG, MAX_LEN, SEED = 4, 12, 20190611
F = np.float32


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=DEV)
    m.load_state_dict(cached_state_dict("TINY", "eos"), strict=True)
    return m.to(DEV).eval().set_precision("fp32")


@pytest.fixture(scope="module")
def images():
    return W.synth_images(N_IMG, W.TINY).to(DEV)


@pytest.fixture(scope="module")
def baseline(model, images):
    """What the existing searches return BEFORE any stochastic call of this module (module fixtures run in the order the
    `runs` fixture asks for them)."""
    model.sampling_seed, model._sampling_calls = 5, 0
    beam = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=2, max_seq_len=MAX_LEN)
    samp = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="sampling", how_many_outputs=3, sample_max_seq_len=10,
                 sos_idx=SOS, eos_idx=EOS)
    return beam, samp, model._sampling_calls


def search(model, images, n, log=None, seed=SEED, **kw):
    model._cand_log = log
    try:
        return model.stochastic_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_samples=n, max_seq_len=MAX_LEN,
                                            seed=seed, **kw)
    finally:
        model._cand_log = None


@pytest.fixture(scope="module")
def runs(baseline, model, images):
    out = {}
    for n in (1, 4):
        log = []
        toks, lps = search(model, images, n, log=log)
        out[n] = (toks, lps.cpu(), log, {k: v.cpu() for k, v in model.last_stochastic_beam.items()})
    return out


@pytest.mark.parametrize("n", (1, 4))
def test_captions_are_distinct_and_in_sampling_order(runs, n):
    toks, lps, _, last = runs[n]
    assert len(toks) == N_IMG and lps.shape[:2] == (N_IMG, n)
    for per in toks:
        assert len(per) == n and all(c[0] == SOS for c in per)
        assert len({tuple(c) for c in per}) == n
    g, kappa, phi = last["gumbel"], last["kappa"], last["sum_logprob"]
    assert tuple(g.shape) == (N_IMG, n) and tuple(kappa.shape) == (N_IMG,) and tuple(phi.shape) == (N_IMG, n)
    assert g.dtype == kappa.dtype == phi.dtype == torch.float32
    assert bool((g[:, :-1] >= g[:, 1:]).all()) and bool((g[:, -1] >= kappa).all()) and bool(torch.isfinite(g).all())
    # sum_logprob: the fp32 sum, in position order, of the returned log-probs
    for b in range(N_IMG):
        for j in range(n):
            cs = F(0)
            for v in lps[b, j, :len(toks[b][j])].numpy():
                cs = F(cs + v)
            assert cs == phi[b, j].numpy(), (b, j)


@pytest.mark.parametrize("n", (1, 4))
def test_logprobs_are_the_models_own(runs, model, images, n):
    toks, lps, _, _ = runs[n]
    agree_with_score_captions(model, images, toks, lps)


@pytest.mark.parametrize("n", (1, 4))
def test_replay_of_the_logged_candidates_gives_the_same_captions_exactly(runs, n):
    toks, lps, log, last = runs[n]
    assert 1 <= len(log) <= MAX_LEN - 1
    k = n + 1
    st = SM.new_state(N_IMG, k, MAX_LEN, SOS)
    g = np.zeros(N_IMG * k, F)
    err = np.zeros(N_IMG * k)                                         # what the device's G may differ from the replay's by
    for t, (cv, ci, cp) in enumerate(log):
        assert tuple(cv.shape) == tuple(ci.shape) == tuple(cp.shape) == (N_IMG * k, k)
        st, gnew, band, offers = SM.step(st, g, cv.numpy(), ci.numpy(), cp.numpy(), EOS)
        for b, o in enumerate(offers):
            assert SM.is_clear(o, k, slack=err[b * k:(b + 1) * k]), "a near tie: the replay cannot decide this step"
        g = gnew.astype(F)
        # a child's G~ follows its parent's G at a slope of at most 1, plus the band of the step and the fp32 store
        err = (err[st["anc"][:, t]] if t else 0.0) + band + SM.EPS * np.abs(np.where(np.isfinite(gnew), gnew, 0.0))
    for b in range(N_IMG):
        for j in range(n):
            ne = int(st["n_elem"][b * k + j])
            assert toks[b][j] == st["tokens"][b, j, :ne].tolist(), (b, j)
            assert np.array_equal(lps[b, j, :ne].numpy(), st["logprobs"][b, j, :ne]), (b, j)
    dev_g = torch.cat([last["gumbel"], last["kappa"][:, None]], dim=1).numpy().astype(np.float64)
    want_g = g.reshape(N_IMG, k).astype(np.float64)
    assert np.array_equal(np.isneginf(dev_g), np.isneginf(want_g))
    with np.errstate(invalid="ignore"):
        diff = np.where(np.isneginf(want_g), 0.0, np.abs(dev_g - want_g))
    print(f"n={n}: worst |G - replay| = {diff.max():.3e}, bound there {err.reshape(N_IMG, k).flat[diff.argmax()]:.3e}")
    assert np.all(diff <= err.reshape(N_IMG, k) + SM.EPS * np.abs(dev_g))


def test_forward_mode_and_captioner_return_what_the_method_returns(runs, model, images):
    from on_device_image_captioning_amd.captioning_model import Captioner
    toks, lps, _, _ = runs[4]
    t2, l2 = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="stochastic_beam_search", num_samples=4,
                   beam_max_seq_len=MAX_LEN, seed=SEED, sos_idx=SOS, eos_idx=EOS)
    assert t2 == toks and torch.equal(l2.cpu(), lps)
    cap = Captioner(dict(sos_idx=SOS, eos_idx=EOS, num_samples=4, beam_max_seq_len=MAX_LEN, seed=SEED), model=model)
    t3, l3 = cap(images, enc_x_num_pads=[0] * N_IMG, mode="stochastic_beam_search")
    assert t3 == toks and torch.equal(l3.cpu(), lps)
    # another seed gives other captions; no seed draws one from torch's generator
    t4, _ = search(model, images, 4, seed=SEED + 1)
    assert t4 != toks
    torch.manual_seed(7)
    a, _ = search(model, images, 4, seed=None)
    torch.manual_seed(7)
    b, _ = search(model, images, 4, seed=None)
    c, _ = search(model, images, 4, seed=None)
    assert a == b and a != c


def test_consensus_over_stochastic_beam_candidates(runs, model, images):
    best, scores = model.consensus_caption(images, [0] * N_IMG, num_candidates=4, source="stochastic_beam", sos_idx=SOS,
                                           eos_idx=EOS, max_seq_len=MAX_LEN, seed=SEED)
    cands, index, _ = model.last_consensus
    assert cands == runs[4][0]                                        # the same seed: the same candidates
    for b, per in enumerate(cands):
        assert len({tuple(c) for c in per}) == 4 and best[b] == per[int(index[b])]
    assert tuple(scores.shape) == (N_IMG,)


@pytest.mark.parametrize("kw", [dict(prefix=[7, 8]), dict(required_words=[9]), dict(no_repeat_ngram_size=2), dict(min_length=2),
                                dict(banned_words=[11]), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9),
                                dict(num_samples=0), dict(num_samples=16)])
def test_every_refused_keyword_raises(model, images, kw):
    n = kw.pop("num_samples", 3)
    with pytest.raises(ValueError, match="stochastic_beam_search|num_samples"):
        search(model, images, n, **kw)


def test_the_existing_searches_return_what_they_returned_before(baseline, runs, model, images):
    (btoks, blps), (stoks, slps), calls_after = baseline
    assert model._sampling_calls == calls_after                       # the stochastic calls left the sampling counter alone
    model.sampling_seed, model._sampling_calls = 5, 0
    toks, lps = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=2,
                                  max_seq_len=MAX_LEN)
    assert toks == btoks and torch.equal(lps.cpu().view(torch.int32), blps.cpu().view(torch.int32))
    toks, lps = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="sampling", how_many_outputs=3, sample_max_seq_len=10,
                      sos_idx=SOS, eos_idx=EOS)
    assert toks == stoks and torch.equal(lps.cpu().view(torch.int32), slps.cpu().view(torch.int32))
