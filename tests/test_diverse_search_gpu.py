"""Diverse (group) beam search end to end on the GPU (`-m gpu`): TINY geometry, the synthetic "eos" checkpoint, four
synthetic images, fp32, max_seq_len 12.

The search is replayed in the numpy model of tests/group_beam_model.py from the candidates the device produced at every
step (the `_cand_log` hook), which takes the decoder's rounding out of the comparison: tokens and log-probs must then be
equal exactly.  The other tests pin what the search means: one group is beam_search, group 0 is never penalised, the
reported log-probs are the model's own (score_captions, the 2e-3 of test_ensemble_sampled_search_scores_equal_score_captions),
no penalty → no diversity, a huge penalty → no two groups append the same word.
"""
import numpy as np
import pytest
import torch

import group_beam_model as M
from conftest import cached_state_dict
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
SOS, EOS = 3, 2
N_IMG, MAX_LEN = 4, 12
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


def diverse(model, images, G, kg, lam, log=None, **kw):
    model._cand_log = log
    try:
        return model.diverse_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_groups=G, group_size=kg,
                                         diversity_penalty=lam, max_seq_len=MAX_LEN, **kw)
    finally:
        model._cand_log = None


def replay(log, G, kg, lam):
    """The logged candidates through the numpy model: (tokens per image and group, log-prob rows, per-step events)."""
    R = G * kg
    st = M.new_state(N_IMG, R, MAX_LEN, SOS)
    events = []
    for cv, ci in log:
        assert tuple(cv.shape) == (N_IMG * R, R)
        st, ev = M.step(st, cv.numpy(), ci.numpy(), G, kg, lam, EOS)
        events.append(ev)
    score = (st["cumul"] / st["n_elem"].astype(F)).astype(F).reshape(N_IMG, G, kg)
    toks, lps = [], []
    for b in range(N_IMG):
        per = []
        for g in range(G):
            i = g * kg + int(np.argmax(score[b, g]))          # first maximum: the lower row
            n = int(st["n_elem"][b * R + i])
            per.append(st["tokens"][b, i, :n].tolist())
            lps.append(st["logprobs"][b, i, :n])
        toks.append(per)
    width = max(len(r) for r in lps)
    lp = np.zeros((N_IMG, G, width), F)
    for n, r in enumerate(lps):
        lp[n // G, n % G, :len(r)] = r
    return toks, lp, events


@pytest.fixture(scope="module")
def runs(model, images):
    """Every (G, kg, penalty) the tests below look at, searched once with the candidate log on."""
    out = {}
    for G, kg, lam in ((3, 2, 0.5), (4, 3, 1.0), (3, 2, 0.0), (3, 2, 1e4), (4, 4, 1e4)):
        log = []
        toks, lps = diverse(model, images, G, kg, lam, log=log)
        out[(G, kg, lam)] = (toks, lps.cpu(), log)
    return out


@pytest.mark.parametrize("G,kg,lam", [(3, 2, 0.5), (4, 3, 1.0), (3, 2, 1e4)])
def test_replay_of_the_logged_candidates_gives_the_same_captions_exactly(runs, G, kg, lam):
    toks, lps, log = runs[(G, kg, lam)]
    assert 1 <= len(log) <= MAX_LEN - 1
    want_toks, want_lp, _ = replay(log, G, kg, lam)
    assert toks == want_toks
    assert tuple(lps.shape) == want_lp.shape and np.array_equal(lps.numpy(), want_lp)
    for per in toks:
        assert len(per) == G and all(c[0] == SOS for c in per)


def test_one_group_is_beam_search(model, images):
    toks, lps = diverse(model, images, 1, 3, 0.5)
    want, wlps = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=1,
                                   max_seq_len=MAX_LEN)
    assert toks == want
    assert lps.shape == wlps.shape and torch.equal(lps.cpu().view(torch.int32), wlps.cpu().view(torch.int32))


def test_group_zero_is_never_penalised(model, images, runs):
    toks, _, _ = runs[(3, 2, 0.5)]
    want, _ = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=2, how_many_outputs=1,
                                max_seq_len=MAX_LEN)
    assert [per[0] for per in toks] == [per[0] for per in want]


@pytest.mark.parametrize("G,kg,lam", [(3, 2, 0.5), (4, 3, 1.0), (3, 2, 1e4)])
def test_reported_log_probs_are_the_models_own(model, images, runs, G, kg, lam):
    toks, lps, _ = runs[(G, kg, lam)]
    caps = [c for per in toks for c in per]
    sc = model.score_captions(images, caps, captions_per_image=G)
    flat = lps.view(N_IMG * G, -1)
    for n, c in enumerate(caps):
        err = float((flat[n, 1:len(c)] - sc.logprobs[n, :len(c) - 1].cpu()).abs().max())
        print(f"caption {n}: max |search - score_captions| = {err:.3e}")
        assert err <= 2e-3, n
        assert not flat[n, len(c):].any(), "padding behind a caption's end is zero"


def test_without_a_penalty_every_group_returns_the_same_caption(runs):
    toks, lps, _ = runs[(3, 2, 0.0)]
    for b, per in enumerate(toks):
        assert all(c == per[0] for c in per), (b, per)
        assert all(torch.equal(lps[b, j], lps[b, 0]) for j in range(len(per))), b


@pytest.mark.parametrize("G,kg", [(3, 2), (4, 4)])
def test_a_huge_penalty_keeps_the_groups_on_different_words(runs, G, kg):
    toks, _, log = runs[(G, kg, 1e4)]
    for per in toks:
        firsts = [c[1] for c in per]
        assert len(set(firsts)) == G, firsts
    _, _, events = replay(log, G, kg, 1e4)
    assert G * kg <= W.TINY.vocab_size
    for t, evs in enumerate(events):
        for b, ev in enumerate(evs):
            per_group = [{int(w) for w, gr in zip(ev["word"][g * kg:(g + 1) * kg], ev["grow"][g * kg:(g + 1) * kg]) if gr}
                         for g in range(G)]
            for g in range(G):
                for h in range(g):
                    assert not (per_group[g] & per_group[h]), (t, b, g, h, per_group)


def test_the_default_penalty_does_diversify(runs):
    toks, _, _ = runs[(3, 2, 0.5)]
    assert any(len({tuple(c) for c in per}) >= 2 for per in toks), toks


def test_captioner_mode_and_forward_mode_return_what_the_method_returns(model, images, runs):
    from on_device_image_captioning_amd.captioning_model import Captioner
    toks, lps, _ = runs[(3, 2, 0.5)]
    args = dict(sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=2, diversity_penalty=0.5, beam_max_seq_len=MAX_LEN)
    cap = Captioner(args, model=model)
    t1, l1 = cap(images, enc_x_num_pads=[0] * N_IMG, mode="diverse_beam_search")
    assert t1 == toks and torch.equal(l1.cpu(), lps)
    t2, l2 = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="diverse_beam_search", **args)
    assert t2 == toks and torch.equal(l2.cpu(), lps)
    t3, l3 = cap.diverse_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=2,
                                     diversity_penalty=0.5, how_many_outputs=2, max_seq_len=MAX_LEN)
    assert t3 == [per[:2] for per in toks] and tuple(l3.shape[:2]) == (N_IMG, 2)


def test_argument_errors(model, images):
    with pytest.raises(ValueError):
        diverse(model, images, 3, 2, 0.5, how_many_outputs=4)
    with pytest.raises(ValueError):
        diverse(model, images, 3, 2, 0.5, how_many_outputs=0)
    with pytest.raises(ValueError):
        diverse(model, images, 5, 4, 0.5)                       # 20 rows per image
    with pytest.raises(ValueError):
        diverse(model, images, 3, 2, -0.1)
    with pytest.raises(ValueError):
        diverse(model, images, 3, 2, float("nan"))
