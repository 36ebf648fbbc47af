"""Pooled beam search end to end on the GPU (`-m gpu`): TINY geometry, the synthetic "eos" checkpoint, four
synthetic images, fp32, max_seq_len 12.

  (a) beam_size = 1 with early_stopping is greedy search: the tokens of beam_search(beam_size=1);
  (b) the search replayed in the float32 model of tests/pool_beam_model.py from the candidates and EOS log-probs the device
      produced at every step (the `_cand_log` hook): the same captions, scores (bit for bit) and order;
  (c) the returned per-token log-probs are the model's own: score_captions on the returned captions, within the 2e-3 the
      prefix and required-words search tests use for the same comparison;
  (d) how_many_outputs = 3: the captions of an image are distinct, and those of a closed image all end in EOS — with
      early_stopping too, under which two of the four images close within the 11 steps (without it none does here: the
      synthetic checkpoint's distributions are flat, and a pool rarely fills before the steps run out);
  (e) banned_words, no_repeat_ngram_size and min_length hold for every pooled caption;
  (f) the best caption's length does not decrease as length_penalty grows over {0, 1, 2} — and changes for one image at
      least (asserted, so that the property cannot pass vacuously on this fixture);
and the three ways in, the refusals, and that beam_search returns what it returned before any pooled call.
"""
import numpy as np
import pytest
import torch

import pool_beam_model as M
from conftest import cached_state_dict
from on_device_image_captioning_amd import weights as W
from test_sample_filter_gpu import agree_with_score_captions

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


def beam(model, images, k, n_out=1, **kw):
    return model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=k, how_many_outputs=n_out,
                             max_seq_len=MAX_LEN, **kw)


@pytest.fixture(scope="module")
def baseline(model, images):
    """beam_search BEFORE any pooled call of this module."""
    return beam(model, images, 3, 2)


def search(model, images, k=3, n_out=1, log=None, **kw):
    model._cand_log = log
    try:
        toks, lps = model.pool_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=k, how_many_outputs=n_out,
                                           max_seq_len=MAX_LEN, **kw)
    finally:
        model._cand_log = None
    return toks, lps.cpu(), model.last_pool_scores, model.last_pool_counts, model.last_pool_closed


@pytest.fixture(scope="module")
def runs(baseline, model, images):
    out = {}
    for alpha in (0.0, 1.0, 2.0):
        log = []
        out[alpha] = search(model, images, 3, 3, log=log, length_penalty=alpha) + (log,)
    return out


def test_a_greedy_equivalence(baseline, model, images):
    want, _ = beam(model, images, 1)
    toks, lps, scores, counts, closed = search(model, images, 1, 1, early_stopping=True)
    assert toks == want
    assert counts.tolist() == [1] * N_IMG and tuple(scores.shape) == (N_IMG, 1)
    for b in range(N_IMG):
        assert bool(closed[b]) == (toks[b][0][-1] == EOS)


@pytest.mark.parametrize("alpha", (0.0, 1.0, 2.0))
def test_b_replay_of_the_logged_candidates_gives_the_same_captions_scores_and_order(runs, alpha):
    toks, lps, scores, counts, closed, log = runs[alpha]
    k, T = 3, MAX_LEN
    assert 1 <= len(log) <= T - 1
    st, pool, scale = M.new_state(N_IMG, k, T), M.new_pool(N_IMG, k, T), M.scale_table(T, alpha)
    st["tokens"][:, :, 0], st["next_tok"][:] = SOS, SOS
    for cv, ci, elp in log:
        assert tuple(cv.shape) == tuple(ci.shape) == (N_IMG * k, k) and tuple(elp.shape) == (N_IMG * k,)
        live = st["row_valid"].astype(bool)
        assert not (ci.numpy()[live] == EOS).any(), "a live row's candidates never hold EOS"
        M.step(st, pool, cv.numpy(), ci.numpy(), elp.numpy(), scale, eos=EOS)
    was_closed = pool["closed"] != 0
    order, score = M.finalize(st, pool, scale)
    assert M.captions(pool, order, 3, SOS, EOS) == toks
    assert np.array_equal(score.view(np.int32), scores.numpy().view(np.int32))
    assert np.array_equal(pool["count"], counts.numpy()) and np.array_equal(was_closed, closed.numpy())
    for b in range(N_IMG):
        for j in range(3):
            n = len(toks[b][j])
            want = pool["logprobs"][b, order[b, j], :n]
            assert np.array_equal(lps[b, j, :n].numpy().view(np.int32), want.view(np.int32)) and not lps[b, j, n:].any()
    assert (np.diff(scores.numpy(), axis=1) <= 0).all()


@pytest.mark.parametrize("alpha", (0.0, 1.0, 2.0))
def test_c_logprobs_are_the_models_own(runs, model, images, alpha):
    toks, lps = runs[alpha][:2]
    agree_with_score_captions(model, images, toks, lps)


@pytest.mark.parametrize("early", (False, True))
@pytest.mark.parametrize("alpha", (0.0, 1.0, 2.0))
def test_d_outputs_are_distinct_and_finished_where_the_image_closed(runs, model, images, alpha, early):
    toks, lps, scores, counts, closed = search(model, images, 3, 3, length_penalty=alpha, early_stopping=True) if early \
        else runs[alpha][:5]
    assert tuple(scores.shape) == (N_IMG, 3) and scores.dtype == torch.float32 and tuple(counts.shape) == (N_IMG,)
    if early:
        assert bool(closed.any()), "no image of the fixture closes: the property would be vacuous"
    for b, per in enumerate(toks):
        assert len(per) == 3 and all(c[0] == SOS for c in per) and len({tuple(c) for c in per}) == 3
        assert int(counts[b]) == 3
        if closed[b]:
            assert all(c[-1] == EOS and EOS not in c[:-1] for c in per), (b, per)


def test_e_constraints_hold_for_every_pooled_caption(runs, model, images):
    free = runs[1.0][0]
    banned = sorted({w for per in free for c in per for w in c[1:-1] if w not in (SOS, EOS)})[:3]
    assert banned
    toks, lps, _, counts, _ = search(model, images, 3, 3, banned_words=banned, no_repeat_ngram_size=2, min_length=5)
    assert counts.tolist() == [3] * N_IMG
    changed = False
    for per in toks:
        for c in per:
            words = c[1:-1] if c[-1] == EOS else c[1:]
            assert not set(banned) & set(c), c
            grams = list(zip(c, c[1:]))
            assert len(set(grams)) == len(grams), c
            assert len(words) >= 5, c
            assert EOS not in words
    changed = toks != free
    assert changed
    agree_with_score_captions(model, images, toks, lps)


def test_f_best_length_is_monotone_in_the_length_penalty(runs):
    lens = {a: [len(runs[a][0][b][0]) for b in range(N_IMG)] for a in (0.0, 1.0, 2.0)}
    print("best caption lengths by length_penalty:", lens)
    for b in range(N_IMG):
        assert lens[0.0][b] <= lens[1.0][b] <= lens[2.0][b], (b, lens)
    assert lens[0.0] != lens[2.0], "no image's best caption changes length on this fixture: pick another min_length / T"


def test_the_three_ways_in_agree(runs, model, images):
    from on_device_image_captioning_amd.captioning_model import Captioner
    want = runs[2.0][0]
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=3, beam_max_seq_len=MAX_LEN, length_penalty=2.0)
    toks, _ = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="pool_beam_search", **args)
    assert toks == want
    cap = Captioner(args, model=model)
    assert cap(images, enc_x_num_pads=[0] * N_IMG, mode="pool_beam_search")[0] == want
    assert cap.pool_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=3,
                                max_seq_len=MAX_LEN, length_penalty=2.0)[0] == want


def test_refusals_reach_the_caller(model, images):
    for kw, msg in ((dict(prefix=[5]), "prefix is not supported"), (dict(required_words=[7]), "required_words is not supported"),
                    (dict(sample_or_max="sample"), "sample_or_max='sample' is not supported"),
                    (dict(length_penalty=-1.0), "length_penalty must be finite"), (dict(k=16), "beam_size must be an integer")):
        with pytest.raises(ValueError, match=msg):
            search(model, images, **kw)
    with pytest.raises(ValueError, match="temperature / top_k / top_p"):
        model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="pool_beam_search", sos_idx=SOS, eos_idx=EOS, top_k=5)


def test_beam_search_returns_what_it_returned_before(runs, baseline, model, images):
    toks, lps = beam(model, images, 3, 2)
    assert toks == baseline[0] and torch.equal(lps, baseline[1])
