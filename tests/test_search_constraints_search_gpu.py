"""Constrained search end to end on the GPU (`-m gpu`): the fixture of tests/test_diverse_search_gpu.py (TINY geometry, the
synthetic "eos" checkpoint, four synthetic images, fp32, max_seq_len 12).

What a constraint means is checked on the returned captions; that the selection is the model's is checked by replaying
the candidates the device logged at every step (`_cand_log`) through tests/group_beam_model.py at one group, exactly,
and by comparing every reported log-prob with score_captions (2e-3, the bound of test_diverse_search_gpu.py).

The n of the no-repeat test is chosen on the CPU from the recorded captions of this checkpoint
(tests/golden/tiny_eos.npz, beam 3, 12 positions): they repeat bigrams, so n = 2; the test asserts that the
unconstrained run on the device repeats one as well, so it cannot pass vacuously.
"""
import os

import numpy as np
import pytest
import torch

import group_beam_model as M
import search_constraints_model as SC
from conftest import GOLDEN, cached_state_dict
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
SOS, EOS = 3, 2
N_IMG, MAX_LEN, K = 4, 12, 3
F = np.float32


def recorded_ngram_choice():
    """n = 2 if a recorded caption of this checkpoint repeats a bigram, else 1 (no GPU: the golden file only)."""
    store = np.load(os.path.join(GOLDEN, "tiny_eos.npz"))
    caps = [[int(v) for v in per[0] if v >= 0] for per in store["beam3_T12.tokens"]]
    return 2 if any(SC.repeats_ngram(c, 2) for c in caps) else 1


NGRAM = recorded_ngram_choice()


def build(seed=None):
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=DEV)
    sd = cached_state_dict("TINY", "eos") if seed is None else W.synth_state_dict(g, seed=seed, variant="eos", eos_idx=EOS)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval().set_precision("fp32")


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return build()


@pytest.fixture(scope="module")
def images():
    return W.synth_images(N_IMG, W.TINY).to(DEV)


def beam(model, images, log=None, k=K, **kw):
    model._cand_log = log
    try:
        toks, lps = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=k, how_many_outputs=1,
                                      max_seq_len=MAX_LEN, **kw)
    finally:
        model._cand_log = None
    return toks, lps.cpu()


def words(c):
    return [w for w in c[1:] if w != EOS]


@pytest.fixture(scope="module")
def plain(model, images):
    return beam(model, images)


@pytest.fixture(scope="module")
def constraint_sets(plain):
    """The constraints of the tests, derived from the unconstrained captions."""
    toks, _ = plain
    banned = sorted({words(per[0])[0] for per in toks if words(per[0])})
    min_length = min(max(len(words(per[0])) for per in toks) + 2, MAX_LEN - 2)
    return dict(bans=dict(banned_words=banned), min_length=dict(min_length=min_length),
                no_repeat=dict(no_repeat_ngram_size=NGRAM),
                all=dict(banned_words=banned, min_length=min_length, no_repeat_ngram_size=NGRAM))


@pytest.fixture(scope="module")
def runs(model, images, constraint_sets):
    out = {}
    for name, kw in constraint_sets.items():
        log = []
        toks, lps = beam(model, images, log=log, **kw)
        out[name] = (toks, lps, log)
    return out


def replay(log, k):
    st = M.new_state(N_IMG, k, MAX_LEN, SOS)
    for cv, ci in log:
        assert tuple(cv.shape) == (N_IMG * k, k)
        st, _ = M.step(st, cv.numpy(), ci.numpy(), 1, k, 0.0, EOS)
    score = (st["cumul"] / st["n_elem"].astype(F)).astype(F).reshape(N_IMG, k)
    toks, lps = [], []
    for b in range(N_IMG):
        i = int(np.argmax(score[b]))
        n = int(st["n_elem"][b * k + i])
        toks.append([st["tokens"][b, i, :n].tolist()])
        lps.append(st["logprobs"][b, i, :n])
    lp = np.zeros((N_IMG, 1, max(len(r) for r in lps)), F)
    for n, r in enumerate(lps):
        lp[n, 0, :len(r)] = r
    return toks, lp


# ------------------------------------------------------------------------------------------------- defaults
def test_defaults_change_nothing(model, images, plain):
    toks, lps = plain
    t2, l2 = beam(model, images, no_repeat_ngram_size=0, min_length=0, banned_words=None)
    assert t2 == toks and torch.equal(l2.view(torch.int32), lps.view(torch.int32))
    t3, l3 = beam(model, images, banned_words=[])
    assert t3 == toks and torch.equal(l3.view(torch.int32), lps.view(torch.int32))
    d0 = model.diverse_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3,
                                   diversity_penalty=0.5, max_seq_len=MAX_LEN)
    d1 = model.diverse_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3,
                                   diversity_penalty=0.5, max_seq_len=MAX_LEN, no_repeat_ngram_size=0, min_length=0,
                                   banned_words=None)
    assert d0[0] == d1[0] and torch.equal(d0[1].cpu().view(torch.int32), d1[1].cpu().view(torch.int32))


def test_ensemble_defaults_change_nothing_and_constraints_hold(model, images, constraint_sets):
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    ens = EsembleCaptioningModel([model, build(seed=7)], DEV)
    kw = dict(sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=1, max_seq_len=MAX_LEN)
    t0, l0 = ens.ensemble_beam_search(images, [0] * N_IMG, **kw)
    t1, l1 = ens.ensemble_beam_search(images, [0] * N_IMG, no_repeat_ngram_size=0, min_length=0, banned_words=None, **kw)
    assert t0 == t1 and torch.equal(l0.cpu().view(torch.int32), l1.cpu().view(torch.int32))
    banned = sorted({words(per[0])[0] for per in t0 if words(per[0])})
    min_length = min(max(len(words(per[0])) for per in t0) + 2, MAX_LEN - 2)
    t2, l2 = ens.ensemble_beam_search(images, [0] * N_IMG, banned_words=banned, min_length=min_length,
                                      no_repeat_ngram_size=NGRAM, **kw)
    assert any(a != b for a, b in zip(t0, t2))
    for per in t2:
        c = per[0]
        assert not set(c) & set(banned) and len(words(c)) >= min_length and not SC.repeats_ngram(c, NGRAM), c
    sc = ens.score_captions(images, [per[0] for per in t2])
    for n, per in enumerate(t2):
        c = per[0]
        err = float((l2[n, 0, 1:len(c)].cpu() - sc.logprobs[n, :len(c) - 1].cpu()).abs().max())
        print(f"ensemble caption {n}: max |search - score_captions| = {err:.3e}")
        assert err <= 2e-3, n
    t3, _ = ens(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="beam_search", sos_idx=SOS, eos_idx=EOS, beam_size=K,
                how_many_outputs=1, beam_max_seq_len=MAX_LEN, banned_words=banned, min_length=min_length,
                no_repeat_ngram_size=NGRAM)
    assert t3 == t2


# ------------------------------------------------------------------------------------------------- each constraint
def test_banned_words_never_appear(plain, runs, constraint_sets):
    banned = constraint_sets["bans"]["banned_words"]
    assert banned and all(words(per[0])[0] in banned for per in plain[0] if words(per[0]))
    toks, _, _ = runs["bans"]
    for per in toks:
        assert not set(per[0]) & set(banned), per
    assert any(a != b for a, b in zip(toks, plain[0]))


def test_min_length_is_kept(plain, runs, constraint_sets, model, images):
    m = constraint_sets["min_length"]["min_length"]
    assert m == min(max(len(words(per[0])) for per in plain[0]) + 2, MAX_LEN - 2)
    toks, _, _ = runs["min_length"]
    for per in toks:
        assert len(words(per[0])) >= m, per
    # and where the unconstrained search does stop early (beam 1), so that the bound bites: asserted, not assumed
    short, _ = beam(model, images, k=1)
    n_short = min(len(words(per[0])) for per in short)
    assert any(per[0][-1] == EOS for per in short) and n_short + 2 <= MAX_LEN - 2, short
    longer, _ = beam(model, images, k=1, min_length=n_short + 2)
    for per in longer:
        assert len(words(per[0])) >= n_short + 2, per
        assert EOS not in per[0][:n_short + 2 + 1]


def test_no_ngram_repeats(plain, runs):
    assert any(SC.repeats_ngram(per[0], NGRAM) for per in plain[0]), "the unconstrained search must repeat an n-gram"
    toks, _, _ = runs["no_repeat"]
    for per in toks:
        assert not SC.repeats_ngram(per[0], NGRAM), per
    assert any(a != b for a, b in zip(toks, plain[0]))


def test_all_three_together(runs, constraint_sets):
    kw = constraint_sets["all"]
    toks, _, _ = runs["all"]
    for per in toks:
        c = per[0]
        assert not set(c) & set(kw["banned_words"]) and len(words(c)) >= kw["min_length"] and \
            not SC.repeats_ngram(c, NGRAM), c


# ------------------------------------------------------------------------------------------------- the selection is the model's
@pytest.mark.parametrize("name", ["bans", "min_length", "no_repeat", "all"])
def test_replay_of_the_logged_candidates_gives_the_same_captions_exactly(runs, name):
    toks, lps, log = runs[name]
    assert 1 <= len(log) <= MAX_LEN - 1
    want_toks, want_lp = replay(log, K)
    assert toks == want_toks
    assert tuple(lps.shape) == want_lp.shape and np.array_equal(lps.numpy(), want_lp)


@pytest.mark.parametrize("name", ["bans", "min_length", "no_repeat", "all"])
def test_logged_candidates_are_admissible_and_sorted(runs, constraint_sets, name):
    """Every candidate row the constrained step handed to odic_beam_step: value descending, then word ascending, and —
    for the steps before any beam can have finished — free of banned words and of EOS before the minimum length."""
    kw = constraint_sets[name]
    _, _, log = runs[name]
    for t, (cv, ci) in enumerate(log):
        cv, ci = cv.numpy(), ci.numpy()
        for r in range(cv.shape[0]):
            key = list(zip((-cv[r]).tolist(), ci[r].tolist()))
            assert key == sorted(key), (t, r)
        if t == 0 or "min_length" in kw and t < kw["min_length"]:
            assert not np.isin(ci, kw.get("banned_words", [])).any(), t
            if t < kw.get("min_length", 0):
                assert not (ci == EOS).any(), t


@pytest.mark.parametrize("name", ["bans", "min_length", "no_repeat", "all"])
def test_reported_log_probs_are_the_models_own(model, images, runs, name):
    toks, lps, _ = runs[name]
    caps = [per[0] for per in toks]
    sc = model.score_captions(images, caps)
    for n, c in enumerate(caps):
        err = float((lps[n, 0, 1:len(c)] - sc.logprobs[n, :len(c) - 1].cpu()).abs().max())
        print(f"{name} caption {n}: max |search - score_captions| = {err:.3e}")
        assert err <= 2e-3, n
        assert not lps[n, 0, len(c):].any(), "padding behind a caption's end is zero"


# ------------------------------------------------------------------------------------------------- diverse search, plumbing
def test_diverse_search_keeps_all_three_constraints_in_every_group(model, images, constraint_sets):
    kw = constraint_sets["all"]
    toks, lps = model.diverse_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3,
                                          diversity_penalty=0.5, max_seq_len=MAX_LEN, **kw)
    for per in toks:
        assert len(per) == 3
        for c in per:
            assert not set(c) & set(kw["banned_words"]) and len(words(c)) >= kw["min_length"] and \
                not SC.repeats_ngram(c, NGRAM), c
    caps = [c for per in toks for c in per]
    sc = model.score_captions(images, caps, captions_per_image=3)
    flat = lps.cpu().view(N_IMG * 3, -1)
    for n, c in enumerate(caps):
        assert float((flat[n, 1:len(c)] - sc.logprobs[n, :len(c) - 1].cpu()).abs().max()) <= 2e-3, n


def test_captioner_and_forward_modes_pass_the_arguments_through(model, images, runs, constraint_sets):
    from on_device_image_captioning_amd.captioning_model import Captioner
    kw = constraint_sets["all"]
    toks, lps, _ = runs["all"]
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=1, beam_max_seq_len=MAX_LEN, **kw)
    cap = Captioner(args, model=model)
    t1, l1 = cap(images, enc_x_num_pads=[0] * N_IMG, mode="beam_search")
    assert t1 == toks and torch.equal(l1.cpu(), lps)
    t2, l2 = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="beam_search", **args)
    assert t2 == toks and torch.equal(l2.cpu(), lps)
    dargs = dict(sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3, diversity_penalty=0.5, beam_max_seq_len=MAX_LEN, **kw)
    want = model.diverse_beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3,
                                     diversity_penalty=0.5, max_seq_len=MAX_LEN, **kw)
    t3, _ = Captioner(dargs, model=model)(images, enc_x_num_pads=[0] * N_IMG, mode="diverse_beam_search")
    t4, _ = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="diverse_beam_search", **dargs)
    assert t3 == want[0] and t4 == want[0]
    with pytest.raises(ValueError):
        model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="beam_search", sample_or_max="sample", **args)
