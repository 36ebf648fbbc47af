"""Required words end to end on the GPU (`-m gpu`): beam_search(required_words=…) on the fixture of
tests/test_search_constraints_search_gpu.py (TINY geometry, the synthetic "eos" checkpoint, four synthetic images, fp32,
max_seq_len 12, beam 3 — here three beams per bank).

The words: for image b, the first 1 + b % 2 words that are absent from its plain beam-3 caption but lie within the top 10 of
a step of the plain beam-10 search on it (the logged candidates, steps in order) — a ragged list, one and two words in turn.
What "required" means is checked on the returned captions; that the selection is the model's is checked by replaying the
logged candidates and required-word log-probs (`_cand_log`) through tests/required_words_model.py, exactly, and by comparing
every reported log-prob with score_captions (2e-3, the bar tests/test_prefix_search_gpu.py uses for the same comparison).

A bank that holds a live row keeps one (a row loses at most C + 1 of its candidates), and the accepting bank of these images
fills within two steps, so every image must end satisfied: the test asserts at least three quarters, and that a required
caption differs from the plain one.
"""
import numpy as np
import pytest
import torch

import required_words_model as RM
import search_constraints_model as SC
from test_search_constraints_search_gpu import (DEV, EOS, K, MAX_LEN, N_IMG, SOS, beam, images, model, plain,  # noqa: F401
                                                words)
from on_device_image_captioning_amd import ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
V = 500
F = np.float32


@pytest.fixture(scope="module")
def required(model, images, plain):
    log = []
    beam(model, images, log=log, k=10)
    out = []
    for b in range(N_IMG):
        have, cands = set(plain[0][b][0]) | {SOS, EOS}, []
        for _, ci in log:
            for w in ci[b * 10:(b + 1) * 10].reshape(-1).tolist():
                if w not in have and w not in cands:
                    cands.append(w)
        out.append(cands[:1 + b % 2])
    assert [len(r) for r in out] == [1, 2, 1, 2], out
    return out


def padded(required):
    C = max(len(r) for r in required)
    return np.array([list(r) + [-1] * (C - len(r)) for r in required], np.int64)


def search(model, images, log=None, **kw):
    toks, lps = beam(model, images, log=log, **kw)
    return toks, lps, model.last_required_satisfied


@pytest.fixture(scope="module")
def run(model, images, required):
    log = []
    toks, lps, sat = search(model, images, log=log, required_words=required)
    return toks, lps, sat, log


def replay(log, required, how_many=1):
    req = padded(required)
    R = K << req.shape[1]
    st = RM.new_state(N_IMG, R, MAX_LEN, SOS)
    for cv, ci, rl in log:
        assert tuple(cv.shape) == (N_IMG * R, R) and tuple(rl.shape) == (N_IMG * R, req.shape[1])
        st, _ = RM.step(st, cv.numpy(), ci.numpy(), rl.numpy(), req, K, EOS, V)
    rows, sat = RM.outputs(st, req, K, how_many, V)
    toks = [[RM.caption(st, b, r)[0] for r in rows[b]] for b in range(N_IMG)]
    lps = [RM.caption(st, b, rows[b][0])[1] for b in range(N_IMG)]
    lp = np.zeros((N_IMG, 1, max(len(r) for r in lps)), F)
    for n, r in enumerate(lps):
        lp[n, 0, :len(r)] = r
    return toks, lp, sat, st, rows


def test_satisfied_captions_hold_their_words_and_end(plain, run, required):
    toks, _, sat, log = run
    assert len(log) == MAX_LEN - 1                                     # (a non-accepting bank never ends: no early stop)
    assert isinstance(sat, list) and len(sat) == N_IMG and all(isinstance(s, bool) for s in sat)
    assert sum(sat) * 4 >= 3 * N_IMG, sat
    assert any(s and per[0] != p[0] for s, per, p in zip(sat, toks, plain[0]))
    _, _, _, st, rows = replay(log, required)
    req = padded(required)
    for b, (per, ok) in enumerate(zip(toks, sat)):
        c = per[0]
        if not ok:
            continue
        assert all(w in c for w in required[b]), (b, c, required[b])
        assert c[-1] == EOS or len(c) == MAX_LEN, c
        assert EOS not in c[:-1]
        # the row lives in the bank whose bits are exactly the words it holds
        r = rows[b][0]
        assert r // K == RM.accepting_bank(RM.used_slots(req[b], V)) == sum(1 << i for i, w in enumerate(req[b]) if w in c)


def test_replay_of_the_logged_candidates_gives_the_same_captions_exactly(run, required):
    toks, lps, sat, log = run
    want_toks, want_lp, want_sat, _, _ = replay(log, required)
    assert toks == want_toks and sat == want_sat
    assert tuple(lps.shape) == want_lp.shape and np.array_equal(lps.numpy(), want_lp)


def test_reported_log_probs_are_the_models_own(model, images, run):
    toks, lps, _, _ = run
    caps = [per[0] for per in toks]
    sc = model.score_captions(images, caps)
    for n, c in enumerate(caps):
        err = float((lps[n, 0, 1:len(c)] - sc.logprobs[n, :len(c) - 1].cpu()).abs().max())
        print(f"caption {n}: max |search - score_captions| = {err:.3e}")
        assert err <= 2e-3, n
        assert not lps[n, 0, len(c):].any(), "padding behind a caption's end is zero"


def test_several_outputs_come_from_the_accepting_bank_in_order(model, images, required, run):
    model._cand_log = log = []
    try:
        toks, lps = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=K,
                                      max_seq_len=MAX_LEN, required_words=required)
    finally:
        model._cand_log = None
    want, _, _, _, _ = replay(log, required, how_many=K)
    assert toks == want and [per[0] for per in toks] == [per[0] for per in run[0]]
    for b, per in enumerate(toks):
        assert all(all(w in c for w in required[b]) for c in per), (b, per)


def test_nothing_required_launches_and_returns_what_plain_beam_search_does(model, images, plain):
    with ops.profile() as recs:
        beam(model, images)
    want = [r[0] for r in recs]
    for nothing in (None, [], [[] for _ in range(N_IMG)]):
        with ops.profile() as recs:
            toks, lps, sat = search(model, images, required_words=nothing)
        assert [r[0] for r in recs] == want
        assert toks == plain[0] and torch.equal(lps.view(torch.int32), plain[1].view(torch.int32)) and sat is None


def test_ragged_lists_equal_the_images_run_one_by_one(model, images, required, run):
    toks, lps, sat, _ = run
    for b in range(N_IMG):
        t1, l1 = model.beam_search(images[b:b + 1], [0], sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=1,
                                   max_seq_len=MAX_LEN, required_words=[required[b]])
        assert t1[0] == toks[b] and model.last_required_satisfied == [sat[b]]
        n = len(t1[0][0])
        assert float((l1.cpu()[0, 0, :n] - lps[b, 0, :n]).abs().max()) <= 1e-4, b


def test_bans_min_length_and_no_repeat_compose(model, images, required, run):
    everything = {w for r in required for w in r}
    banned = sorted({words(per[0])[0] for per in run[0]} - everything)
    min_length = min(max(len(words(per[0])) for per in run[0]) + 2, MAX_LEN - 2)
    assert banned
    log = []
    toks, lps, sat = search(model, images, log=log, required_words=required, banned_words=banned, min_length=min_length,
                            no_repeat_ngram_size=2)
    assert sum(sat) * 4 >= 3 * N_IMG, sat
    for b, (per, ok) in enumerate(zip(toks, sat)):
        c = per[0]
        assert not set(c) & set(banned) and len(words(c)) >= min_length and not SC.repeats_ngram(c, 2), c
        assert not ok or all(w in c for w in required[b]), (b, c)
    want_toks, want_lp, want_sat, _, _ = replay(log, required)
    assert toks == want_toks and sat == want_sat and np.array_equal(lps.numpy(), want_lp)


def test_captioner_and_forward_pass_the_keyword_through(model, images, required, run):
    from on_device_image_captioning_amd.captioning_model import Captioner
    toks, lps, sat, _ = run
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=1, beam_max_seq_len=MAX_LEN, required_words=required)
    t1, l1 = Captioner(args, model=model)(images, enc_x_num_pads=[0] * N_IMG, mode="beam_search")
    assert t1 == toks and torch.equal(l1.cpu(), lps) and model.last_required_satisfied == sat
    t2, l2 = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="beam_search", **args)
    assert t2 == toks and torch.equal(l2.cpu(), lps)


def test_every_refused_combination_raises_before_any_launch(model, images, required):
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    pads = [0] * N_IMG
    kw = dict(sos_idx=SOS, eos_idx=EOS, max_seq_len=MAX_LEN)
    ens = EsembleCaptioningModel([model, model], DEV)
    w = required[0][0]
    refused = [
        lambda: model.beam_search(images, pads, beam_size=K, required_words=required, prefix=[w], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=required, sample_or_max="sample", **kw),
        lambda: model.beam_search(images, pads, beam_size=1, required_words=[10, 11, 12, 13, 14], **kw),
        lambda: model.beam_search(images, pads, beam_size=5, required_words=[10, 11], **kw),
        lambda: model.beam_search(images, pads, beam_size=1, required_words=[10], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[V], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[-1], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[SOS], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[EOS], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[10, 10], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[10], banned_words=[10], **kw),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[10, 11], sos_idx=SOS, eos_idx=EOS, max_seq_len=3),
        lambda: model.beam_search(images, pads, beam_size=K, required_words=[[10]] * (N_IMG - 1), **kw),
        lambda: model.diverse_beam_search(images, pads, num_groups=2, group_size=2, required_words=required, **kw),
        lambda: ens.ensemble_beam_search(images, pads, beam_size=K, required_words=required, **kw),
        lambda: model(enc_x=images, enc_x_num_pads=pads, mode="sampling", sos_idx=SOS, eos_idx=EOS, how_many_outputs=2,
                      sample_max_seq_len=MAX_LEN, required_words=required),
        lambda: model(enc_x=images, enc_x_num_pads=pads, mode="diverse_beam_search", sos_idx=SOS, eos_idx=EOS, num_groups=2,
                      group_size=2, beam_max_seq_len=MAX_LEN, required_words=required),
    ]
    for i, call in enumerate(refused):
        with ops.profile() as recs:
            with pytest.raises(ValueError):
                call()
        assert not recs, (i, [r[0] for r in recs])
