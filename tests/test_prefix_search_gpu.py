"""Search behind a given prefix end to end on the GPU (`-m gpu`): the fixture of
tests/test_search_constraints_search_gpu.py (TINY geometry, the synthetic "eos" checkpoint, four synthetic images, fp32,
max_seq_len 12).

What a prefix means is checked on the returned captions; that the prefill leaves the state P forced steps leave is checked
on the logits of position P (1e-3, the sequence-versus-step bound of this checkpoint, LP_BOUND["eos"] of
test_scoring_gpu.py); that the selection is the model's is checked by replaying the logged candidates through
tests/group_beam_model.py from the reset state of tests/prefix_model.py, exactly, and by comparing every reported log-prob,
the prefix words' included, with score_captions (2e-3, the bar of test_diverse_search_gpu.py).
"""
import numpy as np
import pytest
import torch

import group_beam_model as M
import prefix_model as PM
import search_constraints_model as SC
from conftest import cached_state_dict
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
SOS, EOS = 3, 2
N_IMG, MAX_LEN, K = 4, 12, 3
PADS = [0] * N_IMG
F = np.float32
GREEDY_SEED = 0        # test_greedy_continuation_reproduces_the_caption: chosen on the CPU with the oracle (its docstring)


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
def ensemble(model):
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    return EsembleCaptioningModel([model, build(seed=1)], rank=DEV)


@pytest.fixture(scope="module")
def images():
    return W.synth_images(N_IMG, W.TINY).to(DEV)


def beam(model, images, log=None, k=K, **kw):
    model._cand_log = log
    try:
        toks, lps = model.beam_search(images, [0] * len(images), sos_idx=SOS, eos_idx=EOS, beam_size=k, how_many_outputs=1,
                                      max_seq_len=MAX_LEN, **kw)
    finally:
        model._cand_log = None
    return toks, lps.cpu()


def diverse(model, images, G=3, kg=2, lam=0.5, log=None, **kw):
    model._cand_log = log
    try:
        toks, lps = model.diverse_beam_search(images, PADS, sos_idx=SOS, eos_idx=EOS, num_groups=G, group_size=kg,
                                              diversity_penalty=lam, max_seq_len=MAX_LEN, **kw)
    finally:
        model._cand_log = None
    return toks, lps.cpu()


def ens_beam(ensemble, images, **kw):
    toks, lps = ensemble.ensemble_beam_search(images, PADS, sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=1,
                                              max_seq_len=MAX_LEN, **kw)
    return toks, lps.cpu()


def words(c):
    return [w for w in c[1:] if w != EOS]


def same(a, b):
    return a[0] == b[0] and a[1].shape == b[1].shape and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.fixture(scope="module")
def plain(model, images):
    return beam(model, images)


def stretched(c, P):
    """P words for a prefix out of caption c: its own words, repeated when it has fewer."""
    w = words(c) or [5, 6, 7]
    return [w[i % len(w)] for i in range(P)]


@pytest.fixture(scope="module")
def own_prefixes(plain):
    """Per image the first two words of its unconstrained caption."""
    return [stretched(per[0], 2) for per in plain[0]]


@pytest.fixture(scope="module")
def foreign_prefix(plain):
    """Two words no unconstrained caption starts with (one list for every image)."""
    firsts = {words(per[0])[0] for per in plain[0] if words(per[0])}
    w = [v for v in range(10, 40) if v not in firsts and v not in (SOS, EOS)]
    return [w[0], w[1]]


@pytest.fixture(scope="module")
def runs(model, ensemble, images, own_prefixes, foreign_prefix):
    """Every prefixed search the tests below look at, run once; beam and diverse with the candidate log on."""
    out = {}
    for name, pre in (("own", own_prefixes), ("foreign", foreign_prefix)):
        log = []
        out["beam", name] = beam(model, images, log=log, prefix=pre) + (log, pre)
        log = []
        out["diverse", name] = diverse(model, images, log=log, prefix=pre) + (log, pre)
        out["ensemble", name] = ens_beam(ensemble, images, prefix=pre) + (None, pre)
    return out


def per_image(pre):
    return pre if isinstance(pre[0], list) else [pre] * N_IMG


# ------------------------------------------------------------------------------------------------- 1
def test_no_prefix_and_the_empty_prefix_change_nothing(model, ensemble, images, plain):
    assert same(beam(model, images, prefix=None), plain) and same(beam(model, images, prefix=[]), plain)
    assert same(beam(model, images, prefix=[[]] * N_IMG), plain)
    d = diverse(model, images)
    assert same(diverse(model, images, prefix=None), d) and same(diverse(model, images, prefix=[]), d)
    e = ens_beam(ensemble, images)
    assert same(ens_beam(ensemble, images, prefix=None), e) and same(ens_beam(ensemble, images, prefix=[]), e)


# ------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("P", [1, 4, 9])
def test_prefill_leaves_the_state_of_p_forced_steps(model, images, plain, P):
    from on_device_image_captioning_amd import ops
    eng = model._captioner_engine()
    mem = model.forward_enc(images, PADS)
    kv, enc_len = eng.project_kv(mem), model._enc_lens(N_IMG, mem.shape[1], PADS)
    prefix = torch.tensor([stretched(per[0], P) for per in plain[0]], dtype=torch.int64, device=DEV)
    a = eng.new_state(N_IMG, K, MAX_LEN, kv, enc_len)
    eng.seed_prefix(a, prefix, SOS)
    assert int(a.pos.item()) == P
    eng.step_logits(a, embed=False)
    b = eng.new_state(N_IMG, K, MAX_LEN, kv, enc_len)
    ops.beam_reset(b.beam_state, N_IMG, K, MAX_LEN, SOS)
    b.anc.copy_(torch.arange(b.N, dtype=torch.int32, device=DEV)[:, None].expand(b.N, MAX_LEN))
    for t in range(P + 1):
        b.pos.fill_(t)
        if t:
            b.next_tok.copy_(prefix[:, t - 1].repeat_interleave(K))
        eng.step_logits(b, embed=True)
    err = float((a.logits - b.logits).abs().max())
    print(f"P={P}: max |logits after prefill - logits after {P} forced steps| = {err:.3e} "
          f"(logits scale {float(b.logits.abs().max()):.3e})")
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["own", "foreign"])
def test_every_caption_starts_with_its_prefix(runs, plain, name):
    for kind in ("beam", "diverse", "ensemble"):
        toks, lps, _, pre = runs[kind, name]
        for b, per in enumerate(toks):
            for c in per:
                assert c[:3] == [SOS] + per_image(pre)[b], (kind, b, c)
                assert len(c) <= MAX_LEN and EOS not in c[1:-1]
    if name == "foreign":
        assert all(per[0][1:3] != runs["beam", name][3] for per in plain[0])


# ------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["own", "foreign"])
def test_reported_log_probs_prefix_included_are_the_models_own(model, ensemble, images, runs, name):
    for kind, scorer in (("beam", model), ("diverse", model), ("ensemble", ensemble)):
        toks, lps, _, _ = runs[kind, name]
        G = len(toks[0])
        caps = [c for per in toks for c in per]
        sc = scorer.score_captions(images, caps, captions_per_image=G)
        flat = lps.view(N_IMG * G, -1)
        for n, c in enumerate(caps):
            err = float((flat[n, 1:len(c)] - sc.logprobs[n, :len(c) - 1].cpu()).abs().max())
            print(f"{kind} {name} caption {n}: max |search - score_captions| = {err:.3e}")
            assert err <= 2e-3, (kind, n)
            assert float(flat[n, 0]) == 0.0 and not flat[n, len(c):].any()


# ------------------------------------------------------------------------------------------------- 5
def replay(log, pre, plogp, G, kg, lam):
    R, P = G * kg, len(pre[0])
    st = PM.reset_state(N_IMG, R, MAX_LEN, SOS, pre, plogp, kg)
    for cv, ci in log:
        assert tuple(cv.shape) == (N_IMG * R, R)
        st, _ = M.step(st, cv.numpy(), ci.numpy(), G, kg, lam, EOS)
    assert 1 <= len(log) <= MAX_LEN - 1 - P
    score = (st["cumul"] / st["n_elem"].astype(F)).astype(F).reshape(N_IMG, G, kg)
    toks, lps = [], []
    for b in range(N_IMG):
        per = []
        for g in range(G):
            i = g * kg + int(np.argmax(score[b, g]))
            n = int(st["n_elem"][b * R + i])
            per.append(st["tokens"][b, i, :n].tolist())
            lps.append(st["logprobs"][b, i, :n])
        toks.append(per)
    lp = np.zeros((N_IMG, G, max(len(r) for r in lps)), F)
    for n, r in enumerate(lps):
        lp[n // G, n % G, :len(r)] = r
    return toks, lp


@pytest.mark.parametrize("kind,G,kg,lam", [("beam", 1, 3, 0.0), ("diverse", 3, 2, 0.5)])
@pytest.mark.parametrize("name", ["own", "foreign"])
def test_replay_from_the_reset_state_gives_the_same_captions_exactly(runs, kind, G, kg, lam, name):
    toks, lps, log, pre = runs[kind, name]
    pre = per_image(pre)
    P = len(pre[0])
    plogp = lps[:, 0, 1:P + 1].numpy()                    # the device's prefix log-probs (every row of an image holds them)
    want_toks, want_lp = replay(log, pre, plogp, G, kg, lam)
    assert toks == want_toks
    assert tuple(lps.shape) == want_lp.shape and np.array_equal(lps.numpy(), want_lp)


# ------------------------------------------------------------------------------------------------- 6
def test_constraints_count_the_prefix(model, images, plain, own_prefixes):
    banned = sorted({w for per in plain[0] for w in words(per[0])[2:3]})          # the third word of every caption
    min_length = 8
    for kind, run in (("beam", beam), ("diverse", diverse)):
        toks, _ = run(model, images, prefix=own_prefixes, no_repeat_ngram_size=2, min_length=min_length, banned_words=banned)
        for b, per in enumerate(toks):
            for c in per:
                assert c[:3] == [SOS] + own_prefixes[b]
                assert not SC.repeats_ngram(c, 2), (kind, c)
                assert len(words(c)) >= min_length, (kind, c)
                assert not set(c[3:]) & set(banned), (kind, c)
    # a prefix may hold a banned word: it stays, and does not come back
    w = own_prefixes[0][0]
    toks, _ = beam(model, images, prefix=own_prefixes, banned_words=[w])
    assert toks[0][0][1] == w and w not in toks[0][0][3:]


def test_a_bigram_of_the_prefix_is_not_continued(model, images, plain):
    """Prefix [a, c, a]: its last word begins the bigram (a, c) the prefix already holds, so with no_repeat_ngram_size = 2
    the first free step may not offer c.  c runs over the three candidates that follow [a] (a = the caption's first word);
    at least one (image, c) must offer c again without the constraint, or the check would be vacuous."""
    a = [stretched(per[0], 1) for per in plain[0]]
    log = []
    beam(model, images, log=log, prefix=a)
    first = log[0][1].view(N_IMG, K, K)[:, 0]                    # candidates of every image's first row after [a]
    shown = 0
    for r in range(K):
        pre = [[a[b][0], int(first[b, r]), a[b][0]] for b in range(N_IMG)]
        if any(w in (SOS, EOS) for p in pre for w in p):
            continue
        free, cons = [], []
        beam(model, images, log=free, prefix=pre)
        beam(model, images, log=cons, prefix=pre, no_repeat_ngram_size=2)
        for b in range(N_IMG):
            c = pre[b][1]
            assert c not in cons[0][1].view(N_IMG, K, K)[b, 0].tolist(), (b, pre[b])
            shown += c in free[0][1].view(N_IMG, K, K)[b, 0].tolist()
    print(f"{shown} (image, c) pairs offer c after [a, c, a] without the constraint")
    assert shown >= 1


# ------------------------------------------------------------------------------------------------- 7
def test_greedy_continuation_reproduces_the_caption(images):
    """beam_size = 1: the search behind the first p words of the unprefixed caption must return that caption, for every
    (image, p) whose caption has a top-1 / top-2 margin above 2e-3 at every step (the "sure" rule of test_scoring_gpu.py;
    margins from decode_sequence(want_logits=True)); p in {1, 2, 4, 7} as far as the caption has words.  At least half of
    the pairs must qualify.  Seed 0 of the synthetic "eos" checkpoint was chosen on the CPU with the oracle
    (oracle/expansionnet_ref.py: greedy captions, forward_teacher margins): all 15 of its 15 pairs qualify there, the
    smallest margin being 0.0887 (seeds 1 and 4 caption nothing, seed 3 has a margin of 0.0037)."""
    m = build(seed=GREEDY_SEED)
    eng = m._captioner_engine()
    base, _ = beam(m, images, k=1)
    caps = [per[0] for per in base]
    mem = m.forward_enc(images, PADS)
    T = max(len(c) for c in caps) - 1
    dec = torch.tensor([c[:-1] + [EOS] * (T - len(c) + 1) for c in caps], dtype=torch.int64, device=DEV)
    dec_len = torch.tensor([len(c) - 1 for c in caps], dtype=torch.int32, device=DEV)
    lg = eng.decode_sequence(dec, dec_len, eng.project_kv(mem), m._enc_lens(N_IMG, mem.shape[1], PADS), N_IMG,
                             want_logits=True)
    top2 = torch.log_softmax(lg, -1).topk(2, -1).values.cpu()
    margin = top2[..., 0] - top2[..., 1]
    sure = [bool((margin[b, :len(c) - 1] > 2e-3).all()) for b, c in enumerate(caps)]
    pairs = [(b, p) for b, c in enumerate(caps) for p in (1, 2, 4, 7) if p <= min(len(words(c)), MAX_LEN - 2)]
    ok = [(b, p) for b, p in pairs if sure[b]]
    print(f"{len(ok)} of {len(pairs)} (image, p) pairs qualify; smallest margin {float(min(margin[b, :len(c) - 1].min() for b, c in enumerate(caps))):.4f}")
    assert pairs and 2 * len(ok) >= len(pairs)
    for p in sorted({p for _, p in ok}):
        idx = [b for b, q in ok if q == p]
        toks, _ = beam(m, images[idx], k=1, prefix=[caps[b][1:p + 1] for b in idx])
        for b, per in zip(idx, toks):
            assert per[0] == caps[b], (b, p)


# ------------------------------------------------------------------------------------------------- 8
def test_captioner_and_forward_pass_the_prefix_on(model, images, runs, own_prefixes):
    from on_device_image_captioning_amd.captioning_model import Captioner
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=K, how_many_outputs=1, beam_max_seq_len=MAX_LEN, prefix=own_prefixes)
    toks, lps = Captioner(args, model=model)(images, enc_x_num_pads=PADS, mode="beam_search")
    assert same((toks, lps.cpu()), runs["beam", "own"][:2])
    toks, lps = model(enc_x=images, enc_x_num_pads=PADS, mode="beam_search", **args)
    assert same((toks, lps.cpu()), runs["beam", "own"][:2])
    toks, lps = model(enc_x=images, enc_x_num_pads=PADS, mode="diverse_beam_search", sos_idx=SOS, eos_idx=EOS, num_groups=3,
                      group_size=2, diversity_penalty=0.5, beam_max_seq_len=MAX_LEN, prefix=own_prefixes)
    assert same((toks, lps.cpu()), runs["diverse", "own"][:2])
    with pytest.raises(ValueError, match="deterministic"):
        model(enc_x=images, enc_x_num_pads=PADS, mode="sampling", sos_idx=SOS, eos_idx=EOS, how_many_outputs=2,
              sample_max_seq_len=MAX_LEN, prefix=own_prefixes)
