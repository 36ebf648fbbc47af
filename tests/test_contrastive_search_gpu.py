"""Contrastive beam search end to end on the GPU (`-m gpu`): TINY geometry, the synthetic "eos"
checkpoint, four synthetic images, fp32, max_seq_len 12.

(a) off is beam_search bit for bit; (b) the logged candidates replayed through the numpy beam model give the captions
exactly; (c) every returned per-word score is lp_target − w·max(suppressor, floor) with the log-probs score_captions
gives for that caption on the target and on the distractor images (2e-3, the tolerance of
test_ensemble_sampled_search_scores_equal_score_captions); (d) with one beam and plausibility 1 the words are the greedy
ones for any weight; (e) the search constraints hold; (f) an image without distractors gets beam_search's rows;
(g) caption_regions(distinctive=True) is the search on the resized batch with the sibling indices."""
import math

import numpy as np
import pytest
import torch

import group_beam_model as M
import search_constraints_model as SC
from conftest import cached_state_dict
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
SOS, EOS = 3, 2
N_IMG, MAX_LEN, K = 4, 12, 3
F = np.float32
RAGGED = [[1, 2], [], [0], [0, 1, 2]]


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


def contrastive(model, images, distractors, log=None, k=K, outs=1, **kw):
    model._cand_log = log
    try:
        toks, sc = model.contrastive_beam_search(images, [0] * N_IMG, SOS, EOS, distractors, beam_size=k,
                                                 how_many_outputs=outs, max_seq_len=MAX_LEN, **kw)
    finally:
        model._cand_log = None
    return toks, sc.cpu()


def beam(model, images, k=K, outs=1, **kw):
    toks, lps = model.beam_search(images, [0] * N_IMG, sos_idx=SOS, eos_idx=EOS, beam_size=k, how_many_outputs=outs,
                                  max_seq_len=MAX_LEN, **kw)
    return toks, lps.cpu()


@pytest.fixture(scope="module")
def plain(model, images):
    return beam(model, images)


def same(a, b):
    return a[0] == b[0] and a[1].shape == b[1].shape and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def replay(log, k, outs=1):
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


# ------------------------------------------------------------------------------------------------- (a) off
def test_off_is_beam_search_bit_for_bit(model, images, plain):
    assert same(contrastive(model, images, "others", contrast=0.0, plausibility=0.0), plain)
    assert same(contrastive(model, images, [[], [], [], []]), plain)
    assert same(contrastive(model, images, None, contrast=2.0, plausibility=0.0), plain)
    three = beam(model, images, outs=3)
    assert same(contrastive(model, images, RAGGED, outs=3, contrast=0.0, plausibility=0.0), three)


# ------------------------------------------------------------------------------------------------- (b) replay
@pytest.mark.parametrize("dist,kw", [("others", {}), (RAGGED, dict(contrast=1.0, plausibility=0.02)),
                                     ([[1], [0], [3], [2]], dict(contrast=0.8, suppressor_floor=-3.0))],
                         ids=["others", "ragged", "pairs"])
def test_replay_of_the_logged_candidates_gives_the_same_captions_exactly(model, images, dist, kw):
    log = []
    toks, sc = contrastive(model, images, dist, log=log, **kw)
    assert 1 <= len(log) <= MAX_LEN - 1
    want_toks, want = replay(log, K)
    assert toks == want_toks
    assert tuple(sc.shape) == want.shape and np.array_equal(sc.numpy(), want)


# ------------------------------------------------------------------------------------------------- (c) score identity
def _logprobs_on(model, images, caps, image_of):
    """score_captions of caption n on image image_of[n] → one row of log-probs per caption."""
    sc = model.score_captions(images[torch.tensor(image_of, device=images.device)], caps)
    return sc.logprobs.cpu().double()


@pytest.mark.parametrize("D", [1, 2])
def test_returned_scores_are_target_minus_weighted_suppressor(model, images, plain, D):
    w, floor = 0.6, -6.0
    dist = [[(i + 1 + d) % N_IMG for d in range(D)] for i in range(N_IMG)]
    toks, sc = contrastive(model, images, dist, contrast=w, plausibility=0.05, suppressor_floor=floor)
    caps = [per[0] for per in toks]
    lp_t = _logprobs_on(model, images, caps, list(range(N_IMG)))
    lp_d = torch.stack([_logprobs_on(model, images, caps, [dist[i][d] for i in range(N_IMG)]) for d in range(D)])
    s = lp_d[0] if D == 1 else torch.logsumexp(lp_d, 0) - math.log(D)
    want = lp_t - float(F(w)) * torch.clamp(s, min=floor)
    clamped = 0
    for n, c in enumerate(caps):
        L = len(c) - 1
        err = float((sc[n, 0, 1:len(c)].double() - want[n, :L]).abs().max())
        clamped += int((s[n, :L] < floor).sum())
        print(f"D={D} caption {n}: max |search score - (lp_t - w*s')| = {err:.3e}")
        assert err <= 2e-3, (n, c)
        assert not sc[n, 0, len(c):].any(), "padding behind a caption's end is zero"
    print(f"D={D}: {clamped} words with the suppressor at its floor")
    assert any(a != b for a, b in zip(toks, plain[0])), "the contrast must change a caption of this batch"


# ------------------------------------------------------------------------------------------------- (d) greedy
@pytest.mark.parametrize("w", [0.0, 0.5, 3.0])
def test_one_beam_under_full_plausibility_is_greedy_for_any_weight(model, images, w):
    greedy, _ = beam(model, images, k=1)
    toks, _ = contrastive(model, images, "others", k=1, contrast=w, plausibility=1.0)
    assert toks == greedy


# ------------------------------------------------------------------------------------------------- (e) constraints
def test_constraints_hold_and_the_replay_is_exact(model, images, plain):
    words = lambda c: [t for t in c[1:] if t != EOS]          # noqa: E731
    banned = sorted({words(per[0])[0] for per in plain[0] if words(per[0])})
    log = []
    toks, sc = contrastive(model, images, "others", log=log, outs=K, no_repeat_ngram_size=2, banned_words=banned)
    for b, per in enumerate(toks):
        assert len({tuple(c) for c in per}) == K, (b, per)                       # beam_size distinct rows,
        for j, c in enumerate(per):
            assert torch.isfinite(sc[b, j, :len(c)]).all(), (b, j)               # every one with finite scores,
            assert not set(c) & set(banned) and not SC.repeats_ngram(c, 2), c    # and inside the constraints
    # the first step's candidates are the admissible words of the prefix [SOS]; every step's are sorted
    bad0 = SC.inadmissible([SOS], 0, W.TINY.vocab_size, banned=banned, no_repeat_ngram=2, eos=EOS)
    assert not bad0[log[0][1].numpy()].any()
    for t, (cv, ci) in enumerate(log):
        for r in range(cv.shape[0]):
            key = list(zip((-cv[r]).tolist(), ci[r].tolist()))
            assert key == sorted(key), (t, r)
    log1 = []
    t1, s1 = contrastive(model, images, "others", log=log1, no_repeat_ngram_size=2, banned_words=banned)
    want_toks, want = replay(log1, K)
    assert t1 == want_toks and tuple(s1.shape) == want.shape and np.array_equal(s1.numpy(), want)
    assert t1 == [per[:1] for per in toks]


# ------------------------------------------------------------------------------------------------- (f) ragged lists
def test_an_image_without_distractors_gets_beam_searchs_rows(model, images):
    toks, sc = contrastive(model, images, RAGGED, outs=K, contrast=1.0)
    want, wl = beam(model, images, outs=K)
    b = RAGGED.index([])
    assert toks[b] == want[b]
    L = max(len(c) for c in toks[b])
    assert torch.equal(sc[b, :, :L].view(torch.int32), wl[b, :, :L].view(torch.int32))
    assert not sc[b, :, L:].any() and not wl[b, :, L:].any()


# ------------------------------------------------------------------------------------------------- modes
def test_captioner_mode_and_forward_mode_return_what_the_method_returns(model, images):
    from on_device_image_captioning_amd.captioning_model import Captioner
    toks, sc = contrastive(model, images, "others", contrast=0.7)
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=K, beam_max_seq_len=MAX_LEN, contrast=0.7)
    cap = Captioner(args, model=model)
    t1, s1 = cap(images, enc_x_num_pads=[0] * N_IMG, mode="contrastive_beam_search")
    assert t1 == toks and torch.equal(s1.cpu(), sc)
    t2, s2 = model(enc_x=images, enc_x_num_pads=[0] * N_IMG, mode="contrastive_beam_search", distractors="others", **args)
    assert t2 == toks and torch.equal(s2.cpu(), sc)
    t3, s3 = cap.contrastive_beam_search(images, [0] * N_IMG, SOS, EOS, "others", beam_size=K, max_seq_len=MAX_LEN, contrast=0.7)
    assert t3 == toks and torch.equal(s3.cpu(), sc)


# ------------------------------------------------------------------------------------------------- (g) regions
def test_distinctive_region_captions_are_the_search_with_sibling_indices(model):
    from on_device_image_captioning_amd.captioning_model import Captioner
    from on_device_image_captioning_amd import image_utils as IU
    g = W.TINY
    gen = torch.Generator().manual_seed(11)
    pics = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).to(DEV) for h, w in ((70, 90), (64, 64), (50, 81))]
    regions = [(0, (0, 0, 45, 35)), (2, (5, 5, 60, 40)), (0, (40, 30, 90, 70)), (0, (10, 10, 80, 60)), (2, (0, 0, 81, 50))]
    siblings = [[2, 3], [4], [0, 3], [0, 2], [1]]                                 # picture 1 has no region
    pre = IU.DevicePreprocessor(g.swin_img_size, DEV, max_pixels=256 * 256)
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=K, beam_max_seq_len=MAX_LEN)
    cap = Captioner(args, model=model)
    got = cap.caption_regions(pre, pics, regions, distinctive=True, contrast=0.8)
    batch = pre.resize_regions(pics, regions)
    toks, sc = model.contrastive_beam_search(batch, [0] * len(regions), SOS, EOS, siblings, beam_size=K, max_seq_len=MAX_LEN,
                                             contrast=0.8)
    assert [len(per) for per in got] == [3, 0, 2]
    flat = sorted((rc for per in got for rc in per), key=lambda rc: rc.region)
    for n, rc in enumerate(flat):
        assert rc.region == n and rc.box == tuple(float(v) for v in regions[n][1])
        assert rc.tokens == toks[n] and torch.equal(rc.logprobs.cpu(), sc[n].cpu())
    # the default is what it was: this object's plain search on the batch
    plain = cap.caption_regions(pre, pics, regions)
    want, wl = cap(batch, enc_x_num_pads=[0] * len(regions))
    flat = sorted((rc for per in plain for rc in per), key=lambda rc: rc.region)
    for n, rc in enumerate(flat):
        assert rc.tokens == want[n] and torch.equal(rc.logprobs.cpu(), wl[n].cpu())
    # a lone region is plain beam search
    lone = cap.caption_regions(pre, pics, regions[1:2], distinctive=True)
    one, ol = cap(pre.resize_regions(pics, regions[1:2]), enc_x_num_pads=[0])
    assert lone[2][0].tokens == one[0] and torch.equal(lone[2][0].logprobs.cpu().view(torch.int32), ol[0].cpu().view(torch.int32))
