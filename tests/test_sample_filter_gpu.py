"""odic_logsoftmax_sample_filtered on the device (`-m gpu`): temperature, top-k and nucleus on the draws of
odic_logsoftmax_sample, against the numpy model of sample_filter_model.py (whose rows test_sample_filter_host.py proves
`clear`, so `kept` is compared exactly), and through the searches that take the three keywords."""
import numpy as np
import pytest
import torch

import sample_filter_model as M
import vocab_rows_refs as VR
from guards import guarded, poisoned_input

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
NINF = float("-inf")
IDS = [f"V{V}-k{k}" for V, k in M.SHAPES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def run(ops, X, k, flt, seed=M.SEED, pos=M.POS, want_logp=False, want_kept=True):
    """One launch on the rows X (device) → top_idx, top_val, kept, logp_out on the CPU."""
    N, V = X.shape
    tv = torch.empty(N, k, device=DEV)
    ti = torch.empty(N, k, dtype=torch.int32, device=DEV)
    kept = torch.full((N,), -1, dtype=torch.int32, device=DEV) if want_kept else None
    lp = torch.empty(N, V, device=DEV) if want_logp else None
    p = torch.full((1,), pos, dtype=torch.int32, device=DEV)
    ops.logsoftmax_sample_filtered(X, V, lp, V if want_logp else 0, tv, ti, kept, N, V, k, ops.sample_filter(*flt), seed, p)
    return ti.cpu().long(), tv.cpu(), None if kept is None else kept.cpu().long(), None if lp is None else lp.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. filter off
@pytest.mark.parametrize("V,k", M.SHAPES, ids=IDS)
def test_filter_off_is_logsoftmax_sample_bit_for_bit(ops, V, k):
    X = torch.cat([VR.sample_stack(V, k)[1][::16], torch.randn(24, V, generator=M._gen(V, k, 1)) * 2.0]).to(DEV)
    N = X.shape[0]
    pos = torch.full((1,), M.POS, dtype=torch.int32, device=DEV)
    tv, ti, lp = torch.empty(N, k, device=DEV), torch.empty(N, k, dtype=torch.int32, device=DEV), torch.empty(N, V, device=DEV)
    ops.logsoftmax_sample(X, V, lp, V, tv, ti, N, V, k, M.SEED, pos)
    gi, gv, kept, glp = run(ops, X, k, (1.0, 0, 1.0), want_logp=True)
    assert torch.equal(gi, ti.cpu().long())
    assert torch.equal(bits(gv), bits(tv.cpu()))
    assert torch.equal(bits(glp), bits(lp.cpu()))
    assert kept.tolist() == [V] * N


# ------------------------------------------------------------------------------------------------ 2. kept
@pytest.mark.parametrize("V,k", M.SHAPES, ids=IDS)
def test_kept_is_the_models_count(ops, V, k):
    names, X = M.rows(V)
    Xd = X.to(DEV)
    wrong = []
    for t in M.TEMPERATURES:
        z = M.scaled(X.numpy(), t)
        rk = M.ranked(z)
        for tk in M.TOP_KS:
            for tp in M.TOP_PS + (1.0,):
                m = M.filter_ref(z, tk, tp, k, rk)[1]
                kept = run(ops, Xd, k, (t, tk, tp))[2].numpy()
                wrong += [(t, tk, tp, names[r], int(kept[r]), int(m[r])) for r in np.flatnonzero(kept != m)]
    print(f"sample-filter kept V={V} k={k}: {len(wrong)} wrong (temperature, top_k, top_p, family, kept, model): {wrong[:12]}")
    assert not wrong


@pytest.mark.parametrize("V", M.DENSE_VS)
def test_kept_on_dense_rows_lies_in_the_contracts_band(ops, V):
    """Plain randn·3 rows: hundreds to thousands of words in the nucleus, so the mass sums run over every wave.  kept within
    [m at top_p·(1 - 1e-5), m at top_p·(1 + 1e-5)], every draw inside the first max(m_hi, k) ranks, none twice."""
    X = M.dense_rows(V)
    Xd, k = X.to(DEV), M.DENSE_K
    for flt in M.DENSE_FILTERS:
        order, _, c = M.filter_ref(M.scaled(X.numpy(), flt[0]), flt[1], flt[2], k)
        lo, hi = M.kept_band(c, flt[2])
        gi, gv, kept, _ = run(ops, Xd, k, flt)
        kept = kept.numpy()
        print(f"sample-filter dense V={V} filter {flt}: kept {kept.min()}..{kept.max()}, band width up to {int((hi - lo).max())}, "
              f"kept - m_lo up to {int((kept - lo).max())}")
        assert ((lo <= kept) & (kept <= hi)).all(), (flt, lo.tolist(), kept.tolist(), hi.tolist())
        for r in range(len(X)):
            drawn = gi[r].tolist()
            assert len(set(drawn)) == k and set(drawn) <= set(order[r, :max(int(hi[r]), k)].tolist()), (flt, r, drawn)


# ------------------------------------------------------------------------------------------------ 3. draws
@pytest.mark.parametrize("V,k", M.SHAPES, ids=IDS)
def test_draws_are_the_models_inside_the_draw_set(ops, V, k):
    names, X = M.rows(V)
    N = len(names)
    Xd = X.to(DEV)
    g = M.gumbel(M.noise_bits(M.SEED, np.arange(N), V, M.POS))
    logp, lse = VR.log_softmax_ref(X)
    x64 = X.double().numpy()
    worst, over = 0.0, 0.0
    for flt in M.DRAW_FILTERS:
        z = M.scaled(X.numpy(), flt[0]).astype(np.float64)
        order, m, _ = M.filter_ref(z, flt[1], flt[2], k)
        gi, gv, kept, glp = run(ops, Xd, k, flt, want_logp=True)
        assert kept.tolist() == m.tolist(), flt
        over = max(over, float(VR.ratios(glp, logp, VR.bound_lse_form(logp, lse)).max()))
        got_lp = logp.gather(1, gi)
        over = max(over, float(VR.ratios(gv, got_lp, VR.bound_lse_form(got_lp, lse)).max()))
        for r in range(N):
            what = f"V={V} k={k} filter {flt} row {names[r]}"
            size = max(int(m[r]), k)
            if flt[1] == 1 and k > 1:
                assert size == k and int(m[r]) == 1, what             # m < k: the draw set is extended in rank order
            S = order[r, :size]
            inside = set(S.tolist())
            score = np.full(V, NINF)
            score[S] = z[r, S] + g[r, S]
            drawn = gi[r].tolist()
            assert len(set(drawn)) == k, f"{what}: a word drawn twice {drawn}"
            for j, d in enumerate(drawn):
                best = score.max()
                if best == NINF:                                       # a short row: masked words by ascending index
                    left = [i for i in np.flatnonzero(x64[r] == NINF).tolist() if i not in drawn[:j]]
                    assert d == left[0] and float(gv[r, j]) == NINF, what
                    continue
                assert d in inside, f"{what}: draw {j} = {d} is outside S"
                tol = 8 * 2.0 ** -24 * (abs(z[r, d]) + abs(g[r, d]) + 1.0)
                worst = max(worst, (best - score[d]) / tol)
                assert score[d] >= best - tol, f"{what}: draw {j} = {d} scores {score[d]}, the model's best {best}"
                score[d] = NINF
    print(f"sample-filter draws V={V} k={k}: worst (best - drawn) / tolerance {worst:.3f}, log-prob err / bound {over:.3f}")
    assert over <= 1.0


# ------------------------------------------------------------------------------------------------ 4. frequencies
@pytest.mark.parametrize("flt", M.FREQ_FILTERS, ids=["top_k", "top_k_top_p"])
def test_draw_frequencies_follow_the_filtered_distribution(ops, flt):
    x = M.freq_row()
    X = x[None].expand(M.FREQ_N, M.FREQ_V).contiguous().to(DEV)
    z = M.scaled(x.numpy()[None], flt[0])
    order, m, _ = M.filter_ref(z, flt[1], flt[2], 1)
    S = order[0, :int(m[0])]
    q = np.zeros(M.FREQ_V)
    q[S] = np.exp(z[0, S].astype(np.float64) - z[0].max())
    q /= q.sum()
    gi, gv, kept, _ = run(ops, X, 1, flt, seed=1234, pos=0)
    assert kept.tolist() == [int(m[0])] * M.FREQ_N
    f = np.bincount(gi[:, 0].numpy(), minlength=M.FREQ_V) / M.FREQ_N
    assert ((f > 0) == (q > 0)).all(), (f, q)
    sig = np.abs(f - q)[S] / np.sqrt(q[S] * (1 - q[S]) / M.FREQ_N)
    print(f"sample-filter frequencies {flt}: S = {S.tolist()}, worst deviation {sig.max():.2f} sigma")
    assert sig.max() < 4.0
    want = torch.log_softmax(x.double(), 0)[gi[:, 0]]
    assert float((gv[:, 0].double() - want).abs().max()) <= 2e-6          # the model's own log-probs, not the filtered ones
    assert torch.equal(run(ops, X, 1, flt, seed=1234, pos=0)[0], gi)
    assert not torch.equal(run(ops, X, 1, flt, seed=1235, pos=0)[0], gi)
    assert not torch.equal(run(ops, X, 1, flt, seed=1234, pos=3)[0], gi)


# ------------------------------------------------------------------------------------------------ 5. containment
@pytest.mark.parametrize("V,k", M.SHAPES, ids=IDS)
def test_filtered_draw_stays_inside_its_operands(ops, V, k):
    names, X = M.rows(V)
    N = len(names)
    flt = (0.5, 5, 0.9)
    ref_i, ref_v, ref_kept, ref_lp = run(ops, X.to(DEV), k, flt, want_logp=True)
    gx = poisoned_input(X.to(DEV), N, V, V + 3)
    gx.t[:, V:] = float("nan")
    lp, tv = guarded(N, V, V + 1, torch.float32, DEV), guarded(N, k, k, torch.float32, DEV)
    ti, kept = guarded(N, k, k, torch.int32, DEV), guarded(1, N, N, torch.int32, DEV)
    pos = torch.full((1,), M.POS, dtype=torch.int32, device=DEV)
    ops.logsoftmax_sample_filtered(gx.t, V + 3, lp.t, V + 1, tv.t, ti.t, kept.t.view(-1), N, V, k, ops.sample_filter(*flt),
                                   M.SEED, pos)
    torch.cuda.synchronize()
    for nm, g_ in (("logp_out", lp), ("top_val", tv), ("top_idx", ti), ("kept", kept)):
        g_.assert_untouched(what=f"logsoftmax_sample_filtered V={V} k={k} {nm}")
    assert torch.equal(ti.t.cpu().long(), ref_i) and torch.equal(bits(tv.t.cpu()), bits(ref_v))
    assert torch.equal(kept.t.view(-1).cpu().long(), ref_kept)
    assert torch.equal(bits(lp.t[:, :V].cpu()), bits(ref_lp))


# ------------------------------------------------------------------------------------------------ 6. u = 1
def _hit_rows():
    X = torch.zeros(M.HIT_ROWS, M.HIT_V)
    X[:, M.HIT_WORD] = -40.0
    g = M.gumbel(M.noise_bits(M.HIT_SEED, np.arange(M.HIT_ROWS), M.HIT_V, M.HIT_POS))
    return X, np.argmax(X.double().numpy() + g, -1)


def test_the_all_ones_noise_pattern_does_not_force_its_word(ops):
    X, want = _hit_rows()
    assert want[M.HIT_ROW] != M.HIT_WORD
    got = run(ops, X.to(DEV), 1, (1.0, 0, 1.0), seed=M.HIT_SEED, pos=M.HIT_POS)[0][:, 0]
    assert got.tolist() == want.tolist()
    got = run(ops, X.to(DEV), 1, (0.5, 0, 0.999), seed=M.HIT_SEED, pos=M.HIT_POS)[0][:, 0]
    assert int(got[M.HIT_ROW]) != M.HIT_WORD


def test_the_all_ones_noise_pattern_in_logsoftmax_sample(ops):
    X, want = _hit_rows()
    tv = torch.empty(M.HIT_ROWS, 1, device=DEV)
    ti = torch.empty(M.HIT_ROWS, 1, dtype=torch.int32, device=DEV)
    pos = torch.full((1,), M.HIT_POS, dtype=torch.int32, device=DEV)
    ops.logsoftmax_sample(X.to(DEV), M.HIT_V, None, 0, tv, ti, M.HIT_ROWS, M.HIT_V, 1, M.HIT_SEED, pos)
    assert ti[:, 0].tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------ 7. end to end
TSOS, TEOS = 3, 2
FILTER = dict(temperature=0.8, top_k=20, top_p=0.9)


def _tiny(seed=None, variant="eos"):
    from conftest import cached_state_dict
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank="cuda:0")
    m.load_state_dict(cached_state_dict("TINY", variant) if seed is None else
                      W.synth_state_dict(g, seed=seed, variant=variant, eos_idx=TEOS), strict=True)
    return m.to("cuda:0").eval()


@pytest.fixture(scope="module")
def tiny(ops):
    from on_device_image_captioning_amd import weights as W
    return _tiny(), W.synth_images(2, W.TINY).to("cuda:0")


def agree_with_score_captions(model, img, toks, lps):
    flat = [seq for per in toks for seq in per]
    sc = model.score_captions(img, flat, [0] * img.shape[0], captions_per_image=len(toks[0]))
    lps = lps.reshape(len(flat), -1).cpu()
    for n, seq in enumerate(flat):
        assert seq[0] == TSOS and TEOS not in seq[1:-1]
        np.testing.assert_allclose(lps[n, 1:len(seq)].numpy(), sc.logprobs[n, :len(seq) - 1].cpu().numpy(), atol=2e-3)
        assert float(lps[n, 0]) == 0.0 and float(lps[n, len(seq):].abs().sum()) == 0.0


def test_filtered_sampling_and_sampled_beam_search_report_the_models_logprobs(tiny):
    m, img = tiny
    m.sampling_seed = 5
    toks, lps = m(enc_x=img, enc_x_num_pads=[0, 0], mode="sampling", how_many_outputs=3, sample_max_seq_len=10,
                  sos_idx=TSOS, eos_idx=TEOS, **FILTER)
    agree_with_score_captions(m, img, toks, lps)
    toks, lps = m(enc_x=img, enc_x_num_pads=[0, 0], mode="beam_search", beam_size=3, how_many_outputs=2,
                  beam_max_seq_len=8, sample_or_max="sample", sos_idx=TSOS, eos_idx=TEOS, **FILTER)
    agree_with_score_captions(m, img, toks, lps)


def test_top_k_one_sampling_is_the_greedy_caption(tiny):
    m, img = tiny
    toks, lps = m(enc_x=img, enc_x_num_pads=[0, 0], mode="sampling", how_many_outputs=2, sample_max_seq_len=10,
                  sos_idx=TSOS, eos_idx=TEOS, top_k=1)
    want, wlp = m(enc_x=img, enc_x_num_pads=[0, 0], mode="beam_search", beam_size=1, how_many_outputs=1,
                  beam_max_seq_len=11, sample_or_max="max", sos_idx=TSOS, eos_idx=TEOS)     # (10 steps, as the 10 draws)
    for b in range(2):
        n = len(want[b][0])
        for j in range(2):
            assert toks[b][j] == want[b][0]
            np.testing.assert_allclose(lps[b, j, :n].cpu().numpy(), wlp[b, 0, :n].cpu().numpy(), atol=2e-3)


def test_ensemble_filtered_sampled_search_reports_the_ensembles_logprobs(ops):
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    ens = EsembleCaptioningModel([_tiny(seed=11), _tiny(seed=12)], "cuda:0")
    img = W.synth_images(2, W.TINY).to("cuda:0")
    toks, lps = ens(enc_x=img, enc_x_num_pads=[0, 0], mode="beam_search", beam_size=3, how_many_outputs=2,
                    beam_max_seq_len=8, sample_or_max="sample", sos_idx=TSOS, eos_idx=TEOS, **FILTER)
    agree_with_score_captions(ens, img, toks, lps)


def test_default_controls_change_nothing(tiny):
    m, img = tiny
    calls = dict(sampling=dict(mode="sampling", how_many_outputs=3, sample_max_seq_len=10),
                 beam=dict(mode="beam_search", beam_size=3, how_many_outputs=2, beam_max_seq_len=8, sample_or_max="sample"))
    for kw in calls.values():
        out = []
        for extra in ({}, dict(temperature=1.0, top_k=0, top_p=1.0)):
            m.sampling_seed, m._sampling_calls = 9, 0
            out.append(m(enc_x=img, enc_x_num_pads=[0, 0], sos_idx=TSOS, eos_idx=TEOS, **kw, **extra))
        assert out[0][0] == out[1][0]
        assert torch.equal(bits(out[0][1].cpu()), bits(out[1][1].cpu()))
