"""The sampling controls without a GPU: the numpy model of sample_filter_model.py against torch, the host rules
(search.check_sampling_filter, dispatch), the refusals of odic_logsoftmax_sample_filtered, and that every row the GPU tests
use is `clear`, so that they compare `kept` exactly and leave out no case."""
import ctypes

import numpy as np
import pytest
import torch

import sample_filter_model as M
from on_device_image_captioning_amd import search


# ------------------------------------------------------------------------------------------------------- the model
def test_philox_known_answers():
    assert [int(v) for v in M.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(v) for v in M.philox4x32_10(f, f, f, f, f, f)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_the_hit_constant_is_the_all_ones_pattern():
    b = M.noise_bits(M.HIT_SEED, [M.HIT_ROW], M.HIT_V, M.HIT_POS)[0, M.HIT_WORD]
    assert int(b) >> 8 == 0xFFFFFF
    raw = (np.float32(int(b) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert raw == np.float32(1.0)                                      # what the unclamped form gives: noise +inf
    u = M.uniform_from_bits(np.array([b], dtype=np.uint32))
    assert u[0] < 1.0 and np.isfinite(M.gumbel(np.array([b], dtype=np.uint32))[0])
    assert M.HIT_ROW < M.HIT_ROWS and M.HIT_WORD < M.HIT_V


@pytest.mark.parametrize("top_k,top_p,t", [(0, 0.9, 1.0), (5, 0.5, 0.7), (7, 1.0, 2.0), (0, 0.25, 0.5), (40, 0.999, 1.3)])
def test_model_against_topk_and_cumsum(top_k, top_p, t):
    x = torch.randn(6, 33, generator=M._gen(1, top_k)) * 2.0                  # easy rows: no ties, no masks
    z = torch.from_numpy(M.scaled(x.numpy(), t)).double()
    order, m, c = M.filter_ref(z.numpy(), top_k, top_p, 1)
    kk = 33 if top_k == 0 or top_k >= 33 else top_k
    val, idx = torch.topk(z, kk, dim=-1)
    assert torch.equal(torch.from_numpy(order[:, :kk]), idx)
    q = torch.softmax(val, -1)
    before = q.cumsum(-1) - q
    np.testing.assert_allclose(c, before.numpy(), atol=1e-12)
    want = (before < float(np.float32(top_p))).sum(-1) if top_p < 1.0 else torch.full((6,), kk)
    assert m.tolist() == want.tolist() and (m >= 1).all()
    assert M.draw_sets(order, m, 3)[0] == set(idx[0, :max(int(m[0]), 3)].tolist())


def test_ties_and_masked_words_rank_as_the_contract_says():
    z = np.array([[1.0, 2.0, 2.0, -np.inf, 2.0, 0.0, -0.0, -np.inf]], dtype=np.float32)
    order, m, c = M.filter_ref(z, 0, 0.5, 1)
    assert order[0].tolist() == [1, 2, 4, 0, 5, 6, 3, 7]
    assert int(m[0]) == 2                                              # c = 0, .278, .556: the lower indices of the tie
    assert int(M.filter_ref(z, 2, 1.0, 1)[1][0]) == 2 and int(M.filter_ref(z, 0, 1.0, 1)[1][0]) == 8


def test_every_gpu_test_row_is_clear():
    for V in M.VS:
        names, X = M.rows(V)
        assert len(names) == len(M.FAMILIES) * M.REPS == X.shape[0] and len(set(names)) == len(names)
        for t in M.TEMPERATURES:
            z = M.scaled(X.numpy(), t)
            rk = M.ranked(z)
            for tk in M.TOP_KS:
                for tp in M.TOP_PS:
                    cl = M.clear(M.filter_ref(z, tk, tp, 1, rk)[2], tp)
                    assert cl.all(), (V, t, tk, tp, [names[i] for i in np.flatnonzero(~cl)])
        for flt in M.DRAW_FILTERS:
            assert flt in M.KEPT_FILTERS or flt[2] == 1.0
    z = M.scaled(M.freq_row().numpy()[None], M.FREQ_FILTERS[0][0])
    for t, tk, tp in M.FREQ_FILTERS:
        order, m, c = M.filter_ref(z, tk, tp, 1)
        assert M.clear(c, tp).all() and 2 <= int(m[0]) <= tk
    X = torch.zeros(M.HIT_ROWS, M.HIT_V)
    X[:, M.HIT_WORD] = -40.0
    assert M.clear(M.filter_ref(M.scaled(X.numpy(), 0.5), 0, 0.999, 1)[2], 0.999).all()


def test_dense_rows_have_wide_nuclei_and_narrow_bands():
    for V in M.DENSE_VS:
        X = M.dense_rows(V).numpy()
        widest = 0
        for t, tk, tp in M.DENSE_FILTERS:
            c = M.filter_ref(M.scaled(X, t), tk, tp, M.DENSE_K)[2]
            lo, hi = M.kept_band(c, tp)
            assert (lo >= 1).all() and (lo <= hi).all() and (hi - lo <= 8).all()
            widest = max(widest, int(lo.max()))
        assert widest > 1024                                           # a nucleus over every wave and thread stride


def test_rows_hold_what_their_names_say():
    for V in M.VS:
        names, X = M.rows(V)
        row = dict(zip(names, X))
        z = M.scaled(X.numpy(), 1.0)
        m = dict(zip(names, M.filter_ref(z, 0, 0.9, 1)[1]))
        assert m["peaked"] == m["peaked.1"] == m["peaked.2"] == 1
        assert not torch.equal(row["flat"], row["flat.1"]) and not torch.equal(row["random_a"], row["random_a.2"])
        assert int(torch.isinf(row["masked_a"]).sum()) == min(30, V // 3)
        flat = row["flat"]
        tie = torch.nonzero(flat == 0.0).flatten().tolist()
        order, mm, _ = M.filter_ref(z[names.index("flat")][None], 0, 0.5, 1)
        assert 2 < int(mm[0]) < len(tie) and order[0, 1:int(mm[0])].tolist() == tie[:int(mm[0]) - 1]    # inside the tie
        for nm in ("levels", "levels.1", "levels.2"):
            lv, o5 = row[nm], M.filter_ref(z[names.index(nm)][None], 5, 1.0, 1)[0][0]
            assert float(lv[o5[4]]) == float(lv[o5[5]])                 # the top_k = 5 cut falls inside a tie
        cw = M.crossing_words(V)
        assert set(M.filter_ref(z[names.index("crossing")][None], 0, 0.999, 1)[0][0, :len(cw)].tolist()) == set(cw)
        assert float(row["offset+80"].max()) > 70 and float(row["offset-80"][torch.isfinite(row["offset-80"])].max()) < -70


# ------------------------------------------------------------------------------------------------------ host rules
def test_check_sampling_filter():
    assert search.check_sampling_filter() is None
    assert search.check_sampling_filter(1.0, 0, 1.0) is None
    assert search.check_sampling_filter(1, 0, 1, sampling=False) is None
    f = search.check_sampling_filter(0.8, 20, 0.9)
    assert (f.inv_temperature, f.top_k, f.top_p) == (np.float32(1.25), 20, np.float32(0.9))
    assert search.check_sampling_filter(top_k=3).top_k == 3
    assert search.check_sampling_filter(top_p=0.5).top_p == 0.5
    assert search.check_sampling_filter(temperature=2.0).inv_temperature == 0.5
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1),
                dict(top_p=float("nan")), dict(temperature=1e-40), dict(temperature=1e46)):       # 1/t is inf, or 0, in fp32
        with pytest.raises(ValueError):
            search.check_sampling_filter(**bad)
    for kw in (dict(temperature=0.5), dict(top_k=4), dict(top_p=0.9)):
        with pytest.raises(ValueError, match="diverse_beam_search"):
            search.check_sampling_filter(**kw, sampling=False, where="diverse_beam_search")
        with pytest.raises(ValueError, match="sample_or_max='max'"):
            search.check_sampling_filter(**kw, sampling=False)


class StandIn:
    """A model that records what dispatch calls."""
    def __init__(self):
        self.calls = []

    def beam_search(self, *a, **k):
        self.calls.append(("beam_search", k))

    def get_batch_multiple_sampled_prediction(self, *a, **k):
        self.calls.append(("sampling", k))

    def diverse_beam_search(self, *a, **k):
        self.calls.append(("diverse", k))

    def _search_constraint_args(self, **k):
        return None


def test_dispatch_forwards_the_keys_only_when_present():
    keys = ("temperature", "top_k", "top_p")
    for mode in ("beam_search", "sampling", "diverse_beam_search"):
        m = StandIn()
        search.dispatch(m, mode, dict(sos_idx=1, eos_idx=2), None, None)
        assert not any(k in m.calls[0][1] for k in keys)
    for mode in ("beam_search", "sampling"):
        m = StandIn()
        search.dispatch(m, mode, dict(sos_idx=1, eos_idx=2, top_k=7), None, None)
        assert m.calls[0][1]["top_k"] == 7 and "temperature" not in m.calls[0][1] and "top_p" not in m.calls[0][1]
        m = StandIn()
        search.dispatch(m, mode, dict(sos_idx=1, eos_idx=2, temperature=0.7, top_p=0.9, top_k=0), None, None)
        assert {k: m.calls[0][1][k] for k in keys} == dict(temperature=0.7, top_k=0, top_p=0.9)
    m = StandIn()
    search.dispatch(m, "diverse_beam_search", dict(sos_idx=1, eos_idx=2, temperature=1.0, top_k=0, top_p=1.0), None, None)
    assert not any(k in m.calls[0][1] for k in keys)
    with pytest.raises(ValueError, match="diverse_beam_search"):
        search.dispatch(StandIn(), "diverse_beam_search", dict(sos_idx=1, eos_idx=2, top_p=0.9), None, None)


def test_search_methods_take_the_keywords():
    import inspect
    from on_device_image_captioning_amd.captioning_model import CaptioningModel
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    for fn in (CaptioningModel.beam_search, CaptioningModel.get_batch_multiple_sampled_prediction,
               EsembleCaptioningModel.ensemble_beam_search):
        p = inspect.signature(fn).parameters
        for name, default in (("temperature", 1.0), ("top_k", 0), ("top_p", 1.0)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    with pytest.raises(ValueError, match="sample_or_max='max'"):
        CaptioningModel.beam_search(CaptioningModel(), None, None, 1, 2, sample_or_max="max", top_k=5)


def test_defaults_launch_the_plain_draw(monkeypatch):
    calls = []
    monkeypatch.setattr(search.ops, "logsoftmax_sample", lambda *a, **k: calls.append("plain"))
    monkeypatch.setattr(search.ops, "logsoftmax_sample_filtered", lambda *a, **k: calls.append("filtered"))
    search.draw_candidates(None, None, None, 4, 10, 2, 7, None, search.check_sampling_filter(1.0, 0, 1.0))
    search.draw_candidates(None, None, None, 4, 10, 2, 7, None)
    assert calls == ["plain", "plain"]
    search.draw_candidates(None, None, None, 4, 10, 2, 7, None, search.check_sampling_filter(0.9, 0, 1.0))
    assert calls[-1] == "filtered"

    class St:
        logits, cand_val, cand_idx, pos, beam_state = torch.zeros(4, 10), None, None, None, None
        N, beams, n_img, T = 4, 2, 2, 5

    class Eng:
        def step_logits(self, st):
            pass
    monkeypatch.setattr(search.ops, "ensemble_logprobs", lambda *a, **k: None)
    monkeypatch.setattr(search.ops, "beam_step", lambda *a, **k: None)
    del calls[:]
    search.ensemble_step([Eng()], [St()], torch.zeros(4, 10), 2, sample_seed=3)
    search.ensemble_step([Eng()], [St()], torch.zeros(4, 10), 2, sample_seed=3, sample_filter=search.check_sampling_filter(top_k=3))
    assert calls == ["plain", "filtered"]


# ------------------------------------------------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    return _hip.load()


def test_abi_version_is_unchanged(lib):
    from on_device_image_captioning_amd import _hip
    assert _hip.ABI_VERSION == 27 and lib.odic_abi_version() == 27


def test_refusals_need_no_gpu(lib):
    from on_device_image_captioning_amd import _hip
    EINVAL, P = -1, 16                                                 # dummy non-null pointers: refused before any launch

    def call(flt=(1.25, 5, 0.9), logits=P, ldl=100, logp=None, ldp=0, tv=P, ti=P, N=4, V=100, k=3, null_f=False):
        f = None if null_f else ctypes.byref(_hip.SampleFilter(*flt))
        return lib.odic_logsoftmax_sample_filtered(logits, ldl, logp, ldp, tv, ti, None, N, V, k, f, 1, None, None)

    for t in (0.0, -1.0, float("inf"), float("nan")):
        assert call(flt=(t, 5, 0.9)) == EINVAL
    assert call(flt=(1.0, -1, 0.9)) == EINVAL
    for p in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert call(flt=(1.0, 5, p)) == EINVAL
    assert call(k=0) == EINVAL and call(k=17) == EINVAL and call(k=-1) == EINVAL
    assert call(V=2, ldl=2, k=3) == EINVAL and call(V=0, ldl=0, k=1) == EINVAL and call(V=262145, ldl=262145) == EINVAL
    assert call(ldl=99) == EINVAL and call(logp=P, ldp=99) == EINVAL
    assert call(N=0) == EINVAL and call(N=-3) == EINVAL
    assert call(null_f=True) == EINVAL and call(logits=None) == EINVAL and call(tv=None) == EINVAL and call(ti=None) == EINVAL
