"""Required words without a GPU: the argument rules of search.check_required_words, the properties of the numpy model of
tests/required_words_model.py over random multi-step runs, and the agreement of the header and the ctypes
binding on odic_require_beam_step."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_beam_model as GM
import required_words_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "odic_hip.h")
SOS, EOS, V = 3, 2, 40
F = np.float32


def check(required, n_img=2, **kw):
    from on_device_image_captioning_amd import search
    args = dict(V=V, beam_size=2, banned=None, sos_idx=SOS, eos_idx=EOS, max_seq_len=12, sampling=False)
    args.update(kw)
    return search.check_required_words(required, n_img, **args)


# ------------------------------------------------------------------------------------------------- argument rules
def test_nothing_required_is_none():
    for r in (None, [], (), [[], []], [(), []]):
        assert check(r) is None
    assert check([], sampling=True) is None                           # (nothing required: no rule is reached)


def test_one_list_serves_every_image_and_ragged_lists_are_padded():
    assert check([7, 9]) == [[7, 9], [7, 9]]
    assert check([[7], [9, 8, 5]], n_img=2) == [[7, -1, -1], [9, 8, 5]]
    assert check([[], [9]], n_img=2, beam_size=3) == [[-1], [9]]
    import torch
    assert check(torch.tensor([[7, 9], [5, 6]])) == [[7, 9], [5, 6]]
    assert check([torch.tensor([7]), [5, 6]]) == [[7, -1], [5, 6]]
    with pytest.raises(ValueError, match="3 lists of required words for 2 images"):
        check([[7], [8], [9]])


@pytest.mark.parametrize("C,largest", ((1, 8), (2, 4), (3, 2), (4, 1)))
def test_the_largest_beam_size_per_count_is_stated(C, largest):
    words = list(range(10, 10 + C))
    assert check(words, beam_size=largest) == [words, words]
    with pytest.raises(ValueError, match=rf"beam_size may be {largest} at most"):
        check(words, beam_size=largest + 1)


def test_every_refusal():
    with pytest.raises(ValueError, match="at most 4"):
        check([10, 11, 12, 13, 14], beam_size=1)
    with pytest.raises(ValueError, match="beam_size >= 2"):
        check([10], beam_size=1)
    for bad in (-1, V, V + 5):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            check([bad])
    for bad in (SOS, EOS):
        with pytest.raises(ValueError, match="SOS and EOS"):
            check([10, bad])
    with pytest.raises(ValueError, match="distinct"):
        check([[10, 11], [12, 12]])
    with pytest.raises(ValueError, match="both required and banned"):
        check([10, 11], banned=[5, 11])
    with pytest.raises(ValueError, match="max_seq_len - 2"):
        check([10, 11, 12], max_seq_len=4)
    assert check([10, 11], max_seq_len=4) is not None
    with pytest.raises(ValueError, match="deterministic"):
        check([10], sampling=True)
    assert check([10], V=lambda: V) == [[10], [10]]                    # (V may be a callable, as for the other rules)


def test_the_searches_that_do_not_take_required_words_refuse_them():
    from on_device_image_captioning_amd import search
    for nothing in (None, [], [[], []]):
        search.refuse_required_words(nothing, "here")
    for some in ([5], [[], [5]]):
        with pytest.raises(ValueError, match="not supported in diverse_beam_search"):
            search.refuse_required_words(some, "in diverse_beam_search")


def test_signatures_carry_the_keyword():
    import inspect
    from on_device_image_captioning_amd.captioning_model import CaptioningModel
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    for fn in (CaptioningModel.beam_search, CaptioningModel.diverse_beam_search, EsembleCaptioningModel.ensemble_beam_search):
        p = inspect.signature(fn).parameters["required_words"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_required_outputs_takes_the_accepting_bank_in_finalize_order():
    from on_device_image_captioning_amd import search
    ninf = float("-inf")
    # C = 1, kb = 2: rows 0-1 bank 0, rows 2-3 the accepting bank.  Image 0: both accepting rows live; image 1: none live;
    # image 2 (no word: bank 0 accepts).  The device order repeats row 0 for rows that score -inf.
    order = [[1, 3, 2, 0], [1, 0, 0, 0], [0, 1, 0, 0]]
    cumul = [[-4.0, -1.0, -3.0, -2.0], [-2.0, -1.0, ninf, ninf], [-1.0, -2.0, ninf, ninf]]
    rows, sat = search.required_outputs(order, cumul, [[7], [7], [-1]], 2, 2)
    assert rows.tolist() == [[3, 2], [1, 0], [0, 1]] and sat == [True, False, True]
    rows, sat = search.required_outputs([[1, 2, 0, 0]], [[-4.0, -1.0, -3.0, ninf]], [[7]], 2, 2)
    assert rows.tolist() == [[2, 1]] and sat == [True]                # one accepting row: the outputs go on with the others


# ------------------------------------------------------------------------------------------------- model properties
def random_step_inputs(rng, n_img, R, C, required, t, eos_bias):
    """Quantised log-prob rows [n_img·R, V] (multiples of 1/4), their top-R candidates, and the required words' values."""
    logp = -(rng.integers(0, 24, size=(n_img * R, V)) / 4.0).astype(F)
    if eos_bias:
        logp[rng.uniform(size=n_img * R) < 0.4, EOS] = 0.25
    if t == 0:
        logp[:] = logp[::R].repeat(R, axis=0)                         # seeding: every row of an image the same distribution
    order = np.lexsort((np.broadcast_to(np.arange(V), logp.shape), -logp), axis=1)[:, :R]
    cv, ci = np.take_along_axis(logp, order, 1), order.astype(np.int32)
    req = np.repeat(np.asarray(required, np.int64).reshape(n_img, C), R, axis=0)
    rl = np.where((req >= 0) & (req < V), np.take_along_axis(logp, np.clip(req, 0, V - 1), 1), -np.inf).astype(F)
    return cv, ci, rl


def run(seed, C, kb, T=9, n_img=3):
    rng = np.random.default_rng(seed)
    R = kb << C
    words = [w for w in range(V) if w not in (SOS, EOS)]
    required = np.full((n_img, C), -1, np.int64)
    for b in range(n_img):
        n = C if b != 1 else rng.integers(0, C + 1)                   # image 1: some slots unused
        required[b, :n] = rng.choice(words, size=n, replace=False)
    st = GM.new_state(n_img, R, T, SOS)
    trace = []
    for t in range(T - 1):
        cv, ci, rl = random_step_inputs(rng, n_img, R, C, required, t, eos_bias=t >= 2)
        st, ev = RM.step(st, cv, ci, rl, required, kb, EOS, V)
        trace.append((st, ev, (cv, ci)))
    return required, trace


CASES = ((0, 3), (1, 2), (1, 8), (2, 2), (2, 4), (3, 2), (4, 1))


@pytest.mark.parametrize("C,kb", CASES)
def test_a_live_rows_bank_is_the_set_of_required_words_it_holds(C, kb):
    seen = dict(entered=False, empty_slot=False, finished_stays=False, accepted=False)
    for seed in range(4):
        required, trace = run(seed, C, kb)
        R = kb << C
        for st, evs, _ in trace:
            for ev in evs:
                for k in ("entered", "empty_slot", "finished_stays"):
                    seen[k] |= bool(ev[k])
            live = RM.live_rows(st)
            for b in range(required.shape[0]):
                req = RM.used_slots(required[b], V)
                accept = RM.accepting_bank(req)
                for r in range(R):
                    n = b * R + r
                    if not live[n]:
                        assert st["has_eos"][n] == 1 and st["next_tok"][n] == EOS
                        continue
                    toks = st["tokens"][b, r, :st["n_elem"][n]].tolist()
                    held = sum(1 << c for c, w in enumerate(req) if w >= 0 and w in toks)
                    assert held == r // kb, (C, kb, seed, b, r, toks, req)
                    assert all(toks.count(w) <= 1 or (r // kb >> c) & 1 for c, w in enumerate(req) if w >= 0)
                    if EOS in toks:                                    # EOS only in the accepting bank, and only at the end
                        assert r // kb == accept and toks.index(EOS) == len(toks) - 1
                        seen["accepted"] |= C > 0
    assert seen["entered"] == (C > 0) and seen["finished_stays"]
    assert seen["empty_slot"] == (C > 0) and seen["accepted"] == (C > 0), seen


@pytest.mark.parametrize("kb", (1, 3, 8, 16))
def test_without_required_words_the_model_is_the_group_model_with_one_group(kb):
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        n_img, T = 3, 8
        a = GM.new_state(n_img, kb, T, SOS)
        b = GM.new_state(n_img, kb, T, SOS)
        for t in range(T - 1):
            cv, ci, rl = random_step_inputs(rng, n_img, kb, 0, np.zeros((n_img, 0)), t, eos_bias=t >= 2)
            a, _ = GM.step(a, cv, ci, 1, kb, 0.0, EOS)
            b, _ = RM.step(b, cv, ci, rl, np.zeros((n_img, 0), np.int64), kb, EOS, V)
            for k in GM.STATE_KEYS:
                x, y = a[k].reshape(-1), b[k].reshape(-1)
                assert np.array_equal(x.view(np.int32) if x.dtype == F else x, y.view(np.int32) if y.dtype == F else y), (kb, t, k)


def test_outputs_prefer_the_accepting_bank_and_fall_back():
    required, trace = run(1, 2, 2)
    st = trace[-1][0]
    rows, sat = RM.outputs(st, required, 2, 2, V)
    R = 8
    for b, (pick, ok) in enumerate(zip(rows, sat)):
        accept = RM.accepting_bank(RM.used_slots(required[b], V))
        assert ok == any(st["cumul"][b * R + accept * 2 + j] > -np.inf for j in range(2))
        assert (pick[0] // 2 == accept) == ok
        assert st["cumul"][b * R + pick[0]] > -np.inf


# ------------------------------------------------------------------------------------------------- header / binding
def test_header_declares_and_the_binding_binds_the_entry_point():
    from on_device_image_captioning_amd import _hip
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"int odic_require_beam_step\((.*?)\);", text, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["const float* cand_val", "const int32_t* cand_idx", "int32_t ncand", "const float* logp", "int64_t ldl",
                    "const int64_t* required", "int32_t n_required", "const odic_beam_state* st",
                    "const odic_embed_args* emb", "int32_t n_img", "int32_t bank_beams", "int32_t T", "int64_t eos_idx",
                    "int32_t V", "void* stream"]
    res, argtypes = _hip._SIGNATURES["odic_require_beam_step"]
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert res is ctypes.c_int
    assert list(argtypes) == [P, P, I32, P, I64, P, I32, ctypes.POINTER(_hip.BeamState), ctypes.POINTER(_hip.EmbedArgs),
                              I32, I32, I32, I64, I32, P]
    assert "odic_require_beam_step" in _hip.EXPORTED_SYMBOLS
    assert _hip.ABI_VERSION == 27 and re.search(r"#define ODIC_ABI_VERSION 27\b", text)   # a pure addition


def test_the_library_refuses_bad_arguments_without_a_gpu():
    from on_device_image_captioning_amd import _hip, ops
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _hip.load()
    assert hasattr(ops, "require_beam_step")
    st = _hip.BeamState(*([16] * 11))

    def call(C=2, kb=2, ncand=None, V_=V, ldl=V, logp=16, required=16, T=8, n_img=3, eos=EOS):
        R = kb << C if 0 <= C <= 4 else 0
        return lib.odic_require_beam_step(16, 16, R if ncand is None else ncand, logp, ldl, required, C, ctypes.byref(st),
                                          None, n_img, kb, T, eos, V_, None)

    bad = [dict(C=-1), dict(C=5, kb=1, ncand=32), dict(kb=0, ncand=0), dict(kb=-1, ncand=0), dict(C=2, kb=5), dict(C=0, kb=17),
           dict(C=4, kb=2), dict(ncand=7), dict(ncand=9), dict(C=1, kb=1), dict(ldl=V - 1), dict(V_=0, ldl=0), dict(logp=None),
           dict(required=None), dict(T=1), dict(T=129), dict(n_img=0), dict(n_img=32768), dict(eos=-1), dict(eos=V)]
    for kw in bad:
        assert call(**kw) == -1, kw                                     # ODIC_EINVAL, before any launch
