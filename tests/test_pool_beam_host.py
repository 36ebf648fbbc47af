"""Pooled beam search without a GPU: the float32 model of tests/pool_beam_model.py on hand-built cases whose
outcome can be checked by eye, the refusals of search.check_pool_beam, the `scale` table, and the binding."""
import math
import os
import re

import numpy as np
import pytest
import torch

import pool_beam_model as M

F = np.float32
SOS, EOS = M.SOS, M.EOS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def offer(pool, sm, ln, scale, T, tag=7):
    tok = np.zeros(T, np.int64)
    tok[:ln] = tag
    return M.pool_offer(pool, 0, F(sm), ln, scale, tok, np.zeros(T, F))


def state_at_1(k, T, cumul, lp1=None):
    """One image at position 1: every row [sos, 5 + r] with log-prob lp1[r] (default: its cumul)."""
    st = M.new_state(1, k, T)
    st["tokens"][0, :, 1] = 5 + np.arange(k)
    st["logprobs"][0, :, 1] = np.asarray(cumul if lp1 is None else lp1, F)
    st["cumul"][:] = np.asarray(cumul, F)
    st["n_elem"][:] = 2
    st["pos"][0] = 1
    return st


def cands(k, rows):
    """rows: per row (values of the k words, EOS log-prob) → cv, ci (row r's word c is 10·(r+1) + c), elp."""
    cv = np.array([r[0] for r in rows], F).reshape(k, k)
    ci = np.array([[10 * (r + 1) + c for c in range(k)] for r in range(k)], np.int32)
    return cv, ci, np.array([r[1] for r in rows], F)


# ------------------------------------------------------------------------------------------------- the pool
def test_pool_appends_then_replaces_the_worst_in_serial_order():
    T = 6
    scale = M.scale_table(T, 1.0)
    pool = M.new_pool(1, 3, T)
    assert [offer(pool, s, 2, scale, T) for s in (-4.0, -2.0, -6.0)] == [0, 1, 2]        # scores -2, -1, -3
    assert pool["serial"][0].tolist() == [0, 1, 2] and pool["score"][0].tolist() == [-2.0, -1.0, -3.0]
    assert offer(pool, -5.0, 2, scale, T) == 2                       # -2.5 beats the worst (-3): its slot, the next serial
    assert pool["serial"][0].tolist() == [0, 1, 3] and pool["score"][0].tolist() == [-2.0, -1.0, -2.5]
    assert offer(pool, -9.0, 2, scale, T) == -1 and pool["count"][0] == 3                # worse than all: nothing changes
    assert offer(pool, -3.0, 3, scale, T) == 2                       # -1 by length 3: replaces -2.5
    assert pool["serial"][0].tolist() == [0, 1, 4] and pool["len"][0].tolist() == [2, 2, 3]
    assert pool["sum"][0].tolist() == [-4.0, -2.0, -3.0]


def test_equal_score_does_not_replace_and_the_later_of_two_equals_is_the_worst():
    T = 6
    scale = M.scale_table(T, 0.0)                                    # alpha = 0: score = sum
    pool = M.new_pool(1, 2, T)
    assert [offer(pool, -3.0, 2, scale, T, tag=1), offer(pool, -3.0, 4, scale, T, tag=2)] == [0, 1]
    assert offer(pool, -3.0, 3, scale, T, tag=3) == -1               # equal is not strictly greater
    assert pool["tokens"][0, :, 0].tolist() == [1, 2]
    assert M.pool_worst(pool, 0) == 1                                # a tie goes to the highest serial
    assert offer(pool, -2.0, 3, scale, T, tag=4) == 1 and pool["tokens"][0, :, 0].tolist() == [1, 4]
    st = M.new_state(1, 2, T)
    st["has_eos"][:] = 1
    pool["closed"][0] = 1
    order, score = M.finalize(st, pool, scale)
    assert order[0].tolist() == [1, 0] and score[0].tolist() == [-2.0, -3.0]


def test_finalize_orders_equal_scores_by_serial():
    T = 6
    scale = M.scale_table(T, 0.0)
    pool = M.new_pool(1, 3, T)
    for s in (-2.0, -1.0, -2.0):
        offer(pool, s, 2, scale, T)
    pool["closed"][0] = 1
    order, _ = M.finalize(M.new_state(1, 3, T), pool, scale)
    assert order[0].tolist() == [1, 0, 2]


# ------------------------------------------------------------------------------------------------- the walk
def test_an_eos_beyond_rank_k_is_dropped_and_one_before_it_is_pooled():
    k, T = 2, 6
    st, pool, scale = state_at_1(k, T, [0.0, 0.0], lp1=[0.0, 0.0]), M.new_pool(1, k, T), M.scale_table(T, 1.0)
    # totals: EOS of row 0 -0.125 (rank 0: pooled), word 10 -0.25, EOS of row 1 -0.375 (rank 2 = k: dropped), word 20 -0.5
    cv, ci, elp = cands(k, [((-0.25, -3.0), -0.125), ((-0.5, -4.0), -0.375)])
    M.step(st, pool, cv, ci, elp, scale)
    assert pool["count"][0] == 1 and pool["tokens"][0, 0, :3].tolist() == [SOS, 5, EOS] and pool["len"][0, 0] == 3
    assert pool["sum"][0, 0] == F(-0.125) and pool["score"][0, 0] == F(-0.125) / F(3.0)
    assert pool["logprobs"][0, 0, :3].tolist() == [0.0, 0.0, -0.125]
    assert st["tokens"][0, :, :3].tolist() == [[SOS, 5, 10], [SOS, 6, 20]] and st["cumul"].tolist() == [-0.25, -0.5]
    assert st["has_eos"].tolist() == [0, 0] and st["row_valid"].tolist() == [1, 1] and st["n_elem"].tolist() == [3, 3]
    assert st["anc"][:, 1].tolist() == [0, 1] and st["pos"][0] == 2 and st["done"][0] == 0 and pool["closed"][0] == 0


def test_ties_go_to_the_lower_key_and_the_beam_stays_full():
    k, T = 2, 6
    st, pool, scale = state_at_1(k, T, [-1.0, -1.0]), M.new_pool(1, k, T), M.scale_table(T, 1.0)
    # every total is -1.5: keys in order row 0 word 0, row 0 word 1, row 0 EOS (rank 2: dropped) ...
    cv, ci, elp = cands(k, [((-0.5, -0.5), -0.5), ((-0.5, -0.5), -0.5)])
    M.step(st, pool, cv, ci, elp, scale)
    assert st["tokens"][0, :, 2].tolist() == [10, 11] and st["anc"][:, 1].tolist() == [0, 0] and pool["count"][0] == 0


def test_min_length_keeps_eos_out():
    k, T = 2, 6
    scale = M.scale_table(T, 1.0)
    cv, ci, elp = cands(k, [((-1.0, -2.0), -0.001), ((-1.0, -2.0), -0.001)])
    for min_words, pooled in ((2, 0), (1, 2)):                       # position 1: the caption would hold one word
        st, pool = state_at_1(k, T, [-1.0, -1.5]), M.new_pool(1, k, T)
        M.step(st, pool, cv, ci, elp, scale, min_words=min_words)
        assert pool["count"][0] == pooled
        assert not (st["tokens"][0, :, 2] == EOS).any() and st["has_eos"].tolist() == [0, 0]


def test_a_row_without_candidates_leaves_empty_rows():
    k, T = 3, 6
    st, pool, scale = state_at_1(k, T, [-1.0, -np.inf, -np.inf]), M.new_pool(1, k, T), M.scale_table(T, 1.0)
    cv, ci, elp = cands(k, [((-0.5, -np.inf, np.nan), -np.inf)] + [((-0.1, -0.2, -0.3), -0.1)] * 2)
    M.step(st, pool, cv, ci, elp, scale)
    assert st["tokens"][0, :, 2].tolist() == [10, EOS, EOS] and st["anc"][:, 1].tolist() == [0, 1, 2]
    assert st["cumul"].tolist() == [-1.5, -np.inf, -np.inf] and st["has_eos"].tolist() == [0, 1, 1] and pool["count"][0] == 0


# ------------------------------------------------------------------------------------------------- closing
def closing_case(alpha, worst_sum, early=False, T=4):
    """k = 1, the pool full with one hypothesis of length 2; the row goes on with cumul -2."""
    st, pool, scale = state_at_1(1, T, [-1.0]), M.new_pool(1, 1, T), M.scale_table(T, alpha)
    offer(pool, worst_sum, 2, scale, T)
    cv, ci, elp = cands(1, [((-1.0,), -50.0)])
    M.step(st, pool, cv, ci, elp, scale, early=early)
    return st, pool


def test_the_bound_divides_by_scale_T_and_closes_on_equality():
    # alpha = 1, T = 4: the best a live row of cumul -2 can still reach is -2 / 4 = -0.5
    st, pool = closing_case(1.0, -1.25)                              # worst -0.625 < -0.5: open
    assert pool["closed"][0] == 0 and st["row_valid"][0] == 1 and st["done"][0] == 0
    st, pool = closing_case(1.0, -1.0)                               # worst -0.5 >= -0.5: closed
    assert pool["closed"][0] == 1 and st["row_valid"][0] == 0 and st["done"][0] == 1
    assert st["tokens"][0, 0, :3].tolist() == [SOS, 5, 10] and st["cumul"][0] == -2.0       # the step itself is applied
    # the length in the bound is T, not the row's own 3: -2 / 3 = -0.667 would have closed the first case too
    assert F(-1.25) / F(2.0) >= F(-2.0) / F(3.0)
    # alpha = 0: the bound is the cumul itself
    assert closing_case(0.0, -2.5)[1]["closed"][0] == 0 and closing_case(0.0, -2.0)[1]["closed"][0] == 1


def test_early_stopping_closes_a_full_pool_whatever_the_scores():
    st, pool = closing_case(1.0, -40.0, early=True)
    assert pool["closed"][0] == 1 and st["row_valid"][0] == 0 and st["done"][0] == 1
    st, pool, scale = state_at_1(2, 6, [-1.0, -1.0]), M.new_pool(1, 2, 6), M.scale_table(6, 1.0)
    offer(pool, -1.0, 2, scale, 6)
    cv, ci, elp = cands(2, [((-1.0, -2.0), -50.0)] * 2)
    M.step(st, pool, cv, ci, elp, scale, early=True)                 # not full: open
    assert pool["closed"][0] == 0 and st["done"][0] == 0


def test_a_closed_image_is_left_alone_and_done_waits_for_the_others():
    k, T = 1, 6
    scale = M.scale_table(T, 1.0)
    st, pool = M.new_state(2, k, T), M.new_pool(2, k, T)
    st["tokens"][:, 0, 1], st["logprobs"][:, 0, 1], st["cumul"][:], st["n_elem"][:], st["pos"][0] = 5, -1.0, -1.0, 2, 1
    M.pool_offer(pool, 0, F(-0.1), 2, scale, np.zeros(T, np.int64), np.zeros(T, F))
    cv, ci, elp = np.full((2, 1), -1.0, F), np.full((2, 1), 9, np.int32), np.full(2, -50.0, F)
    M.step(st, pool, cv, ci, elp, scale)
    assert pool["closed"].tolist() == [1, 0] and st["row_valid"].tolist() == [0, 1] and st["done"][0] == 0
    before, pool_before = M.copy(st), M.copy(pool)
    M.step(st, pool, cv * F(5.0), ci, np.full(2, -0.001, F), scale)  # image 1 pools its EOS (-2.001 / 4) and closes: its row has -7 / 6
    assert st["pos"][0] == 3 and st["done"][0] == 1 and pool["closed"].tolist() == [1, 1]
    for key in ("tokens", "logprobs", "cumul", "n_elem", "row_valid", "next_tok"):
        assert np.array_equal(st[key].reshape(2, -1)[0], before[key].reshape(2, -1)[0]), key
    for key in M.POOL_KEYS:
        assert np.array_equal(pool[key][0], pool_before[key][0]), key


# ------------------------------------------------------------------------------------------------- finalize
def test_finalize_offers_the_unfinished_rows_of_an_open_image_only():
    k, T = 3, 5
    scale = M.scale_table(T, 1.0)
    st, pool = M.new_state(2, k, T), M.new_pool(2, k, T)
    st["tokens"][:, :, 1:4] = [[[5, 6, 7]] * k] * 2
    st["n_elem"][:] = 4
    st["cumul"][:] = [-4.0, -np.inf, -2.0, -1.0, -1.0, -1.0]
    st["has_eos"][:] = [0, 1, 0, 0, 0, 0]
    M.pool_offer(pool, 0, F(-0.9), 3, scale, np.array([SOS, 9, EOS, 0, 0]), np.zeros(T, F))       # score -0.3
    pool["closed"][1] = 1                                            # image 1 closed with an empty pool: stays empty
    order, score = M.finalize(st, pool, scale)
    assert pool["count"].tolist() == [3, 0] and pool["closed"].tolist() == [2, 3]
    assert order.tolist() == [[0, 2, 1], [-1, -1, -1]] and score[0].tolist() == [F(-0.9) / F(3.0), -0.5, -1.0]
    assert np.isneginf(score[1]).all()
    assert pool["tokens"][0, 1].tolist() == [SOS, 5, 6, 7, 0] and pool["len"][0].tolist() == [3, 4, 4]     # no EOS appended
    assert M.captions(pool, order, 2) == [[[SOS, 9, EOS], [SOS, 5, 6, 7]], [[SOS, EOS], [SOS, EOS]]]


@pytest.mark.parametrize("kind", M.KINDS)
def test_the_kernel_cases_keep_the_pool_invariants(kind):
    for n_img, k, T, alpha in ((1, 1, 3, 0.0), (3, 3, 8, 0.7), (3, 15, 8, 2.0), (1, 2, 3, 1.0)):
        c = M.case(kind, n_img, k, T, alpha)
        st, pool = M.copy(c["st"]), M.copy(c["pool"])
        for cv, ci, elp in c["steps"]:
            M.step(st, pool, cv, ci, elp, c["scale"], c["min_words"], c["early"])
            for b in range(n_img):
                cnt = int(pool["count"][b])
                assert 0 <= cnt <= k and len(set(pool["serial"][b, :cnt].tolist())) == cnt
                assert not np.isnan(pool["score"][b, :cnt]).any()
                if pool["closed"][b]:
                    assert cnt == k and not st["row_valid"][b * k:(b + 1) * k].any()
        order, score = M.finalize(st, pool, c["scale"])
        for b in range(n_img):
            cnt = int(pool["count"][b])
            assert sorted(order[b, :cnt].tolist()) == list(range(cnt)) and (order[b, cnt:] == -1).all()
            assert (np.diff(score[b, :cnt]) <= 0).all()


def test_the_cases_reach_what_they_are_named_for():
    c = M.case("all_eos", 3, 3, 8, 1.0)
    st, pool = M.copy(c["st"]), M.copy(c["pool"])
    M.step(st, pool, *c["steps"][0], c["scale"])
    assert pool["count"].tolist() == [3, 3, 3] and pool["serial"][0].max() == 4       # image 0 overflowed twice
    c = M.case("close_one", 3, 3, 8, 1.0)
    st, pool = M.copy(c["st"]), M.copy(c["pool"])
    dones = []
    for s in c["steps"]:
        M.step(st, pool, *s, c["scale"], c["min_words"], c["early"])
        dones.append((int(st["done"][0]), pool["closed"].tolist()))
    assert dones == [(0, [1, 0, 0]), (0, [1, 0, 0]), (1, [1, 1, 1])]
    c = M.case("empty", 1, 15, 8, 1.0)
    st, pool = M.copy(c["st"]), M.copy(c["pool"])
    M.step(st, pool, *c["steps"][0], c["scale"])
    assert (st["cumul"] > -np.inf).sum() == 1 and st["has_eos"].sum() == 14
    c = M.case("min_length", 1, 3, 8, 1.0)
    st, pool = M.copy(c["st"]), M.copy(c["pool"])
    M.step(st, pool, *c["steps"][0], c["scale"], c["min_words"])
    assert pool["count"][0] == 0


# ------------------------------------------------------------------------------------------------- the host layer
def test_check_pool_beam_refusals():
    from on_device_image_captioning_amd import search as S
    assert S.check_pool_beam(3, 1, 1) == 1.0 and S.check_pool_beam(15, 15, 0.0) == 0.0
    assert S.check_pool_beam(3, 3, 0.7, prefix=[], required_words=[[], []], sample_or_max="max") == 0.7
    for kw, msg in ((dict(prefix=[5]), "prefix is not supported in pool_beam_search"),
                    (dict(required_words=[[7]]), "required_words is not supported in pool_beam_search"),
                    (dict(sample_or_max="sample"), "sample_or_max='sample' is not supported in pool_beam_search"),
                    (dict(ensemble=True), "an ensemble is not supported in pool_beam_search")):
        with pytest.raises(ValueError, match=msg):
            S.check_pool_beam(3, 1, 1.0, **kw)
    for alpha in (-0.5, float("inf"), float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="length_penalty must be finite and >= 0"):
            S.check_pool_beam(3, 1, alpha)
    for k in (16, 0, 2.5, True):
        with pytest.raises(ValueError, match=r"beam_size must be an integer in \[1, 15\]"):
            S.check_pool_beam(k, 1, 1.0)
    for n in (0, 4):
        with pytest.raises(ValueError, match="how_many_outputs must be an integer in"):
            S.check_pool_beam(3, n, 1.0)


def test_the_ensemble_refuses_through_check_pool_beam():
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel as E
    with pytest.raises(ValueError, match="an ensemble is not supported in pool_beam_search"):
        E.pool_beam_search(None, None, [0], 1, 2)


def test_scale_table_is_the_float64_power_rounded_once():
    from on_device_image_captioning_amd import ops
    differs = 0
    for alpha in (0.0, 0.7, 1.0, 2.0, 0.3333):
        for T in (3, 20, 128):
            want = np.array([np.float32(math.pow(float(L), alpha)) for L in range(T + 1)], np.float32)
            got = ops.pool_scale(T, alpha)
            assert got.dtype == torch.float32 and got.shape == (T + 1,)
            assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (alpha, T)
            assert np.array_equal(M.scale_table(T, alpha).view(np.int32), want.view(np.int32))
            single = np.power(np.arange(T + 1, dtype=np.float32), np.float32(alpha))      # a float32 power: not the rule
            differs += int((single.view(np.int32) != want.view(np.int32)).sum())
    assert differs > 0                                               # the two roundings do differ somewhere: the rule matters
    assert M.scale_table(5, 0.0).tolist() == [1.0] * 6 and M.scale_table(3, 2.0).tolist() == [0.0, 1.0, 4.0, 9.0]


def test_binding_and_header_carry_the_pool_entry_points():
    from on_device_image_captioning_amd import _hip
    text = open(os.path.join(ROOT, "include", "odic_hip.h")).read()
    for name in ("odic_pool_reset", "odic_pool_beam_step", "odic_pool_beam_finalize"):
        assert name in _hip.EXPORTED_SYMBOLS and re.search(rf"\bint {name}\(", text)
    assert _hip.ABI_VERSION == 27 and re.search(r"#define ODIC_ABI_VERSION 27\b", text)              # a pure addition
    fields = re.search(r"typedef struct odic_pool_args \{(.*?)\} odic_pool_args;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\b(\w+)\s*[;,]", fields)
    assert names == [n for n, _ in _hip.PoolArgs._fields_]
    lib = _hip.load()
    assert lib.odic_pool_beam_step(None, None, None, 0, None, None, None, 1, 3, 8, 2, 10, None) == -1
    st = _hip.BeamState(*([16] * 11))
    pool = _hip.PoolArgs(*([16] * 9), 0, 0)
    import ctypes
    assert lib.odic_pool_beam_step(16, 16, 16, 10, ctypes.byref(pool), ctypes.byref(st), None, 1, 16, 8, 2, 10, None) == -1
    assert lib.odic_pool_beam_step(16, 16, 16, 10, ctypes.byref(pool), ctypes.byref(st), None, 1, 3, 8, 10, 10, None) == -1
    assert lib.odic_pool_beam_finalize(ctypes.byref(pool), ctypes.byref(st), None, 16, 1, 3, 8, None) == -1
    assert lib.odic_pool_reset(None, 1, None) == -1
