"""token_stats_model.py checked without a GPU: the fp32 model of token_stats_kernel sits inside the derived bounds of the
float64 reference with room to spare, its exact rules (ties, flagged targets, the status word, non-finite rows) are the ones
the kernel's code spells, and the case generator covers what it says it covers."""
import math

import numpy as np
import pytest
import torch

import token_stats_model as TM


def _all_ratios():
    worst = {}
    for f, V in TM.cases():
        x = TM.row(f, V)
        tg = TM.default_target(f, x)
        lt, s, am, ml, flagged = TM.kernel_model(x, tg)
        rlt, rs, ram, rml = TM.reference(x, tg)
        b = TM.bounds(x, tg)
        assert not flagged and am == ram, (f, V, am, ram)
        worst[(f, V)] = (TM.ratio(lt, rlt, b["logp_target"]), TM.ratio(s, rs, b["sum_logp"]), TM.ratio(ml, rml, b["max_logp"]))
    return worst


@pytest.fixture(scope="module")
def worst():
    return _all_ratios()


def test_model_is_inside_its_bounds_with_room_to_spare(worst):
    for f in TM.FAMILIES:
        rs = [r for (ff, _), r in worst.items() if ff == f]
        print(f"token-stats model {f:16s} worst err/bound: logp_target {max(r[0] for r in rs):.3f}, "
              f"sum_logp {max(r[1] for r in rs):.3f}, max_logp {max(r[2] for r in rs):.3f}")
    tot = [max(r[i] for r in worst.values()) for i in range(3)]
    print(f"token-stats model worst of all: logp_target {tot[0]:.3f}, sum_logp {tot[1]:.3f}, max_logp {tot[2]:.3f}")
    bad = {k: r for k, r in worst.items() if max(r) > TM.EMU_ROOM}
    assert not bad, bad
    # the figures the module's docstring quotes are the measured ones (two decimals, rounded up)
    for name, t in zip(("logp_target", "sum_logp", "max_logp"), tot):
        assert t <= TM.EMU_WORST[name] <= t + 0.02, (name, t)


def test_bounds_are_of_the_size_of_the_formats():
    """A bound that no wrong kernel could miss would prove nothing: on a `randn3` row the log-prob bound is a few fp32 ulp
    of the log-prob, far below the 2e-6·scale the scoring test uses, and the sum_logp bound is below 2e-6·|sum|."""
    for V in (257, 10000):
        x = TM.row("randn3", V)
        lt, s, _, ml = TM.reference(x, 5)
        b = TM.bounds(x, 5)
        scale = np.abs(np.asarray(x, np.float64) - x.max() + ml).max()
        assert b["logp_target"] < 2e-6 * scale and b["max_logp"] < 2e-6 * scale and b["sum_logp"] < 2e-6 * abs(s)
        assert b["max_logp"] > 2.0 ** -23                      # and never below one rounding of expf


def test_argmax_rule_is_the_stable_sort(worst):
    for f, V in TM.cases():
        x = TM.row(f, V)
        want = int(torch.argsort(torch.from_numpy(x).double()[None], dim=-1, descending=True, stable=True)[0, 0])
        assert TM.block_argmax(x)[1] == want, (f, V)
        assert float(TM.block_argmax(x)[0]) == float(x.max())


def test_tie_cases_are_ties_at_the_stated_indices():
    seen = set()
    for f, V in TM.cases():
        if not f.startswith("tie_"):
            continue
        x = TM.row(f, V)
        top = np.flatnonzero(x == x.max())
        assert len(top) == 2, (f, V, top)
        if f == "tie_i_i256":
            assert top[1] - top[0] == TM.NT                    # one thread's first and second element
        else:
            assert tuple(top) == tuple(sorted(TM.TIES[f](V))), (f, V, top)
        assert TM.block_argmax(x)[1] == top[0]
        seen.add(f)
    assert seen == {f for f in TM.FAMILIES if f.startswith("tie_")}
    # where the ties sit in the block: (thread, wave) = (i % 256, (i % 256) // 64)
    wave = lambda i: (i % TM.NT) // TM.WAVE                    # noqa: E731
    assert (wave(63), wave(64)) == (0, 1) and (wave(191), wave(192)) == (2, 3) and (wave(255), wave(256)) == (3, 0)
    assert wave(200) == TM.NWAVES - 1 and wave(261) == 0 and 200 < 261      # the wave reduced last holds the lower index


def test_every_v_has_at_least_four_families():
    assert TM.V_EDGES == (1, 2, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1025, 10000, 10003)
    for V in TM.V_EDGES:
        assert len(TM.families_at(V)) >= 4, V
        assert len(TM.families_at(V)) <= 40
    assert set(TM.families_at(10003)) == set(TM.FAMILIES)
    with pytest.raises(ValueError):
        TM.row("tie_63_64", 64)
    for need in ("randn3", "offset+1e4", "offset-1e4", "offset+1e30", "offset-1e30", "dominant", "uniform", "uniform_negzero",
                 "two_level", "underflow", "masked"):
        assert need in TM.FAMILIES


def test_families_are_what_their_names_say():
    V = 1025
    lg = lambda f: -TM.reference(TM.row(f, V))[3]              # noqa: E731
    assert lg("dominant") == 0.0                               # every other word underflows: logsumexp is the maximum
    x = np.asarray(TM.row("dominant", V), np.float64)
    assert 990 < np.median(x.max() - x) < 1010
    assert lg("uniform") == pytest.approx(math.log(V), abs=1e-12) and lg("uniform_negzero") == pytest.approx(math.log(V), abs=1e-12)
    assert np.signbit(TM.row("uniform_negzero", V)).all()
    x = TM.row("two_level", V)
    assert (x == 0).sum() == V - V // 2 and (x == -200).sum() == V // 2
    x = TM.row("underflow", V)
    assert (np.exp((x - x.max()).astype(np.float32)) == 0).mean() > 0.5          # expf underflows for most words
    x = TM.row("masked", V)
    assert np.isneginf(x).sum() == V // 3 and np.isfinite(x.max())
    for s in ("+", "-"):
        assert abs(float(TM.row(f"offset{s}1e30", V).mean())) == pytest.approx(1e30, rel=1e-6)
        assert abs(float(TM.row(f"offset{s}1e4", V).mean())) == pytest.approx(1e4, rel=1e-3)


def test_flagged_targets_and_the_status_word():
    V = 65
    X = np.stack([TM.row("randn3", V, seed=s) for s in range(8)])
    edges = TM.target_edges(V)
    assert edges == [0, 64, 65, -1, 2 ** 40, -2 ** 63] and len(edges) == len(TM.TARGET_EDGES)
    tg = edges + [7, 33]
    flagged = [False, False, True, True, True, True, False, False]
    for s_in, s_out in ((0, 1), (4, 5)):
        rows, status = TM.launch_model(X, tg, s_in)
        assert status == s_out
        for r, fl, x, t in zip(rows, flagged, X, tg):
            assert r[4] == fl
            if fl:
                assert float(r[0]) == 0.0                       # the flagged-target rule: exactly 0, not a log-prob
            else:
                assert float(r[0]) < 0.0 and TM.ratio(r[0], TM.reference(x, t)[0], TM.bounds(x, t)["logp_target"]) <= TM.EMU_ROOM
    for s_in in (0, 4):
        assert TM.launch_model(X, [0, 1, 2, 3, 4, 5, 6, V - 1], s_in)[1] == s_in       # no flagged row: untouched
    rows, status = TM.launch_model(X, None, 4)
    assert status == 4 and all(r[0] is None and not r[4] for r in rows)


def test_the_nonfinite_table_is_complete_and_the_model_follows_it():
    for name, c in TM.NONFINITE.items():
        for out in TM.OUTPUTS:
            assert out in c, (name, out)
        assert c["argmax"] in ("lowest_max", "finite_max", "zero", "emulated")
        assert all(c[o] in ("nan", "-inf", "finite") for o in ("logp_target", "sum_logp", "max_logp"))
    for want in ("masked_target", "pos_inf_one", "all_neg_inf", "nan_at_max", "nan_elsewhere"):
        assert want in TM.NONFINITE
    for V in (5, 64, 300, 513):
        for name in TM.nonfinite_at(V):
            x = TM.nonfinite_row(name, V)
            tg = TM.default_target(name, x) if name == "masked_target" else V // 2
            lt, s, am, ml, flagged = TM.kernel_model(x, tg)
            c = TM.NONFINITE[name]
            assert TM.in_class(lt, c["logp_target"]) and TM.in_class(s, c["sum_logp"]) and TM.in_class(ml, c["max_logp"]), (name, V)
            assert am == TM.nonfinite_argmax(name, x) and 0 <= am < V and not flagged, (name, V, am)
            assert float(TM.kernel_model(x, V)[0]) == 0.0 and TM.kernel_model(x, V)[4]      # flagged wins over NaN
    # torch.log_softmax, the oracle's form, puts the same class in every float output
    for name in ("pos_inf_one", "all_neg_inf", "nan_at_0", "nan_at_max"):
        assert bool(torch.isnan(torch.log_softmax(torch.from_numpy(TM.nonfinite_row(name, 64)).double(), -1)).all())
    x = TM.nonfinite_row("masked_target", 64)
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1)
    assert bool((lp[torch.from_numpy(np.isneginf(x))] == TM.NINF).all()) and float(lp.sum()) == TM.NINF


def test_a_nan_hides_exactly_the_lanes_behind_it():
    """Worked from wave_argmax, not from a run: a pair reaches lane 0 through lanes l & 31, l & 15, ... l & 1; a lane holding
    a NaN neither adopts nor is adopted.  NaN at lane 16: lane 48 (48 ^ 32 = 16) is hidden and nothing else is."""
    assert TM.lanes_hidden_by(16) == [48] and TM.lanes_hidden_by(32) == []
    assert TM.lanes_hidden_by(1) == [l for l in range(3, 64, 2)]
    assert TM.lanes_hidden_by(4) == [12, 20, 28, 36, 44, 52, 60]
    x = np.arange(64, dtype=np.float32) * 0
    for nan_lane, top, want in ((16, 48, 6), (16, 49, 49), (32, 0, 0), (1, 63, 6), (4, 60, 6), (4, 61, 61)):
        x[:] = 0
        x[6], x[top], x[nan_lane] = 1.0, 2.0, np.nan          # (lane 6 travels 6, 2, 0: behind none of them)
        assert TM.block_argmax(x)[1] == want, (nan_lane, top)
    # a NaN that is not its thread's first element is skipped altogether, whatever sits at the thread's first
    x = np.zeros(600, np.float32)
    x[300], x[44], x[400] = np.nan, 1.0, 3.0
    assert TM.block_argmax(x) == (np.float32(3.0), 400)
    lt, s, am, ml, _ = TM.kernel_model(x, 400)
    assert am == 400 and all(math.isnan(float(v)) for v in (lt, s, ml))       # arg-max and the sums disagree about the row


def test_empty_threads_and_waves_lose_against_a_real_minus_inf():
    for V in (1, 2, 5, 63):
        assert TM.block_argmax(np.full(V, TM.NINF, np.float32)) == (np.float32(TM.NINF), 0)
        x = TM.row("randn3", V)
        assert TM.block_argmax(x)[1] == int(np.argmax(x))
    lt, s, am, ml, _ = TM.kernel_model(np.array([-3.5], np.float32), 0)
    assert (float(lt), float(s), am, float(ml)) == (0.0, 0.0, 0, 0.0)          # V = 1: every output exact


def test_dec_embed_reference():
    emb = np.arange(12, dtype=np.float32).reshape(4, 3)
    pos = np.arange(6, dtype=np.float32).reshape(2, 3) * 0.5
    tok = np.array([[0, 3], [4, -1], [2 ** 40, TM.INT64_MIN]], dtype=object)
    y, prod, valid = TM.dec_embed_ref(tok, emb, pos, 2.0, [0, 1, 7])
    assert np.array_equal(y[0, 1], emb[3] * 2.0 + pos[1]) and np.array_equal(y[0, 0], emb[0] * 2.0 + pos[0])
    for n in (1, 2):
        assert np.array_equal(y[n], pos) and not prod[n].any()          # outside the table: exactly pos_table[t]
    assert valid.tolist() == [[0, 0], [1, 0], [1, 1]]
    assert TM.ulp32(1.0) == 2.0 ** -23 and TM.ulp32(1.99) == 2.0 ** -23 and TM.ulp32(-2.0) == 2.0 ** -22
