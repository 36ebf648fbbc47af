"""The numpy model of the diverse beam search step (tests/group_beam_model.py) against two independent statements of the
same rule — no GPU.

  * Candidate sufficiency: fed only the top-R candidates of every row (what odic_logsoftmax_topk hands the kernel with
    k = R), the model selects exactly what a brute force over the whole penalised vocabulary selects.
  * At one group the model is the existing step's rule (the lowest flat index of the k x k table).
"""
import numpy as np
import pytest

import group_beam_model as M

F = np.float32
LAMBDAS = (0.0, 0.3, 0.5, 1e4)
SHAPES = ((1, 3), (2, 2), (3, 3), (4, 4), (5, 3), (2, 8), (16, 1), (3, 1), (2, 5))


def sorted_rows(logp):
    """Every row's words by value descending, then word ascending: (values, words), each [rows, V]."""
    order = np.stack([np.lexsort((np.arange(r.size), -r.astype(np.float64))) for r in logp])
    return np.take_along_axis(logp, order, 1), order.astype(np.int32)


def random_case(rng, G, kg):
    R = G * kg
    V = int(rng.integers(max(8, R), 31))
    logp = (-np.round(rng.uniform(0.0, 3.0, size=(R, V)), 1)).astype(F)       # rounded to 0.1: ties are common
    t = int(rng.integers(0, 4))
    cumul = (-np.round(rng.uniform(0.0, 4.0, size=R), 1)).astype(F)
    has_eos = (rng.uniform(size=R) < 0.3).astype(np.int32) if t > 0 else np.zeros(R, np.int32)
    if t == 0:
        logp[:] = logp[0]                                                       # one distribution in every row
    return logp, cumul, has_eos, t


def brute_force(logp, cumul, has_eos, t, G, kg, lam):
    """Group by group over the WHOLE vocabulary, with the count kept as an array over the words."""
    R, V = logp.shape
    count = np.zeros(V, np.int64)
    picks = []
    for g in range(G):
        rows = [g * kg] if t == 0 else range(g * kg, g * kg + kg)
        table = []
        for j, row in enumerate(rows):
            if t > 0 and has_eos[row]:
                top = int(np.lexsort((np.arange(V), -logp[row].astype(np.float64)))[0])
                for w in range(V):
                    v = F(0.0) if w == top else F(-999.0)
                    table.append((-float(F(cumul[row] + v)), j, w, row, float(v), 0))
            else:
                for w in range(V):
                    v = F(logp[row, w] - F(F(lam) * F(count[w])))
                    table.append((-float(v if t == 0 else F(cumul[row] + v)), j, w, row, float(logp[row, w]), 1))
        table.sort(key=lambda x: x[:3])
        for x in table[:kg]:
            picks.append((x[3], x[2], x[4], x[5]))
        for x in table[:kg]:
            if x[5]:
                count[x[2]] += 1
    return picks


@pytest.mark.parametrize("lam", LAMBDAS)
def test_top_R_candidates_are_enough_for_the_penalised_selection(lam):
    rng = np.random.default_rng(1234 + int(lam * 10) % 97)
    n = 0
    for G, kg in SHAPES:
        R = G * kg
        for _ in range(40):
            logp, cumul, has_eos, t = random_case(rng, G, kg)
            sv, si = sorted_rows(logp)
            parent, word, lp, grow, _ = M.select_image(sv[:, :R], si[:, :R], cumul, has_eos, t, G, kg, lam)
            want = brute_force(logp, cumul, has_eos, t, G, kg, lam)
            got = [(int(parent[q]), int(word[q]), float(lp[q]), int(grow[q])) for q in range(R)]
            assert got == want, (G, kg, lam, t)
            # and the whole vocabulary as candidates changes nothing either
            full = M.select_image(sv, si, cumul, has_eos, t, G, kg, lam)
            assert [(int(full[0][q]), int(full[1][q])) for q in range(R)] == [(p, w) for p, w, _, _ in want]
            n += 1
    assert n == 40 * len(SHAPES)


def test_the_random_cases_do_exercise_penalties_ties_and_finished_beams():
    rng = np.random.default_rng(7)
    seen = dict(same_word_wanted=0, tie_across_beams=0, tie_within_beam_after_penalty=0, finished=0)
    for G, kg in SHAPES:
        for _ in range(40):
            logp, cumul, has_eos, t = random_case(rng, G, kg)
            sv, si = sorted_rows(logp)
            R = G * kg
            *_, grow, ev = M.select_image(sv[:, :R], si[:, :R], cumul, has_eos, t, G, kg, 0.5)
            for k in ev:
                seen[k] += bool(ev[k])
            seen["finished"] += int((grow == 0).any())
    assert all(v > 10 for v in seen.values()), seen


@pytest.mark.parametrize("k", (1, 2, 3, 5, 9, 16))
def test_one_group_is_the_existing_rule(k):
    rng = np.random.default_rng(100 + k)
    for _ in range(60):
        logp, cumul, has_eos, t = random_case(rng, 1, k)
        sv, si = sorted_rows(logp)
        for lam in LAMBDAS:
            parent, word, lp, grow, _ = M.select_image(sv[:, :k], si[:, :k], cumul, has_eos, t, 1, k, lam)
            p0, w0, l0 = M.single_group_rule(sv[:, :k], si[:, :k], cumul, has_eos, t)
            assert np.array_equal(parent, p0) and np.array_equal(word, w0) and np.array_equal(lp.view(np.int32), l0.view(np.int32))


def test_the_state_update_of_the_model():
    """Three hand-checked steps: 2 groups x 1 beam, 4 words, eos = 0, penalty 1."""
    st = M.new_state(1, 2, 4, sos=3)
    cv = np.array([[-0.25, -0.5], [-0.25, -0.5]], F)
    ci = np.array([[1, 2], [1, 2]], np.int32)
    st, ev = M.step(st, cv, ci, 2, 1, 1.0, eos=0)                 # group 0 takes word 1; group 1 pays 1.0 for it → word 2
    assert st["tokens"][0, :, :2].tolist() == [[3, 1], [3, 2]] and ev[0]["same_word_wanted"]
    assert st["logprobs"][0, :, 1].tolist() == [-0.25, -0.5] and st["cumul"].tolist() == [-0.25, -0.5]
    assert st["anc"][:, 0].tolist() == [0, 1] and st["n_elem"].tolist() == [2, 2] and int(st["pos"][0]) == 1
    cv = np.array([[-0.5, -1.0], [-0.125, -2.0]], F)
    ci = np.array([[0, 2], [0, 1]], np.int32)
    st, ev = M.step(st, cv, ci, 2, 1, 1.0, eos=0)                 # both want eos: group 1 at -0.125 - 1 still beats -2
    assert st["tokens"][0, :, 2].tolist() == [0, 0] and st["has_eos"].tolist() == [1, 1]
    assert st["logprobs"][0, :, 2].tolist() == [-0.5, -0.125] and st["cumul"].tolist() == [-0.75, -0.625]
    assert st["row_valid"].tolist() == [1, 1] and int(st["done"][0]) == 0 and ev[0]["all_finished"]
    st, ev = M.step(st, cv, ci, 2, 1, 1.0, eos=0)                 # finished: rank 0 at 0, nothing grows, done rises
    assert st["tokens"][0, :, 3].tolist() == [0, 0] and st["logprobs"][0, :, 3].tolist() == [0.0, 0.0]
    assert st["n_elem"].tolist() == [3, 3] and st["row_valid"].tolist() == [0, 0] and int(st["done"][0]) == 1
    assert st["cumul"].tolist() == [-0.75, -0.625] and int(st["pos"][0]) == 3
    again, _ = M.step(st, cv, ci, 2, 1, 1.0, eos=0)               # the prefix is full: nothing changes
    assert all(np.array_equal(again[k], st[k]) for k in M.STATE_KEYS)
