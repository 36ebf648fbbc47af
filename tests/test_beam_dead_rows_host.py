"""The dead-row models of tests/beam_dead_rows_model.py on the host (no GPU): they agree with the older models where no
-inf occurs, the rules the kernels had BEFORE the dead-row convention fail the assertions of test_beam_dead_rows_gpu.py
(shown here on the CPU only — those rules read out of bounds on a device), and the case generator reaches every class."""
import numpy as np
import pytest

import beam_dead_rows_model as D
import group_beam_model as M

F = np.float32
NEG = D.NEG
SHAPES = tuple((1, k) for k in D.BEAMS) + tuple(s for s in D.GROUP_SHAPES if s[0] > 1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_state(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in M.STATE_KEYS)


# ------------------------------------------------------------------------------------------------- the older models
def test_without_inf_the_model_is_the_search_loop_restatement_bit_for_bit():
    n_img, k, T, sos, eos = 6, 3, 14, 5, 7
    N = n_img * k
    rng = np.random.default_rng(3)
    for search in range(2):
        loop = D.SearchLoop(n_img, k, T, sos, eos)
        st = M.new_state(n_img, k, T, sos)
        finished = False
        for step in range(T - 1):
            cv, cw = D.search_loop_candidates(rng, N, k, step, eos)
            valid, nxt = loop.advance(cv, cw, step)
            st, _ = D.plain_step(st, cv, cw, eos)
            L = step + 2
            assert st["tokens"][:, :, :L].tolist() == loop.toks
            assert np.array_equal(bits(st["logprobs"][:, :, :L]), bits(np.array(loop.lps, dtype=F)))
            assert np.array_equal(bits(st["cumul"].reshape(n_img, k)), bits(np.array(loop.cumul(), dtype=F)))
            assert st["n_elem"].reshape(n_img, k).tolist() == loop.n_elem
            assert st["row_valid"].tolist() == valid and st["next_tok"].tolist() == nxt
            assert np.array_equal(st["anc"][:, :step + 1], loop.anc[:, :step + 1])
            finished |= not any(valid)
            assert int(st["done"][0]) == int(finished) and int(st["pos"][0]) == step + 1
        assert finished
        order, score = D.finalize(st["cumul"], st["n_elem"], n_img, k)
        cum = loop.cumul()
        for b in range(n_img):
            sc = [F(cum[b][j] / F(loop.n_elem[b][j])) for j in range(k)]
            assert order[b].tolist() == sorted(range(k), key=lambda j: (-sc[j], j))
            assert np.array_equal(bits(score[b]), bits(np.array(sc, F)))


@pytest.mark.parametrize("k", D.BEAMS)
def test_without_inf_the_model_is_single_group_rule(k):
    rng = np.random.default_rng(50 + k)
    for _ in range(40):
        cv = -np.sort(rng.integers(0, 9, size=(k, k)).astype(F) * 0.5, axis=1)
        ci = np.stack([np.sort(rng.choice(D.V, size=k, replace=False)) for _ in range(k)]).astype(np.int32)
        cumul = (-rng.integers(0, 40, size=k) / 4.0).astype(F)
        has_eos = (rng.uniform(size=k) < 0.3).astype(np.int32)
        for t in (0, 2):
            a = D.plain_select(cv, ci, cumul, has_eos, t, D.EOS)
            b = M.single_group_rule(cv, ci, cumul, has_eos, t)
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("k", D.BEAMS + (4,))
def test_one_group_of_the_group_model_is_the_plain_model_on_every_case(k):
    for batch in D.batches(1, k):
        plain, group = D.run(batch, 1, k, plain=True), D.run(batch, 1, k, plain=False)
        for (sa, ya, _), (sb, yb, _) in zip(plain, group):
            assert same_state(sa, sb), batch["classes"]
            assert np.array_equal(bits(ya), bits(yb))


# ------------------------------------------------------------------------------------------------- the old rules fail
def old_finalize_order(score):
    """The ranking before: a taken row's score overwritten with -inf, every round restarting at bi = 0, bv = -inf."""
    sc, out = [float(v) for v in score], []
    for _ in sc:
        bi, bv = 0, -np.inf
        for j, v in enumerate(sc):
            if v > bv:
                bv, bi = v, j
        sc[bi] = -np.inf
        out.append(bi)
    return out


def test_the_old_finalize_rule_lists_a_row_twice_on_the_fixture_scores():
    broken = 0
    for name, cumul, n_elem in D.FINALIZE_ROWS:
        k = len(cumul)
        order, score = D.finalize(np.array(cumul, F), np.array(n_elem), 1, k)
        assert sorted(order[0].tolist()) == list(range(k)), name
        old = old_finalize_order(score[0])
        if sorted(old) != list(range(k)):
            broken += 1
            assert old != order[0].tolist()
        else:
            assert old == order[0].tolist(), name                       # no dead row behind a live one: unchanged
    assert old_finalize_order([NEG, F(-0.5), NEG]) == [1, 0, 0]
    assert D.finalize(np.array([NEG, -2.0, NEG], F), np.array([3, 4, 3]), 1, 3)[0].tolist() == [[1, 0, 2]]
    assert broken >= 5


def old_plain_decode(cv, ci, cumul, has_eos, k):
    """beam_select before: the key of a round that finds nothing, 0x7fffffff, decoded as a flat candidate index.  Only
    the parents are formed here (the word was read at that index, outside the table)."""
    val = np.array([[(0.0 if c == 0 else -999.0) if has_eos[j] else cv[j, c] for c in range(k)] for j in range(k)], F)
    with np.errstate(invalid="ignore"):
        tot = (np.asarray(cumul, F)[:, None] + val).astype(F).reshape(-1)
    parents = []
    for _ in range(k):
        live = [i for i in range(k * k) if tot[i] > NEG]
        bi = min(live, key=lambda i: (-float(tot[i]), i)) if live else 0x7fffffff
        if live:
            tot[bi] = NEG
        parents.append(bi // k)
    return parents


@pytest.mark.parametrize("k", D.BEAMS)
def test_the_old_plain_decode_leaves_the_image_on_the_short_row_cases(k):
    outside = 0
    for batch in D.batches(1, k):
        for name, im in zip(batch["classes"], batch["images"]):
            parents = old_plain_decode(im["cv"], im["ci"], im["cumul"], im["he"], k)
            new = D.plain_select(im["cv"], im["ci"], im["cumul"], im["he"], D.T0, D.EOS)[0]
            assert all(0 <= p < k for p in new)
            if D.finite_totals(im) < k:
                assert any(not 0 <= p < k for p in parents), name
                outside += 1
            else:
                assert parents == new.tolist(), name
    assert outside >= (3 if k > 1 else 2)


def old_group_fill(cv, ci, cumul, has_eos, G, kg, lam):
    """group_beam_select before: a slot without a finite total left takes "the group's first one" (parent = the group's
    first row, word / value = that row's rank-0 candidate)."""
    parent, word, lp, grow, _ = M.select_image(cv, ci, cumul, has_eos, D.T0, G, kg, lam, D.EOS)
    for q in range(G * kg):
        if lp[q] == NEG and parent[q] == q and word[q] == D.EOS:      # (the slots the new rule leaves EMPTY)
            row0 = (q // kg) * kg
            parent[q], word[q], lp[q] = row0, ci[row0, 0], (F(0.0) if has_eos[row0] else cv[row0, 0])
    return parent, word, lp


def test_the_old_group_fill_puts_one_live_caption_into_a_group_twice():
    twice = 0
    for G, kg in D.GROUP_SHAPES:
        if kg == 1:
            continue
        for batch in D.batches(G, kg):
            for name, im in zip(batch["classes"], batch["images"]):
                new = M.select_image(im["cv"], im["ci"], im["cumul"], im["he"], D.T0, G, kg, D.PENALTY, D.EOS)
                old = old_group_fill(im["cv"], im["ci"], im["cumul"], im["he"], G, kg, D.PENALTY)
                for who, (parent, word, lp) in (("new", new[:3]), ("old", old)):
                    for g in range(G):
                        live = [(int(parent[q]), int(word[q])) for q in range(g * kg, g * kg + kg)
                                if im["cumul"][parent[q]] > NEG and lp[q] > NEG]
                        if who == "new":
                            assert len(set(live)) == len(live), (name, G, kg)
                        else:
                            twice += len(set(live)) != len(live)
    assert twice >= 3


# ------------------------------------------------------------------------------------------------- the case generator
def test_every_case_class_occurs_and_the_control_image_holds_no_inf():
    for G, kg in SHAPES:
        R = G * kg
        seen = {}
        for batch in D.batches(G, kg):
            assert batch["classes"][D.CONTROL] == "control" and len(batch["classes"]) == D.N_IMG
            rows = slice(D.CONTROL * R, (D.CONTROL + 1) * R)
            st = batch["state"]
            assert np.isfinite(st["cumul"][rows]).all() and np.isfinite(st["logprobs"][D.CONTROL]).all()
            assert not st["has_eos"][rows].any()
            assert all(np.isfinite(cv[rows]).all() for cv, _ in batch["cands"])
            for cv, ci in batch["cands"]:                               # rows as the group step wants them
                for n in range(cv.shape[0]):
                    assert len(set(ci[n].tolist())) == R
                    key = list(zip((-cv[n]).tolist(), ci[n].tolist()))
                    assert key == sorted(key)
            for name, im in zip(batch["classes"], batch["images"]):
                seen[name] = seen.get(name, 0) + 1
                n, live = D.finite_totals(im), [r for r in range(R) if im["cumul"][r] > NEG]
                if name.startswith("c1"):
                    assert n == R and len(live) == 1
                elif name == "c2_dead_interleaved":
                    assert n >= R and (R == 1 or len(live) < R)
                elif name == "c2_short_rows":
                    assert n >= R and (R == 1 or (im["cv"] == NEG).any())
                elif name == "c2_tie_across_dead":
                    if R >= 3:
                        tot = im["cumul"][:, None] + im["cv"]
                        assert im["status"][:3] == ["live", "dead", "live"] and tot[0, 0] == tot[2, 0] == np.max(tot)
                        assert (tot.reshape(-1) == tot[0, 0]).sum() == 2
                elif name.startswith("c3"):
                    assert n == dict(c3_k_minus_1=R - 1, c3_one=1, c3_zero=0)[name]
                elif name == "c4_finished_among_dead":
                    assert n == R and len(live) == 1 and im["he"][live[0]]
                elif name == "c4_empty_beside_live":
                    assert im["cumul"][0] == NEG and im["he"][0] and im["lp"][0, D.T0] == NEG
                elif name.startswith("c5"):
                    odd = [g for g in range(G) if any(s != "live" for s in im["status"][g * kg:(g + 1) * kg]) or
                           D.finite_totals(im, range(g * kg, g * kg + kg)) < kg * R]
                    assert len(odd) == 1 and odd[0] > 0                  # one group; the groups before it are healthy
                    assert all(D.finite_totals(im, range(g * kg, g * kg + kg)) == kg * R
                               for g in range(G) if g != odd[0])
                    rows = range(odd[0] * kg, odd[0] * kg + kg)
                    want = dict(c5_k_minus_1=kg - 1, c5_one=1, c5_zero=0, c5_penalised_only_one_left=1,
                                c5_finished_among_dead=R, c5_empty_beside_live=(kg - 1) * R)
                    assert D.finite_totals(im, rows) == want[name]
                    if name == "c5_finished_among_dead":
                        assert [im["status"][r] for r in rows if im["cumul"][r] > NEG] == ["fin"]
        assert seen.pop("control") == len(D.batches(G, kg))
        want = 12 + (6 if G > 1 else 0)
        assert len(seen) == want and all(v == 1 for v in seen.values()), (G, kg, seen)


def test_the_cases_do_what_their_class_says():
    """From the model alone: EMPTY rows appear behind the found ones and stay; chosen copies of a finished row carry -999;
    the penalised candidate is taken; `done` both rises and stays down."""
    seen = dict(empty=0, whole_image_empty=0, filler_999=0, penalised_taken=0, done_rises=0, done_stays_down=0)
    for G, kg in SHAPES:
        R = G * kg
        for batch in D.batches(G, kg):
            for plain in ((True, False) if G == 1 else (False,)):
                trace = D.run(batch, G, kg, plain)
                was = np.zeros((D.N_IMG, R), bool)
                for s, (st, _, evs) in enumerate(trace):
                    e = D.empty_rows(st, D.EOS)
                    t = int(st["pos"][0])
                    anc_self = st["anc"][:, t - 1].reshape(D.N_IMG, R) == np.arange(D.N_IMG * R).reshape(D.N_IMG, R)
                    assert not (was & anc_self & ~e).any(), "an EMPTY row that stays in its slot stays EMPTY"
                    dead_parent = batch["state"]["cumul"][st["anc"][:, D.T0]] == NEG if s == 0 else None
                    if s == 0:                                          # a dead row is nobody's parent but an EMPTY row's
                        assert (~dead_parent.reshape(D.N_IMG, R) | e).all()
                    assert not e[D.CONTROL].any()
                    seen["empty"] += int(e.sum())
                    seen["whole_image_empty"] += int(e.all(axis=1).sum())
                    seen["filler_999"] += int((st["logprobs"][:, :, t] == F(-999.0)).sum())
                    was = e
                    for b, name in enumerate(batch["classes"]):
                        if s == 0 and name == "c3_zero":
                            assert e[b].all()
                        if s == 0 and name == "c5_penalised_only_one_left":
                            q = (G - 1) * kg
                            assert st["tokens"][b, q, t] == 7 and st["cumul"][b * R + q] > NEG and e[b, q + 1:q + kg].all()
                            seen["penalised_taken"] += 1
                done = [int(st["done"][0]) for st, _, _ in trace]
                assert done == sorted(done)
                seen["done_rises" if done[-1] else "done_stays_down"] += 1
    assert all(v > 0 for v in seen.values()), seen
    assert seen["filler_999"] >= 8 and seen["whole_image_empty"] >= 8
