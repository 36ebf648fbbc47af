"""odic_beam_step, odic_group_beam_step and odic_beam_finalize(_best) on DEAD rows (`-m gpu`) against the float32 numpy
models of tests/beam_dead_rows_model.py, exactly: rows with cumul = -inf, candidates of value -inf (the short-row rule of
the top-k kernels), finished rows and EMPTY rows, down to images with fewer than k totals above -inf.

The states are written directly at position 2 (no decoder), then three steps run.  Candidates and log-probs are multiples
of 1/64, the embedding tables small dyadic numbers: every sum of the step is exact in fp32, a tie is a real tie, and every
comparison below is of bits.  All operands live in guarded buffers (tests/guards.py) laid out as in
tests/test_group_beam_gpu.py.  tests/test_beam_dead_rows_host.py shows on the CPU which of these assertions the rules
before the dead-row convention fail.
"""
import functools
import types

import numpy as np
import pytest
import torch

import beam_dead_rows_model as D
import group_beam_model as M
import guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDY = 13
F = np.float32
NEG = D.NEG
SPEC = (("tokens", torch.int64, D.T), ("logprobs", torch.float32, D.T), ("anc", torch.int32, D.T),
        ("cumul", torch.float32, 1), ("n_elem", torch.int32, 1), ("has_eos", torch.int32, 1),
        ("row_valid", torch.int32, 1), ("next_tok", torch.int64, 1), ("pos", torch.int32, 0), ("done", torch.int32, 0),
        ("ctr", torch.int32, 0))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


@functools.lru_cache(maxsize=None)
def model(G, kg, i, plain, only_image=None):
    """The numpy model of batch i, computed once and shared."""
    return D.run(D.batches(G, kg)[i], G, kg, plain, only_image)


class DeviceState:
    """A model state on the device, the embedding output and nothing else, every array inside a guarded allocation."""

    def __init__(self, ops, st, n_img, R, T=D.T):
        from on_device_image_captioning_amd import _hip
        N = n_img * R
        self.n_img, self.R, self.N, self.T, self.g = n_img, R, N, T, {}
        for name, dt, per in SPEC:
            n = N * T if per > 1 else N if per == 1 else 1
            src = torch.zeros(1, n, dtype=dt) if name == "ctr" else torch.from_numpy(np.ascontiguousarray(st[name])).reshape(1, n)
            self.g[name] = guards.poisoned_input(src.to(dt), 1, n, n, device=DEV)
        self.state = _hip.BeamState(*(self.g[name].data_ptr() for name, _, _ in SPEC))
        embed, pos_table = D.tables()
        self.embed, self.pos_table = torch.from_numpy(embed).to(DEV), torch.from_numpy(pos_table).to(DEV)
        self.y = guards.poisoned_input(torch.zeros(N, D.DIM), N, D.DIM, LDY, device=DEV)
        self.emb = ops.embed_args(self.embed, self.pos_table, self.y.t, LDY, D.DIM, D.SCALE)

    def arrays(self):
        out = {name: self.g[name].t.cpu().numpy().reshape(-1) for name, _, _ in SPEC}
        out["y"] = self.y.t[:, :D.DIM].cpu().numpy()
        return out

    def assert_contained(self, what):
        for name in self.g:
            self.g[name].assert_untouched(what=f"{what} {name}")
        self.y.assert_untouched(what=f"{what} y")


def upload(cv, ci):
    n, c = cv.shape
    return (guards.poisoned_input(torch.from_numpy(cv), n, c, c, device=DEV),
            guards.poisoned_input(torch.from_numpy(ci), n, c, c, device=DEV))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_state_equals_model(got, st, y, what):
    for k in M.STATE_KEYS:                                             # (whole arrays: the columns behind t+1 keep the input)
        assert np.array_equal(bits(got[k]), bits(st[k].reshape(-1))), f"{what}: {k}\n{got[k]}\n{st[k].reshape(-1)}"
    assert np.array_equal(bits(got["y"]), bits(y)), f"{what}: embedding rows"
    assert int(got["ctr"][0]) == 0, f"{what}: the arrival counter is re-armed"


def run_steps(ops, batch, G, kg, plain, what, trace, only_image=None):
    """Three steps of one kernel on a batch (or on one of its images alone), every assertion after every step.
    → the device state and the arrays after every step."""
    R = G * kg
    st0, cands, n_img = batch["state"], batch["cands"], D.N_IMG
    if only_image is not None:
        b, rows, n_img = only_image, slice(only_image * R, (only_image + 1) * R), 1
        st0 = {k: (v[b:b + 1] if k in ("tokens", "logprobs") else v if k in ("pos", "done") else v[rows]) for k, v in st0.items()}
        st0 = dict(st0, anc=st0["anc"] - b * R)
        cands = [(np.ascontiguousarray(cv[rows]), np.ascontiguousarray(ci[rows])) for cv, ci in cands]
    dev = DeviceState(ops, st0, n_img, R)
    snaps = []
    for s, (cv, ci) in enumerate(cands):
        gv, gi = upload(cv, ci)
        if plain:
            ops.beam_step(gv.t, gi.t, dev.state, n_img, R, D.T, D.EOS, emb=dev.emb)
        else:
            ops.group_beam_step(gv.t, gi.t, dev.state, n_img, G, kg, D.T, D.EOS, D.PENALTY, emb=dev.emb)
        torch.cuda.synchronize()
        got = dev.arrays()
        st, y, _ = trace[s]
        assert_state_equals_model(got, st, y, f"{what} step {s}")
        dev.assert_contained(f"{what} step {s}")
        for g_, name, src in ((gv, "cand_val", cv), (gi, "cand_idx", ci)):
            g_.assert_untouched(what=name)
            assert np.array_equal(bits(g_.t.cpu().numpy()), bits(src)), f"{what} step {s}: {name} was written"
        snaps.append(got)
    return dev, snaps


def check_rules(batch, snaps, G, kg, trace, what):
    """What the dead-row convention promises, read from the DEVICE's arrays (the model enters only through `done`)."""
    R, n_img = G * kg, D.N_IMG
    embed, pos_table = D.tables()
    own = np.arange(n_img * R).reshape(n_img, R)
    was_empty = np.zeros((n_img, R), bool)
    prev_cumul = batch["state"]["cumul"]
    for s, got in enumerate(snaps):
        t = D.T0 + s                                                    # the position this step processed
        tok = got["tokens"].reshape(n_img, R, D.T)
        lp = got["logprobs"].reshape(n_img, R, D.T)
        cumul, he = got["cumul"].reshape(n_img, R), got["has_eos"].reshape(n_img, R)
        parent = got["anc"].reshape(n_img * R, D.T)[:, t].reshape(n_img, R)
        assert ((parent >= own[:, :1]) & (parent < own[:, :1] + R)).all(), f"{what} step {s}: a parent outside its image"
        empty = (cumul == NEG) & (he == 1) & (tok[:, :, t + 1] == D.EOS) & (lp[:, :, t + 1] == NEG) & (parent == own)
        fresh = lp[:, :, t + 1] == NEG
        assert (fresh == empty).all(), f"{what} step {s}: a stored log-prob of -inf marks an EMPTY row and nothing else"
        # a dead row is the parent of nothing but the EMPTY row in its own slot
        assert ((prev_cumul[parent.reshape(-1)].reshape(n_img, R) > NEG) | empty).all(), f"{what} step {s}"
        assert not (was_empty & (parent == own) & ~empty).any(), f"{what} step {s}: an EMPTY row came back"
        want_y = (embed[D.EOS] * F(D.SCALE) + pos_table[t + 1]).astype(F)
        for b, r in zip(*np.nonzero(empty)):
            assert np.array_equal(bits(got["y"][b * R + r]), bits(want_y)), f"{what} step {s}: input row of an EMPTY row"
        assert not empty[D.CONTROL].any()
        for b, name in enumerate(batch["classes"]):
            if name in ("c3_zero",):                                    # the whole image is EMPTY and stays EMPTY
                assert empty[b].all(), f"{what} step {s}: {name}"
            if name == "c1_live_first" and s == 0 and G == 1:       # the seeding of a prefix search, from position 2
                assert (parent[b] == own[b, 0]).all() and (cumul[b] > NEG).all()
            if kg > 1:                                                  # no live caption twice in a group
                for g in range(G):
                    live = [tuple(tok[b, q, :t + 2]) for q in range(g * kg, g * kg + kg) if cumul[b, q] > NEG]
                    assert len(set(live)) == len(live), f"{what} step {s}: image {b} group {g} holds a caption twice"
        # `done`: the step that no row entered still growing (a row that became EMPTY at this step did enter growing)
        entered_growing = got["row_valid"].any()
        assert int(got["done"][0]) == int(trace[s][0]["done"][0])
        assert int(got["done"][0]) == int(not entered_growing or (s > 0 and int(snaps[s - 1]["done"][0])))
        was_empty, prev_cumul = empty, got["cumul"]


def batch_ids(G, kg):
    return range(len(D.batches(G, kg)))


PLAIN_CASES = [(k, i) for k in D.BEAMS for i in batch_ids(1, k)]
GROUP_CASES = [(G, kg, i) for G, kg in D.GROUP_SHAPES for i in batch_ids(G, kg)]


# ------------------------------------------------------------------------------------------------- the steps
@pytest.mark.parametrize("k,i", PLAIN_CASES)
def test_beam_step_on_dead_rows_equals_the_model_exactly(ops, k, i):
    batch = D.batches(1, k)[i]
    what = f"beam_step k={k} {batch['classes']}"
    _, snaps = run_steps(ops, batch, 1, k, True, what, model(1, k, i, True))
    check_rules(batch, snaps, 1, k, model(1, k, i, True), what)
    # one group of the group step leaves the state bitwise as the plain step does
    _, other = run_steps(ops, batch, 1, k, False, what + " (one group)", model(1, k, i, True))
    for a, b in zip(snaps, other):
        assert all(np.array_equal(bits(a[name]), bits(b[name])) for name in a)
    # the control image alone: the other images do not reach it
    _, alone = run_steps(ops, batch, 1, k, True, what + " (control alone)", model(1, k, i, True, D.CONTROL), D.CONTROL)
    rows = slice(D.CONTROL * k, (D.CONTROL + 1) * k)
    for a, b in zip(snaps, alone):
        for name, _, per in SPEC[:8]:
            x = a[name].reshape(D.N_IMG * k, -1)[rows]
            assert np.array_equal(bits(x - (D.CONTROL * k if name == "anc" else 0)), bits(b[name].reshape(k, -1))), name
        assert np.array_equal(bits(a["y"][rows]), bits(b["y"]))


@pytest.mark.parametrize("G,kg,i", GROUP_CASES)
def test_group_beam_step_on_dead_rows_equals_the_model_exactly(ops, G, kg, i):
    batch = D.batches(G, kg)[i]
    what = f"group_beam_step G={G} kg={kg} {batch['classes']}"
    _, snaps = run_steps(ops, batch, G, kg, False, what, model(G, kg, i, False))
    check_rules(batch, snaps, G, kg, model(G, kg, i, False), what)
    R = G * kg
    _, alone = run_steps(ops, batch, G, kg, False, what + " (control alone)", model(G, kg, i, False, D.CONTROL), D.CONTROL)
    rows = slice(D.CONTROL * R, (D.CONTROL + 1) * R)
    for a, b in zip(snaps, alone):
        for name, _, per in SPEC[:8]:
            x = a[name].reshape(D.N_IMG * R, -1)[rows]
            assert np.array_equal(bits(x - (D.CONTROL * R if name == "anc" else 0)), bits(b[name].reshape(R, -1))), name
        assert np.array_equal(bits(a["y"][rows]), bits(b["y"]))


# ------------------------------------------------------------------------------------------------- finalize
def finalize_both(ops, dev, n_img, k, T):
    """Both kernels on a device state, outputs in guarded buffers → (order, score) of odic_beam_finalize and (order, score,
    out_tok, out_len) of odic_beam_finalize_best, as numpy."""
    mk = lambda r, c, dt: guards.guarded(r, c, c, dt, DEV)             # noqa: E731
    o1, s1 = mk(n_img, k, torch.int32), mk(n_img, k, torch.float32)
    o2, s2, ot, ol = mk(n_img, k, torch.int32), mk(n_img, k, torch.float32), mk(n_img, T, torch.int32), mk(1, n_img, torch.int32)
    before = dev.arrays()
    ops.beam_finalize(dev.state, o1.t, s1.t, n_img, k)
    ops.beam_finalize_best(dev.state, o2.t, s2.t, ot.t, ol.t, n_img, k, T, D.EOS)
    torch.cuda.synchronize()
    for g in (o1, s1, o2, s2, ot, ol):
        g.assert_untouched(what="finalize output")
    dev.assert_contained("finalize")
    after = dev.arrays()
    assert all(np.array_equal(bits(before[n]), bits(after[n])) for n in before), "finalize writes the state"
    return [g.t.cpu().numpy() for g in (o1, s1)], [g.t.cpu().numpy() for g in (o2, s2, ot, ol)]


def assert_finalize_equals_model(a, b, st, n_img, k, what):
    order, score, out_tok, out_len = D.finalize_best(st["tokens"], st["cumul"], st["n_elem"], n_img, k, D.EOS)
    for b_ in range(n_img):
        assert sorted(a[0][b_].tolist()) == list(range(k)), f"{what}: order of image {b_} is no permutation: {a[0][b_]}"
    assert np.array_equal(a[0], order), f"{what}: order\n{a[0]}\n{order}"
    assert np.array_equal(bits(a[1]), bits(score)), f"{what}: score"
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), f"{what}: the two kernels differ"
    assert np.array_equal(b[2], out_tok), f"{what}: out_tok\n{b[2]}\n{out_tok}"
    assert np.array_equal(b[3].reshape(-1), out_len), f"{what}: out_len"


@pytest.mark.parametrize("k", D.BEAMS)
def test_finalize_on_the_states_the_steps_leave(ops, k):
    for i in batch_ids(1, k):
        batch, trace = D.batches(1, k)[i], model(1, k, i, True)
        dev, _ = run_steps(ops, batch, 1, k, True, f"k={k} batch {i}", trace)
        a, b = finalize_both(ops, dev, D.N_IMG, k, D.T)
        assert_finalize_equals_model(a, b, trace[-1][0], D.N_IMG, k, f"k={k} {batch['classes']}")


@pytest.mark.parametrize("name,cumul,n_elem", D.FINALIZE_ROWS, ids=[r[0] for r in D.FINALIZE_ROWS])
def test_finalize_on_hand_made_scores(ops, name, cumul, n_elem):
    k, n_img, T = len(cumul), 3, D.T
    rng = np.random.default_rng(len(name))
    st = M.new_state(n_img, k, T, D.SOS)
    st["tokens"][:, :, 1:] = rng.integers(4, D.V, size=(n_img, k, T - 1))
    # image 0: the rows as given; image 1: reversed; image 2: all finite (the rows' n_elem as scores)
    st["cumul"][:] = np.concatenate([cumul, cumul[::-1], [-float(n) for n in n_elem]]).astype(F)
    st["n_elem"][:] = np.concatenate([n_elem, n_elem[::-1], n_elem[::-1]])
    st["has_eos"][:] = 1
    dev = DeviceState(ops, st, n_img, k, T)
    a, b = finalize_both(ops, dev, n_img, k, T)
    assert_finalize_equals_model(a, b, st, n_img, k, name)
    if name == "dead_live_dead":
        assert a[0][0].tolist() == [1, 0, 2]
    if "all_dead" in name or name == "one_dead":
        assert a[0][0].tolist() == list(range(k)) and b[3].reshape(-1)[0] == n_elem[0]    # row 0 is emitted


def test_rank_beams_on_a_required_words_state_is_a_permutation_with_the_dead_rows_last(ops):
    from on_device_image_captioning_amd import search
    n_img, kb, C, T, V = 3, 2, 1, D.T, D.V
    R = kb << C
    N = n_img * R
    st = M.new_state(n_img, R, T, D.SOS)
    dev = DeviceState(ops, st, n_img, R, T)
    ops.beam_reset(dev.state, n_img, R, T, D.SOS, emb=dev.emb)
    required = torch.tensor([[5], [9], [-1]], dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(2)
    for s in range(3):
        logp = torch.log_softmax(torch.randn(N, V, generator=g) * 2.0, dim=-1)
        val, idx = torch.sort(logp, dim=-1, descending=True, stable=True)
        ops.require_beam_step(val[:, :R].contiguous().to(DEV), idx[:, :R].to(torch.int32).contiguous().to(DEV), logp.to(DEV),
                              required, dev.state, n_img, kb, T, D.EOS, emb=dev.emb)
    torch.cuda.synchronize()
    got = dev.arrays()
    cumul = got["cumul"].reshape(n_img, R)
    assert (cumul == NEG).any() and (cumul > NEG).any(axis=1).all()     # the state does hold dead rows
    ns = types.SimpleNamespace(n_img=n_img, beams=R, tokens=dev.g["tokens"].t, beam_state=dev.state)
    order, score = search.rank_beams(ns)
    order, score = order.cpu().numpy(), score.cpu().numpy()
    want, want_score = D.finalize(got["cumul"], got["n_elem"], n_img, R)
    assert np.array_equal(order, want) and np.array_equal(bits(score), bits(want_score))
    for b in range(n_img):
        assert sorted(order[b].tolist()) == list(range(R))
        dead = [int(j) for j in order[b] if cumul[b, j] == NEG]
        assert dead == sorted(dead) and order[b].tolist()[R - len(dead):] == dead
