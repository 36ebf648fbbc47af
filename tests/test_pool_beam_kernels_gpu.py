"""odic_pool_beam_step and odic_pool_beam_finalize on the GPU (`-m gpu`), driven directly with synthetic
candidates against the float32 model of tests/pool_beam_model.py: after every chained step tokens, log-probs, ancestors,
cumul, n_elem, has_eos, row_valid, next_tok, pos, done and every pool field are BIT-EQUAL to the model's, and after the
finalize the order and the scores too.  Every array lives inside a poisoned allocation (tests/guards.py) whose bands must
come back unchanged.

The kinds (pool_beam_model.case): all_eos — every row's EOS best at once, k offers into a pool that overflows; ties —
dyadic values, exact ties between totals across rows and between EOS and a word; equal_scores — equal sums and lengths
against equal entries already pooled; dead — dead rows, rows of -inf candidates, -inf EOS; nan — NaN candidates and NaN
EOS log-probs; close_one — image 0 closes by the bound at the first step while the others run on, are left alone, and
*done rises only when the last has closed (early stopping); last — the last position t = T - 2, then a step that must
change nothing; min_length — EOS best everywhere but not yet allowed; empty — one live row with one candidate: k - 1
EMPTY rows; seed — t = 0 over a state whose cumul / n_elem / has_eos hold garbage.
"""
import ctypes

import numpy as np
import pytest
import torch

import guards
import pool_beam_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
STATE = ("tokens", "logprobs", "anc", "cumul", "n_elem", "has_eos", "row_valid", "next_tok", "pos", "done", "ctr")
POOL = M.POOL_KEYS + ("scale",)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def put(a) -> guards.Guarded:
    """A numpy array as one guarded row on the device."""
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(1, -1))
    return guards.poisoned_input(t, 1, t.shape[1], t.shape[1], device=DEV)


class Device:
    """The beam state and the pool of a case, every array inside a guarded allocation."""

    def __init__(self, ops, c):
        from on_device_image_captioning_amd import _hip
        self.n_img, self.k, self.T = c["st"]["tokens"].shape
        self.g = {name: put(c["st"][name]) for name in M.STATE_KEYS}
        self.g["ctr"] = put(np.zeros(1, np.int32))
        self.p = {name: put(c["pool"][name]) for name in M.POOL_KEYS}
        self.p["scale"] = put(c["scale"])
        self.state = _hip.BeamState(*(self.g[n].data_ptr() for n in STATE))
        self.pool = _hip.PoolArgs(*(self.p[n].data_ptr() for n in POOL), c["min_words"], 1 if c["early"] else 0)
        self.ops = ops

    def step(self, cv, ci, elp):
        gs = [put(cv), put(ci), put(M.logp_rows(elp))]
        raw = [g_.raw.clone() for g_ in gs]
        N = self.n_img * self.k
        self.ops.pool_beam_step(gs[0].t.view(N, self.k), gs[1].t.view(N, self.k), gs[2].t.view(N, M.V), self.pool, self.state,
                                self.n_img, self.k, self.T, M.EOS)
        torch.cuda.synchronize()
        for g_, b, name in zip(gs, raw, ("cand_val", "cand_idx", "logp")):
            assert torch.equal(g_.raw, b), f"{name} was written"

    def finalize(self):
        order = guards.guarded(self.n_img, self.k, self.k, torch.int32, DEV)
        score = guards.guarded(self.n_img, self.k, self.k, torch.float32, DEV)
        self.ops.pool_beam_finalize(self.pool, self.state, order.t, score.t, self.n_img, self.k, self.T)
        torch.cuda.synchronize()
        order.assert_untouched(what="order")
        score.assert_untouched(what="score")
        return order.t.cpu().numpy(), score.t.cpu().numpy()

    def check(self, st, pool, what):
        for name, g_ in list(self.g.items()) + list(self.p.items()):
            g_.assert_untouched(what=f"{what} {name}")
        for name in M.STATE_KEYS:
            got = self.g[name].t.cpu().numpy().reshape(st[name].shape)
            assert np.array_equal(bits(got), bits(st[name])), f"{what}: {name}\n{got}\n{st[name]}"
        for name in M.POOL_KEYS:
            got = self.p[name].t.cpu().numpy().reshape(pool[name].shape)
            assert np.array_equal(bits(got), bits(pool[name])), f"{what}: pool {name}\n{got}\n{pool[name]}"
        assert int(self.g["ctr"].t.cpu().item()) == 0, f"{what}: the arrival counter is re-armed"


@pytest.mark.parametrize("k,T", [(k, T) for k in (1, 2, 3, 15) for T in (3, 8)])
@pytest.mark.parametrize("kind", M.KINDS)
def test_steps_and_finalize_equal_the_model_bit_for_bit(ops, kind, k, T):
    for n_img in (1, 3):
        for alpha in (0.0, 0.7, 1.0, 2.0):
            c = M.case(kind, n_img, k, T, alpha)
            dev = Device(ops, c)
            st, pool = M.copy(c["st"]), M.copy(c["pool"])
            what = f"{kind} n_img={n_img} k={k} T={T} alpha={alpha}"
            for i, (cv, ci, elp) in enumerate(c["steps"]):
                M.step(st, pool, cv, ci, elp, c["scale"], c["min_words"], c["early"])
                dev.step(cv, ci, elp)
                dev.check(st, pool, f"{what} step {i}")
            want_order, want_score = M.finalize(st, pool, c["scale"])
            order, score = dev.finalize()
            dev.check(st, pool, f"{what} finalize")
            assert np.array_equal(order, want_order), f"{what}: order\n{order}\n{want_order}"
            assert np.array_equal(bits(score), bits(want_score)), f"{what}: score\n{score}\n{want_score}"


def test_a_second_finalize_offers_nothing_again(ops):
    c = M.case("dead", 3, 3, 8, 1.0)
    dev = Device(ops, c)
    st, pool = M.copy(c["st"]), M.copy(c["pool"])
    first = dev.finalize()
    want = M.finalize(st, pool, c["scale"])
    again = dev.finalize()
    dev.check(st, pool, "finalize twice")
    for a, b in zip(first + again, want + want):
        assert np.array_equal(bits(a), bits(b))


def test_reset_and_refusals(ops):
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    c = M.case("all_eos", 3, 3, 8, 1.0)
    dev = Device(ops, c)
    arrays = [("state " + n, g_) for n, g_ in dev.g.items()] + [("pool " + n, g_) for n, g_ in dev.p.items()]
    before = {n: g_.raw.clone() for n, g_ in arrays}
    cv, ci, lp = put(c["steps"][0][0]), put(c["steps"][0][1]), put(M.logp_rows(c["steps"][0][2]))
    s, p = ctypes.byref(dev.state), ctypes.byref(dev.pool)

    def call(cv=cv.data_ptr(), ci=ci.data_ptr(), lp=lp.data_ptr(), ldl=M.V, pool=p, state=s, n_img=3, k=3, T=8, eos=M.EOS, V=M.V):
        return lib.odic_pool_beam_step(cv, ci, lp, ldl, pool, state, None, n_img, k, T, eos, V, None)

    no_score = _hip.PoolArgs(*[None if n == "score" else dev.p[n].data_ptr() for n in POOL], 0, 0)
    neg_min = _hip.PoolArgs(*[dev.p[n].data_ptr() for n in POOL], -1, 0)
    for kw in (dict(cv=None), dict(ci=None), dict(lp=None), dict(pool=None), dict(state=None), dict(k=16), dict(k=0),
               dict(T=1), dict(T=129), dict(n_img=0), dict(eos=-1), dict(eos=M.V), dict(ldl=M.V - 1), dict(V=0),
               dict(pool=ctypes.byref(no_score)), dict(pool=ctypes.byref(neg_min))):
        assert call(**kw) == -1, kw
    assert lib.odic_pool_beam_finalize(p, s, None, None, 3, 3, 8, None) == -1
    assert lib.odic_pool_beam_finalize(p, s, 16, 16, 3, 16, 8, None) == -1
    torch.cuda.synchronize()
    for n, g_ in arrays:
        assert torch.equal(g_.raw, before[n]), n
    ops.pool_reset(dev.pool, 3)
    torch.cuda.synchronize()
    for n, g_ in arrays:
        if n in ("pool count", "pool closed"):
            g_.assert_untouched(what=n)
            assert not g_.t.any()
        else:
            assert torch.equal(g_.raw, before[n]), n
