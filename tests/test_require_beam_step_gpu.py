"""odic_require_beam_step on the GPU (`-m gpu`) against the float32 numpy model of tests/required_words_model.py, exactly.

The kernel is fed directly (no decoder): log-prob rows that are multiples of 1/4 in [-6, 0], so that every sum of the step is
exact in fp32 and ties occur at every level of the order (total, source row, word); their top-R are the candidates.  The
embedding table, the position table and the scale are small dyadic numbers (a fused multiply-add then rounds like the two
operations).  Six chained steps from odic_beam_reset, so that banks fill, empty and finish; after every step every state
array and the embedding rows are compared with the model bit for bit on the live rows, and the empty rows are checked for
cumul = -inf, has_eos = 1, next_tok = EOS.  All operands live in guarded buffers (tests/guards.py); the log-prob rows have
ldl > V with +inf in the pad columns: a read there would win every ranking.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guards
import required_words_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_IMG, V, T, D, LDY, LDL = 3, 40, 8, 8, 13, 45
SOS, EOS = 3, 2
SCALE = 4.0
STEPS = 6
CASES = ((0, 3), (1, 2), (1, 8), (2, 2), (2, 4), (3, 2), (4, 1))
F = np.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


# ------------------------------------------------------------------------------------------------- inputs and the model
def tables():
    rng = np.random.default_rng(5)
    embed = (rng.integers(-16, 17, size=(V, D)) / 8.0).astype(F)
    pos_table = (rng.integers(-16, 17, size=(T, D)) / 8.0).astype(F)
    return embed, pos_table


@functools.lru_cache(maxsize=None)
def required_ids(C: int):
    """[N_IMG, C]: image 0 has C words; image 1 has every slot unused; image 2 has C words, the second one (C >= 2) an id
    >= V, which the kernel must treat as an unused slot."""
    rng = np.random.default_rng(70 + C)
    words = [w for w in range(V) if w not in (SOS, EOS)]
    req = np.full((N_IMG, C), -1, np.int64)
    if C:
        req[0] = rng.choice(words, size=C, replace=False)
        req[2] = rng.choice(words, size=C, replace=False)
        if C >= 2:
            req[2, 1] = V + 3
    return req


@functools.lru_cache(maxsize=None)
def inputs(C: int, kb: int):
    """Per step (logp [N, V], cand_val [N, R], cand_idx [N, R]).  Step 1 puts image 0's first required word on top of
    every row of that image (a required word as rank-0 candidate) and EOS on top of the rows of image 2 (EOS as rank-0
    candidate outside the accepting bank); from step 3 on EOS leads in many rows, so that accepting banks finish."""
    R = kb << C
    N = N_IMG * R
    rng = np.random.default_rng(1000 + 17 * C + kb)
    req = required_ids(C)
    out = []
    for t in range(STEPS):
        logp = -(rng.integers(1, 25, size=(N, V)) / 4.0).astype(F)
        if t == 1:
            if C:
                logp[:R, req[0, 0]] = 0.0
            logp[2 * R:, EOS] = 0.0
        if t >= 3:
            logp[rng.uniform(size=N) < 0.5, EOS] = 0.0
        if t >= 3 and C == 0:                                          # every row ends at once: `done` rises at the next step
            logp -= F(20.0)                                            # (with required words a non-accepting bank never ends)
            logp[:, EOS] = 0.0
        order = np.lexsort((np.broadcast_to(np.arange(V), logp.shape), -logp), axis=1)[:, :R]
        out.append((logp, np.take_along_axis(logp, order, 1).astype(F), order.astype(np.int32)))
    return out


def required_logp(logp, req, R):
    r = np.repeat(req, R, axis=0)
    return np.where((r >= 0) & (r < V), np.take_along_axis(logp, np.clip(r, 0, V - 1), 1), -np.inf).astype(F)


@functools.lru_cache(maxsize=None)
def model_run(C: int, kb: int):
    """The numpy model over the six steps, computed once per case: [(state, y, events)] after every step."""
    R = kb << C
    embed, pos_table = tables()
    st = RM.new_state(N_IMG, R, T, SOS)
    y = np.zeros((N_IMG * R, D), F)
    y[:] = embed[SOS] * F(SCALE) + pos_table[0]                        # what odic_beam_reset writes
    emb = dict(embed=embed, pos_table=pos_table, scale=SCALE, y=y)
    req = required_ids(C)
    trace = []
    for logp, cv, ci in inputs(C, kb):
        st, ev = RM.step(st, cv, ci, required_logp(logp, req, R), req, kb, EOS, V, emb=emb)
        trace.append((st, y.copy(), ev))
    return trace


# ------------------------------------------------------------------------------------------------- device side
class DeviceState:
    """The beam state, the embedding output and the required ids, every array inside a guarded allocation."""
    SPEC = (("tokens", torch.int64, T), ("logprobs", torch.float32, T), ("anc", torch.int32, T), ("cumul", torch.float32, 1),
            ("n_elem", torch.int32, 1), ("has_eos", torch.int32, 1), ("row_valid", torch.int32, 1),
            ("next_tok", torch.int64, 1), ("pos", torch.int32, 0), ("done", torch.int32, 0), ("ctr", torch.int32, 0))

    def __init__(self, ops, R, C=0):
        from on_device_image_captioning_amd import _hip
        N = N_IMG * R
        self.R, self.N, self.g = R, N, {}
        for name, dt, per in self.SPEC:
            n = N * per if per else 1
            self.g[name] = guards.poisoned_input(torch.zeros(1, n, dtype=dt), 1, n, n, device=DEV)
        self.state = _hip.BeamState(*(self.g[name].data_ptr() for name, _, _ in self.SPEC))
        embed, pos_table = tables()
        self.embed, self.pos_table = torch.from_numpy(embed).to(DEV), torch.from_numpy(pos_table).to(DEV)
        self.y = guards.poisoned_input(torch.zeros(N, D), N, D, LDY, device=DEV)
        self.emb = ops.embed_args(self.embed, self.pos_table, self.y.t, LDY, D, SCALE)
        self.req = guards.poisoned_input(torch.from_numpy(required_ids(C)), N_IMG, C, C, device=DEV) if C else None

    def arrays(self):
        out = {name: self.g[name].t.cpu().numpy().reshape(-1) for name, _, _ in self.SPEC}
        out["y"] = self.y.t[:, :D].cpu().numpy()
        return out

    def guarded(self):
        return list(self.g.values()) + [self.y] + ([self.req] if self.req is not None else [])

    def assert_contained(self, what):
        for name in self.g:
            self.g[name].assert_untouched(what=f"{what} {name}")
        self.y.assert_untouched(what=f"{what} y")
        if self.req is not None:
            self.req.assert_untouched(what=f"{what} required")


def upload(logp, cv, ci):
    """→ (logp with ldl = LDL and +inf in the pad columns, cand_val, cand_idx), guarded, and the raw bytes of all three."""
    n, c = cv.shape
    gl = guards.poisoned_input(torch.from_numpy(logp), n, V, LDL, device=DEV)
    gl.t[:, V:] = float("inf")
    gs = (gl, guards.poisoned_input(torch.from_numpy(cv), n, c, c, device=DEV),
          guards.poisoned_input(torch.from_numpy(ci), n, c, c, device=DEV))
    return gs, [g.raw.clone() for g in gs]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_state_equals_model(got, st, y, R, what):
    live = RM.live_rows(st)
    assert np.array_equal(got["cumul"] > -np.inf, live), f"{what}: the live rows\n{got['cumul']}\n{st['cumul']}"
    for k in RM.STATE_KEYS:
        want = st[k].reshape(-1)
        if k in ("pos", "done"):
            assert np.array_equal(got[k], want), f"{what}: {k}"
            continue
        per = want.size // live.size
        a, b = bits(got[k]).reshape(live.size, per)[live], bits(want).reshape(live.size, per)[live]
        assert np.array_equal(a, b), f"{what}: {k} of the live rows\n{a}\n{b}"
    assert np.array_equal(bits(got["y"])[live], bits(y)[live]), f"{what}: embedding rows of the live rows"
    empty = ~live
    assert np.all(np.isneginf(got["cumul"][empty])) and np.all(got["has_eos"][empty] == 1) and \
        np.all(got["next_tok"][empty] == EOS), f"{what}: the empty rows"
    assert int(got["ctr"][0]) == 0, f"{what}: the arrival counter is re-armed"


def run_step(ops, dev, gs, C, kb):
    gl, gv, gi = gs
    ops.require_beam_step(gv.t, gi.t, gl.t[:, :V], dev.req.t if C else None, dev.state, N_IMG, kb, T, EOS, emb=dev.emb)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("C,kb", CASES)
def test_six_chained_steps_equal_the_numpy_model_exactly(ops, C, kb):
    R = kb << C
    dev = DeviceState(ops, R, C)
    ops.beam_reset(dev.state, N_IMG, R, T, SOS, emb=dev.emb)
    trace = model_run(C, kb)
    y2 = torch.zeros(dev.N, D, device=DEV)
    for t, (logp, cv, ci) in enumerate(inputs(C, kb)):
        gs, raw = upload(logp, cv, ci)
        run_step(ops, dev, gs, C, kb)
        st, y, _ = trace[t]
        got = dev.arrays()
        assert_state_equals_model(got, st, y, R, f"C={C} kb={kb} step {t}")
        dev.assert_contained(f"C={C} kb={kb} step {t}")
        for g_, before, name in zip(gs, raw, ("logp", "cand_val", "cand_idx")):
            assert torch.equal(g_.raw, before), f"{name} was written"
        # the embedding tail: what odic_dec_embed makes of the chosen words at the new position, on every row
        assert t + 2 < T
        ops.dec_embed(dev.g["next_tok"].t.view(-1), dev.embed, dev.pos_table, dev.g["pos"].t.view(-1), y2, D, dev.N, D, SCALE)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got["y"]), bits(y2.cpu().numpy())), f"C={C} kb={kb} step {t}: embedding tail"


def test_the_inputs_reach_every_case_the_selection_has():
    """From the model alone: what the comparison above covers."""
    seen = dict(required_is_rank0=False, required_outside_candidates=False, eos_rank0_refused=False, tie_across_rows=False,
                tie_within_row=False, entered=False, empty_slot=False, finished_stays=False,
                unused_image_beside_a_full_one=False, id_beyond_the_vocabulary=False, a_bank_fills_up=False,
                an_accepting_row_finishes=False, done_rises=False)
    for C, kb in CASES:
        R, req = kb << C, required_ids(C)
        if C:
            seen["unused_image_beside_a_full_one"] |= bool((req[1] < 0).all() and (req[0] >= 0).all())
            seen["id_beyond_the_vocabulary"] |= bool((req >= V).any())
        trace = model_run(C, kb)
        live_before = None
        for st, _, evs in trace:
            for ev in evs:
                for k in ev:
                    if k in seen:
                        seen[k] |= bool(ev[k])
            live = RM.live_rows(st).reshape(N_IMG, 1 << C, kb).sum(axis=2)       # live rows per bank
            if live_before is not None and C and kb > 1:
                seen["a_bank_fills_up"] |= bool(((live_before > 0) & (live_before < kb) & (live == kb)).any())
            live_before = live
            for b in range(N_IMG):
                accept = RM.accepting_bank(RM.used_slots(req[b], V))
                rows = slice(b * R + accept * kb, b * R + accept * kb + kb)
                seen["an_accepting_row_finishes"] |= bool(C and accept and (RM.live_rows(st)[rows] & (st["has_eos"][rows] == 1)).any())
            seen["done_rises"] |= bool(st["done"][0])
    assert all(seen.values()), seen


@pytest.mark.parametrize("k", (1, 3, 8, 16))
def test_without_required_words_the_state_is_bitwise_what_beam_step_leaves(ops, k):
    a, b = DeviceState(ops, k), DeviceState(ops, k)
    ops.beam_reset(a.state, N_IMG, k, T, SOS, emb=a.emb)
    ops.beam_reset(b.state, N_IMG, k, T, SOS, emb=b.emb)
    rng = np.random.default_rng(300 + k)
    for t in range(STEPS):
        logp = -(rng.integers(1, 25, size=(N_IMG * k, V)) / 4.0).astype(F)
        if t >= 2:
            logp[rng.uniform(size=N_IMG * k) < 0.4, EOS] = 0.0
        order = np.lexsort((np.broadcast_to(np.arange(V), logp.shape), -logp), axis=1)[:, :k]
        (gl, gv, gi), _ = upload(logp, np.take_along_axis(logp, order, 1).astype(F), order.astype(np.int32))
        ops.beam_step(gv.t, gi.t, a.state, N_IMG, k, T, EOS, emb=a.emb)
        # once with the log-prob rows, once with neither them nor the ids (both may be NULL at n_required = 0)
        if t % 2:
            ops.require_beam_step(gv.t, gi.t, gl.t[:, :V], None, b.state, N_IMG, k, T, EOS, emb=b.emb)
        else:
            from on_device_image_captioning_amd import _hip
            assert _hip.load().odic_require_beam_step(gv.data_ptr(), gi.data_ptr(), k, None, V, None, 0, ctypes.byref(b.state),
                                                      ctypes.byref(b.emb), N_IMG, k, T, EOS, V, None) == 0
        torch.cuda.synchronize()
        x, y = a.arrays(), b.arrays()
        for name in x:
            assert np.array_equal(bits(x[name]), bits(y[name])), (k, t, name)
        b.assert_contained(f"k={k} step {t}")


def test_invalid_arguments_are_refused_and_write_nothing(ops):
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    C, kb = 2, 2
    R = kb << C
    dev = DeviceState(ops, R, C)
    logp, cv, ci = inputs(C, kb)[0]
    (gl, gv, gi), _ = upload(logp, cv, ci)
    everything = dev.guarded() + [gl, gv, gi]
    raw = [g.raw.clone() for g in everything]
    s, e = ctypes.byref(dev.state), ctypes.byref(dev.emb)

    def call(C_=C, kb_=kb, ncand=None, V_=V, ldl=LDL, lp=True, req=True, T_=T, n_img=N_IMG, eos=EOS):
        R_ = kb_ << C_ if 0 <= C_ <= 4 else 0
        return lib.odic_require_beam_step(gv.data_ptr(), gi.data_ptr(), R_ if ncand is None else ncand,
                                          gl.data_ptr() if lp else None, ldl, dev.req.data_ptr() if req else None, C_, s, e,
                                          n_img, kb_, T_, eos, V_, None)

    bad = [dict(C_=-1), dict(C_=5, kb_=1, ncand=32), dict(kb_=0, ncand=0), dict(kb_=-1, ncand=0), dict(kb_=5), dict(C_=0, kb_=17),
           dict(C_=4, kb_=2), dict(C_=3, kb_=4), dict(kb_=1 << 30, ncand=0), dict(ncand=R - 1), dict(ncand=R + 1), dict(C_=1, kb_=1),
           dict(ldl=V - 1), dict(V_=0, ldl=0), dict(V_=-3), dict(lp=False), dict(req=False), dict(T_=1), dict(T_=129), dict(n_img=0),
           dict(n_img=32768), dict(eos=-1), dict(eos=V)]
    for kw in bad:
        assert call(**kw) == -1, kw                                   # ODIC_EINVAL
    torch.cuda.synchronize()
    for g, before in zip(everything, raw):
        assert torch.equal(g.raw, before)
    with pytest.raises(RuntimeError, match="ODIC_EINVAL"):
        ops.require_beam_step(gv.t, gi.t, gl.t[:, :V], dev.req.t[:, :1].contiguous(), dev.state, N_IMG, 1, T, EOS, emb=dev.emb)
    with pytest.raises(ValueError, match="int64"):
        ops.require_beam_step(gv.t, gi.t, gl.t[:, :V], dev.req.t.int(), dev.state, N_IMG, kb, T, EOS, emb=dev.emb)
