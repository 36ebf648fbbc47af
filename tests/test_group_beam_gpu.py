"""odic_group_beam_step on the GPU (`-m gpu`) against the float32 numpy model of tests/group_beam_model.py, exactly.

Candidates are fed directly (no decoder): multiples of 1/64 in [-12, 0], so that every product, difference and sum of
the step is exact in fp32 and a tie is a real tie; the embedding table, the position table and the scale are small
dyadic numbers for the same reason (a fused multiply-add then rounds like the two operations).  Five steps from
odic_beam_reset; after every step every state array and the embedding rows are compared with the model bit for bit.
All operands live in guarded buffers (tests/guards.py): the padding columns of y (ldy > d) and the bands around the
compact state and candidate arrays must keep their poison.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import group_beam_model as M
import guards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_IMG, T, D, V, LDY = 3, 6, 8, 24, 13
SOS, EOS = 3, 2
SCALE = 4.0
SHAPES = ((1, 3), (2, 2), (3, 3), (4, 4), (5, 3), (2, 8), (16, 1))
LAMBDAS = (0.0, 0.5, 1024.0)
STEPS = T - 1
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
def candidates(R: int):
    """Per step (cand_val, cand_idx) [N_IMG·R, R]: R distinct words per row, values descending, equal values by word.
    Most rows draw from a coarse grid (multiples of 1/2: ties, also after a penalty of 1/2) and from few words (the groups
    collide); image 2 at step 1 and every image at step 3 put EOS first and far ahead, so that whole images finish."""
    rng = np.random.default_rng(1000 + R)
    out = []
    for t in range(STEPS):
        cv = np.empty((N_IMG * R, R), F)
        ci = np.empty((N_IMG * R, R), np.int32)
        for n in range(N_IMG * R):
            b = n // R
            pool = [w for w in range(min(V, R + 3)) if not (w == EOS and t == 0)] if rng.uniform() < 0.7 else list(range(V))
            words = rng.choice(pool, size=R, replace=False) if len(pool) >= R else rng.choice(V, size=R, replace=False)
            if rng.uniform() < 0.75:
                vals = -rng.integers(0, 9, size=R) * 32                 # multiples of 1/2 in [-4, 0]
            else:
                vals = -rng.integers(0, 769, size=R)                    # multiples of 1/64 in [-12, 0]
            if (b == 2 and t == 1) or t == 3:
                words = np.concatenate([[EOS], rng.choice([w for w in range(V) if w != EOS], size=R - 1, replace=False)])
                vals = np.concatenate([[0], -640 - rng.integers(0, 5, size=R - 1) * 32])       # EOS at 0, the rest <= -10
            order = np.lexsort((words, -vals))
            cv[n], ci[n] = (vals[order] / 64.0).astype(F), words[order].astype(np.int32)
        out.append((cv, ci))
    return out


@functools.lru_cache(maxsize=None)
def model_run(G: int, kg: int, lam: float):
    """The numpy model over the five steps, computed once per case: [(state, y, events)] after every step."""
    R = G * kg
    embed, pos_table = tables()
    st = M.new_state(N_IMG, R, T, SOS)
    y = np.zeros((N_IMG * R, D), F)
    y[:] = embed[SOS] * F(SCALE) + pos_table[0]                        # what odic_beam_reset writes
    emb = dict(embed=embed, pos_table=pos_table, scale=SCALE, y=y)
    trace = []
    for cv, ci in candidates(R):
        st, ev = M.step(st, cv, ci, G, kg, lam, EOS, emb=emb)
        trace.append((st, y.copy(), ev))
    return trace


# ------------------------------------------------------------------------------------------------- device side
class DeviceState:
    """The beam state, the embedding output and nothing else, every array inside a guarded allocation."""
    SPEC = (("tokens", torch.int64, T), ("logprobs", torch.float32, T), ("anc", torch.int32, T), ("cumul", torch.float32, 1),
            ("n_elem", torch.int32, 1), ("has_eos", torch.int32, 1), ("row_valid", torch.int32, 1),
            ("next_tok", torch.int64, 1), ("pos", torch.int32, 0), ("done", torch.int32, 0), ("ctr", torch.int32, 0))

    def __init__(self, ops, R):
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

    def arrays(self):
        out = {name: self.g[name].t.cpu().numpy().reshape(-1) for name, _, _ in self.SPEC}
        out["y"] = self.y.t[:, :D].cpu().numpy()
        return out

    def assert_contained(self, what):
        for name in self.g:
            self.g[name].assert_untouched(what=f"{what} {name}")
        self.y.assert_untouched(what=f"{what} y")


def upload_candidates(cv, ci):
    n, c = cv.shape
    return (guards.poisoned_input(torch.from_numpy(cv), n, c, c, device=DEV),
            guards.poisoned_input(torch.from_numpy(ci), n, c, c, device=DEV))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_state_equals_model(got, st, y, what):
    for k in M.STATE_KEYS:
        assert np.array_equal(bits(got[k]), bits(st[k].reshape(-1))), f"{what}: {k}\n{got[k]}\n{st[k].reshape(-1)}"
    assert np.array_equal(bits(got["y"]), bits(y)), f"{what}: embedding rows"
    assert int(got["ctr"][0]) == 0, f"{what}: the arrival counter is re-armed"


# ------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("G,kg", SHAPES)
def test_five_steps_equal_the_numpy_model_exactly(ops, G, kg, lam):
    R = G * kg
    dev = DeviceState(ops, R)
    ops.beam_reset(dev.state, N_IMG, R, T, SOS, emb=dev.emb)
    trace = model_run(G, kg, lam)
    for t, (cv, ci) in enumerate(candidates(R)):
        gv, gi = upload_candidates(cv, ci)
        ops.group_beam_step(gv.t, gi.t, dev.state, N_IMG, G, kg, T, EOS, lam, emb=dev.emb)
        torch.cuda.synchronize()
        st, y, _ = trace[t]
        assert_state_equals_model(dev.arrays(), st, y, f"G={G} kg={kg} penalty={lam} step {t}")
        dev.assert_contained(f"G={G} kg={kg} step {t}")
        for g_, name in ((gv, "cand_val"), (gi, "cand_idx")):
            g_.assert_untouched(what=name)
            assert torch.equal(g_.t.cpu(), torch.from_numpy(cv if name == "cand_val" else ci)), f"{name} was written"
    # a sixth call finds the prefix full and changes nothing
    before = dev.arrays()
    ops.group_beam_step(gv.t, gi.t, dev.state, N_IMG, G, kg, T, EOS, lam, emb=dev.emb)
    torch.cuda.synchronize()
    after = dev.arrays()
    assert all(np.array_equal(bits(before[k]), bits(after[k])) for k in before)


def test_the_inputs_reach_every_case_the_selection_has():
    """From the model alone: what the comparison above covers."""
    seen = dict(same_word_wanted=False, tie_across_beams=False, tie_within_beam_after_penalty=False,
                beam_finishes_at_step_2_group_goes_on=False, image_finishes_early=False, done_rises_with_the_last_image=False)
    for G, kg in SHAPES:
        for lam in LAMBDAS:
            trace = model_run(G, kg, lam)
            R = G * kg
            for t, (st, _, evs) in enumerate(trace):
                for b, ev in enumerate(evs):
                    for k in ("same_word_wanted", "tie_across_beams", "tie_within_beam_after_penalty"):
                        seen[k] |= bool(ev[k]) and (G > 1 or k == "tie_across_beams")
                    he = st["has_eos"][b * R:(b + 1) * R]
                    if t == 2 and any(not he[(r // kg) * kg:(r // kg + 1) * kg].all() for r in ev["finished_now"]):
                        seen["beam_finishes_at_step_2_group_goes_on"] = True
                fin = [ev["all_finished"] for ev in evs]
                if any(fin) and not all(fin):
                    assert int(st["done"][0]) == 0
                    seen["image_finishes_early"] = True
            done = [int(st["done"][0]) for st, _, _ in trace]
            if done[-1] and any(any(ev["all_finished"] for ev in evs) and not all(ev["all_finished"] for ev in evs)
                                for _, _, evs in trace):
                first = done.index(1)
                assert first >= 2
                # `done` rises at the first step that no beam of any image entered still growing, and not before
                assert all(ev["all_finished"] for ev in trace[first - 1][2]) and \
                    not all(ev["all_finished"] for ev in trace[first - 2][2])
                seen["done_rises_with_the_last_image"] = True
    assert all(seen.values()), seen


@pytest.mark.parametrize("k", (1, 3, 8, 16))
def test_one_group_leaves_the_state_bitwise_as_beam_step_does(ops, k):
    a, b = DeviceState(ops, k), DeviceState(ops, k)
    ops.beam_reset(a.state, N_IMG, k, T, SOS, emb=a.emb)
    ops.beam_reset(b.state, N_IMG, k, T, SOS, emb=b.emb)
    for t, (cv, ci) in enumerate(candidates(k)):
        gv, gi = upload_candidates(cv, ci)
        ops.beam_step(gv.t, gi.t, a.state, N_IMG, k, T, EOS, emb=a.emb)
        ops.group_beam_step(gv.t, gi.t, b.state, N_IMG, 1, k, T, EOS, 0.5, emb=b.emb)
        torch.cuda.synchronize()
        x, y = a.arrays(), b.arrays()
        for name in x:
            assert np.array_equal(bits(x[name]), bits(y[name])), (k, t, name)


def test_invalid_arguments_are_refused_and_write_nothing(ops):
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    R = 4
    dev = DeviceState(ops, R)
    cv, ci = candidates(R)[0]
    gv, gi = upload_candidates(cv, ci)
    raw = [g.raw.clone() for g in list(dev.g.values()) + [dev.y, gv, gi]]
    s, e = ctypes.byref(dev.state), ctypes.byref(dev.emb)

    def call(ncand=R, n_img=N_IMG, groups=2, group_beams=2, T_=T, penalty=0.5):
        return lib.odic_group_beam_step(gv.data_ptr(), gi.data_ptr(), ncand, s, e, n_img, groups, group_beams, T_, EOS,
                                        penalty, None)

    bad = [dict(groups=0), dict(groups=-1), dict(group_beams=0), dict(groups=17, group_beams=1, ncand=17),
           dict(groups=3, group_beams=6, ncand=18), dict(groups=1 << 16, group_beams=1 << 16, ncand=0),
           dict(ncand=R - 1), dict(ncand=R + 1), dict(T_=1), dict(T_=129), dict(n_img=0), dict(n_img=32768),
           dict(penalty=-0.5), dict(penalty=float("inf")), dict(penalty=float("nan")), dict(penalty=-float("inf"))]
    for kw in bad:
        assert call(**kw) == -1, kw                                   # ODIC_EINVAL
    torch.cuda.synchronize()
    for g, before in zip(list(dev.g.values()) + [dev.y, gv, gi], raw):
        assert torch.equal(g.raw, before)
    with pytest.raises(RuntimeError, match="ODIC_EINVAL"):
        ops.group_beam_step(gv.t, gi.t, dev.state, N_IMG, 2, 2, T, EOS, -1.0, emb=dev.emb)
