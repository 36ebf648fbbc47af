"""odic_logsoftmax_sample_scored and odic_stochastic_beam_step on the GPU (`-m gpu`).

  1. the scored draw: words, log-probs and log-prob rows bit for bit odic_logsoftmax_sample's; the perturbed scores against
     the exact noise of tests/sample_filter_model.py; short rows; leading dimensions;
  2. one step on every case of tests/stochastic_beam_model.py against the float64 model: integer state exact, gscore within
     the model's band, cumul and log-probs bitwise; every operand in a guarded buffer (tests/guards.py);
  3. the four invariants over four chained steps of a table-driven run;
  4. refused calls write nothing;
  5. the distribution: 32000 identical images, every complete caption enumerated — the captions of an image are distinct,
     row 0 follows p and row 1 the exact second-draw marginal of sampling without replacement.
"""
import ctypes
import statistics

import numpy as np
import pytest
import torch

import guards
import sample_filter_model as SF
import stochastic_beam_model as SM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SOS, EOS, D, LDY = SM.SOS, SM.EOS, SM.D, 13


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


# ------------------------------------------------------------------------------------------------- 1. the scored draw
DRAW_SEED, DRAW_POS, DRAW_N = 20190611, 3, 6


@pytest.mark.parametrize("V,k", [(V, k) for V in (5, 1023, 1025, 4099) for k in (1, 3, 16) if k <= V])
def test_scored_draw_is_the_plain_draw_plus_its_perturbed_scores(ops, V, k):
    rng = np.random.default_rng(V * 31 + k)
    x = (rng.standard_normal((DRAW_N, V)) * 3.0).astype(F)
    x[1] += F(40.0)                                                   # an offset row: |lse| large
    if V > 64:
        x[2, rng.choice(V, size=V // 3, replace=False)] = -np.inf     # masked words
    ldl, ldp = V + 5, V + 3
    gx = guards.poisoned_input(torch.from_numpy(x), DRAW_N, V, ldl, device=DEV)
    pos = torch.tensor([DRAW_POS], dtype=torch.int32, device=DEV)
    out = {}
    for name in ("plain", "scored"):
        lp = guards.guarded(DRAW_N, V, ldp, torch.float32, DEV)
        tv, ti = guards.guarded(DRAW_N, k, k, torch.float32, DEV), guards.guarded(DRAW_N, k, k, torch.int32, DEV)
        tp = guards.guarded(DRAW_N, k, k, torch.float32, DEV)
        if name == "plain":
            ops.logsoftmax_sample(gx.t, ldl, lp.t, ldp, tv.t, ti.t, DRAW_N, V, k, DRAW_SEED, pos)
        else:
            ops.logsoftmax_sample_scored(gx.t, ldl, lp.t, ldp, tv.t, ti.t, tp.t, DRAW_N, V, k, DRAW_SEED, pos)
        torch.cuda.synchronize()
        for g_, what in ((lp, "logp_out"), (tv, "top_val"), (ti, "top_idx")):
            g_.assert_untouched(what=f"{name} {what}")
        if name == "plain":
            tp.assert_all_poison("top_pert of the plain draw")
        else:
            tp.assert_untouched(what="top_pert")
        out[name] = (lp.t[:, :V].cpu().numpy(), tv.t.cpu().numpy(), ti.t.cpu().numpy(), tp.t.cpu().numpy())
    for a, b, what in zip(out["plain"][:3], out["scored"][:3], ("logp_out", "top_val", "top_idx")):
        assert np.array_equal(bits(a), bits(b)), f"V={V} k={k}: {what} differs from odic_logsoftmax_sample"
    _, tv, ti, tp = out["scored"]
    _, _, gum, lse = SM.scored_draw(x, k, DRAW_SEED, DRAW_POS)
    xs, gs = np.take_along_axis(x.astype(np.float64), ti, 1), np.take_along_axis(gum, ti, 1)
    want = xs + gs - lse[:, None]
    tol = 2e-6 + 2.0 ** -23 * (np.abs(xs) + np.abs(lse)[:, None] + np.abs(gs))
    err = np.abs(tp - want)
    print(f"V={V} k={k}: worst |top_pert - model| / tol = {np.nanmax(err / tol):.3f}")
    assert np.all(err <= tol), (V, k, float(np.nanmax(err / tol)))
    assert np.all(tp[:, :-1] > tp[:, 1:]), f"V={V} k={k}: top_pert is not strictly descending in draw order"
    assert np.all(np.isfinite(tv))


def test_scored_draw_short_row_gives_minus_infinity(ops):
    V, k = 5, 3
    x = np.full((2, V), -np.inf, F)
    x[0, [1, 3]] = [0.5, -0.25]
    x[1] = [0.1, 0.2, 0.3, 0.4, 0.5]
    gx = guards.poisoned_input(torch.from_numpy(x), 2, V, V + 4, device=DEV)
    tv, ti, tp = (guards.guarded(2, k, k, dt, DEV) for dt in (torch.float32, torch.int32, torch.float32))
    tv0, ti0 = guards.guarded(2, k, k, torch.float32, DEV), guards.guarded(2, k, k, torch.int32, DEV)
    ops.logsoftmax_sample_scored(gx.t, V + 4, None, 0, tv.t, ti.t, tp.t, 2, V, k, 5, None)
    ops.logsoftmax_sample(gx.t, V + 4, None, 0, tv0.t, ti0.t, 2, V, k, 5, None)
    torch.cuda.synchronize()
    v, i, p = tv.t.cpu().numpy(), ti.t.cpu().numpy(), tp.t.cpu().numpy()
    assert np.array_equal(bits(v), bits(tv0.t.cpu().numpy())) and np.array_equal(i, ti0.t.cpu().numpy())
    assert sorted(i[0, :2].tolist()) == [1, 3] and i[0, 2] == 0
    assert np.isneginf(v[0, 2]) and np.isneginf(p[0, 2]) and np.all(np.isfinite(p[0, :2])) and np.all(np.isfinite(p[1]))
    for g_ in (tv, ti, tp):
        g_.assert_untouched()


# ------------------------------------------------------------------------------------------------- 2. one step vs the model
class DeviceState:
    """A beam state, gscore, the embedding output and the candidates, every array inside a guarded allocation."""
    SPEC = (("tokens", torch.int64, "T"), ("logprobs", torch.float32, "T"), ("anc", torch.int32, "T"),
            ("cumul", torch.float32, 1), ("n_elem", torch.int32, 1), ("has_eos", torch.int32, 1), ("row_valid", torch.int32, 1),
            ("next_tok", torch.int64, 1), ("pos", torch.int32, 0), ("done", torch.int32, 0), ("ctr", torch.int32, 0))

    def __init__(self, ops, st: dict, gscore, T: int, with_emb=True):
        from on_device_image_captioning_amd import _hip
        n_img, k, _ = st["tokens"].shape
        N = n_img * k
        self.N, self.k, self.n_img, self.T, self.g = N, k, n_img, T, {}
        for name, dt, per in self.SPEC:                               # (one guarded row per beam row: the bands stay small)
            rows, cols = (N, T if per == "T" else 1) if per else (1, 1)
            src = torch.zeros(1, dtype=dt) if name == "ctr" else torch.from_numpy(np.ascontiguousarray(st[name]).reshape(-1))
            self.g[name] = guards.poisoned_input(src.view(rows, cols), rows, cols, cols, device=DEV)
        self.g["gscore"] = guards.poisoned_input(torch.from_numpy(np.asarray(gscore, F)).view(N, 1), N, 1, 1, device=DEV)
        self.state = _hip.BeamState(*(self.g[name].data_ptr() for name, _, _ in self.SPEC))
        self.emb = None
        if with_emb:
            embed, pos_table = SM.tables(T)
            self.embed, self.pos_table = torch.from_numpy(embed).to(DEV), torch.from_numpy(pos_table).to(DEV)
            self.y = guards.poisoned_input(torch.zeros(N, D), N, D, LDY, device=DEV)
            self.emb = ops.embed_args(self.embed, self.pos_table, self.y.t, LDY, D, SM.SCALE)
            self.g["y"] = self.y

    def arrays(self):
        out = {name: g_.t.cpu().numpy().reshape(-1) for name, g_ in self.g.items() if name != "y"}
        if "y" in self.g:
            out["y"] = self.y.t[:, :D].cpu().numpy()
        return out

    def raw(self):
        return {name: g_.raw.clone() for name, g_ in self.g.items()}

    def assert_contained(self, what):
        for name, g_ in self.g.items():
            g_.assert_untouched(what=f"{what} {name}")


def upload_candidates(c):
    N, k = c["cv"].shape
    gs = [guards.poisoned_input(torch.from_numpy(c[key]), N, k, k, device=DEV) for key in ("cv", "ci", "cp")]
    return gs, [g_.raw.clone() for g_ in gs]


@pytest.mark.parametrize("kind,n_img,k,T", SM.CASES)
def test_one_step_equals_the_model(ops, kind, n_img, k, T):
    c = SM.case(kind, n_img, k, T)
    dev = DeviceState(ops, c["st"], c["gscore"], T)
    before = dev.raw()
    (gv, gi, gp), raw = upload_candidates(c)
    ops.stochastic_beam_step(gv.t, gi.t, gp.t, dev.g["gscore"].t.view(-1), dev.state, n_img, k, T, EOS, emb=dev.emb)
    torch.cuda.synchronize()
    what = f"{kind} n_img={n_img} k={k} T={T}"
    dev.assert_contained(what)
    for g_, b, name in zip((gv, gi, gp), raw, ("cand_val", "cand_idx", "cand_pert")):
        assert torch.equal(g_.raw, b), f"{what}: {name} was written"
    if c["t"] + 1 >= T:                                               # the prefix is full: nothing changes
        for name, b in before.items():
            assert torch.equal(dev.g[name].raw, b), f"{what}: {name} changed at *pos = T - 1"
        return
    got, want = dev.arrays(), c["new"]
    live = want["cumul"] > -np.inf
    assert np.array_equal(got["cumul"] > -np.inf, live), f"{what}: the live rows\n{got['cumul']}\n{want['cumul']}"
    for key in SM.STATE_KEYS:
        w = want[key].reshape(-1)
        if key in ("pos", "done"):
            assert np.array_equal(got[key], w), f"{what}: {key}"
            continue
        per = w.size // live.size
        a, b = bits(got[key]).reshape(live.size, per)[live], bits(w).reshape(live.size, per)[live]
        assert np.array_equal(a, b), f"{what}: {key} of the live rows\n{a}\n{b}"
    assert np.array_equal(bits(got["y"])[live], bits(c["emb"]["y"])[live]), f"{what}: embedding rows"
    empty = ~live
    assert np.all(np.isneginf(got["gscore"][empty])) and np.all(got["has_eos"][empty] == 1) and \
        np.all(got["next_tok"][empty] == EOS), f"{what}: the empty rows"
    assert int(got["ctr"][0]) == 0, f"{what}: the arrival counter is re-armed"
    err = np.abs(got["gscore"][live].astype(np.float64) - c["gnew"][live])
    band = c["band"][live] + SM.EPS * np.abs(c["gnew"][live])         # + the model's value rounded to fp32
    print(f"{what}: worst |gscore - model| = {err.max():.3e}, band there {band[err.argmax()]:.3e}")
    assert np.all(err <= band), f"{what}: gscore outside the band: {err} vs {band}"
    exact = c["band"][live] == 0                                      # inherited / finished: a copy of an fp32 input
    assert np.array_equal(bits(got["gscore"][live][exact]), bits(c["gnew"][live][exact].astype(F))), f"{what}: inherited G"
    SM.check_invariants(c["st"], c["gscore"], {k_: got[k_].reshape(want[k_].shape) for k_ in SM.STATE_KEYS}, got["gscore"],
                        what)


def test_seeding_does_not_read_gscore(ops):
    """At *pos == 0 gscore need not be initialised: NaN there changes nothing."""
    c = SM.case("seed", 3, 5, 6)
    a = DeviceState(ops, c["st"], c["gscore"], 6)
    b = DeviceState(ops, c["st"], np.full_like(c["gscore"], np.nan), 6)
    for dev in (a, b):
        (gv, gi, gp), _ = upload_candidates(c)
        ops.stochastic_beam_step(gv.t, gi.t, gp.t, dev.g["gscore"].t.view(-1), dev.state, 3, 5, 6, EOS, emb=dev.emb)
    torch.cuda.synchronize()
    x, y = a.arrays(), b.arrays()
    for name in x:
        assert np.array_equal(bits(x[name]), bits(y[name])), name


# ------------------------------------------------------------------------------------------------- 3. invariants, chained
def table_logits(V: int, seed: int, eos_bias: float = 0.0) -> np.ndarray:
    t = (np.random.default_rng(seed).standard_normal((V, V)) * 1.2).astype(F)
    t[:, EOS] += F(eos_bias)
    return t


def run_table_search(ops, table: np.ndarray, n_img: int, k: int, T: int, seed: int, steps: int, check=None):
    """A search fed by logits = table[next_tok]; → the final device arrays.  check(before, g_before, after, g_after, t)."""
    V = table.shape[0]
    st = SM.new_state(n_img, k, T, SOS)
    dev = DeviceState(ops, st, np.zeros(n_img * k, F), T, with_emb=False)
    ops.beam_reset(dev.state, n_img, k, T, SOS)
    tab = torch.from_numpy(table).to(DEV)
    N = n_img * k
    cv, cp = (torch.empty(N, k, dtype=torch.float32, device=DEV) for _ in range(2))
    ci = torch.empty(N, k, dtype=torch.int32, device=DEV)
    for t in range(steps):
        before = dev.arrays() if check else None
        logits = tab[dev.g["next_tok"].t.view(-1)].contiguous()
        ops.logsoftmax_sample_scored(logits, V, None, 0, cv, ci, cp, N, V, k, seed, dev.g["pos"].t.view(-1))
        ops.stochastic_beam_step(cv, ci, cp, dev.g["gscore"].t.view(-1), dev.state, n_img, k, T, EOS)
        if check:
            torch.cuda.synchronize()
            check(before, dev.arrays(), t)
    torch.cuda.synchronize()
    dev.assert_contained("table search")
    return dev.arrays()


@pytest.mark.parametrize("k", (2, 5, 16))
def test_invariants_hold_over_four_chained_steps(ops, k):
    n_img, T, V = 3, 6, 24
    shape = lambda a: {key: a[key].reshape(s) for key, s in (("tokens", (n_img, k, T)), ("anc", (n_img * k, T)),
                                                              ("cumul", (-1,)), ("pos", (-1,)))}      # noqa: E731

    def check(before, after, t):
        SM.check_invariants(shape(before), before["gscore"], shape(after), after["gscore"], f"k={k} step {t}")
        assert int(after["ctr"][0]) == 0

    got = run_table_search(ops, table_logits(V, 3, eos_bias=2.5), n_img, k, T, 99, 4, check)
    assert int(got["pos"][0]) == 4
    assert bool((got["has_eos"] == 1).any()) and bool((got["has_eos"] == 0).any())       # finished beside growing rows


# ------------------------------------------------------------------------------------------------- 4. refusals
def test_refused_calls_write_nothing(ops):
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    c = SM.case("mixed", 3, 5, 6)
    dev = DeviceState(ops, c["st"], c["gscore"], 6)
    (gv, gi, gp), raw = upload_candidates(c)
    before = dev.raw()
    s, e = ctypes.byref(dev.state), ctypes.byref(dev.emb)
    gs = dev.g["gscore"].data_ptr()

    def call(cv=gv.data_ptr(), ci=gi.data_ptr(), cp=gp.data_ptr(), g=gs, state=s, emb=e, n_img=3, k=5, T=6, eos=EOS):
        return lib.odic_stochastic_beam_step(cv, ci, cp, g, state, emb, n_img, k, T, eos, None)

    no_anc = _hip.BeamState(*[None if n == "anc" else dev.g[n].data_ptr() for n, _, _ in DeviceState.SPEC])
    bad_emb = _hip.EmbedArgs(dev.embed.data_ptr(), dev.pos_table.data_ptr(), None, LDY, D, SM.SCALE, 6)
    for kw in (dict(cv=None), dict(ci=None), dict(cp=None), dict(g=None), dict(state=None), dict(state=ctypes.byref(no_anc)),
               dict(emb=ctypes.byref(bad_emb)), dict(n_img=0), dict(n_img=32768), dict(k=0), dict(k=17), dict(T=1), dict(T=129),
               dict(eos=-1)):
        assert call(**kw) == -1, kw                                   # ODIC_EINVAL
    x = torch.zeros(4, 100, device=DEV)
    tv, ti, tp = (guards.guarded(4, 3, 3, dt, DEV) for dt in (torch.float32, torch.int32, torch.float32))
    for args in ((None, tv, ti, tp, 3), (x, tv, ti, None, 3), (x, None, ti, tp, 3), (x, tv, ti, tp, 0), (x, tv, ti, tp, 17)):
        ptr = [None if a is None else a.data_ptr() for a in args[:4]]
        assert lib.odic_logsoftmax_sample_scored(ptr[0], 100, None, 0, ptr[1], ptr[2], ptr[3], 4, 100, args[4], 7, None, None) < 0
    with pytest.raises(RuntimeError, match="ODIC_EINVAL"):
        ops.stochastic_beam_step(gv.t, gi.t, gp.t, dev.g["gscore"].t.view(-1), dev.state, 3, 5, 6, -1, emb=dev.emb)
    torch.cuda.synchronize()
    for name, b in before.items():
        assert torch.equal(dev.g[name].raw, b), name
    for g_, b in zip((gv, gi, gp), raw):
        assert torch.equal(g_.raw, b)
    for g_ in (tv, ti, tp):
        g_.assert_all_poison("a refused draw")


# ------------------------------------------------------------------------------------------------- 5. the distribution
DIST_V, DIST_T, DIST_K, DIST_N, DIST_SEED = 6, 4, 3, 32000, 20190611


def enumerate_captions(table: np.ndarray):
    """Every complete caption of the table model (ends with EOS, or holds DIST_T - 1 words) → {words: probability}, float64."""
    x = table.astype(np.float64)
    logp = x - (x.max(1, keepdims=True) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)))
    out = {}

    def walk(prefix, last, lp):
        for w in range(DIST_V):
            p2, l2 = prefix + (w,), lp + logp[last, w]
            if w == EOS or len(p2) == DIST_T - 1:
                out[p2] = np.exp(l2)
            else:
                walk(p2, w, l2)

    walk((), SOS, 0.0)
    return out


def captions_of(arr, n_img, k, T):
    """Row captions as integer keys: the words behind SOS up to the row's length, base DIST_V + 1."""
    tok = arr["tokens"].reshape(n_img, k, T)
    ne = arr["n_elem"].reshape(n_img, k)
    key = np.zeros((n_img, k), np.int64)
    for j in range(1, T):
        key = key * (DIST_V + 1) + np.where(j < ne, tok[:, :, j] + 1, 0)
    return key


def caption_key(words):
    key = 0
    for j in range(DIST_T - 1):
        key = key * (DIST_V + 1) + (words[j] + 1 if j < len(words) else 0)
    return key


def test_the_captions_follow_sampling_without_replacement(ops):
    assert SOS < DIST_V and EOS < DIST_V
    table = table_logits(DIST_V, 17)
    assert np.all(np.isfinite(table))                                 # no masked words
    p = enumerate_captions(table)
    assert abs(sum(p.values()) - 1.0) < 1e-12 and len(p) == 1 + 5 + 25 + 125
    got = run_table_search(ops, table, DIST_N, DIST_K, DIST_T, DIST_SEED, DIST_T - 1)
    keys = captions_of(got, DIST_N, DIST_K, DIST_T)
    assert np.all(got["cumul"] > -np.inf)
    # (a) the captions of an image are pairwise distinct, always
    srt = np.sort(keys, axis=1)
    assert np.all(srt[:, :-1] != srt[:, 1:])
    assert set(np.unique(keys).tolist()) <= {caption_key(w) for w in p}
    # (b) row 0 follows p; (c) row 1 the second draw of sampling without replacement
    words = list(p)
    pv = np.array([p[w] for w in words])
    second = np.array([sum(pv[a] * pv[s] / (1.0 - pv[a]) for a in range(len(words)) if a != s) for s in range(len(words))])
    assert abs(second.sum() - 1.0) < 1e-9
    cells = [(row, s, q[s]) for row, q in ((0, pv), (1, second)) for s in range(len(words)) if DIST_N * q[s] >= 50]
    C = len(cells)
    z = statistics.NormalDist().inv_cdf(1.0 - 1e-3 / (2.0 * C))
    assert C * 2.0 * (1.0 - statistics.NormalDist().cdf(z)) <= 1e-3 * (1 + 1e-9) and C >= 20
    worst = 0.0
    for row, s, q in cells:
        n = int(np.sum(keys[:, row] == caption_key(words[s])))
        dev = abs(n - DIST_N * q) / np.sqrt(DIST_N * q * (1.0 - q))
        worst = max(worst, dev)
    print(f"{C} cells compared, bound z = {z:.3f} standard deviations, worst deviation {worst:.3f}")
    assert worst <= z, (worst, z)
    # the same seed gives the same captions, another seed others
    again = run_table_search(ops, table, DIST_N, DIST_K, DIST_T, DIST_SEED, DIST_T - 1)
    assert np.array_equal(again["tokens"], got["tokens"]) and np.array_equal(bits(again["gscore"]), bits(got["gscore"]))
    other = run_table_search(ops, table, DIST_N, DIST_K, DIST_T, DIST_SEED + 1, DIST_T - 1)
    assert not np.array_equal(captions_of(other, DIST_N, DIST_K, DIST_T), keys)
