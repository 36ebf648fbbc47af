"""odic_topk_rows_constrained on the GPU (`-m gpu`) against the numpy model of tests/search_constraints_model.py,
exactly: values bit for bit, indices equal.

`logp` is fed directly: multiples of 1/64, so that a tie is a real tie.  Six rows, T = 12:
  row 0  its unconstrained top-1 is on the ban list;
  row 1  EOS is its best word (in the top-k for every k): gone while pos < min_words, back at pos == min_words;
  row 2  prefix SOS a b a b c a b: the last n-1 words occur twice before, followed by a and by c — two words banned by
         two different start positions j, for n = 1, 2, 3; a and c are its two best words;
  row 3  200 words (every word where V < 200) tie at the best value: more than 128 tie at the k-th value where V allows;
  row 4  row 0 again, but finished (row_valid = 0): must equal odic_topk_rows bit for bit;
  row 5  prefix words outside [0, V) (and the ban list holds ids outside [0, V)): ignored.
All operands live in guarded buffers (tests/guards.py) with ldl > V: nothing outside top_val / top_idx may change.
A (V, k, ban list) that breaks n_banned + T + k <= V must be refused with ODIC_EINVAL and write nothing.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guards
import search_constraints_model as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T = 6, 12
SOS, EOS = 3, 2
A, B, C_ = 5, 6, 7
VS = (17, 64, 65, 4097, 10000, 10241)            # 10241: above the 10240 boundary of the register / streaming paths
KS = (1, 3, 9, 16)
POS = 7
MINW = 9
F = np.float32
EINVAL = -1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


# ------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(V: int):
    rng = np.random.default_rng(V)
    logp = (-rng.integers(64, 640, size=(N, V)) / 64.0).astype(F)           # multiples of 1/64 in (-10, -1]
    logp[1, EOS] = F(1.0 / 64)
    logp[2, A], logp[2, C_] = F(0.5), F(0.25)
    tie = rng.choice(V, size=min(V, 200), replace=False)
    logp[3, tie] = F(0.0)
    logp[4] = logp[0]
    tokens = rng.integers(8, min(V, 16), size=(N, T)).astype(np.int64)
    tokens[:, 0] = SOS
    tokens[2, :8] = [SOS, A, B, A, B, C_, A, B]
    tokens[4] = tokens[0]
    tokens[5, 1:6] = [V, -1, V + 1000, 1 << 40, -(1 << 40)]
    row_valid = np.ones(N, np.int32)
    row_valid[4] = 0
    top0 = int(np.lexsort((np.arange(V), -logp[0].astype(np.float64)))[0])
    banned = [top0, V + 100] if V < 64 else [top0, -5, V, V + 100, 9, int(1 << 30)]
    return logp, tokens, row_valid, np.array(banned, np.int32)


#: name → (banned?, no_repeat_ngram, min_words, pos)
CONFIGS = {
    "none": (False, 0, 0, POS),
    "banned": (True, 0, 0, POS),
    "min_words_before": (False, 0, MINW, MINW - 1),
    "min_words_reached": (False, 0, MINW, MINW),
    "ngram1": (False, 1, 0, POS),
    "ngram2": (False, 2, 0, POS),
    "ngram3": (False, 3, 0, POS),
    "ngram4_prefix_too_short": (False, 4, 0, 1),          # pos + 1 < n - 1
    "ngram12_prefix_too_short": (False, 12, 0, 9),
    "all": (True, 2, MINW, POS),
    "all_at_step_0": (True, 1, MINW, 0),
}


def model(V, k, name):
    logp, tokens, row_valid, banned = inputs(V)
    use_ban, g, mw, pos = CONFIGS[name]
    return SC.topk_rows_constrained(logp, k, tokens, pos, row_valid, banned.tolist() if use_ban else [], g, mw, EOS)


def plain(V, k):
    logp, tokens, _, _ = inputs(V)
    return SC.topk_rows_constrained(logp, k, tokens, 0)


class Device:
    """Every operand of the call for one V, each inside a guarded allocation; outputs per k."""

    def __init__(self, V):
        logp, tokens, row_valid, banned = inputs(V)
        self.V, self.ldl = V, V + 7
        g = lambda a, r, c, ld: guards.poisoned_input(torch.from_numpy(a.reshape(r, c)), r, c, ld, device=DEV)   # noqa: E731
        self.logp = g(logp, N, V, self.ldl)
        self.tokens = g(tokens, N, T, T)
        self.row_valid = g(row_valid, 1, N, N)
        self.banned = g(banned, 1, banned.size, banned.size)
        self.pos = g(np.zeros(1, np.int32), 1, 1, 1)
        self.inputs = dict(logp=self.logp, tokens=self.tokens, row_valid=self.row_valid, banned=self.banned, pos=self.pos)
        self.before = {k: v.raw.clone() for k, v in self.inputs.items() if k != "pos"}

    def constraints(self, name, **over):
        from on_device_image_captioning_amd import _hip
        use_ban, g, mw, pos = CONFIGS[name]
        self.pos.t.fill_(pos)
        f = dict(tokens=self.tokens.data_ptr(), pos=self.pos.data_ptr(), row_valid=self.row_valid.data_ptr(),
                 banned=self.banned.data_ptr() if use_ban else None, n_banned=self.banned.cols if use_ban else 0,
                 no_repeat_ngram=g, min_words=mw, eos_idx=EOS, T=T)
        f.update(over)
        return _hip.SearchConstraints(**f)

    def outputs(self, k):
        return guards.guarded(N, k, k, torch.float32, DEV), guards.guarded(N, k, k, torch.int32, DEV)

    def assert_inputs_untouched(self, what):
        for name, g in self.inputs.items():
            g.assert_untouched(what=f"{what} {name}")
            if name != "pos":
                assert torch.equal(g.raw, self.before[name]), f"{what}: {name} was written"


@functools.lru_cache(maxsize=2)
def device(V):
    return Device(V)


def run(dev, k, cons):
    from on_device_image_captioning_amd import _hip
    tv, ti = dev.outputs(k)
    rc = _hip.load().odic_topk_rows_constrained(dev.logp.data_ptr(), dev.ldl, ctypes.byref(cons), tv.data_ptr(), ti.data_ptr(),
                                                N, dev.V, k, None)
    torch.cuda.synchronize()
    return rc, tv, ti


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def fits(V, k, name):
    n_banned = inputs(V)[3].size if CONFIGS[name][0] else 0
    return n_banned + T + k <= V


# ------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("k", KS)
def test_every_constraint_equals_the_numpy_model_exactly_in_guarded_buffers(ops, V, k):
    dev = device(V)
    want_plain = None
    for name in CONFIGS:
        what = f"V={V} k={k} {name}"
        rc, tv, ti = run(dev, k, dev.constraints(name))
        if not fits(V, k, name):
            assert rc == EINVAL, what
            tv.assert_all_poison(what)
            ti.assert_all_poison(what)
            continue
        assert rc == 0, what
        wv, wi = model(V, k, name)
        gv, gi = tv.t.cpu().numpy(), ti.t.cpu().numpy()
        assert np.array_equal(gi, wi), f"{what}: indices\n{gi}\n{wi}"
        assert np.array_equal(bits(gv), bits(wv)), f"{what}: values"
        tv.assert_untouched(what=what + " top_val")
        ti.assert_untouched(what=what + " top_idx")
        dev.assert_inputs_untouched(what)
        # the finished row, and every row without an active constraint: odic_topk_rows bit for bit
        if want_plain is None:
            pv = torch.empty(N, k, dtype=torch.float32, device=DEV)
            pi = torch.empty(N, k, dtype=torch.int32, device=DEV)
            ops.topk_rows(dev.logp.t[:, :V], pv, pi, k)
            want_plain = (pv.cpu().numpy(), pi.cpu().numpy())
        rows = slice(0, N) if name in ("none", "ngram4_prefix_too_short", "ngram12_prefix_too_short", "min_words_reached") \
            else slice(4, 5)
        assert np.array_equal(gi[rows], want_plain[1][rows]) and np.array_equal(bits(gv[rows]), bits(want_plain[0][rows])), what


@pytest.mark.parametrize("V", (37, 513, 10241))
@pytest.mark.parametrize("k", (1, 9, 16))
def test_tied_rows_equal_the_numpy_model_exactly(ops, V, k):
    """An all-equal row (every round a V-way tie: indices ascending, the inadmissible ones skipped) and rows on a coarse
    grid (randn().round(): ties at every rank), with and without constraints.  V = 37 is shorter than the block, at
    V = 513 most register slots of a thread are empty, V = 10241 streams the row and looks the bitmap up per round."""
    _, tokens, _, banned = inputs(V)
    tokens = tokens[:3]                                               # row 2: the prefix whose bigrams repeat
    banned = np.concatenate([banned, np.array([0, 1, V - 1], np.int32)])      # the first two and the last word
    assert banned.size + T + k <= V
    g = torch.Generator().manual_seed(V)
    grid = lambda: torch.randn(V, generator=g).round().numpy().astype(F)      # noqa: E731
    logp = np.stack([np.full(V, -0.25, F), grid(), grid()])
    d = lambda a: torch.from_numpy(a).to(DEV)                         # noqa: E731
    tok, bn = d(tokens), d(banned)
    pos = torch.full((1,), POS, dtype=torch.int32, device=DEV)
    tv = torch.empty(3, k, dtype=torch.float32, device=DEV)
    ti = torch.empty(3, k, dtype=torch.int32, device=DEV)
    for what, kw in (("none", {}), ("all", dict(banned=bn, no_repeat_ngram=2, min_words=MINW))):
        ops.topk_rows_constrained(d(logp), ops.search_constraints(tok, pos, T, EOS, **kw), tv, ti, k)
        wv, wi = SC.topk_rows_constrained(logp, k, tokens, POS, None, banned.tolist() if kw else [],
                                          kw.get("no_repeat_ngram", 0), kw.get("min_words", 0), EOS)
        assert np.array_equal(ti.cpu().numpy(), wi), f"V={V} k={k} {what}: indices\n{ti.cpu().numpy()}\n{wi}"
        assert np.array_equal(bits(tv.cpu().numpy()), bits(wv)), f"V={V} k={k} {what}: values"
    assert wi[0, 0] == 3 and (np.diff(wi[0]) > 0).all()               # all equal: words 0, 1 banned, 2 = EOS too early


def test_the_inputs_reach_every_case_the_selection_has():
    """From the model alone: what the comparison above covers."""
    seen = dict(top1_banned=0, eos_removed_and_back=0, two_words_by_two_starts=0, prefix_too_short=0, ties_over_128=0,
                finished_row=0, ids_out_of_range=0, refused=0)
    for V in VS:
        logp, tokens, row_valid, banned = inputs(V)
        assert ((banned < 0) | (banned >= V)).any() and ((tokens[5] < 0) | (tokens[5] >= V)).any()
        seen["ids_out_of_range"] += 1
        for k in KS:
            pv, pi = plain(V, k)
            for name in CONFIGS:
                if not fits(V, k, name):
                    seen["refused"] += 1
            if fits(V, k, "banned"):
                _, wi = model(V, k, "banned")
                assert pi[0, 0] in banned and pi[0, 0] not in wi[0]
                seen["top1_banned"] += 1
                assert row_valid[4] == 0 and np.array_equal(wi[4], pi[4]) and pi[4, 0] in banned        # finished: kept
                seen["finished_row"] += 1
            if fits(V, k, "min_words_before"):
                assert EOS in pi[1]
                assert EOS not in model(V, k, "min_words_before")[1][1] and EOS in model(V, k, "min_words_reached")[1][1]
                seen["eos_removed_and_back"] += 1
            for g in (1, 2, 3):
                p = tokens[2].tolist()
                starts = [j for j in range(0, POS - g + 2) if p[j:j + g - 1] == p[POS - g + 2:POS + 1]]
                followers = {p[j + g - 1] for j in starts}
                assert {A, C_} <= followers and len(starts) >= 2
                if fits(V, k, f"ngram{g}"):
                    wi = model(V, k, f"ngram{g}")[1]
                    assert pi[2, 0] == A and A not in wi[2] and C_ not in wi[2]
                    seen["two_words_by_two_starts"] += 1
            for name in ("ngram4_prefix_too_short", "ngram12_prefix_too_short"):
                _, g, _, pos = CONFIGS[name]
                assert pos + 1 < g - 1
                if fits(V, k, name):
                    assert np.array_equal(model(V, k, name)[1], pi)
                    seen["prefix_too_short"] += 1
            if V >= 4097:
                assert int((logp[3] == pv[3, k - 1]).sum()) > 128
                seen["ties_over_128"] += 1
    assert all(seen.values()), seen


def test_invalid_arguments_are_refused_and_write_nothing(ops):
    V, k = 64, 3
    dev = device(V)
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    tv, ti = dev.outputs(k)

    def call(name="all", N_=N, V_=V, k_=k, ldl=None, logp=True, cons=True, tvp=True, tip=True, **over):
        c = dev.constraints(name, **over)
        return lib.odic_topk_rows_constrained(dev.logp.data_ptr() if logp else None, dev.ldl if ldl is None else ldl,
                                              ctypes.byref(c) if cons else None, tv.data_ptr() if tvp else None,
                                              ti.data_ptr() if tip else None, N_, V_, k_, None)

    nb = dev.banned.cols
    bad = [dict(V_=nb + T + k - 1), dict(k_=0), dict(k_=-1), dict(k_=17), dict(no_repeat_ngram=-1), dict(no_repeat_ngram=T + 1),
           dict(min_words=-1), dict(T=1), dict(T=129), dict(T=0), dict(n_banned=-1), dict(n_banned=1025, V_=4097, ldl=4104),
           dict(V_=262145, ldl=262145 + 7), dict(N_=0), dict(ldl=V - 1), dict(logp=False), dict(cons=False), dict(tvp=False),
           dict(tip=False), dict(tokens=None), dict(pos=None), dict(banned=None)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    tv.assert_all_poison("refused calls: top_val")
    ti.assert_all_poison("refused calls: top_idx")
    dev.assert_inputs_untouched("refused calls")
    assert call() == 0                                               # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="ODIC_EINVAL"):
        ops.topk_rows_constrained(dev.logp.t[:, :V], dev.constraints("all", min_words=-1), tv.t, ti.t, k)


def test_ops_wrappers_build_the_struct_the_kernel_reads(ops):
    V, k = 65, 9
    logp, tokens, row_valid, banned = inputs(V)
    d = lambda a: torch.from_numpy(a).to(DEV)                        # noqa: E731
    tok, rv, bn = d(tokens), d(row_valid), d(banned)
    pos = torch.full((1,), POS, dtype=torch.int32, device=DEV)
    cons = ops.search_constraints(tok, pos, T, EOS, row_valid=rv, banned=bn, no_repeat_ngram=2, min_words=MINW)
    tv = torch.empty(N, k, dtype=torch.float32, device=DEV)
    ti = torch.empty(N, k, dtype=torch.int32, device=DEV)
    ops.topk_rows_constrained(d(logp), cons, tv, ti, k)
    wv, wi = model(V, k, "all")
    assert np.array_equal(ti.cpu().numpy(), wi) and np.array_equal(bits(tv.cpu().numpy()), bits(wv))
    # without row_valid every row is a growing row
    cons = ops.search_constraints(tok, pos, T, EOS, banned=bn)
    ops.topk_rows_constrained(d(logp), cons, tv, ti, k)
    wv, wi = SC.topk_rows_constrained(logp, k, tokens, POS, None, banned.tolist())
    assert np.array_equal(ti.cpu().numpy(), wi) and np.array_equal(bits(tv.cpu().numpy()), bits(wv))
