"""odic_token_stats and odic_dec_embed_seq on hard rows and at the block's edges (`-m gpu`), against token_stats_model.py.

Every operand lives in a tests/guards.py buffer: outputs are `guarded` (all poison before the launch, bands and padding
checked afterwards), the logits are a `poisoned_input` with ldl = V + 5 (V odd: no row is 16-byte aligned; a read of a gap
column is a NaN in every output of the row), the embedding and position tables sit in poisoned allocations too.

Bounds: token_stats_model.bounds (derived there from the fp32 / fp64 formats and the depth of the kernel's sums), times
GPU_FACTOR = 1.0; `randn3` rows also keep the 2e-6·scale of test_scoring_gpu.test_token_stats.  The worst err/bound per
family is printed.  dec_embed_seq: 1 ulp of fp32 at the larger of |embed·scale| and |y| per element — an fmaf rounds
once (half an ulp of y), a multiply-then-add twice (half an ulp of the product, half an ulp of y)."""
import ctypes

import numpy as np
import pytest
import torch

import guards
import token_stats_model as TM

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
EINVAL, ENULL = -1, -2
PAD = 5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def _outs(R):
    """(logp_target, sum_logp, max_logp, argmax) as guarded compact [R] buffers."""
    return [guards.guarded(1, R, R, torch.float32, DEV) for _ in range(3)] + [guards.guarded(1, R, R, torch.int32, DEV)]


def _launch(ops, X, targets, status=0, with_target=True):
    """One odic_token_stats launch over the fp32 rows X [R, V]: (logp_target, sum_logp, max_logp, argmax, status) on the
    CPU, after checking that nothing outside the operands changed."""
    X = torch.from_numpy(np.ascontiguousarray(X))
    R, V = X.shape
    xg = guards.poisoned_input(X, R, V, V + PAD, device=DEV)
    before = xg.raw.clone()
    lt, sl, ml, am = _outs(R)
    st = torch.full((1,), status, dtype=torch.int32, device=DEV)
    if with_target:
        tg = torch.tensor([int(t) for t in targets], dtype=torch.int64, device=DEV)
        ops.token_stats(xg.t, V + PAD, tg, lt.t, sl.t, am.t, ml.t, st, R, V)
    else:
        ops.token_stats(xg.t, V + PAD, None, None, sl.t, am.t, ml.t, None, R, V)
    torch.cuda.synchronize()
    for g, nm in ((lt, "logp_target"), (sl, "sum_logp"), (ml, "max_logp"), (am, "argmax")):
        if nm == "logp_target" and not with_target:
            g.assert_all_poison("token_stats logp_target without a target")
        else:
            g.assert_untouched(what="token_stats " + nm)
    assert torch.equal(xg.raw, before), "token_stats wrote to its logits"
    return lt.t.view(-1).cpu(), sl.t.view(-1).cpu(), ml.t.view(-1).cpu(), am.t.view(-1).cpu(), int(st)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_row(name, x, tg, lt, sl, ml, am, worst):
    """One finite-maximum row against the float64 reference (tg None: logp_target is not looked at); returns the failures
    as strings."""
    rlt, rs, ram, rml = TM.reference(x, tg)
    b = TM.bounds(x, tg)
    r = (0.0 if tg is None else TM.ratio(lt, rlt, b["logp_target"]), TM.ratio(sl, rs, b["sum_logp"]),
         TM.ratio(ml, rml, b["max_logp"]))
    worst[name] = tuple(max(a, c) for a, c in zip(worst.get(name, (0.0, 0.0, 0.0)), r))
    bad = []
    if max(r) > TM.GPU_FACTOR:
        bad.append(f"{name} V={len(x)}: err/bound logp_target {r[0]:.3f} sum_logp {r[1]:.3f} max_logp {r[2]:.3f}")
    if am != ram or am != TM.block_argmax(x)[1]:
        bad.append(f"{name} V={len(x)}: argmax {am}, reference {ram}")
    if name == "randn3" and tg is not None:                         # test_token_stats's bound, per row
        lp = np.asarray(x, np.float64) - x.max() + rml
        scale = np.abs(lp).max()
        if abs(lt - rlt) > 2e-6 * scale or abs(ml - rml) > 2e-6 * scale or abs(sl - rs) > 2e-6 * abs(rs):
            bad.append(f"{name} V={len(x)}: outside 2e-6·scale")
    return bad


# ------------------------------------------------------------------------------------------ every (family, V)
@pytest.mark.parametrize("V", TM.V_EDGES)
def test_token_stats_every_family(ops, V):
    names, X = TM.stack(V)
    assert 1 <= len(names) <= 40
    tg = [TM.default_target(f, x) for f, x in zip(names, X)]
    lt, sl, ml, am, st = _launch(ops, X, tg)
    assert st == 0
    worst, bad = {}, []
    for r, f in enumerate(names):
        bad += _check_row(f, X[r], tg[r], float(lt[r]), float(sl[r]), float(ml[r]), int(am[r]), worst)
    for f in names:
        print(f"token-stats V={V} {f:16s} err/bound: logp_target {worst[f][0]:.3f} sum_logp {worst[f][1]:.3f} "
              f"max_logp {worst[f][2]:.3f}")
    assert not bad, bad
    # with and without `target`: the same bits in the three outputs that do not depend on it
    _, sl2, ml2, am2, _ = _launch(ops, X, None, with_target=False)
    assert torch.equal(_bits(sl2), _bits(sl)) and torch.equal(_bits(ml2), _bits(ml)) and torch.equal(am2, am)


# ----------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize("V", [5, 257])
def test_token_stats_targets_and_the_status_word(ops, V):
    X = np.stack([TM.row("randn3", V, seed=s) for s in range(8)])
    tg = TM.target_edges(V) + [1, V // 2]                       # flagged and unflagged rows in one launch
    flagged = [False, False, True, True, True, True, False, False]
    base = None
    for s_in, s_out in ((0, 1), (4, 5)):
        lt, sl, ml, am, st = _launch(ops, X, tg, status=s_in)
        want, want_st = TM.launch_model(X, tg, s_in)
        assert st == s_out == want_st                           # OR-ed in, never cleared
        worst, bad = {}, []
        for r in range(8):
            assert want[r][4] == flagged[r]
            if flagged[r]:
                assert _bits(lt[r:r + 1]).item() == 0, (r, float(lt[r]))          # exactly +0.0
                bad += _check_row("flagged", X[r], None, 0.0, float(sl[r]), float(ml[r]), int(am[r]), worst)
            else:
                bad += _check_row("unflagged", X[r], tg[r], float(lt[r]), float(sl[r]), float(ml[r]), int(am[r]), worst)
        assert not bad, bad
        if base is None:
            base = (lt, sl, ml, am)
        else:                                                   # the status word on entry changes no output
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(base, (lt, sl, ml, am)))
    for s_in in (0, 4):                                         # no flagged row: status as it was
        assert _launch(ops, X, [0, V - 1, 1, 2, 3, 4, V // 2, V - 2], status=s_in)[4] == s_in


# --------------------------------------------------------------------------------------------- non-finite rows
def _same(got: float, want: float) -> bool:
    return (np.isnan(got) and np.isnan(want)) or got == want


@pytest.mark.parametrize("V", [5, 64, 257, 1025])
def test_token_stats_nonfinite_rows_follow_the_table(ops, V):
    names = TM.nonfinite_at(V)
    assert len(names) >= 6
    rows, labels = [TM.row("randn3", V, seed=100)], ["finite"]
    for i, n in enumerate(names):                               # a finite neighbour on both sides of every hard row
        rows += [TM.nonfinite_row(n, V), TM.row("randn3", V, seed=101 + i)]
        labels += [n, "finite"]
    X = np.stack(rows)
    tg = [TM.default_target(n, x) if n == "masked_target" else V // 2 for n, x in zip(labels, X)]
    lt, sl, ml, am, st = _launch(ops, X, tg)
    assert st == 0
    want, _ = TM.launch_model(X, tg)
    fin = [r for r, n in enumerate(labels) if n == "finite"]
    worst, bad = {}, []
    for r, n in enumerate(labels):
        if n == "finite":
            bad += _check_row("finite neighbour", X[r], tg[r], float(lt[r]), float(sl[r]), float(ml[r]), int(am[r]), worst)
            continue
        c = TM.NONFINITE[n]
        got = dict(logp_target=float(lt[r]), sum_logp=float(sl[r]), max_logp=float(ml[r]))
        for o, v in got.items():
            if not TM.in_class(v, c[o]):
                bad.append(f"{n} V={V}: {o} = {v}, the table says {c[o]}")
        # NaN as NaN, ±inf exactly; the one finite entry of the table (max_logp of a masked row) within its bound
        if not (_same(got["logp_target"], float(want[r][0])) and _same(got["sum_logp"], float(want[r][1]))):
            bad.append(f"{n} V={V}: logp_target / sum_logp {got}, model {want[r][:2]}")
        if c["max_logp"] == "finite":
            if TM.ratio(got["max_logp"], TM.reference(X[r])[3], TM.bounds(X[r])["max_logp"]) > TM.GPU_FACTOR:
                bad.append(f"{n} V={V}: max_logp {got['max_logp']}")
        if int(am[r]) != TM.nonfinite_argmax(n, X[r]) or int(am[r]) != want[r][2]:
            bad.append(f"{n} V={V}: argmax {int(am[r])}, table {TM.nonfinite_argmax(n, X[r])}, model {want[r][2]}")
    assert not bad, bad
    # the finite neighbours are what they are without the hard rows in the launch
    lt2, sl2, ml2, am2, _ = _launch(ops, X[fin], [tg[r] for r in fin])
    for a, b in ((lt, lt2), (sl, sl2), (ml, ml2), (am, am2)):
        assert torch.equal(_bits(a[fin]), _bits(b))


# --------------------------------------------------------------------------------------------- R = 1, R = 70000
def test_token_stats_one_row_and_seventy_thousand(ops):
    worst = {}
    for V in (1, 257):
        x = TM.row("randn3", V, seed=7)
        lt, sl, ml, am, st = _launch(ops, x[None], [V - 1])
        assert st == 0
        assert not _check_row("R=1", x, V - 1, float(lt[0]), float(sl[0]), float(ml[0]), int(am[0]), worst)
    R, V = 70000, 5
    base = TM.row("randn3", V, seed=8)
    rot = np.stack([np.roll(base, s) for s in range(V)])        # row r is the base row rotated by r % V
    X = rot[np.arange(R) % V]
    tg = (np.arange(R) // V) % V
    lt, sl, ml, am, st = _launch(ops, X, tg)
    assert st == 0
    a0 = int(np.argmax(base))
    assert torch.equal(am.long(), torch.from_numpy((a0 + np.arange(R)) % V))
    bad = []
    for s in range(V):                                          # five distinct rows x five targets
        for t in range(V):
            sel = np.flatnonzero((np.arange(R) % V == s) & (tg == t))
            for o in (lt, sl, ml):
                assert len(torch.unique(_bits(o[sel]))) == 1    # the same row and target: the same bits, whichever block
            r = int(sel[0])
            bad += _check_row("R=70000", X[r], t, float(lt[r]), float(sl[r]), float(ml[r]), int(am[r]), worst)
    print("token-stats R=1 / R=70000 err/bound:", {k: tuple(round(v, 3) for v in w) for k, w in worst.items()})
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- refusals
def test_token_stats_refusals_write_nothing(ops):
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    R, V = 3, 7
    xg = guards.poisoned_input(torch.from_numpy(np.stack([TM.row("randn3", V, seed=s) for s in range(R)])), R, V, V + PAD,
                               device=DEV)
    lt, sl, ml, am = _outs(R)
    stg = guards.guarded(1, 1, 1, torch.int32, DEV)
    tg = torch.zeros(R, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    ok = dict(x=xg.t, ldl=V + PAD, tg=tg, lt=lt.t, sl=sl.t, am=am.t, ml=ml.t, st=stg.t, R=R, V=V)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.odic_token_stats(p(a["x"]), a["ldl"], p(a["tg"]), p(a["lt"]), p(a["sl"]), p(a["am"]), p(a["ml"]), p(a["st"]),
                                    a["R"], a["V"], None)
    for kw, code in ((dict(R=0), EINVAL), (dict(R=-1), EINVAL), (dict(V=0), EINVAL), (dict(ldl=V - 1), EINVAL),
                     (dict(x=None), ENULL), (dict(sl=None), ENULL), (dict(am=None), ENULL), (dict(ml=None), ENULL),
                     (dict(lt=None), ENULL), (dict(st=None), ENULL)):
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    for g, nm in ((lt, "logp_target"), (sl, "sum_logp"), (ml, "max_logp"), (am, "argmax"), (stg, "status")):
        g.assert_all_poison("refused odic_token_stats: " + nm)
    with pytest.raises(RuntimeError, match="ODIC_EINVAL"):
        ops.token_stats(xg.t, V - 1, tg, lt.t, sl.t, am.t, ml.t, stg.t, R, V)
    assert call() == 0                                          # and the arguments they were derived from run
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ odic_dec_embed_seq
VOCAB, POS_ROWS = 11, 6


def _embed_case(d, T):
    """Tokens that walk through the edge ids, dec_len through {0, 1, T, T + 5}; N·T >= 8."""
    N = 8 if T == 1 else 4
    g = np.random.Generator(np.random.Philox(key=[d, T]))
    emb = g.standard_normal((VOCAB, d)).astype(np.float32)
    pos = g.standard_normal((POS_ROWS, d)).astype(np.float32)
    ids = [0, VOCAB - 1, VOCAB, -1, TM.INT64_MIN, 2 ** 40]
    tok = np.array([ids[i] if i < len(ids) else int(g.integers(VOCAB)) for i in g.permutation(N * T)],
                   dtype=object).reshape(N, T)
    lens = np.array(([0, 1, T, T + 5] * 2)[:N], dtype=np.int32)
    return N, emb, pos, tok, lens


@pytest.mark.parametrize("T", [1, POS_ROWS])
@pytest.mark.parametrize("d", [1, 100, 256, 300, 1024])
def test_dec_embed_seq_edges(ops, d, T):
    N, emb, pos, tok, lens = _embed_case(d, T)
    scale = float(np.float32(np.sqrt(d)))
    want, prod, valid = TM.dec_embed_ref(tok, emb, pos, scale, lens)
    eg = guards.poisoned_input(torch.from_numpy(emb), VOCAB, d, d, device=DEV)         # a read outside the table: NaN
    pg = guards.poisoned_input(torch.from_numpy(pos), POS_ROWS, d, d, device=DEV)
    tk = guards.poisoned_input(torch.tensor(tok.astype(np.int64).reshape(1, -1)), 1, N * T, N * T, device=DEV)
    ln = torch.from_numpy(lens).to(DEV)
    outs = {}
    for with_valid in (True, False):
        yg = guards.guarded(N * T, d, d + 3, torch.float32, DEV)
        rv = guards.guarded(1, N * T, N * T, torch.int32, DEV)
        ops.dec_embed_seq(tk.t.view(N, T), eg.t, pg.t, yg.t, d + 3, N, T, d, scale, ln if with_valid else None,
                          rv.t if with_valid else None)
        torch.cuda.synchronize()
        yg.assert_untouched(what="dec_embed_seq y")
        if with_valid:
            rv.assert_untouched(what="dec_embed_seq row_valid")
            assert np.array_equal(rv.t.view(N, T).cpu().numpy(), valid)
        else:
            rv.assert_all_poison("dec_embed_seq row_valid = NULL")
        outs[with_valid] = yg.t[:, :d].cpu()
    assert torch.equal(_bits(outs[True]), _bits(outs[False]))
    got = outs[True].double().numpy().reshape(N, T, d)
    assert np.isfinite(got).all()
    tol = TM.ulp32(np.maximum(np.abs(prod), np.abs(want)))     # 1 ulp of fp32 (module docstring)
    err = np.abs(got - want) / tol
    print(f"dec_embed_seq d={d} T={T}: worst error {err.max():.3f} ulp")
    assert err.max() <= 1.0
    outside = np.array([[not (0 <= t < VOCAB) for t in r] for r in tok])
    assert outside.sum() == 4
    assert np.array_equal(got[outside], np.broadcast_to(pos[None, :T].astype(np.float64), got.shape)[outside])


def test_dec_embed_seq_refusals_write_nothing(ops):
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    d, T = 8, POS_ROWS
    N, emb, pos, tok, lens = _embed_case(d, T)
    e, ps = torch.from_numpy(emb).to(DEV), torch.from_numpy(pos).to(DEV)
    tk, ln = torch.tensor(tok.astype(np.int64)).to(DEV), torch.from_numpy(lens).to(DEV)
    yg = guards.guarded(N * T, d, d + 3, torch.float32, DEV)
    rv = guards.guarded(1, N * T, N * T, torch.int32, DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    ok = dict(ln=ln, rv=rv.t, ldy=d + 3, N=N, T=T, pos_rows=POS_ROWS)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.odic_dec_embed_seq(p(tk), p(e), p(ps), p(a["ln"]), p(a["rv"]), p(yg.t), a["ldy"], a["N"], a["T"], d, VOCAB,
                                      a["pos_rows"], 2.0, None)
    for kw, code in ((dict(pos_rows=T - 1), EINVAL), (dict(ldy=d - 1), EINVAL), (dict(ln=None), ENULL),
                     (dict(N=65536, T=32768, pos_rows=32768), EINVAL)):          # N·T = 2^31: only the counts are passed
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    yg.assert_all_poison("refused odic_dec_embed_seq: y")
    rv.assert_all_poison("refused odic_dec_embed_seq: row_valid")
    assert call() == 0
    torch.cuda.synchronize()
    yg.assert_untouched(what="dec_embed_seq y")
