"""The decoder's dynamic expansion on hard rows (`-m gpu`): odic_dynexp_step, odic_dynexp_seq and odic_dynexp_fill_caches
against the float64 reference of tests/dynexp_refs.py, entry by entry:  |got − want| <= rtol·|want| + atol·rowscale with the
family's pair (8 x the error of a float32 evaluation measured on the CPU; test_dynexp_refs_host.py).  The families: gauss,
one_sided (normalisers that are exactly 0 beyond t = 0), eps_regime (normalisers of 1e-11 .. 1e-7 against eps = 1e-9), peaked
(weights over more than three decades), cancel (qexp·key and cond·key of ±2^10 that cancel to O(1)) and the probe, whose
output channels ARE the coefficients ca / cb, wja / wjb, wea / web: a failure names (sequence, step, kind, index).

Shapes: N = 3, (T, d, E) = (20, 128, 4) and (40, 192, 16): t + 1 crosses 16 / 17 and 32 / 33, where the step kernel halves the
lanes per key position.  Outputs and caches live in guarded, poisoned buffers (tests/guards.py): every cache entry no step
wrote is NaN, and the entries of `anc` at positions >= t hold an out-of-range slot.  y_in is zero on valid rows (the
comparison then sees what the block adds, unrounded) and normal data on padded rows, which must come back bit-equal."""
import numpy as np
import pytest
import torch

import dynexp_refs as DX
import dynexp_step_model as M
import guards

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
F32 = torch.float32
N = DX.N_SEQ
PREFIX = {"T20": 17, "T40": 34}                  # P of the prefill tests: the two steps behind it are t + 1 = 18, 19 / 35, 36
STEP_CASES = [(f, s, p) for f in DX.FAMILIES for s in DX.SHAPES for p in DX.PLANS]
SEQ_CASES = [(f, s, i) for f in DX.FAMILIES for s in DX.SHAPES for i in (0, 1)]
FILL_CASES = [(f, s) for f in ("eps_regime", "one_sided", "peaked") for s in DX.SHAPES]
ids = lambda c: "-".join(str(v) for v in c)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def cache_widths(T, d, E):
    return dict(cond=d, key=d, va=d, vb=d, wfa=T * E, wfb=T * E, qk=E)


def guarded_caches(T, d, E):
    """One guarded buffer per cache, [T·N rows, width], all poison: NaN wherever no kernel writes."""
    return {k: guards.guarded(T * N, w, w, F32, DEV) for k, w in cache_widths(T, d, E).items()}


def finite_caches(T, d, E):
    return {k: torch.zeros(T * N, w, dtype=F32, device=DEV) for k, w in cache_widths(T, d, E).items()}


def tensors(c):
    return [c[k].t if isinstance(c[k], guards.Guarded) else c[k] for k in M.CACHES]


def run_steps(ops, dt, plan_kind, caches, steps=None, finite=False):
    """Steps `steps` (default: all T) of the search on the device; anc is rewritten from the plan before every step (finite:
    the entries at positions >= t hold the row's own slot instead of the sentinel).  Returns (y, y_in) [T, N, d] on the CPU; rows
    of steps that did not run are NaN."""
    T, d, E = dt.dims
    plan = DX.plan_of(dt.shape, plan_kind)
    lin = dt.lin.transpose(0, 1).contiguous().to(DEV)                                       # [T, N, 5d]
    y_in = DX.y_in_of(dt, plan.valid)
    y_in_d = y_in.to(DEV)
    anc_np = plan.anc.copy()
    if finite:
        anc_np = np.where(anc_np == M.SENTINEL, np.arange(N, dtype=np.int32)[None, :, None], anc_np).astype(np.int32)
    anc_all, valid_all = torch.from_numpy(anc_np).to(DEV), torch.from_numpy(plan.valid).to(DEV)
    qe, be = dt.qexp.to(DEV), dt.bexp.to(DEV)
    anc = torch.empty(N, T, dtype=torch.int32, device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    gy = guards.guarded(T * N, d, d, F32, DEV)
    y = gy.t.view(T, N, d)
    for t in (range(T) if steps is None else steps):
        pos.fill_(t)
        anc.copy_(anc_all[t])
        ops.dynexp_step(lin[t], 5 * d, qe, be, *tensors(caches), anc, valid_all[t], pos, y_in_d[t], d, y[t], d, N, T, d, E)
    torch.cuda.synchronize()
    gy.assert_untouched(what="y")
    for k in M.CACHES:
        if isinstance(caches[k], guards.Guarded):
            caches[k].assert_untouched(what=k)
    return y.cpu(), y_in


_RUNS = {}


def search_run(ops, case):
    """The NaN-cache, sentinel-anc run of a step case, once."""
    if case not in _RUNS:
        f, s, p = case
        dt = DX.data(f, s, p)
        _RUNS[case] = run_steps(ops, dt, p, guarded_caches(*dt.dims))
    return _RUNS[case]


def added(y, y_in, live):
    """What the block added on the live rows (float64; y_in is 0 there), 0 elsewhere — after checking that every other row is
    bit-equal to y_in."""
    live = torch.as_tensor(live).bool()
    dead = ~live
    same = (y.view(torch.int32) == y_in.view(torch.int32)).all(-1)
    assert bool(same[dead].all()), f"padded rows (step, sequence) {torch.nonzero(dead & ~same)[:4].tolist()} are not bit-equal to y_in"
    return torch.where(live[..., None], y.double(), torch.zeros((), dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------- step
@pytest.mark.parametrize("case", STEP_CASES, ids=ids)
def test_step_matches_the_reference_entry_by_entry(ops, case):
    f, s, p = case
    dt = DX.data(f, s, p)
    plan = DX.plan_of(s, p)
    y, y_in = search_run(ops, case)
    out = added(y, y_in, plan.valid)
    DX.assert_search(dt, p, out, DX.search_ref(dt, p), f"step {ids(case)}")


@pytest.mark.parametrize("family", DX.FAMILIES)
def test_step_reads_no_cache_entry_behind_t_and_no_anc_entry_from_t_on(ops, family):
    """include/odic_hip.h: cache entries at positions > t (and forward weights at i > j) and anc entries at positions >= t are
    not read.  NaN / an out-of-range slot there gives the bits of the run with zeros / the row's own slot there."""
    case = (family, "T40", "reorder")
    dt = DX.data(*case)
    y, _ = search_run(ops, case)
    y_fin, _ = run_steps(ops, dt, "reorder", finite_caches(*dt.dims), finite=True)
    same = (y.view(torch.int32) == y_fin.view(torch.int32)).all(-1)
    assert bool(same.all()), f"rows (step, sequence) {torch.nonzero(~same)[:4].tolist()} differ"


# --------------------------------------------------------------------------------------------------------- sequence
def run_seq(ops, dt, lens, poison_padded):
    T, d, E = dt.dims
    lin = dt.lin.clone()
    valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]                         # [N, T]
    if poison_padded:
        lin[~valid] = float("nan")
    y_in = DX.y_in_of(dt, valid)
    gy = guards.guarded(N * T, d, d, F32, DEV)
    ops.dynexp_seq(lin.view(N * T, 5 * d).to(DEV), 5 * d, dt.qexp.to(DEV), dt.bexp.to(DEV),
                   torch.tensor(lens, dtype=torch.int32, device=DEV), y_in.view(N * T, d).to(DEV), d, gy.t, d, N, T, d, E)
    torch.cuda.synchronize()
    gy.assert_untouched(what="y")
    return gy.t.view(N, T, d).cpu(), y_in, valid


@pytest.mark.parametrize("case", SEQ_CASES, ids=ids)
def test_sequence_pass_matches_the_reference_entry_by_entry(ops, case):
    """dec_len (T, 1, 0) and (T, T//2, 7).  The header: lin rows at positions >= dec_len[n] are not read — NaN there gives the
    same bits; padded rows are bit-equal to y_in."""
    f, s, i = case
    dt = DX.data(f, s)
    lens = DX.seq_lens(dt.dims[0])[i]
    y, y_in, valid = run_seq(ops, dt, lens, poison_padded=True)
    out = added(y.transpose(0, 1), y_in.transpose(0, 1), valid.T)
    DX.assert_search(dt, "identity", out, DX.search_ref(dt, "identity"), f"seq {ids(case)} lens {lens}", live=valid.T)
    y2, _, _ = run_seq(ops, dt, lens, poison_padded=False)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), "NaN in lin rows behind dec_len changed the output"


# ---------------------------------------------------------------------------------------------------------- prefill
def run_fill(ops, dt, P, caches, lin=None):
    T, d, E = dt.dims
    lin = dt.lin[:, :P].reshape(N * P, 5 * d).contiguous().to(DEV) if lin is None else lin
    ops.dynexp_fill_caches(lin, 5 * d, dt.qexp.to(DEV), dict(zip(M.CACHES, tensors(caches))), N, P, 1, N, T, d, E)
    torch.cuda.synchronize()


def fill_then_steps(ops, dt, P, steps):
    """Fill of a P-position prefix into guarded caches, then ordinary steps behind it (identity ancestry)."""
    caches = guarded_caches(*dt.dims)
    run_fill(ops, dt, P, caches)
    y, y_in = run_steps(ops, dt, "identity", caches, steps=steps)
    return caches, y, y_in


@pytest.mark.parametrize("case", FILL_CASES, ids=ids)
def test_prefill_caches_and_the_steps_behind_them(ops, case):
    f, s = case
    dt = DX.data(f, s)
    T, d, E = dt.dims
    P = PREFIX[s]
    ref = DX.search_ref(dt, "identity")
    caches, y, y_in = fill_then_steps(ops, dt, P, (P, P + 1))
    for k in ("wfa", "wfb"):
        got = caches[k].t.cpu().view(T, N, T, E)[:P]                                        # [t, n, i, e]
        want = ref.fw[k][:P].permute(0, 1, 3, 2)                                            # [t, n, e, i] -> [t, n, i, e]
        written = (torch.arange(T)[None, :] <= torch.arange(P)[:, None])[:, None, :, None].expand(P, N, T, E)
        assert bool(torch.isnan(got[~written]).all()), f"{k}: an entry at i > t was written"
        got = torch.where(written, got, torch.zeros(())).reshape(P, N, T * E)
        zero = (want.reshape(P, N, T * E) == 0) & (got != 0)
        assert not bool(zero.any()), f"{k}: (t, sequence, i·E + e) {torch.nonzero(zero)[0].tolist()} is not 0 where the reference weight is"
        DX.assert_entries(got, want.reshape(P, N, T * E), f, f"fill {ids(case)} {k}",
                          lambda ix: f"sequence {ix[1]}, position {ix[0]}, {k}[i = {ix[2] // E}][e = {ix[2] % E}]")
    DX.assert_entries(caches["qk"].t.cpu().view(T, N, E)[:P], ref.fw["qk"][:P], f, f"fill {ids(case)} qk",
                      lambda ix: f"sequence {ix[1]}, position {ix[0]}, qk[{ix[2]}]")
    live = torch.zeros(T, N, dtype=torch.bool)
    live[P:P + 2] = True
    y[:P], y[P + 2:] = y_in[:P], y_in[P + 2:]                                               # (steps that did not run)
    DX.assert_search(dt, "identity", added(y, y_in, live), ref, f"fill {ids(case)} + steps {P}, {P + 1}", live=live)


@pytest.mark.parametrize("shape", list(DX.SHAPES))
def test_fill_reads_no_row_behind_the_prefix(ops, shape):
    """The header: lin holds n_seq·P rows and nothing behind them is read.  With NaN behind the last row (a guarded input) the
    caches hold the bits of the run on a plain tensor."""
    dt = DX.data("eps_regime", shape)
    T, d, E = dt.dims
    P = PREFIX[shape]
    a, b = guarded_caches(T, d, E), guarded_caches(T, d, E)
    run_fill(ops, dt, P, a)
    g = guards.poisoned_input(dt.lin[:, :P].reshape(N * P, 5 * d).contiguous().to(DEV), N * P, 5 * d, 5 * d)
    run_fill(ops, dt, P, b, lin=g.t)
    for k in M.CACHES:
        a[k].assert_untouched(what=k)
        assert torch.equal(a[k].t.view(torch.int32), b[k].t.view(torch.int32)), k


# ------------------------------------------------------------------------------------------------ three ways, one answer
@pytest.mark.parametrize("case", [(f, s) for f in DX.FAMILIES for s in DX.SHAPES], ids=ids)
def test_three_ways_one_answer(ops, case):
    """The step replay, the whole-sequence pass and fill + steps each meet the bound on the rows they share (positions P ..
    T − 1 of the identity plan); their largest pairwise difference is printed, as a fraction of the rowscale."""
    f, s = case
    dt = DX.data(f, s)
    T, d, E = dt.dims
    P = PREFIX[s]
    ref = DX.search_ref(dt, "identity")
    live = torch.zeros(T, N, dtype=torch.bool)
    live[P:] = True
    ys, yi = search_run(ops, (f, s, "identity"))
    step = torch.where(live[..., None], ys.double(), torch.zeros((), dtype=torch.float64))
    yq, yqi, valid = run_seq(ops, dt, (T,) * N, poison_padded=False)
    seq = torch.where(live[..., None], yq.transpose(0, 1).double(), torch.zeros((), dtype=torch.float64))
    _, yf, yfi = fill_then_steps(ops, dt, P, range(P, T))
    yf[:P] = yfi[:P]
    fill = added(yf, yfi, live)
    outs = dict(step=step, seq=seq, fill=fill)
    for k, v in outs.items():
        DX.assert_search(dt, "identity", v, ref, f"{k} {ids(case)}", live=live)
    rs = ref.out.abs().amax(-1, keepdim=True).clamp_min(1e-300)
    for a, b in (("step", "seq"), ("step", "fill"), ("seq", "fill")):
        print(f"{ids(case)}: {a} vs {b}: largest difference {float(((outs[a] - outs[b]).abs() / rs)[live].max()):.3e} of the rowscale")
