"""Two decoder kernels on hard rows (`-m gpu`): the fp32 skinny GEMM with the LayerNorm folded in (odic_gemm with ln_colsum) on
constant, zero, offset, outlier and near-eps rows at every decomposition, and odic_cross_attn_step on key ranges that reach
the second 12-sweep trip, every chunk remainder, enc_len 0 / 1 and one-hot score rows.

Cases, inputs, float64 references and bounds come from decoder_refs.py; test_decoder_refs_host.py checks them without a GPU.
Every figure is printed before it is asserted.
"""
import pytest
import torch

import decoder_refs as DR
from decoder_refs import F64

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()          # fail loudly if the extension is missing
    return o


def _ids(cases):
    return [c.name for c in cases]


# ---------------------------------------------------------------------------------------------- folded-LayerNorm GEMM
_FOLD = {}


def fold_data(ops, case):
    """Per case, once: the inputs on the device, the folded weights, the float64 reference and the unfused pair's output."""
    if case.name not in _FOLD:
        buf, W, b, g, be, res = DR.fold_inputs(case)
        want = DR.fold_ref(case, buf, W, b, g, be, res)
        dW, db, dg, dbe = W.to(DEV), b.to(DEV), g.to(DEV), be.to(DEV)
        dres = res.to(DEV) if res is not None else None
        x = DR.fold_rows(buf, case.K).contiguous().to(DEV)
        unfused = ops.gemm(ops.layernorm(x, dg, dbe, eps=DR.FOLD_EPS), dW, db, dres, act=case.act).cpu()
        pre = DR.fold_bias_prime(W, b, be)                       # what a constant row gives before the activation
        pre = torch.relu(pre) if case.act == DR.ACT_RELU else pre
        _FOLD[case.name] = dict(buf=buf.to(DEV), folded=ops.fold_layernorm(dW, db, dg, dbe), res=dres, want=want,
                                scale=float(want.abs().max()), unfused=unfused, pre=pre, res_cpu=res)
    return _FOLD[case.name]


def fold_launch(ops, case, D, tile_cfg):
    """The engine's call: A = columns K.. of the wider (NaN-filled) buffer, lda = 3K."""
    Wf, bf, cs = D["folded"]
    M, N, K = case.M, case.N, case.K
    got = ops.gemm(D["buf"][:, K:], Wf, bf, D["res"], M=M, N=N, K=K, lda=3 * K, ldw=K, ldc=N, act=case.act,
                   ln_fold=(cs, DR.FOLD_EPS), tile_cfg=tile_cfg)
    return got.reshape(M, N).cpu()


def row_report(got, want, scale, case, what):
    """Worst error / scale of the ordinary rows and of every hard row against `want`, each with its bound; prints them all and
    returns the ones over their bound."""
    rows = DR.fold_hard_rows(case.M)
    o = torch.ones(case.M, dtype=torch.bool)
    o[sorted(rows.values())] = False
    figures = [("ordinary", DR.max_err(got[o], want[o])[0] / scale, DR.FOLD_BOUND)]
    figures += [(k, DR.max_err(got[rows[k]], want[rows[k]])[0] / scale, DR.fold_row_bound(case, k)) for k in DR.HARD_KINDS]
    print(f"{what}: " + ", ".join(f"{k} {e:.2e}" for k, e, _ in figures) + f" (of scale {scale:.3g})")
    return [(k, f"{e:.3e}", bd) for k, e, bd in figures if not e <= bd]


@pytest.mark.parametrize("tile_cfg", DR.FOLD_TILE_CFGS)
@pytest.mark.parametrize("case", DR.FOLD_CASES, ids=_ids(DR.FOLD_CASES))
def test_folded_layernorm_gemm_hard_rows(ops, case, tile_cfg):
    """Against float64: ordinary rows within 3e-5 of the case's scale, every hard row within max(3e-5, 4 x the float32 CPU
    error recorded for it); the constant and the zero row give bias' (no NaN from rstd = 1/sqrt(eps))."""
    D = fold_data(ops, case)
    got = fold_launch(ops, case, D, tile_cfg)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    over = row_report(got, D["want"], D["scale"], case, f"folded LN gemm {case.name} tile_cfg {tile_cfg}")
    rows = DR.fold_hard_rows(case.M)
    for kind in ("const", "zero"):
        pre = D["pre"] + D["res_cpu"][rows[kind]].double() if D["res_cpu"] is not None else D["pre"]
        DR.assert_within(got[rows[kind]], pre, DR.fold_row_bound(case, kind), f"  {kind} row = bias'", scale=D["scale"])
    assert not over, over


@pytest.mark.parametrize("tile_cfg", DR.FOLD_TILE_CFGS)
@pytest.mark.parametrize("case", DR.FOLD_CASES, ids=_ids(DR.FOLD_CASES))
def test_folded_layernorm_gemm_agrees_with_the_unfused_pair(ops, case, tile_cfg):
    """ops.gemm(ops.layernorm(x)) on the same inputs: itself within every row's bound of float64, and the folded launch within
    the sum of the two bounds of it — what a search sees when one batch size takes the folded form and another the pair."""
    D = fold_data(ops, case)
    over = row_report(D["unfused"], D["want"], D["scale"], case, f"unfused pair {case.name}")
    assert not over, over
    got = fold_launch(ops, case, D, tile_cfg)
    rows = DR.fold_hard_rows(case.M)
    diff = (got.double() - D["unfused"].double()).abs().amax(1) / D["scale"]                    # per row
    bound = torch.full((case.M,), 2.0 * DR.FOLD_BOUND, dtype=F64)
    for kind, r in rows.items():
        bound[r] = 2.0 * DR.fold_row_bound(case, kind)
    o = torch.ones(case.M, dtype=torch.bool)
    o[sorted(rows.values())] = False
    print(f"folded vs unfused {case.name} tile_cfg {tile_cfg}: ordinary {float(diff[o].max()):.2e}, " +
          ", ".join(f"{k} {float(diff[r]):.2e}" for k, r in rows.items()))
    bad = torch.nonzero(~(diff <= bound)).flatten().tolist()
    assert not bad, [(r, float(diff[r]), float(bound[r])) for r in bad]


@pytest.mark.parametrize("tile_cfg", (-1, 0))
def test_folded_layernorm_gemm_alpha(ops, tile_cfg):
    """alpha != 1 with the fold: the header's formula rstd·(alpha·A·W'ᵀ − mean·ln_colsum) + bias', the one path that reads the
    values of ln_colsum.  Ordinary rows and the zero row within 3e-5 of scale.  (The formula itself subtracts mean·colsum from
    a product that no longer contains it, so the offset, constant and outlier rows are large numbers here, not LayerNorm rows:
    they are compared at their own scale, row by row, with the same bound.)"""
    case = DR.FOLD_CASES[1]
    D = fold_data(ops, case)
    Wf, bf, cs = D["folded"]
    M, N, K = case.M, case.N, case.K
    got = ops.gemm(D["buf"][:, K:], Wf, bf, M=M, N=N, K=K, lda=3 * K, ldw=K, ldc=N, alpha=DR.FOLD_ALPHA,
                   ln_fold=(cs, DR.FOLD_EPS), tile_cfg=tile_cfg).reshape(M, N).cpu()
    want = DR.fold_alpha_ref(case, *DR.fold_inputs(case))
    rows = DR.fold_hard_rows(M)
    o = torch.ones(M, dtype=torch.bool)
    o[sorted(rows.values())] = False
    DR.assert_within(got[o], want[o], DR.FOLD_BOUND, f"folded LN gemm alpha {DR.FOLD_ALPHA} tile_cfg {tile_cfg}: ordinary rows")
    for kind, r in rows.items():
        DR.assert_within(got[r], want[r], DR.FOLD_BOUND, f"  {kind} row, at its own scale")


# ---------------------------------------------------------------------------------------------- cross-attention step
_XATTN = {}


def xattn_data(case):
    if case.name not in _XATTN:
        ins = DR.xattn_inputs(case)
        want = DR.xattn_ref(case, *ins)
        _XATTN[case.name] = dict(ins=ins, dev=[t.to(DEV) for t in ins], want=want, scale=float(want.abs().max()))
    return _XATTN[case.name]


def xattn_launch(ops, case, D):
    q, kv, lens, valid = D["dev"]
    out = torch.full((case.N, case.d), float("nan"), device=DEV)
    ops.cross_attn_step(q, case.d, kv, 3 * case.d, case.d, 2 * case.d, lens, valid, out, case.d, case.N, DR.XATTN_N_IMG,
                        case.S, case.d, case.heads)
    return out.cpu()


@pytest.mark.parametrize("case", DR.XATTN_CASES, ids=_ids(DR.XATTN_CASES))
def test_cross_attn_step_hard_rows(ops, case):
    """Against the float64 formula of test_cross_attn_step within max(2e-5, 4 x the recorded float32 CPU error) of the case's
    scale; a planted (row, head) returns its key's value row, a masked row the plain average of all S value rows."""
    D = xattn_data(case)
    got = xattn_launch(ops, case, D)
    bound, scale = DR.xattn_bound(case), D["scale"]
    DR.assert_within(got, D["want"], bound, f"cross_attn_step {case.name}")
    q, kv, lens, valid = D["ins"]
    d, dk = case.d, case.dk
    for img, beam, h, key in case.plants:
        if key < case.lens[img]:
            DR.assert_within(got[img * case.beams + beam, h * dk:(h + 1) * dk], kv[img, key, 2 * d + h * dk:2 * d + (h + 1) * dk],
                             bound, f"  image {img} beam {beam} head {h}: value row of key {key}", scale=scale)
    masked = [n for n in range(case.N) if not valid[n] or case.lens[n // case.beams] == 0]
    assert len(masked) >= 2
    for n in masked:
        DR.assert_within(got[n], kv[n // case.beams, :, 2 * d:].double().mean(0), bound, f"  row {n}: average of all value rows",
                         scale=scale)


@pytest.mark.parametrize("name", DR.XATTN_PROBS_CROSS_CHECK)
def test_cross_attn_step_is_cross_attn_probs_times_v(ops, name):
    """odic_cross_attn_probs (per head) times V in float64 against odic_cross_attn_step: two separate implementations of the same
    softmax, within twice the bound."""
    case = next(c for c in DR.XATTN_CASES if c.name == name)
    D = xattn_data(case)
    got = xattn_launch(ops, case, D)
    q, kv, lens, valid = D["dev"]
    width = case.heads * case.S
    p = torch.full((case.N, width), float("nan"), device=DEV)
    ops.cross_attn_probs(q, case.d, kv, 3 * case.d, case.d, lens, valid, p, width, case.N, DR.XATTN_N_IMG, case.S, case.d,
                         case.heads, per_head=True)
    p = p.cpu().double().view(DR.XATTN_N_IMG, case.beams, case.heads, case.S)
    V = D["ins"][1][:, :, 2 * case.d:].double().view(DR.XATTN_N_IMG, case.S, case.heads, case.dk)
    pv = torch.einsum("ibhs,ishc->ibhc", p, V).reshape(case.N, case.d)
    DR.assert_within(got, pv, 2.0 * DR.xattn_bound(case), f"cross_attn_step vs cross_attn_probs·V {name}", scale=D["scale"])


def test_cross_attn_step_refuses_more_than_2048_keys(ops):
    """S = 2049 is refused before any launch: the output keeps its sentinel."""
    S, d, heads, beams = DR.XATTN_REFUSED_S, 32, 2, 2
    N = DR.XATTN_N_IMG * beams
    q, kv = DR._randn(N, d, seed=1).to(DEV), DR._randn(DR.XATTN_N_IMG, S, 3 * d, seed=2).to(DEV)
    lens = torch.full((DR.XATTN_N_IMG,), S, dtype=torch.int32, device=DEV)
    valid = torch.ones(N, dtype=torch.int32, device=DEV)
    out = torch.full((N, d), 7.0, device=DEV)
    with pytest.raises(RuntimeError):
        ops.cross_attn_step(q, d, kv, 3 * d, d, 2 * d, lens, valid, out, d, N, DR.XATTN_N_IMG, S, d, heads)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((N, d), 7.0))
    ops.cross_attn_step(q, d, kv[:, :S - 1].contiguous(), 3 * d, d, 2 * d, lens - 1, valid, out, d, N, DR.XATTN_N_IMG, S - 1, d,
                        heads)                                     # S = 2048 with the same operands is taken
    torch.cuda.synchronize()
    assert bool((out.cpu() != 7.0).all())
