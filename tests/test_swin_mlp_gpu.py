"""odic_swin_mlp: the MLP half of a width-192 Swin block (norm2 → fc1 → GELU → fc2 + residual) in ONE launch, against the
two launches it replaces — odic_gemm(a_ln = x, GELU, bf16 out), then odic_gemm(hidden, W2, residual = x, fp32 out).

The contract is BIT identity: every output element is the same accumulator chain over ascending 32-deep steps and both
epilogue expressions are written as in the kernels replaced, so every comparison below is torch.equal, not a tolerance."""
import ctypes as C

import pytest
import torch

from conftest import cached_state_dict
from guards import guarded, poisoned_input
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
BM, CW = 128, 192                        # rows per panel (four waves of 2 x 16), stage width


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def _lib():
    from on_device_image_captioning_amd import _hip
    return _hip, _hip.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _problem(ops, M, seed=5):
    """Seeded rows (normal x 3, one constant row, one row with a single 1e4 outlier) and an MLP with random gamma / beta
    folded into fc1 (CPU generator: the same values on every machine)."""
    gen = torch.Generator().manual_seed(seed + M)
    x = torch.randn(M, CW, generator=gen) * 3.0
    x[1] = 0.75
    x[M - 2, 17] = 1e4
    W1, b1 = torch.randn(4 * CW, CW, generator=gen) * 0.06, torch.randn(4 * CW, generator=gen) * 0.2
    W2, b2 = torch.randn(CW, 4 * CW, generator=gen) * 0.04, torch.randn(CW, generator=gen) * 0.2
    gamma, beta = 1.0 + 0.2 * torch.randn(CW, generator=gen), 0.1 * torch.randn(CW, generator=gen)
    W1f, b1f, _ = ops.fold_layernorm_bf16(W1.to(DEV), b1.to(DEV), gamma.to(DEV), beta.to(DEV))
    return x.to(DEV), W1f, b1f, W2.to(DEV).to(torch.bfloat16).contiguous(), b2.to(DEV), 0.5


def _two_launches(ops, x, W1f, b1f, W2b, b2, alpha2):
    h = ops.gemm(None, W1f, b1f, a_ln=x, act=ops.ACT_GELU, out_dtype=torch.bfloat16)
    return ops.gemm(h, W2b, b2, residual=x, alpha=alpha2, tile_cfg=0, out_dtype=torch.float32)


@pytest.mark.parametrize("panels", [1, 9])          # one panel; more than 8 (the block index passes the eight XCDs)
def test_swin_mlp_is_bit_identical_to_the_two_launches(ops, panels):
    x, W1f, b1f, W2b, b2, alpha2 = _problem(ops, panels * BM)
    ref = _two_launches(ops, x, W1f, b1f, W2b, b2, alpha2)
    assert bool(torch.isfinite(ref).all()) and float((ref - x).abs().max()) > 0.1       # (the MLP term is not lost in x)
    x0 = x.clone()
    got = ops.swin_mlp(x, W1f, b1f, W2b, b2, alpha2)
    assert torch.equal(x, x0), "out of place: x was written"
    xin = x.clone()
    ret = ops.swin_mlp(xin, W1f, b1f, W2b, b2, alpha2, out=xin)
    torch.cuda.synchronize()
    assert ret.data_ptr() == xin.data_ptr()
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert torch.equal(xin, ref), float((xin - ref).abs().max())


def test_swin_mlp_ldx_gap_columns_and_guard_rows(ops):
    """x with ldx = C + 64 (poison — NaN as fp32 — in the gap columns and around the rows), out a view with ldo = C + 64 into
    a poisoned allocation: the gap columns and the bands in front and behind are byte-identical afterwards, no NaN is read
    into the result, and the result is the compact call's bit for bit."""
    _hip, lib = _lib()
    M, ld = 3 * BM, CW + 64
    x, W1f, b1f, W2b, b2, alpha2 = _problem(ops, M)
    ref = ops.swin_mlp(x, W1f, b1f, W2b, b2, alpha2)
    gx = poisoned_input(x, M, CW, ld, device=DEV)
    gw1, gb1 = poisoned_input(W1f, 4 * CW, CW, CW), poisoned_input(b1f, 1, 4 * CW, 4 * CW)
    gw2, gb2 = poisoned_input(W2b, CW, 4 * CW, 4 * CW), poisoned_input(b2, 1, CW, CW)
    o = guarded(M, CW, ld, torch.float32, DEV)
    _hip.check(lib.odic_swin_mlp(gx.data_ptr(), ld, gw1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(), gb2.data_ptr(), alpha2,
                                 o.data_ptr(), ld, M, CW, 1e-5, _stream()), "odic_swin_mlp")
    torch.cuda.synchronize()
    o.assert_untouched(what="swin_mlp output")
    for gi in (gx, gw1, gb1, gw2, gb2):
        gi.assert_untouched(what="swin_mlp input")
    assert torch.equal(o.t[:, :CW], ref), "ldx / ldo changed the result"
    # in place inside the padded layout: the same rows, the gap columns still poison
    _hip.check(lib.odic_swin_mlp(gx.data_ptr(), ld, gw1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(), gb2.data_ptr(), alpha2,
                                 gx.data_ptr(), ld, M, CW, 1e-5, _stream()), "odic_swin_mlp")
    torch.cuda.synchronize()
    gx.assert_untouched(what="swin_mlp in place")
    assert torch.equal(gx.t[:, :CW], ref)


def test_swin_mlp_refusals_launch_nothing(ops):
    _hip, lib = _lib()
    M = BM
    x, W1f, b1f, W2b, b2, alpha2 = _problem(ops, M)
    big = torch.zeros(M + 16, 256 + 8, device=DEV)                       # an x large enough for every refused shape
    o = guarded(M + 16, 256, 256 + 8, torch.float32, DEV)

    def call(xp, ldx, w2p, outp, ldo, m, c):
        return lib.odic_swin_mlp(xp, ldx, W1f.data_ptr(), b1f.data_ptr(), w2p, b2.data_ptr(), alpha2, outp, ldo, m, c, 1e-5,
                                 _stream())
    assert call(big.data_ptr(), CW, W2b.data_ptr(), o.data_ptr(), CW, BM + 16, CW) == -1          # not whole panels
    assert call(big.data_ptr(), 256, W2b.data_ptr(), o.data_ptr(), 256, BM, 256) == -1            # width
    assert call(big.data_ptr(), CW + 2, W2b.data_ptr(), o.data_ptr(), CW, BM, CW) == -1           # ldx % 4
    assert call(big.data_ptr(), CW, W2b.data_ptr(), o.data_ptr() + 4, CW, BM, CW) == -1           # misaligned out
    assert call(big.data_ptr(), CW, None, o.data_ptr(), CW, BM, CW) == -2                         # NULL W2
    torch.cuda.synchronize()
    o.assert_all_poison(what="refused odic_swin_mlp calls")
    xb = torch.zeros(BM + 16, CW, device=DEV)
    out = torch.full_like(xb, 7.0)
    with pytest.raises(RuntimeError, match="odic_swin_mlp"):
        ops.swin_mlp(xb, W1f, b1f, W2b, b2, alpha2, out=out)
    with pytest.raises(RuntimeError):
        ops.swin_mlp(torch.zeros(BM, 256, device=DEV), W1f, b1f, W2b, b2, alpha2)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.fixture(scope="module")
def swin_l(ops):
    from on_device_image_captioning_amd.engine import SwinEngine
    eng = SwinEngine(cached_state_dict("FULL", "xavier"), W.FULL, torch.device(DEV), "bf16")
    assert eng.fuse_mlp and "fc1_lnr" in eng.stages[0][0][0]
    return eng


def test_engine_backbone_features_do_not_change_by_a_bit(ops, swin_l):
    """Swin-L, B = 2, seed 91 (test_fused_stage0_launches_leave_the_backbone_features_unchanged's set-up): fuse_mlp on
    against off; under ops.profile() the fused pass records one swin_mlp launch per stage-0 block in place of two
    gemm_bf16 launches."""
    eng = swin_l
    img = W.synth_images(2, W.FULL, seed=91).to(DEV)
    try:
        eng.fuse_mlp = False
        two = eng.forward(img).clone()
        with ops.profile() as recs:
            eng.forward(img)
            names_two = [r[0] for r in recs]
        eng.fuse_mlp = True
        fused = eng.forward(img).clone()
        with ops.profile() as recs:
            eng.forward(img)
            names_fused = [r[0] for r in recs]
    finally:
        eng.fuse_mlp = True
    assert torch.equal(fused, two), float((fused - two).abs().max())
    n_blocks = len(eng.stages[0][0])
    assert n_blocks == 2
    assert names_two.count("swin_mlp") == 0 and names_fused.count("swin_mlp") == n_blocks
    assert names_two.count("gemm_bf16") - names_fused.count("gemm_bf16") == 2 * n_blocks
    assert len(names_two) - len(names_fused) == n_blocks


def test_engine_forward_captures_at_a_batch_size_never_run_eagerly(ops, swin_l):
    """No tuner behind odic_swin_mlp: a hipGraph capture at a new batch size must not raise, and its replay equals the
    eager pass."""
    eng = swin_l
    img = W.synth_images(3, W.FULL, seed=92).to(DEV)                     # (B = 3: no test of this module runs it eagerly first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eng.forward(img)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = eng.forward(img)
    assert torch.equal(replayed, eager), float((replayed - eager).abs().max())
