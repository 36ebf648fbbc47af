"""Every query-key pair of the window-attention kernels against the fp64 reference (tests/window_probe.py).

  * ops.window_attention — the fp32 parity kernel, the bf16 kernel with the table, the packed-bias kernel in bf16 and fp16 and
    the split-fp16 kernel — on the four probe families, at 12 x 12 windows with shifts 0, 1, 5, 6, 7, 11 (odd shifts put
    a region boundary inside a four-key accumulator quad), one window, a 2 x 2 and a 3 x 3 window grid (all nine seam
    classes next to an interior window; 27 windows, which the packed kernels' block grid rounds up to 32);
  * the fp32 kernel at windows of 1, 2, 4, 7 and 11;
  * the two fused kernels, bit for bit the two launches they replace and inside their fp64 bound at shifts 1, 5, 7, 11,
    and the tiled one probed directly: one-hot rows and a qkv weight whose columns are the probe values.

The bounds are window_probe.BOUNDS — two roundings of the output format, or the exp argument's fp32 rounding — and hold
for every pair; a failure names (image, window, head, query, key).
"""
import ctypes as C

import pytest
import torch

import window_probe as wp
from test_hip_ops import assert_close
from test_swin_qkv_attention_tiled_gpu import _case, _two_launches

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
WS = 12

# (B, res, shift) at ws = 12
GEOMETRIES = [(1, 12, 0), (1, 12, 1), (1, 12, 11), (2, 24, 5), (1, 24, 6), (3, 36, 7)]
# (res, ws, shift), fp32 kernel only
SMALL_WINDOWS = [(14, 7, 3), (21, 7, 0), (8, 4, 1), (6, 2, 1), (3, 1, 0), (22, 11, 10)]
# path → (storage dtype, packed bias, output format of window_probe.BOUNDS)
PATHS = {
    "fp32": (torch.float32, False, "fp32"),
    "bf16-table": (torch.bfloat16, False, "bf16"),
    "bf16-packed": (torch.bfloat16, True, "bf16"),
    "fp16-packed": (torch.float16, True, "fp16"),
    "h2-packed": (None, True, "h2"),
}
FUSED_SHIFTS = [1, 5, 7, 11]
FUSED_SHAPES = sorted({(B, res) for B, res, _ in GEOMETRIES})


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def _attend(ops, geo, fam, path):
    dt, packed, _ = PATHS[path]
    table = fam.table.to(DEV)
    dense = ops.shifted_bias_prescaled(table, geo.ws, wp.SCALE) if packed else None

    def attend(qkv):
        x = qkv.to(DEV)
        x = ops.h2_from_f32(x) if dt is None else x.to(dt)
        out = ops.window_attention(x, table, geo.B, geo.res, geo.C, geo.heads, geo.ws, geo.shift, scale=wp.SCALE,
                                   bias_shifted_prescaled=dense)
        assert out.shape == (geo.B * geo.L, geo.C) and out.dtype == x.dtype
        return ops.h2_to_f32(out) if dt is None else out.float()
    return attend


def _probe_and_check(ops, geo, name, path):
    fam = wp.family(name, geo)
    P = wp.probe(geo, fam, _attend(ops, geo, fam, path))
    want = wp.p_want(name, geo)
    fmt = PATHS[path][2]
    what = f"{path} {name} B{geo.B} res{geo.res} ws{geo.ws} shift{geo.shift}"
    wp.assert_pairs(P, want, fmt, what)
    if name == "mask":
        wp.assert_mask_is_additive(P, want, geo, fmt, what)


@pytest.mark.parametrize("name", wp.FAMILIES)
@pytest.mark.parametrize("B,res,shift", GEOMETRIES)
@pytest.mark.parametrize("path", list(PATHS))
def test_every_pair(ops, path, B, res, shift, name):
    _probe_and_check(ops, wp.Geometry(B, res, WS, shift), name, path)


@pytest.mark.parametrize("name", wp.FAMILIES)
@pytest.mark.parametrize("res,ws,shift", SMALL_WINDOWS)
def test_every_pair_fp32_small_windows(ops, res, ws, shift, name):
    _probe_and_check(ops, wp.Geometry(2, res, ws, shift), name, "fp32")


# ------------------------------------------------------------------------------------------------- the fused kernels
@pytest.mark.parametrize("shift", FUSED_SHIFTS)
@pytest.mark.parametrize("B,res", FUSED_SHAPES)
def test_fused_192_equals_two_launches_at_odd_shifts(ops, B, res, shift):
    """test_hip_ops.py::test_swin_qkv_attention_fused's recipe at the shifts and window grids it does not run."""
    geo = wp.Geometry(B, res, WS, shift)
    C_, heads = geo.C, geo.heads
    g = torch.Generator().manual_seed(11 + shift + res)
    x = torch.randn(B * geo.L, C_, generator=g) * 1.5 + torch.randn(B * geo.L, 1, generator=g) * 3.0
    Wq = torch.randn(3 * C_, C_, generator=g) * 0.06
    bq = torch.randn(3 * C_, generator=g) * 0.2
    gamma, beta = 1.0 + 0.2 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g) * 0.3
    Wf, bf, _ = ops.fold_layernorm_bf16(Wq.to(DEV), bq.to(DEV), gamma.to(DEV), beta.to(DEV))
    dense = ops.shifted_bias_prescaled(table.to(DEV), WS, 32 ** -0.5)
    xd = x.to(DEV)
    got = ops.swin_qkv_attention(xd, Wf, bf, dense, B, res, C_, heads, WS, shift)
    # the LayerNorm-while-reading product takes whole 256-row panels: pad with rows of their own, a row's chain is its own
    pad = -xd.shape[0] % 256
    xp = torch.cat([xd, torch.randn(pad, C_, generator=g).to(DEV)]) if pad else xd
    qkv = ops.gemm(None, Wf, bf, a_ln=xp, out_dtype=torch.bfloat16)[:B * geo.L]
    two = ops.window_attention(qkv, table.to(DEV), B, res, C_, heads, WS, shift, bias_shifted_prescaled=dense)
    assert got.dtype == torch.bfloat16 and got.shape == two.shape
    assert torch.equal(got, two), float((got.float() - two.float()).abs().max())
    xn = torch.nn.functional.layer_norm(x.double(), (C_,), gamma.double(), beta.double(), 1e-5)
    want = wp.attention_fp64(geo, xn @ Wq.double().T + bq.double(), table, 32 ** -0.5)
    assert_close(got, want, 2.5e-2, f"fused qkv+attention B{B} res{res} shift {shift} vs fp64")


@pytest.mark.parametrize("shift", FUSED_SHIFTS)
@pytest.mark.parametrize("B,res", FUSED_SHAPES)
def test_fused_tiled_equals_two_launches_at_odd_shifts(ops, B, res, shift):
    """test_swin_qkv_attention_tiled_gpu.py::test_bit_equal_to_gemm_cfg41_then_window_attention's recipe, width 384."""
    geo = wp.Geometry(B, res, WS, shift, heads=12)
    C_, heads = geo.C, geo.heads
    xn, Wq, bq, table = _case(ops, B, res, C_, heads, 100 + C_ + shift + res, "random")
    dxn, dWq, dbq, dtable = (t.to(DEV) for t in (xn, Wq, bq, table))
    dense = ops.shifted_bias_prescaled(dtable, WS, 32 ** -0.5)
    assert ops.swin_qkv_attention_tiled_supported(B * geo.L, C_, heads, WS, res)
    got = ops.swin_qkv_attention_tiled(dxn, dWq, dbq, dense, B, res, C_, heads, WS, shift)
    two = _two_launches(ops, dxn, dWq, dbq, dtable, dense, B, res, C_, heads, shift)
    assert got.dtype == torch.bfloat16 and got.shape == two.shape
    assert torch.equal(got, two), float((got.float() - two.float()).abs().max())
    want = wp.attention_fp64(geo, xn.double() @ Wq.double().T + bq.double(), table, 32 ** -0.5)
    assert_close(got, want, 2.5e-2, f"tiled qkv+attention B{B} res{res} shift {shift} vs fp64")


@pytest.mark.parametrize("name", ["bias", "score"])
@pytest.mark.parametrize("B,res,shift", GEOMETRIES)
def test_every_pair_through_the_tiled_kernel(ops, B, res, shift, name):
    """xn is the one-hot of a token's window slot, row (part, head, d) of w_qkv holds the probe value of each slot in its
    first 144 columns and b_qkv = 0: the kernel's own qkv product yields q, k and the one-hot v exactly."""
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    geo = wp.Geometry(B, res, WS, shift, heads=12)
    C_, heads, N = geo.C, geo.heads, geo.N
    fam = wp.family(name, geo, False)
    table = fam.table.to(DEV)
    dense = ops.shifted_bias_prescaled(table, WS, wp.SCALE)
    xn = torch.zeros(B, geo.L, C_)
    xn[:, geo.tok().reshape(-1), torch.arange(N).repeat(geo.nW)] = 1.0
    dxn = xn.reshape(B * geo.L, C_).to(DEV, torch.bfloat16)
    bq = torch.zeros(3 * C_, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for r in range(geo.nchunk):
        Wq = torch.zeros(3, heads, wp.HD, C_)
        for part, vals in enumerate((fam.q[0, 0], fam.k[0, 0], wp.one_hot_v(geo, r))):       # (heads, N, 32) each
            Wq[part, :, :, :N] = vals.transpose(1, 2)
        dWq = Wq.reshape(3 * C_, C_).to(DEV, torch.bfloat16)
        out = torch.empty(B * geo.L, C_, dtype=torch.bfloat16, device=DEV)
        _hip.check(lib.odic_swin_qkv_attention_tiled(dxn.data_ptr(), dWq.data_ptr(), bq.data_ptr(), dense.data_ptr(),
                                                     out.data_ptr(), B, res, C_, heads, WS, shift, wp.SCALE, stream),
                   "odic_swin_qkv_attention_tiled")
        outs.append(out.float())
    P = wp.collect(geo, outs)
    wp.assert_pairs(P, wp.p_want(name, geo, False), "bf16", f"tiled {name} B{B} res{res} shift{shift}")
