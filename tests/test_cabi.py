"""The drop-in boundary without a GPU: libodic_hip.so builds, loads, and exports exactly the entry
points include/odic_hip.h declares; the Python binding covers every one of them; and the product
path refuses to run on the CPU (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "odic_hip.h")


def header_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(odic_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_header_symbols_are_exported_and_bound(lib):
    from on_device_image_captioning_amd import _hip
    syms = header_symbols()
    assert len(syms) >= 16
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in syms:
        assert hasattr(raw, name), f"{name} declared in odic_hip.h but not exported"
    assert sorted(_hip.EXPORTED_SYMBOLS) == syms, "ctypes binding and header disagree"


def test_abi_version_and_build_string(lib):
    from on_device_image_captioning_amd import _hip
    assert lib.odic_abi_version() == _hip.ABI_VERSION
    assert b"gfx950" in lib.odic_build_info()


def test_argument_validation_needs_no_gpu(lib):
    from on_device_image_captioning_amd import _hip
    # NULL pointers / bad shapes are rejected before any launch
    assert lib.odic_gemm(None, None) == -2
    a = _hip.GemmArgs()
    a.A, a.W, a.out = 16, 16, 16
    a.M, a.N, a.K, a.batch = 0, 4, 4, 1
    assert lib.odic_gemm(ctypes.byref(a), None) == -1
    assert lib.odic_layernorm(None, 0, None, None, None, 1, 4, 1e-5, 0, None) == -2
    assert lib.odic_window_attention(16, 16, None, 16, 1, 12, 100, 3, 12, 0, 1.0, 1, None) == -1   # heads*32 != C
    # odic_beam_step: per-token log-probs are staged in LDS for at most 128 positions, and the arrival counter
    # packs {arrivals, growing images} into one int32: both limits are rejected, not overrun
    st = _hip.BeamState(*([16] * 11))
    assert lib.odic_beam_step(16, 16, ctypes.byref(st), None, 4, 3, 129, 77, None) == -1
    assert lib.odic_beam_step(16, 16, ctypes.byref(st), None, 32768, 3, 20, 77, None) == -1
    assert lib.odic_beam_step(16, 16, ctypes.byref(st), None, 4, 17, 20, 77, None) == -1
    # the retired one-launch search step and the diagnostic entry points are gone from the library and the binding
    # (the names appear nowhere in the file, so not in its dynamic symbol table either)
    with open(_hip.LIB_PATH, "rb") as f:
        blob = f.read()
    assert not [n for n in (b"odic_beam_search_step", b"odic_dbg_") if n in blob] and \
        not [n for n in _hip.EXPORTED_SYMBOLS if n == "odic_beam_search_step" or n.startswith("odic_dbg_")]
    emb = _hip.EmbedArgs(16, 16, None, 512, 512, 1.0, 20)             # embedding tail asked for without an output
    assert lib.odic_beam_step(16, 16, ctypes.byref(st), ctypes.byref(emb), 4, 3, 20, 77, None) == -2
    assert lib.odic_beam_reset(None, None, 4, 3, 20, 79, None) == -2
    assert lib.odic_copy(16, 32, 24, None) == -1 and lib.odic_copy(None, 32, 32, None) == -2
    assert lib.odic_beam_finalize_best(ctypes.byref(st), 16, 16, None, 16, 4, 3, 20, 77, None) == -2
    assert lib.odic_logsoftmax_sample(16, 8, None, 0, 16, 16, 4, 8, 9, 0, None, None) == -1           # k > V
    # a bf16 tile configuration the library does not carry (17: a retired persistent form) is refused by the dispatch
    a = _hip.GemmArgs()
    a.A, a.W, a.out = 16, 16, 16
    a.M, a.N, a.K, a.batch, a.lda, a.ldw, a.ldc = 256, 256, 64, 1, 64, 64, 256
    a.in_dtype, a.out_dtype, a.tile_cfg = _hip.BF16, _hip.BF16, 17
    assert lib.odic_gemm(ctypes.byref(a), None) == -1


def test_product_path_has_no_cpu_fallback():
    from on_device_image_captioning_amd import ops, weights as W
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.layernorm(torch.zeros(4, 8), torch.ones(8), torch.zeros(8))
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank="cpu")
    if not torch.cuda.is_available():          # (with a GPU a host-resident model runs on it: tests/test_e2e_gpu.py)
        with pytest.raises(RuntimeError, match="no CPU"):
            m(enc_x=W.synth_images(1, g), enc_x_num_pads=[0], mode="beam_search", sos_idx=3, eos_idx=2)
        with pytest.raises(RuntimeError, match="no CPU"):
            m.forward_enc(W.synth_images(1, g), [0])


def test_reference_api_surface():
    """Names, defaults and error behaviour of the reference's Python boundary."""
    import inspect
    from on_device_image_captioning_amd.captioning_model import Captioner, CaptioningModel
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import E2E_ExpansionNet_Captioner, End_ExpansionNet_v2
    sig = inspect.signature(CaptioningModel.forward)
    assert list(sig.parameters)[:7] == ["self", "enc_x", "dec_x", "enc_x_num_pads", "dec_x_num_pads",
                                        "apply_log_softmax", "mode"]
    assert sig.parameters["mode"].default == "forward"
    bs = inspect.signature(CaptioningModel.beam_search)
    assert [bs.parameters[k].default for k in ("beam_size", "how_many_outputs", "max_seq_len", "sample_or_max")] == \
        [3, 1, 20, "max"]
    ctor = list(inspect.signature(End_ExpansionNet_v2.__init__).parameters)
    for kw in ("swin_img_size", "swin_window_size", "final_swin_dim", "d_model", "N_enc", "N_dec", "ff", "num_heads",
               "num_exp_enc_list", "num_exp_dec", "output_word2idx", "output_idx2word", "max_seq_len", "drop_args",
               "rank"):
        assert kw in ctor
    with pytest.raises(ValueError):
        Captioner({"sos_idx": 1, "eos_idx": 2})
    with pytest.raises(ValueError):
        E2E_ExpansionNet_Captioner({"sos_idx": 1, "eos_idx": 2}, split_encoder=True)


def test_preprocess_matches_recorded_checksums(tmp_path):
    """The two small demo JPEGs are stored in tests/golden/demo_material and checked against the checksums recorded
    from them.  The two large ones (3456x4608 and 3394x4134, several MB) are not stored: their downscale factors are
    covered by seeded synthetic JPEGs of the same sizes, compared with the oracle's preprocessing exactly."""
    import json
    import numpy as np
    from PIL import Image
    from on_device_image_captioning_amd.image_utils import preprocess_image
    from oracle import expansionnet_ref as R
    img_dir = os.path.join(ROOT, "tests", "golden", "demo_material")
    helper = json.load(open(os.path.join(ROOT, "tests", "golden", "helpers.json")))
    stored = sorted(os.listdir(img_dir))
    assert stored == ["micheal.jpg", "tatin.jpg"]
    for fn in stored:
        want = helper["preprocess_pil_checksums"][fn]
        t = preprocess_image(os.path.join(img_dir, fn), 384)
        assert tuple(t.shape) == (1, 3, 384, 384) and t.dtype == torch.float32
        assert abs(float(t.double().sum()) - want["sum"]) < 1e-2
        assert abs(float(t.double().abs().sum()) - want["abssum"]) < 1e-2
    rng = np.random.default_rng(0)
    for w, h in ((3456, 4608), (3394, 4134)):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([xx * 255 // w, yy * 255 // h, (xx + yy) % 256], -1) + rng.integers(-20, 21, size=(h, w, 3))
        path = str(tmp_path / f"synth_{w}x{h}.jpg")
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), "RGB").save(path, quality=90)
        t = preprocess_image(path, 384)
        assert tuple(t.shape) == (1, 3, 384, 384) and t.dtype == torch.float32
        assert torch.equal(t, R.preprocess_image(path, 384))


def test_preprocess_non_rgb_becomes_a_black_canvas(tmp_path):
    """utils/image_utils.py:18-19: a file whose mode is not RGB is REPLACED by PIL_Image.new('RGB', size) — an
    all-black image, not a conversion — before Resize / ToTensor / Normalize.  Grey-scale, RGBA and palette files
    all map to the same tensor, the normalised zero image."""
    from PIL import Image
    from on_device_image_captioning_amd.image_utils import preprocess_image
    import numpy as np
    rng = np.random.default_rng(0)
    want = ((torch.zeros(3) - torch.tensor([0.485, 0.456, 0.406])) / torch.tensor([0.229, 0.224, 0.225]))
    for mode, shape, ext in (("L", (50, 70), "png"), ("RGBA", (40, 60, 4), "png"), ("P", (30, 30), "png")):
        path = str(tmp_path / f"img_{mode}.{ext}")
        Image.fromarray(rng.integers(1, 255, size=shape, dtype=np.uint8), "L" if mode == "P" else mode).convert(mode).save(path)
        t = preprocess_image(path, 96)
        assert tuple(t.shape) == (1, 3, 96, 96) and t.dtype == torch.float32
        assert torch.equal(t, want.view(1, 3, 1, 1).expand(1, 3, 96, 96))
    rgb = str(tmp_path / "rgb.png")
    Image.fromarray(rng.integers(1, 255, size=(20, 20, 3), dtype=np.uint8), "RGB").save(rgb)
    assert not torch.equal(preprocess_image(rgb, 96), want.view(1, 3, 1, 1).expand(1, 3, 96, 96))
