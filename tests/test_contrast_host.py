"""Contrastive beam search without a GPU: the numpy model of tests/contrast_model.py keeps its own rules,
every structured row family is clear (so the GPU test may ask for exact words there), the dense rows are unclear within
the cap, check_contrast and the C entry point refuse what the header says, and the mode reaches its method."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import contrast_model as CM

SOS, EOS = 3, 4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "odic_hip.h")
SMALL = [(V, k, M) for V, k, M in CM.shapes() if V <= 259]


def _cases(V, k, M):
    names, x, count, refs = CM.batch(V, k, M)
    for (w, pl, fl, extra), ref in zip(CM.SETTINGS, refs):
        for n, name in enumerate(names):
            yield name, x[:, n], int(count[n]), w, CM.log_alpha_of(pl), fl, CM.min_keep_of(k, extra, V), ref[n]


# ------------------------------------------------------------------------------------------------- the model's own rules
def test_off_is_the_log_softmax_and_its_top_k():
    for V, k, M in SMALL:
        names, x, count, _ = CM.batch(V, k, M)
        for n in range(len(names)):
            ref = torch.log_softmax(torch.from_numpy(x[0, n]).double(), -1).numpy()
            for c, w in ((0, 1.0), (int(count[n]), 0.0)):
                r = CM.reference(x[:, n], c, w, -np.inf, -20.0, k, k)
                fin = np.isfinite(ref)
                assert np.array_equal(np.isfinite(r["out"]), fin) and np.allclose(r["out"][fin], ref[fin], rtol=0, atol=1e-12)
                assert r["kept"] == V and r["mask"].all()
                assert r["top"].tolist() == np.argsort(-x[0, n].astype(np.float64), kind="stable")[:k].tolist()


def test_the_suppressor_is_the_log_of_the_mean_probability_and_is_clamped():
    V, k, M = 259, 3, 8
    names, x, _, _ = CM.batch(V, k, M)
    for n, name in enumerate(names[:len(CM.STRUCTURED)]):
        for c in (1, 2, 7):
            r = CM.reference(x[:, n], c, 0.5, -np.inf, -20.0, k, k)
            lp = torch.log_softmax(torch.from_numpy(x[:c + 1, n]).double(), -1).numpy()
            with np.errstate(divide="ignore"):
                s = np.log(np.exp(lp[1:]).mean(0))
            want = lp[0] - 0.5 * np.maximum(s, -20.0)
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(r["out"]), fin), name
            # (the direct form underflows below exp(-745): compare where it does not)
            ok = fin & (s > -600)
            assert np.allclose(r["out"][ok], want[ok], rtol=0, atol=1e-9), name
            if name == "masked_all":
                dead = np.isinf(x[1:c + 1, n]).all(0) & fin
                assert dead.any() and np.allclose(r["out"][dead], lp[0][dead] + 0.5 * 20.0, rtol=0, atol=1e-12)
            if name == "below_floor":
                assert (s[fin] < -20.0).any()


def test_the_cut_keeps_the_plausible_words_and_never_fewer_than_min_keep():
    rng = np.random.default_rng(5)
    for V in (17, 259):
        x = rng.standard_normal(V).astype(np.float32)
        x[3] = x[9] = x[11] = x.max() - np.float32(1.0)
        for alpha in (1.0, 0.5, 0.1, 1e-6):
            la = CM.log_alpha_of(alpha)
            for mk in (1, 3, 16):
                mask, m = CM.admissible(x, la, mk)
                assert m == int(((x - x.max()).astype(np.float32) >= la).sum()) and m >= 1
                assert int(mask.sum()) == max(m, mk)
                order = np.argsort(-x.astype(np.float64), kind="stable")
                assert mask[order[:max(m, mk)]].all()
        mask, m = CM.admissible(x, CM.log_alpha_of(0.0), 1)
        assert m == V and mask.all()
    # a cut inside a level of equal logits takes the lower indices
    x = np.array([0, 5, 9, 5, 5, 1, 5], dtype=np.float32)
    mask, m = CM.admissible(x, CM.log_alpha_of(0.5), 3)
    assert m == 1 and mask.tolist() == [False, True, True, True, False, False, False]


def test_the_fp32_form_stays_inside_the_derived_bound_and_a_missing_floor_does_not():
    worst, no_floor = 0.0, 0.0
    for V, k, M in SMALL:
        for name, x, c, w, la, fl, mk, r in _cases(V, k, M):
            out, top = CM.f32_form(x, c, w, la, fl, mk, k)
            fin = np.isfinite(r["out"])
            assert np.array_equal(np.isfinite(out), fin) and not np.isnan(out).any(), name
            ratio = np.abs(out[fin].astype(np.float64) - r["out"][fin]) / r["bound"][fin]
            worst = max(worst, float(ratio.max()))
            if r["clear"]:
                assert top.tolist() == r["top"].tolist(), (name, V, k, M)
            if name == "below_floor" and c > 0:
                bad, _ = CM.f32_form(x, c, w, la, fl, mk, k, clamp=False)
                with np.errstate(invalid="ignore"):
                    no_floor = max(no_floor, float(np.nanmax(np.abs(bad[fin].astype(np.float64) - r["out"][fin]) / r["bound"][fin])))
    assert worst <= 1.0, worst
    assert no_floor > 1e3, no_floor


def test_every_structured_family_is_clear_and_the_dense_rows_are_within_the_cap():
    dense = unclear = 0
    for V, k, M in CM.shapes():
        for name, x, c, w, la, fl, mk, r in _cases(V, k, M):
            if name == "dense":
                dense += 1
                unclear += not r["clear"]
            else:
                assert r["clear"], (name, V, k, M, c, w)
    assert dense >= 300 and unclear <= CM.MAX_UNCLEAR_DENSE * dense, (unclear, dense)


def test_the_families_hold_what_their_names_say():
    V, k, M = 259, 3, 8
    row = {f: CM.family_row(f, V, k, M) for f in CM.STRUCTURED}
    assert (row["ties"][0] == row["ties"][0].max()).sum() >= k + 2
    assert np.isinf(row["target_masked"][0]).sum() >= V // 7 and np.isfinite(row["target_masked"][0]).sum() > k
    assert np.isinf(row["masked_all"][1:]).all(0).any()
    some = np.isinf(row["masked_some"][1:])
    assert (some.any(0) & ~some.all(0)).any()
    assert np.array_equal(row["identical"][0], row["identical"][1])
    assert row["offset"][0].min() > 70 and row["offset"][1].max() < -70 and row["offset"][2].min() > 70
    assert np.sort(row["dominant"][0])[-1] - np.sort(row["dominant"][0])[-2] >= 29
    assert np.isfinite(row["short"][0]).sum() == k - 1
    assert np.isfinite(CM.family_row("short", V, 1, M)[0]).sum() == 1            # never a row without a finite word
    mask, m = CM.admissible(row["tie_cut"][0], CM.log_alpha_of(0.1), k + 2)
    level = row["tie_cut"][0] == 5.0
    assert m == 1 and level.sum() >= k + 3 and 0 < (mask & level).sum() < level.sum()


# ------------------------------------------------------------------------------------------------- header / binding
def test_header_declares_and_the_binding_binds_the_entry_point():
    from on_device_image_captioning_amd import _hip, ops
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"int odic_contrast_topk\((.*?)\);", text, flags=re.S).group(1)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* const* logits", "int32_t M", "int64_t ldl", "const int32_t* count", "const odic_contrast_args* a",
        "float* score_out", "int64_t lds", "float* top_val", "int32_t* top_idx", "int32_t* kept", "int32_t N", "int32_t V",
        "int32_t k", "void* stream"]
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    res, argtypes = _hip._SIGNATURES["odic_contrast_topk"]
    assert res is ctypes.c_int and list(argtypes) == [ctypes.POINTER(P), I32, I64, P, ctypes.POINTER(_hip.ContrastArgs), P, I64,
                                                      P, P, P, I32, I32, I32, P]
    struct = re.search(r"typedef struct odic_contrast_args \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);", struct) == [("float", "weight"), ("float", "log_alpha"), ("float", "floor"),
                                                      ("int32_t", "min_keep")]
    assert [(n, t) for n, t in _hip.ContrastArgs._fields_] == [("weight", ctypes.c_float), ("log_alpha", ctypes.c_float),
                                                              ("floor", ctypes.c_float), ("min_keep", I32)]
    assert _hip.ABI_VERSION == 27 and re.search(r"#define ODIC_ABI_VERSION 27\b", text)   # a pure addition
    a = ops.contrast_args(0.5, 0.1, -20.0, 5)
    assert (a.weight, a.floor, a.min_keep) == (0.5, -20.0, 5) and a.log_alpha == float(np.float32(math.log(0.1)))
    assert ops.contrast_args(0.5, 0.0, -20.0, 5).log_alpha == float("-inf") and ops.contrast_args(1, 1.0, 0, 1).log_alpha == 0.0


def test_the_library_refuses_bad_arguments_without_a_gpu():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _hip.load()
    nan, inf = float("nan"), float("inf")

    def call(M=2, ptrs=None, ldl=100, count=16, args=(0.5, -2.0, -20.0, 3), no_args=False, score=None, lds=0, tv=16, ti=16,
             kept=None, N=4, V=100, k=3, no_logits=False):
        arr = (ctypes.c_void_p * 9)(*(ptrs if ptrs is not None else [16] * max(M, 0) + [None] * (9 - max(M, 0))))
        a = _hip.ContrastArgs(*args)
        return lib.odic_contrast_topk(None if no_logits else arr, M, ldl, count, None if no_args else ctypes.byref(a), score, lds,
                                      tv, ti, kept, N, V, k, None)

    for kw in (dict(no_logits=True), dict(no_args=True), dict(tv=None), dict(ti=None), dict(count=None),
               dict(ptrs=[16, None] + [None] * 6), dict(ptrs=[None, 16] + [None] * 6)):
        assert call(**kw) == -2, kw                                     # ODIC_ENULL, before any launch
    for kw in (dict(M=0), dict(M=9), dict(k=0), dict(k=17), dict(k=3, V=2), dict(V=262145, ldl=262145), dict(N=0), dict(ldl=99),
               dict(score=16, lds=99), dict(args=(0.5, -2.0, -20.0, 2)), dict(args=(0.5, -2.0, -20.0, 101)),
               dict(args=(-0.1, -2.0, -20.0, 3)), dict(args=(inf, -2.0, -20.0, 3)), dict(args=(nan, -2.0, -20.0, 3)),
               dict(args=(0.5, 0.1, -20.0, 3)), dict(args=(0.5, nan, -20.0, 3)), dict(args=(0.5, -2.0, 0.5, 3)),
               dict(args=(0.5, -2.0, -inf, 3)), dict(args=(0.5, -2.0, nan, 3))):
        assert call(**kw) == -1, kw                                     # ODIC_EINVAL, before any launch


# ------------------------------------------------------------------------------------------------- Python arguments
def test_check_contrast_accepts_and_refuses_as_specified():
    from on_device_image_captioning_amd import search
    c = search.check_contrast("others", 4)
    assert c["lists"] == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]] and c["D"] == 3
    assert (c["contrast"], c["plausibility"], c["suppressor_floor"]) == (0.5, 0.1, -20.0)
    assert search.check_contrast("others", 8)["D"] == 7 and search.check_contrast("others", 1)["D"] == 0
    c = search.check_contrast([[1], [], (0, 3), torch.tensor([1])], 4, contrast=0, plausibility=0, suppressor_floor=0)
    assert c["lists"] == [[1], [], [0, 3], [1]] and c["D"] == 2
    assert search.check_contrast(None, 3)["lists"] == [[], [], []]
    assert search.check_contrast([[], []], 2, prefix=[], required_words=[[], []], sample_or_max="max")["D"] == 0
    assert search.check_contrast(torch.tensor([[1], [0]]), 2)["lists"] == [[1], [0]]
    with pytest.raises(ValueError, match="at most 7"):
        search.check_contrast("others", 9)
    with pytest.raises(ValueError, match="at most 7"):
        search.check_contrast([list(range(1, 9))] + [[]] * 8, 9)
    for bad, n, msg in (("all", 2, "'others'"), ([[1]], 2, "one per image"), ([[0], []], 2, "its own distractor"),
                        ([[2], []], 2, "outside the batch"), ([[-1], []], 2, "outside the batch"),
                        ([[1, 1], [], []], 3, "distinct"), ([[1.5], []], 2, "integers"), ([1, 0], 2, "one sequence")):
        with pytest.raises(ValueError, match=msg):
            search.check_contrast(bad, n)
    for kw in (dict(contrast=-0.1), dict(contrast=float("inf")), dict(contrast=float("nan")), dict(plausibility=-0.1),
               dict(plausibility=1.5), dict(plausibility=float("nan")), dict(suppressor_floor=0.5),
               dict(suppressor_floor=float("-inf")), dict(suppressor_floor=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            search.check_contrast("others", 2, **kw)
    for key, value in dict(prefix=[7, 8], required_words=[5], sample_or_max="sample").items():
        with pytest.raises(ValueError, match=re.escape(key) + r".* not supported in contrastive_beam_search"):
            search.check_contrast("others", 2, **{key: value})


def test_the_method_checks_its_arguments_and_the_dispatch_maps_its_keys():
    from on_device_image_captioning_amd import search
    from on_device_image_captioning_amd.captioning_model import CaptioningModel, Captioner
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    sig = inspect.signature(CaptioningModel.contrastive_beam_search)
    assert list(sig.parameters)[:9] == ["self", "enc_input", "enc_input_num_pads", "sos_idx", "eos_idx", "distractors",
                                        "beam_size", "how_many_outputs", "max_seq_len"]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert (d["beam_size"], d["how_many_outputs"], d["max_seq_len"], d["contrast"], d["plausibility"], d["suppressor_floor"],
            d["no_repeat_ngram_size"], d["min_length"], d["banned_words"]) == (3, 1, 20, 0.5, 0.1, -20.0, 0, 0, None)
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("contrast", "plausibility", "suppressor_floor"))
    assert hasattr(Captioner, "contrastive_beam_search")
    assert list(inspect.signature(Captioner.caption_regions).parameters)[:5] == ["self", "preprocessor", "images", "regions",
                                                                                 "distinctive"]
    assert inspect.signature(Captioner.caption_regions).parameters["distinctive"].default is False

    class Host(CaptioningModel):                                  # no encoder, no engine: a check that passes would raise
        def __init__(self):
            super().__init__()

        def _vocab_size(self):
            return 40

        def forward_enc(self, *a):
            raise AssertionError("device work")

    m = Host()
    x = torch.zeros(3, 2)
    for kw in (dict(distractors=[[0], [], []]), dict(distractors="others", contrast=-1), dict(distractors="others", plausibility=2),
               dict(distractors="others", suppressor_floor=1), dict(distractors="others", prefix=[5]),
               dict(distractors="others", required_words=[5]), dict(distractors="others", sample_or_max="sample"),
               dict(distractors="others", min_length=30), dict(distractors="others", banned_words=[EOS])):
        with pytest.raises(ValueError):
            m.contrastive_beam_search(x, [0] * 3, SOS, EOS, **kw)
    with pytest.raises(AssertionError, match="device work"):      # a call that passes the checks goes on to the encoder
        m.contrastive_beam_search(x, [0] * 3, SOS, EOS, "others")
    calls = []
    m.contrastive_beam_search = lambda *a, **k: calls.append((a, k)) or "cbs"
    args = dict(sos_idx=SOS, eos_idx=EOS, distractors=[[1], [0]], contrast=0.25, plausibility=0.2, suppressor_floor=-9.0,
                beam_size=4, how_many_outputs=2, beam_max_seq_len=9, num_groups=5, min_length=2)
    assert search.dispatch(m, "contrastive_beam_search", args, "x", [0, 0]) == "cbs"
    assert calls == [(("x", [0, 0]), dict(sos_idx=SOS, eos_idx=EOS, distractors=[[1], [0]], beam_size=4, how_many_outputs=2,
                                         max_seq_len=9, sample_or_max="max", contrast=0.25, plausibility=0.2,
                                         suppressor_floor=-9.0, min_length=2))]
    assert Captioner(dict(sos_idx=SOS, eos_idx=EOS), model=m)("x", mode="contrastive_beam_search") == "cbs"
    assert calls[-1] == (("x", [0]), dict(sos_idx=SOS, eos_idx=EOS, distractors="others", beam_size=5, how_many_outputs=1,
                                         max_seq_len=20, sample_or_max="max"))
    with pytest.raises(ValueError, match="temperature"):
        search.dispatch(m, "contrastive_beam_search", dict(args, temperature=0.5), "x", [0, 0])
    ens = EsembleCaptioningModel([m, m], rank="cpu")
    with pytest.raises(NotImplementedError, match="single model"):
        ens.contrastive_beam_search(None, [0], SOS, EOS, "others")


def test_caption_regions_checks_the_siblings_before_any_device_work():
    from on_device_image_captioning_amd.captioning_model import Captioner

    class NoDevice:
        def resize_regions(self, *a):
            raise AssertionError("device work")

    cap = Captioner(dict(sos_idx=SOS, eos_idx=EOS), model=object())
    box = (0, 0, 4, 4)
    with pytest.raises(ValueError, match="at most 7"):
        cap.caption_regions(NoDevice(), [None], [(0, box)] * 9, distinctive=True)
    with pytest.raises(ValueError, match="distinctive=True only"):
        cap.caption_regions(NoDevice(), [None], [(0, box)], contrast=0.3)
    with pytest.raises(AssertionError, match="device work"):
        cap.caption_regions(NoDevice(), [None, None], [(0, box)] * 8 + [(1, box)], distinctive=True)
    assert cap.caption_regions(NoDevice(), [None, None], [], distinctive=True) == [[], []]
