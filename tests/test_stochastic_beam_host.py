"""Stochastic beam search without a GPU: the numpy model of tests/stochastic_beam_model.py keeps the four
invariants on its case list, every case is clear (the device's choice is determined by the model and the band), the header
and the ctypes binding agree on the two entry points, the built library refuses bad arguments, and the Python argument
errors."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import stochastic_beam_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "odic_hip.h")
SOS, EOS = SM.SOS, SM.EOS
F = np.float32


# ------------------------------------------------------------------------------------------------- the model
def test_the_transform_is_the_textbook_formula_where_that_can_be_formed():
    """G~ = -log(e^-G - e^-Z + e^-g) directly, in float64, where nothing over- or underflows."""
    rng = np.random.default_rng(0)
    for _ in range(200):
        phi = F(-rng.uniform(0, 20))
        G = F(phi + rng.gumbel())
        pert0 = F(-rng.uniform(0, 3))
        pert = F(pert0 - rng.uniform(1e-3, 10))
        got, band, exact = SM.child(G, phi, pert, pert0)
        Z, g = float(phi) + float(pert0), float(phi) + float(pert)
        want = -math.log(math.exp(-float(G)) - math.exp(-Z) + math.exp(-g))
        assert not exact and abs(got - want) <= 1e-9 * max(1.0, abs(want)), (G, phi, pert, pert0, got, want)
        assert got <= float(G) and 0 < band < 1e-4
    assert SM.child(F(-3.5), F(-4), F(-1), F(-1)) == (-3.5, 0.0, True)


def test_log1mexp_takes_the_stable_branch_on_both_sides_of_ln2():
    for d in (-1e-30, -1e-7, -0.5, -SM.LN2 + 1e-9, -SM.LN2 - 1e-9, -3.0, -50.0, -700.0):
        want = math.log1p(-math.exp(d)) if d < -1e-3 else math.log(-math.expm1(d))
        assert abs(SM.log1mexp(d) - want) <= 1e-12 * max(1.0, abs(want)), d


@pytest.mark.parametrize("kind,n_img,k,T", SM.CASES)
def test_the_model_keeps_the_invariants_and_every_case_is_clear(kind, n_img, k, T):
    c = SM.case(kind, n_img, k, T)
    assert all(SM.is_clear(o, k) for o in c["offers"])           # (case() looked for such a salt; this is the check)
    if c["t"] + 1 >= T:
        for key in SM.STATE_KEYS:
            assert np.array_equal(c["new"][key], c["st"][key]), key
        assert np.array_equal(c["gnew"], c["gscore"].astype(np.float64))
        return
    SM.check_invariants(c["st"], c["gscore"], c["new"], c["gnew"].astype(F), f"{kind} {n_img} {k} {T}")
    # in float64 too, before the rounding of the comparison above
    for b in range(n_img):
        g = c["gnew"][b * k:(b + 1) * k]
        assert np.all(g[:-1] >= g[1:])


def test_the_cases_reach_what_they_are_named_for():
    seen = dict(empty_rows=False, tie_inherits_twice=False, both_sides_of_ln2=False, near_700=False, done=False,
                finished_beside_growing=False)
    for kind, n_img, k, T in SM.CASES:
        c = SM.case(kind, n_img, k, T)
        st, new, t = c["st"], c["new"], c["t"]
        if t + 1 >= T:
            continue
        seen["empty_rows"] |= kind == "few_offers" and bool(np.isneginf(new["cumul"]).any()) and bool(np.isneginf(c["gnew"]).any())
        if kind == "tie":
            for b in range(n_img):
                par = new["anc"][b * k:(b + 1) * k, t]
                g = c["gnew"][b * k:(b + 1) * k]
                for p in set(par.tolist()):
                    seen["tie_inherits_twice"] |= int(np.sum((par == p) & (g == float(c["gscore"][p])))) >= 2
        if kind == "ln2":
            d = (c["cp"][:, 1:] - c["cp"][:, :1]).astype(np.float64)
            seen["both_sides_of_ln2"] |= bool(((d > -SM.LN2) & (d < 0)).any() and (d < -SM.LN2).any())
        seen["near_700"] |= kind == "large" and bool((np.abs(st["cumul"]) > 600).any() and (np.abs(c["gscore"]) > 600).any())
        seen["done"] |= kind == "all_finished" and bool(new["done"][0])
        seen["finished_beside_growing"] |= kind == "mixed" and bool(st["has_eos"].any() and not st["has_eos"].all())
    assert all(seen.values()), seen


def test_the_band_scales_with_the_operands_and_stays_small():
    for kind, n_img, k, T in SM.CASES:
        c = SM.case(kind, n_img, k, T)
        for offers in c["offers"]:
            for o in offers:
                j = o["row"]
                S = max(1.0, abs(float(c["gscore"][j])), abs(float(c["st"]["cumul"][j])), float(np.abs(c["cp"][np.isfinite(c["cp"])]).max()))
                assert o["band"] <= SM.EPS * (18 * S + 7 * 110 + 12.5)        # |L| <= |log 2^-149| < 110 for fp32 d


# ------------------------------------------------------------------------------------------------- header / binding
def test_header_declares_and_the_binding_binds_the_entry_points():
    from on_device_image_captioning_amd import _hip, ops
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    P, I32, I64, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    proto = re.search(r"int odic_stochastic_beam_step\((.*?)\);", text, flags=re.S).group(1)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* cand_val", "const int32_t* cand_idx", "const float* cand_pert", "float* gscore",
        "const odic_beam_state* st", "const odic_embed_args* emb", "int32_t n_img", "int32_t beams", "int32_t T",
        "int64_t eos_idx", "void* stream"]
    res, argtypes = _hip._SIGNATURES["odic_stochastic_beam_step"]
    assert res is ctypes.c_int
    assert list(argtypes) == [P, P, P, P, ctypes.POINTER(_hip.BeamState), ctypes.POINTER(_hip.EmbedArgs), I32, I32, I32, I64, P]
    proto = re.search(r"int odic_logsoftmax_sample_scored\((.*?)\);", text, flags=re.S).group(1)
    assert [" ".join(a.split()) for a in proto.split(",")] == [
        "const float* logits", "int64_t ldl", "float* logp_out", "int64_t ldp", "float* top_val", "int32_t* top_idx",
        "float* top_pert", "int32_t N", "int32_t V", "int32_t k", "uint64_t seed", "const int32_t* pos", "void* stream"]
    res, argtypes = _hip._SIGNATURES["odic_logsoftmax_sample_scored"]
    assert res is ctypes.c_int and list(argtypes) == [P, I64, P, I64, P, P, P, I32, I32, I32, U64, P, P]
    for name in ("odic_stochastic_beam_step", "odic_logsoftmax_sample_scored"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert hasattr(ops, "stochastic_beam_step") and hasattr(ops, "logsoftmax_sample_scored")
    assert _hip.ABI_VERSION == 27 and re.search(r"#define ODIC_ABI_VERSION 27\b", text)   # a pure addition
    # the state struct is what it was: eleven pointers
    assert [n for n, _ in _hip.BeamState._fields_] == ["tokens", "logprobs", "anc", "cumul", "n_elem", "has_eos", "row_valid",
                                                       "next_tok", "pos", "done", "ctr"]


def test_the_library_refuses_bad_arguments_without_a_gpu():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _hip.load()
    assert lib.odic_abi_version() == 27
    st = _hip.BeamState(*([16] * 11))

    def step(cv=16, ci=16, cp=16, g=16, state=st, emb=None, n_img=3, k=5, T=8, eos=EOS):
        return lib.odic_stochastic_beam_step(cv, ci, cp, g, ctypes.byref(state) if state is not None else None, emb, n_img, k,
                                             T, eos, None)

    no_tokens = _hip.BeamState(*([None] + [16] * 10))
    no_ctr = _hip.BeamState(*([16] * 10 + [None]))
    bad_emb = _hip.EmbedArgs(16, None, 16, 8, 8, 1.0, 4)
    bad_d = _hip.EmbedArgs(16, 16, 16, 8, 0, 1.0, 4)
    bad = [dict(cv=None), dict(ci=None), dict(cp=None), dict(g=None), dict(state=None), dict(state=no_tokens), dict(state=no_ctr),
           dict(emb=ctypes.byref(bad_emb)), dict(emb=ctypes.byref(bad_d)), dict(n_img=0), dict(n_img=32768), dict(k=0),
           dict(k=17), dict(k=-1), dict(T=1), dict(T=129), dict(eos=-1)]
    for kw in bad:
        assert step(**kw) == -1, kw                                     # ODIC_EINVAL, before any launch

    def draw(x=16, tv=16, ti=16, tp=16, N=4, V=100, k=3):
        return lib.odic_logsoftmax_sample_scored(x, V, None, 0, tv, ti, tp, N, V, k, 7, None, None)

    for kw in (dict(x=None), dict(tv=None), dict(ti=None), dict(tp=None)):
        assert draw(**kw) == -2, kw                                     # ODIC_ENULL, as odic_logsoftmax_sample
    for kw in (dict(N=0), dict(V=0), dict(k=0), dict(k=17), dict(V=2, k=3)):
        assert draw(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------- Python arguments
def test_check_stochastic_beam_accepts_the_defaults_and_refuses_the_rest():
    from on_device_image_captioning_amd import search
    assert search.check_stochastic_beam(1) == 1 and search.check_stochastic_beam(15) == 15
    assert search.check_stochastic_beam(4, prefix=[], required_words=[[], []], banned_words=[]) == 4
    for n in (0, 16, -1, 2.5, True):
        with pytest.raises(ValueError, match="num_samples"):
            search.check_stochastic_beam(n)
    refused = dict(prefix=[7, 8], required_words=[5], no_repeat_ngram_size=2, min_length=3, banned_words=[9],
                   temperature=0.7, top_k=5, top_p=0.9)
    for key, value in refused.items():
        name = "temperature / top_k / top_p" if key in ("temperature", "top_k", "top_p") else key
        with pytest.raises(ValueError, match=re.escape(f"{name} ") + r"(is|are) not supported in stochastic_beam_search"):
            search.check_stochastic_beam(4, **{key: value})
    with pytest.raises(ValueError, match="prefix is not supported"):
        search.check_stochastic_beam(4, prefix=torch.tensor([[7], [8]]))


def test_the_method_checks_its_arguments_before_any_device_work():
    from on_device_image_captioning_amd.captioning_model import CaptioningModel, Captioner
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    sig = inspect.signature(CaptioningModel.stochastic_beam_search)
    assert list(sig.parameters)[:8] == ["self", "enc_input", "enc_input_num_pads", "sos_idx", "eos_idx", "num_samples",
                                        "max_seq_len", "seed"]
    assert sig.parameters["num_samples"].default == 5 and sig.parameters["max_seq_len"].default == 20
    assert sig.parameters["seed"].default is None
    assert hasattr(Captioner, "stochastic_beam_search")

    class Host(CaptioningModel):                                  # no encoder, no engine: a check that passes would raise
        def __init__(self):
            super().__init__()

        def _vocab_size(self):
            return 10

        def forward_enc(self, *a):
            raise AssertionError("device work")

    m = Host()
    for kw in (dict(num_samples=0), dict(num_samples=16), dict(prefix=[4]), dict(required_words=[[4]]), dict(min_length=1),
               dict(no_repeat_ngram_size=1), dict(banned_words=[4]), dict(temperature=2.0), dict(top_k=3), dict(top_p=0.5),
               dict(num_samples=10)):                             # 11 rows > 10 words
        with pytest.raises(ValueError):
            m.stochastic_beam_search(None, [0], SOS, EOS, **kw)
    with pytest.raises(ValueError, match="'sampling', 'diverse' or 'stochastic_beam'"):
        m.consensus_caption(None, [0], num_candidates=3, source="beam", sos_idx=SOS, eos_idx=EOS)
    with pytest.raises(ValueError, match="num_samples"):
        m.consensus_caption(None, [0], num_candidates=16, source="stochastic_beam", sos_idx=SOS, eos_idx=EOS)
    # the dispatch knows the mode and passes its keys
    from on_device_image_captioning_amd import search
    calls = []
    m.stochastic_beam_search = lambda *a, **k: calls.append((a, k)) or "sbs"
    assert search.dispatch(m, "stochastic_beam_search", dict(sos_idx=SOS, eos_idx=EOS, num_samples=3, beam_max_seq_len=9,
                                                             seed=11, beam_size=7), "x", [0]) == "sbs"
    assert calls == [(("x", [0]), dict(sos_idx=SOS, eos_idx=EOS, num_samples=3, max_seq_len=9, seed=11))]
    assert Captioner(dict(sos_idx=SOS, eos_idx=EOS, num_samples=2), model=m)("x", mode="stochastic_beam_search") == "sbs"
    assert calls[-1] == (("x", [0]), dict(sos_idx=SOS, eos_idx=EOS, num_samples=2, max_seq_len=20, seed=None))
    # the ensemble refuses the mode and the method
    ens = EsembleCaptioningModel([m, m], rank="cpu")
    with pytest.raises(AssertionError, match="only beam search"):
        ens(enc_x=None, mode="stochastic_beam_search", sos_idx=SOS, eos_idx=EOS)
    with pytest.raises(NotImplementedError, match="single model"):
        ens.stochastic_beam_search(None, [0], SOS, EOS)
