"""Search behind a given prefix, the parts that need no GPU: the argument rules (raised before any
device work), header / binding agreement of the two entry points with the ABI number of the header, the built library refusing bad
arguments, and the reason the reset works: tests/prefix_model.py's reset state fed to the step model of
tests/group_beam_model.py chooses at position P exactly what a seeding at position 0 chooses from the same candidates."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import group_beam_model as M
import prefix_model as PM

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "odic_hip.h")
SOS, EOS = 3, 2
F = np.float32


# ------------------------------------------------------------------------------------------------- public interface
@pytest.fixture(scope="module")
def model():
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank="cpu")

    def no_device(*a, **k):
        raise AssertionError("the argument check must come before any device work")
    m.forward_enc = no_device
    m._captioner_engine = no_device
    return m


# two images, max_seq_len 12 (10 prefix words at most), V = 500
BAD = [dict(prefix=[[5, 6], [7]]),                               # ragged
       dict(prefix=[[5, 6], [7, 8], [9, 10]]),                   # three prefixes for two images
       dict(prefix=list(range(10, 21))),                         # 11 words > max_seq_len - 2
       dict(prefix=[5, 500]), dict(prefix=[-1]),                 # outside [0, V)
       dict(prefix=[5, SOS]), dict(prefix=[[5, 6], [EOS, 6]]),   # SOS / EOS inside
       dict(prefix=[5, 6], sample_or_max="sample")]


@pytest.mark.parametrize("kw", BAD, ids=[str(i) for i in range(len(BAD))])
def test_searches_refuse_a_bad_prefix_before_any_device_call(model, kw):
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.captioning_model import Captioner
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    img = W.synth_images(2, W.TINY)
    with pytest.raises(ValueError):
        model.beam_search(img, [0, 0], sos_idx=SOS, eos_idx=EOS, beam_size=3, max_seq_len=12, **kw)
    with pytest.raises(ValueError):
        model(enc_x=img, enc_x_num_pads=[0, 0], mode="beam_search", sos_idx=SOS, eos_idx=EOS, beam_size=3,
              beam_max_seq_len=12, **kw)
    with pytest.raises(ValueError):
        Captioner(dict(sos_idx=SOS, eos_idx=EOS, beam_size=3, beam_max_seq_len=12, **kw), model=model)(
            img, enc_x_num_pads=[0, 0], mode="beam_search")
    ens = EsembleCaptioningModel([model, model], rank="cpu")
    ens.forward_enc = model.forward_enc
    with pytest.raises(ValueError):
        ens.ensemble_beam_search(img, [0, 0], sos_idx=SOS, eos_idx=EOS, beam_size=3, max_seq_len=12, **kw)
    if "sample_or_max" not in kw:
        with pytest.raises(ValueError):
            model.diverse_beam_search(img, [0, 0], sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=1, max_seq_len=12, **kw)
        with pytest.raises(ValueError):
            model(enc_x=img, enc_x_num_pads=[0, 0], mode="diverse_beam_search", sos_idx=SOS, eos_idx=EOS, num_groups=3,
                  group_size=1, beam_max_seq_len=12, **kw)


def test_sampling_mode_refuses_a_prefix_and_the_rules_accept_what_can_work(model):
    from on_device_image_captioning_amd import search, weights as W
    img = W.synth_images(2, W.TINY)
    with pytest.raises(ValueError, match="deterministic"):
        model(enc_x=img, enc_x_num_pads=[0, 0], mode="sampling", sos_idx=SOS, eos_idx=EOS, how_many_outputs=2,
              sample_max_seq_len=12, prefix=[5, 6])
    kw = dict(V=500, max_seq_len=12, sos_idx=SOS, eos_idx=EOS)
    assert search.check_prefix(None, 2, **kw) is None and search.check_prefix([], 2, **kw) is None
    assert search.check_prefix([[], []], 2, **kw) is None
    assert search.check_prefix([], 2, sampling=True, **kw) is None             # no prefix: nothing to refuse
    assert search.check_prefix([5, 6], 2, **kw) == [[5, 6], [5, 6]]
    assert search.check_prefix(torch.tensor([[5, 6], [7, 8]]), 2, **kw) == [[5, 6], [7, 8]]
    assert search.check_prefix(list(range(10, 20)), 2, **kw) == [list(range(10, 20))] * 2      # max_seq_len - 2 words
    # a prefix may hold banned words: the two rule sets do not look at each other
    assert search.check_constraints(0, 0, [5], V=500, max_seq_len=12, rows_per_image=3, sos_idx=SOS, eos_idx=EOS)["banned"] == [5]


def test_signatures_carry_the_keyword_only_prefix():
    import inspect
    from on_device_image_captioning_amd.captioning_model import CaptioningModel
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    for fn in (CaptioningModel.beam_search, CaptioningModel.diverse_beam_search, EsembleCaptioningModel.ensemble_beam_search):
        p = inspect.signature(fn).parameters["prefix"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn


# ------------------------------------------------------------------------------------------------- header / binding
def prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S).group(1)
    return [" ".join(a.split()) for a in args.split(",")], text


def test_header_and_binding_agree_and_the_abi_is_still_26():
    from on_device_image_captioning_amd import _hip
    ctype = lambda a: (ctypes.c_void_p if "*" in a else                                     # noqa: E731
                       {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[a.split()[0]])
    args, text = prototype("odic_dynexp_fill_caches")
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "lin", "ldlin", "qexp", "cond_c", "key_c", "va_c", "vb_c", "wfa_c", "wfb_c", "qk_c", "n_seq", "P",
        "rows_per_image", "N_cache", "T_cache", "d", "E", "eps", "stream"]
    res, argtypes = _hip._SIGNATURES["odic_dynexp_fill_caches"]
    assert res is ctypes.c_int and list(argtypes) == [ctype(a) for a in args]
    args, _ = prototype("odic_beam_reset_prefix")
    assert [a.split()[-1].lstrip("*") for a in args] == ["st", "emb", "prefix", "prefix_logp", "n_img", "beams",
                                                        "group_beams", "T", "P", "sos_idx", "stream"]
    res, argtypes = _hip._SIGNATURES["odic_beam_reset_prefix"]
    want = [ctypes.POINTER(_hip.BeamState), ctypes.POINTER(_hip.EmbedArgs)] + [ctype(a) for a in args[2:]]
    assert res is ctypes.c_int and list(argtypes) == want
    assert _hip.ABI_VERSION == 27 and re.search(r"#define ODIC_ABI_VERSION 27\b", text)


def test_a_library_without_a_symbol_is_reported_as_stale(monkeypatch):
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setitem(_hip._SIGNATURES, "odic_no_such_entry_point", (ctypes.c_int, []))
    with pytest.raises(RuntimeError, match="rebuild"):
        _hip.load()


def test_the_library_refuses_bad_arguments_without_a_gpu():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _hip.load()
    assert lib.odic_abi_version() == 27

    def fill(lin=16, ldlin=320, qexp=16, c=16, n_seq=2, P=5, rpi=3, N=6, T=12, d=64, E=16, **kw):
        ptr = dict(cond=c, key=c, va=c, vb=c, wfa=c, wfb=c, qk=c)
        ptr.update(kw)
        return lib.odic_dynexp_fill_caches(lin, ldlin, qexp, ptr["cond"], ptr["key"], ptr["va"], ptr["vb"], ptr["wfa"],
                                           ptr["wfb"], ptr["qk"], n_seq, P, rpi, N, T, d, E, 1e-9, None)

    for kw in (dict(P=0), dict(P=12), dict(P=13), dict(T=129, P=128), dict(E=12), dict(E=64), dict(d=96), dict(d=0),
               dict(n_seq=0), dict(n_seq=3), dict(rpi=6), dict(rpi=0), dict(N=0), dict(ldlin=319), dict(ldlin=322),
               dict(lin=8), dict(qexp=24)):
        assert fill(**kw) == -1, kw                                     # ODIC_EINVAL, before any launch
    for kw in (dict(lin=None), dict(qexp=None), dict(cond=None), dict(wfb=None), dict(qk=None)):
        assert fill(**kw) == -2, kw                                     # ODIC_ENULL

    def reset(n_img=2, beams=6, gb=2, T=12, P=4, st=True, emb=None, prefix=16, logp=16, **kw):
        f = {n: 16 for n, _ in _hip.BeamState._fields_}
        f.update(kw)
        s = _hip.BeamState(**f)
        e = None if emb is None else ctypes.byref(_hip.EmbedArgs(**emb))
        return lib.odic_beam_reset_prefix(ctypes.byref(s) if st else None, e, prefix, logp, n_img, beams, gb, T, P, SOS, None)

    ok_emb = dict(embed=16, pos_table=16, y=16, ldy=64, d=64, scale=8.0, pos_rows=20)
    for kw in (dict(P=0), dict(P=11), dict(gb=4), dict(gb=0), dict(beams=17, gb=17), dict(beams=0), dict(T=1), dict(T=129),
               dict(n_img=0), dict(n_img=32768), dict(emb=dict(ok_emb, pos_rows=4)), dict(emb=dict(ok_emb, d=0))):
        assert reset(**kw) == -1, kw
    for kw in (dict(st=False), dict(prefix=None), dict(logp=None), dict(anc=None), dict(cumul=None),
               dict(emb=dict(ok_emb, y=None))):
        assert reset(**kw) == -2, kw


# ------------------------------------------------------------------------------------------------- why -inf rows seed
def candidates(rng, n_img, R, V=40):
    """[n_img·R, R] candidates as the top-k launch writes them (value descending, then word ascending).  Values are
    multiples of 1/64 in (-8, 0): with the dyadic prefix log-probs below every total is exact in float32, so the order
    of the totals is the order of the values."""
    cv, ci = np.zeros((n_img * R, R), F), np.zeros((n_img * R, R), np.int32)
    for n in range(n_img * R):
        w = rng.choice(np.arange(4, V), size=R, replace=False)
        v = -rng.integers(1, 512, size=R).astype(F) / F(64)
        order = sorted(range(R), key=lambda i: (-v[i], w[i]))
        cv[n], ci[n] = v[order], w[order]
    return cv, ci


@pytest.mark.parametrize("G,kg", [(1, 3), (3, 2)])
def test_the_first_free_step_is_a_seeding_from_position_p(G, kg):
    rng = np.random.default_rng(7 + G)
    n_img, R, T, P, lam = 3, G * kg, 10, 4, 0.5
    prefix = rng.integers(4, 40, size=(n_img, P))
    plogp = -rng.integers(1, 256, size=(n_img, P)).astype(F) / F(32)
    st = PM.reset_state(n_img, R, T, SOS, prefix, plogp, group_beams=kg)
    assert np.isneginf(st["cumul"].reshape(n_img, G, kg)[:, :, 1:]).all()
    assert np.isfinite(st["cumul"].reshape(n_img, G, kg)[:, :, 0]).all()
    cv, ci = candidates(rng, n_img, R)
    new, events = M.step(st, cv, ci, G, kg, lam, EOS)
    seed, _ = M.step(M.new_state(n_img, R, T, SOS), cv, ci, G, kg, lam, EOS)          # *pos == 0 on the same candidates
    for b in range(n_img):
        # only the first row of every group is ever a parent
        assert events[b]["parent"].tolist() == [(r // kg) * kg for r in range(R)]
        for r in range(R):
            assert new["tokens"][b, r, :P + 1].tolist() == [SOS] + prefix[b].tolist()
            assert new["tokens"][b, r, P + 1] == seed["tokens"][b, r, 1]              # the words of the seeding
            assert new["logprobs"][b, r, P + 1] == seed["logprobs"][b, r, 1]          # at their own log-probs
            assert new["anc"][b * R + r, :P + 1].tolist() == [b * R] * P + [b * R + (r // kg) * kg]
            want = F(0.0)
            for v in list(plogp[b]) + [seed["logprobs"][b, r, 1]]:
                want = F(want + v)
            assert new["cumul"][b * R + r] == want and np.isfinite(want)
    assert int(new["pos"][0]) == P + 1 and (new["n_elem"] == P + 2).all()
    if G == 1:        # the single-group rule of odic_beam_step, transcribed separately, agrees
        for b in range(n_img):
            rows = slice(b * R, (b + 1) * R)
            parent, word, lp = M.single_group_rule(cv[rows], ci[rows], st["cumul"][rows], st["has_eos"][rows], P)
            s_parent, s_word, s_lp = M.single_group_rule(cv[rows], ci[rows], st["cumul"][rows], st["has_eos"][rows], 0)
            assert parent.tolist() == s_parent.tolist() == [0] * R
            assert word.tolist() == s_word.tolist() and lp.tolist() == s_lp.tolist()
