"""What every search enqueues, step by step (`-m gpu`): TINY geometry, the synthetic "eos" checkpoint, four synthetic
images, fp32, max_seq_len 12 — the fixture of tests/test_diverse_search_gpu.py.

Each flavour runs once under ops.profile(); between its one beam_reset and its one beam_finalize the launch families
(the names ops.py gives its launches: odic_topk_rows, odic_topk_rows_constrained and odic_logsoftmax_sample all count as
"logsoftmax_topk", odic_group_beam_step as "beam_step") must be a whole number of the step written out below, and that
number must be the one the poll rule of search.run_steps gives for the step at which the device raised `done`.

With the fixture's checkpoints every one of those searches has a row that grows to the last position, so the host never
stops them.  The early stops are asserted on a third checkpoint, "eager": the fixture's with 300 added to the EOS bias.
EOS then leads every row by more than 200 in the logit (the other logits lie within a few tens of each other), so every
word but EOS costs 200 to 400 in log-prob, EOS about 0, and both stay far above the -999 a finished row's spare
candidates carry.  Plain beam 3: step 0 takes EOS and two other words, step 1 ends those two, step 2 finds nothing
growing and raises `done`; the host sees it after step 3 and has enqueued 4 steps.  With min_length 5 EOS is inadmissible
in steps 0-4, all three rows take it in step 5, step 6 raises `done`, the host sees it after step 7: 8 steps.
"""
import pytest
import torch

import search_constraints_model as SC
from conftest import cached_state_dict
from on_device_image_captioning_amd import ops, search
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
SOS, EOS = 3, 2
N_IMG, MAX_LEN = 4, 12
STEPS = MAX_LEN - 1

# one decoder position of TINY (two layers): the LayerNorms folded into the products (≤ 192 rows) …
LAYER = ["gemm_f32", "dynexp_step", "gemm_f32", "cross_attn_step", "gemm_f32", "gemm_f32", "gemm_f32"]
DECODER = LAYER + LAYER + ["gemm_f32", "gemm_f32"]
# … or launched on their own (ODIC_FOLD_LN=0)
LAYER_LN = ["layernorm", "gemm_f32", "dynexp_step", "layernorm", "gemm_f32", "cross_attn_step", "gemm_f32", "layernorm",
            "gemm_f32", "gemm_f32"]
DECODER_LN = LAYER_LN + LAYER_LN + ["gemm_f32", "layernorm", "gemm_f32"]


def step_families(flavour, folded):
    dec = DECODER if folded else DECODER_LN
    return {
        # the chosen words' embedding is written by beam_step itself: no dec_embed
        "beam": dec + ["logsoftmax_topk", "beam_step"],
        "diverse": dec + ["logsoftmax_topk", "beam_step"],
        # the top-k launch also writes the log-prob rows, odic_topk_rows_constrained re-selects from them
        "constrained": dec + ["logsoftmax_topk", "logsoftmax_topk", "beam_step"],
        "sample": ["dec_embed"] + dec + ["logsoftmax_topk", "beam_step"],
        # a decoder pass per member, then the average, its (admissible) top-k, the bookkeeping
        "ensemble": (["dec_embed"] + dec) * 2 + ["ensemble_logprobs", "logsoftmax_topk", "beam_step"],
        # (the same families: ops.py gives odic_topk_rows and odic_topk_rows_constrained one name, no flops and the same
        # bytes, so the profile cannot tell them apart — the test looks at the captions for that)
        "ensemble_constrained": (["dec_embed"] + dec) * 2 + ["ensemble_logprobs", "logsoftmax_topk", "beam_step"],
        "eager": dec + ["logsoftmax_topk", "beam_step"],
        "eager_constrained": dec + ["logsoftmax_topk", "logsoftmax_topk", "beam_step"],
    }[flavour]


EARLY = {"eager": 4, "eager_constrained": 8}            # steps enqueued, by the reasoning of the module docstring


def steps_the_poll_rule_gives(done_step):
    """The host looks after steps 3 and 7 of the 11 (t >= 1, (t + 1) % 4 == 0, t + 1 < 11) and stops at the first look
    that comes at or after the step that raised `done`."""
    if done_step is not None and done_step <= 3:
        return 4
    if done_step is not None and done_step <= 7:
        return 8
    return STEPS


def words(caption):
    return [w for w in caption if w not in (SOS, EOS)]


def build(state_dict):
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=DEV)
    m.load_state_dict(state_dict, strict=True)
    return m.to(DEV).eval().set_precision("fp32")


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return build(cached_state_dict("TINY", "eos"))


@pytest.fixture(scope="module")
def eager():
    sd = dict(cached_state_dict("TINY", "eos"))
    bias = sd["vocab_linear.bias"].clone()
    bias[EOS] += 300.0
    sd["vocab_linear.bias"] = bias
    return build(sd)


@pytest.fixture(scope="module")
def ensemble(model):
    """Two members: the fixture's and the "eos" checkpoint of seed 1."""
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    return EsembleCaptioningModel([model, build(W.synth_state_dict(W.TINY, seed=1, variant="eos", eos_idx=EOS))], rank=DEV)


@pytest.fixture(scope="module")
def images():
    return W.synth_images(N_IMG, W.TINY).to(DEV)


def run(flavour, model, ensemble, images, eager=None):
    pads = [0] * N_IMG
    cons = dict(no_repeat_ngram_size=2, min_length=5)
    beam = dict(sos_idx=SOS, eos_idx=EOS, beam_size=3, max_seq_len=MAX_LEN)
    if flavour.startswith("eager"):
        return eager.beam_search(images, pads, **beam, **(cons if flavour == "eager_constrained" else {}))
    if flavour == "beam":
        return model.beam_search(images, pads, **beam)
    if flavour == "sample":
        return model.beam_search(images, pads, sample_or_max="sample", **beam)
    if flavour == "constrained":
        return model.beam_search(images, pads, **beam, **cons)
    if flavour == "diverse":
        return model.diverse_beam_search(images, pads, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3,
                                         max_seq_len=MAX_LEN)
    return ensemble.ensemble_beam_search(images, pads, **beam, **(cons if flavour == "ensemble_constrained" else {}))


@pytest.mark.parametrize("flavour", ["beam", "sample", "diverse", "constrained", "ensemble", "ensemble_constrained",
                                     "eager", "eager_constrained"])
def test_a_search_enqueues_whole_steps_and_as_many_as_the_poll_rule_gives(model, ensemble, eager, images, flavour,
                                                                          monkeypatch):
    seen = []
    run_steps = search.run_steps

    def spy(st, steps, step_fn):                         # which state the search ran on (its counters are read below)
        seen.append((st, steps))
        return run_steps(st, steps, step_fn)
    monkeypatch.setattr(search, "run_steps", spy)
    run(flavour, model, ensemble, images, eager)                                 # warm-up: code load
    with ops.profile() as recs:
        toks, lps = run(flavour, model, ensemble, images, eager)
    fam = [r[0] for r in recs]
    st, steps = seen[-1]
    assert steps == STEPS and st.T == MAX_LEN
    assert fam.count("beam_reset") == 1 and fam.count("beam_finalize") == 1 and fam[-1] == "beam_finalize"
    body = fam[fam.index("beam_reset") + 1:-1]
    one = step_families(flavour, model._captioner_engine().fuse_ln)
    n = body.count("beam_step")
    print(f"{flavour}: {n} steps of {len(one)} launches")
    assert body == one * n
    if flavour == "constrained":                         # the second of the two is the selection: it computes nothing
        sel = [r for r in recs[fam.index("beam_reset") + 1:] if r[0] == "logsoftmax_topk"]
        assert all(r[1] > 0 for r in sel[0::2]) and all(r[1] == 0 for r in sel[1::2])
    # the step that raised `done`: a row that appends EOS at step t has t + 2 tokens and is still counted as growing
    # there, so `done` rises one step after the last row ended — if the search got that far
    finished = bool(st.has_eos.all())
    done_step = int(st.n_elem.max()) - 1 if finished else None
    if done_step is not None and done_step > STEPS - 1:
        done_step = None
    assert int(st.done) == (done_step is not None and done_step < n)
    print(f"{flavour}: done raised at step {done_step}, position counter {int(st.pos)}")
    assert int(st.pos) == n == steps_the_poll_rule_gives(done_step)
    if flavour in EARLY:                                 # the host did stop these, and where the reasoning says
        assert n == EARLY[flavour] < STEPS and int(st.done) == 1 and done_step == n - 2
    if flavour == "ensemble_constrained":                # the selection was the constrained one: the captions keep the rules
        plain, _ = run("ensemble", model, ensemble, images)
        assert any(len(words(per[0])) < 5 or SC.repeats_ngram(per[0], 2) for per in plain), plain
        for per in toks:
            assert len(words(per[0])) >= 5 and not SC.repeats_ngram(per[0], 2), per
    assert len(toks) == N_IMG and all(c[0] == SOS for per in toks for c in per)
