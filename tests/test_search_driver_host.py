"""The host side of the searches (on_device_image_captioning_amd/search.py) without a GPU: when the step loop looks at
the `done` flag, what the read-out makes of a beam state, the argument rules of the constrained searches, and what the
mode dispatch passes to the model.
"""
import types

import pytest
import torch

from on_device_image_captioning_amd import search as S

SOS, EOS = 3, 2


# ------------------------------------------------------------------------------------------------- the step loop
class CountedFlag:
    """Stands in for the device's int32[1] `done`: counts the reads and remembers after which step each came."""

    def __init__(self, steps_run, set_after=None):
        self.value = torch.zeros(1, dtype=torch.int32)
        self.steps_run, self.set_after, self.read_at = steps_run, set_after, []

    def item(self):
        t = self.steps_run[-1]
        self.read_at.append(t)
        if self.set_after is not None and t >= self.set_after:
            self.value.fill_(1)
        return self.value.item()


def run(steps, set_after=None):
    ran = []
    st = types.SimpleNamespace(done=CountedFlag(ran, set_after))
    S.run_steps(st, steps, ran.append)
    return ran, st.done.read_at


# after which steps t the host looks, for steps = 1 .. 24: t >= 1, (t + 1) % 4 == 0, t + 1 < steps — written out
POLLED = {1: [], 2: [], 3: [], 4: [], 5: [3], 6: [3], 7: [3], 8: [3], 9: [3, 7], 10: [3, 7], 11: [3, 7], 12: [3, 7],
          13: [3, 7, 11], 14: [3, 7, 11], 15: [3, 7, 11], 16: [3, 7, 11], 17: [3, 7, 11, 15], 18: [3, 7, 11, 15],
          19: [3, 7, 11, 15], 20: [3, 7, 11, 15], 21: [3, 7, 11, 15, 19], 22: [3, 7, 11, 15, 19],
          23: [3, 7, 11, 15, 19], 24: [3, 7, 11, 15, 19]}


def test_poll_interval_is_the_one_the_table_was_written_for():
    from on_device_image_captioning_amd import captioning_model
    assert S._DONE_POLL == 4 and captioning_model._DONE_POLL == 4


@pytest.mark.parametrize("steps", range(1, 25))
def test_done_is_read_exactly_at_the_polled_steps_and_every_step_runs_while_it_stays_clear(steps):
    ran, read_at = run(steps)
    assert ran == list(range(steps))
    assert read_at == POLLED[steps]


@pytest.mark.parametrize("steps", range(1, 25))
def test_the_loop_stops_right_after_the_first_polled_step_that_finds_done_and_at_no_other(steps):
    for set_after in range(steps):                       # `done` turns 1 during step set_after
        ran, read_at = run(steps, set_after)
        later = [t for t in POLLED[steps] if t >= set_after]
        last = later[0] if later else steps - 1          # no poll left: the loop runs out
        assert ran == list(range(last + 1)), (steps, set_after)
        assert read_at == [t for t in POLLED[steps] if t <= last]


# ------------------------------------------------------------------------------------------------- the read-out
def cpu_state():
    """n_img 2, beams 3, T 6; row lengths 2, 6, 4 | 3, 3, 5; token b,i,t = 100·b + 10·i + t, log-prob = -(token) / 8."""
    tokens = torch.tensor([[[100 * b + 10 * i + t for t in range(6)] for i in range(3)] for b in range(2)], dtype=torch.int64)
    return types.SimpleNamespace(n_img=2, beams=3, T=6, tokens=tokens, logprobs=-tokens.to(torch.float32) / 8,
                                 n_elem=torch.tensor([2, 6, 4, 3, 3, 5], dtype=torch.int32))


def test_read_out_cuts_at_the_row_length_and_pads_to_the_longest_chosen_row():
    st = cpu_state()
    before = (st.tokens.clone(), st.logprobs.clone(), st.n_elem.clone())
    toks, lp = S.read_captions(st, torch.tensor([[2, 0], [1, 1]], dtype=torch.int32), 2)
    assert toks == [[[20, 21, 22, 23], [0, 1]], [[110, 111, 112], [110, 111, 112]]]      # the same beam may be read twice
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (2, 2, 4)                    # longest chosen row: 4, not T = 6
    want = torch.tensor([[[20, 21, 22, 23], [0, 1, 0, 0]], [[110, 111, 112, 0], [110, 111, 112, 0]]], dtype=torch.float32) / -8
    assert torch.equal(lp, want)
    assert all(torch.equal(a, b) for a, b in zip(before, (st.tokens, st.logprobs, st.n_elem)))


def test_read_out_of_one_output_per_image():
    toks, lp = S.read_captions(cpu_state(), torch.tensor([[1], [2]]), 1)
    assert toks == [[[10, 11, 12, 13, 14, 15]], [[120, 121, 122, 123, 124]]]
    assert tuple(lp.shape) == (2, 1, 6)
    assert lp[0, 0].tolist() == [-10 / 8, -11 / 8, -12 / 8, -13 / 8, -14 / 8, -15 / 8]
    assert lp[1, 0].tolist() == [-120 / 8, -121 / 8, -122 / 8, -123 / 8, -124 / 8, 0.0]
    # a wider `rows` than outputs asked for: only the first how_many_outputs columns are read
    toks2, lp2 = S.read_captions(cpu_state(), torch.tensor([[1, 0, 2], [2, 0, 1]]), 1)
    assert toks2 == toks and torch.equal(lp2, lp)


# ------------------------------------------------------------------------------------------------- the constraint rules
def check(n=0, m=0, banned=None, **kw):
    args = dict(V=500, max_seq_len=12, rows_per_image=3, sos_idx=SOS, eos_idx=EOS)
    args.update(kw)
    return S.check_constraints(n, m, banned, **args)


# the cases of tests/test_search_constraints_host.py (V 500, max_seq_len 12, 3 rows per image) with the message of each
BAD = [(dict(n=-1), "no_repeat_ngram_size and min_length must be >= 0"),
       (dict(m=-1), "no_repeat_ngram_size and min_length must be >= 0"),
       (dict(m=11), "min_length 11 > max_seq_len - 2 = 10: no caption could end"),
       (dict(banned=range(10, 10 + 500 - 12 - 3 + 1)),
        "486 banned words + 12 positions + 3 candidates per row exceed the vocabulary (500 words): a row could run out of "
        "admissible words"),
       (dict(banned=[7, EOS]), "the SOS and EOS ids cannot be banned (min_length is the control over where a caption ends)"),
       (dict(banned=[SOS]), "the SOS and EOS ids cannot be banned (min_length is the control over where a caption ends)"),
       (dict(banned=range(10, 1035), V=4000), "at most 1024 banned words"),
       (dict(n=2, sampling=True), None), (dict(banned=[7], sampling=True), None), (dict(m=3, sampling=True), None)]
SAMPLING = ("no_repeat_ngram_size / min_length / banned_words apply to the deterministic searches only: drawing under "
            "constraints (sample_or_max='sample', mode='sampling') is not supported")


@pytest.mark.parametrize("kw,message", BAD, ids=[",".join(k) + str(i) for i, (k, _) in enumerate(BAD)])
def test_every_rule_raises_with_its_message(kw, message):
    with pytest.raises(ValueError) as e:
        check(**kw)
    assert str(e.value) == (message or SAMPLING)


def test_rules_that_pass():
    assert check() is None
    assert check(banned=[], sampling=True) is None
    assert check(V=lambda: 1 / 0) is None                                   # the vocabulary is not asked for without a constraint
    ok = check(m=10, banned=range(10, 10 + 500 - 12 - 3), V=lambda: 500)    # the largest admissible ban list and length
    assert ok == dict(no_repeat_ngram=0, min_words=10, banned=list(range(10, 495)))
    assert check(n=2, banned=[9, 7, 9]) == dict(no_repeat_ngram=2, min_words=0, banned=[7, 9])
    # the order of the rules: the sign before the sampling refusal, that before the length, that before the ban list
    with pytest.raises(ValueError, match="must be >= 0"):
        check(n=-1, m=11, sampling=True)
    with pytest.raises(ValueError, match="deterministic"):
        check(m=11, banned=[EOS], sampling=True)
    with pytest.raises(ValueError, match="no caption could end"):
        check(m=11, banned=[EOS])


# ------------------------------------------------------------------------------------------------- the mode dispatch
class Recorder:
    """A model that records which search method was called and with what."""

    def __init__(self):
        self.calls = []

    def _record(name):
        def method(self, *a, **k):
            self.calls.append((name, a, k))
            return name
        return method

    beam_search = _record("beam_search")
    diverse_beam_search = _record("diverse_beam_search")
    get_batch_multiple_sampled_prediction = _record("get_batch_multiple_sampled_prediction")
    _search_constraint_args = _record("_search_constraint_args")


DEFAULTS = {
    "beam_search": ("beam_search", dict(sos_idx=-999, eos_idx=-999, beam_size=5, how_many_outputs=1, max_seq_len=20,
                                        sample_or_max="max")),
    "diverse_beam_search": ("diverse_beam_search", dict(sos_idx=-999, eos_idx=-999, num_groups=3, group_size=3,
                                                        diversity_penalty=0.5, how_many_outputs=None, max_seq_len=20)),
    "sampling": ("get_batch_multiple_sampled_prediction", dict(num_outputs=1, sos_idx=-999, eos_idx=-999, max_seq_len=20)),
}
GIVEN = dict(sos_idx=SOS, eos_idx=EOS, beam_size=4, how_many_outputs=2, beam_max_seq_len=9, sample_max_seq_len=7,
             sample_or_max="sample", num_groups=2, group_size=4, diversity_penalty=1.5, no_repeat_ngram_size=2, min_length=3,
             banned_words=[9], something_else=1)
CONS = dict(no_repeat_ngram_size=2, min_length=3, banned_words=[9])
PASSED = {
    "beam_search": dict(sos_idx=SOS, eos_idx=EOS, beam_size=4, how_many_outputs=2, max_seq_len=9, sample_or_max="sample", **CONS),
    "diverse_beam_search": dict(sos_idx=SOS, eos_idx=EOS, num_groups=2, group_size=4, diversity_penalty=1.5,
                                how_many_outputs=2, max_seq_len=9, **CONS),
    "sampling": dict(num_outputs=2, sos_idx=SOS, eos_idx=EOS, max_seq_len=7),
}


@pytest.mark.parametrize("mode", ["beam_search", "diverse_beam_search", "sampling"])
def test_dispatch_passes_the_defaults_and_the_given_keys(mode):
    method, kw = DEFAULTS[mode]
    for args, want in (({}, kw), (GIVEN, PASSED[mode])):
        m = Recorder()
        assert S.dispatch(m, mode, args, "x", [0]) == method
        name, a, k = m.calls[-1]
        assert (name, a, k) == (method, ("x", [0]), want)
        if mode == "sampling":                           # the refusal of constraints comes first, with the same length
            cons = {key: args[key] for key in CONS if key in args}
            assert m.calls[:-1] == [("_search_constraint_args", (), dict(
                cons, sos_idx=want["sos_idx"], eos_idx=want["eos_idx"], max_seq_len=want["max_seq_len"], rows_per_image=1,
                sampling=True))]
        else:
            assert len(m.calls) == 1


def test_dispatch_refuses_an_unknown_mode():
    m = Recorder()
    with pytest.raises(ValueError, match="unknown mode 'greedy'"):
        S.dispatch(m, "greedy", dict(sos_idx=SOS, eos_idx=EOS), "x", [0])
    assert m.calls == []


def model_without_device():
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank="cpu")

    def no_device(*a, **k):
        raise AssertionError("the argument check must come before any call of the model")
    m.forward_enc = m._captioner_engine = m.get_batch_multiple_sampled_prediction = no_device
    return m


def test_the_sampling_mode_refuses_constraint_keys_before_it_calls_the_model():
    from on_device_image_captioning_amd.captioning_model import Captioner
    m = model_without_device()
    for kw in (dict(no_repeat_ngram_size=2), dict(min_length=2), dict(banned_words=[9])):
        args = dict(sos_idx=SOS, eos_idx=EOS, how_many_outputs=2, sample_max_seq_len=12, **kw)
        for call in (lambda: S.dispatch(m, "sampling", args, None, [0]),
                     lambda: m(enc_x=None, enc_x_num_pads=[0], mode="sampling", **args),
                     lambda: Captioner(args, model=m)(None, enc_x_num_pads=[0], mode="sampling")):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == SAMPLING


def test_the_callers_of_the_dispatch_keep_their_own_checks():
    from on_device_image_captioning_amd.captioning_model import Captioner
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel
    rec = Recorder()
    cap = Captioner(dict(sos_idx=SOS, eos_idx=EOS, beam_size=2), model=rec)
    assert cap.apply_log_softmax is False
    assert cap("x", enc_x_num_pads=[0]) == "beam_search" and cap.apply_log_softmax is True
    assert rec.calls == [("beam_search", ("x", [0]), dict(DEFAULTS["beam_search"][1], sos_idx=SOS, eos_idx=EOS, beam_size=2))]
    with pytest.raises(AssertionError):
        Captioner(dict(beam_size=2), model=rec)("x")
    with pytest.raises(KeyError):
        Captioner(dict(sos_idx=SOS), model=rec)("x")
    with pytest.raises(ValueError, match="unknown mode"):
        cap("x", mode="greedy")
    m = model_without_device()
    with pytest.raises(AssertionError):
        m(enc_x=None, mode="beam_search", beam_size=2)
    with pytest.raises(ValueError, match="unknown mode"):
        m(enc_x=None, mode="greedy", sos_idx=SOS, eos_idx=EOS)
    ens = EsembleCaptioningModel([m, m], rank="cpu")
    with pytest.raises(AssertionError, match="only beam search"):
        ens(enc_x=None, mode="sampling", sos_idx=SOS, eos_idx=EOS)
    called = []
    ens.ensemble_beam_search = lambda *a, **k: called.append((a, k)) or "ensemble"
    assert ens(enc_x="x", enc_x_num_pads=[0], sos_idx=SOS, eos_idx=EOS, min_length=2) == "ensemble"
    assert called == [(("x", [0]), dict(DEFAULTS["beam_search"][1], sos_idx=SOS, eos_idx=EOS, min_length=2))]
