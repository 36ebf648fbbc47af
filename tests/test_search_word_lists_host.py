"""“One word list for all images, or one per image” without a GPU: what search.check_prefix, check_required_words,
refuse_required_words and the prefix refusals of check_stochastic_beam / check_contrast make of every form a caller may
give — None, empty, flat, nested, tensors, ragged, a wrong count, a 0-d tensor among the ids.  The expected outcomes are
literals: what the five functions returned or raised (exception type and full message) before they shared one reader
(search.per_image_word_lists) and the prefix refusals one predicate (search.names_a_word); the shared code must reproduce
every one.  And the candidate log (search.logged): nothing without a list, one tuple per step of each search's arity with one.
"""
import types

import pytest
import torch

from on_device_image_captioning_amd import search as S

SOS, EOS = 3, 2
T = torch.tensor

# name → (the value, made anew for every call; the number of images)
INPUTS = {
    "none": (lambda: None, 2),
    "empty list": (lambda: [], 2),
    "empty tuple": (lambda: (), 2),
    "empty lists": (lambda: [[], []], 2),
    "flat list": (lambda: [5, 6], 2),
    "flat tuple": (lambda: (5, 6), 2),
    "flat list, 3 images": (lambda: [5, 6], 3),
    "tensor 1-D": (lambda: T([5, 6]), 2),
    "tensor 2-D": (lambda: T([[5, 6], [7, 8]]), 2),
    "tensor 2-D, no columns": (lambda: torch.zeros(2, 0, dtype=torch.int64), 2),
    "list of tensors": (lambda: [T([5, 6]), T([7, 8])], 2),
    "list of tuples": (lambda: [(5, 6), (7, 8)], 2),
    "tuple of lists": (lambda: ([5, 6], [7, 8]), 2),
    "ragged": (lambda: [[5], [6, 7]], 2),
    "ragged, one empty": (lambda: [[], [5]], 2),
    "2 lists for 3 images": (lambda: [[5], [6]], 3),
    "2 empty lists for 3 images": (lambda: [[], []], 3),
    "tensor 2-D, 2 rows for 3 images": (lambda: T([[5, 6], [7, 8]]), 3),
    "scalar tensor elements": (lambda: [T(5), T(6)], 2),
    "id and scalar tensor": (lambda: [5, T(6)], 2),
    "list and id mixed": (lambda: [[5], 6], 2),
}

CALLS = {
    "check_prefix": lambda v, n: S.check_prefix(v, n, V=500, max_seq_len=12, sos_idx=SOS, eos_idx=EOS),
    "check_required_words": lambda v, n: S.check_required_words(v, n, V=500, beam_size=2, banned=None, sos_idx=SOS,
                                                                eos_idx=EOS, max_seq_len=12),
    "refuse_required_words": lambda v, n: S.refuse_required_words(v, "in diverse_beam_search"),
    "check_stochastic_beam": lambda v, n: S.check_stochastic_beam(4, prefix=v),
    "check_contrast": lambda v, n: S.check_contrast(None, n, prefix=v)["D"],
}

REFUSED = ("ValueError", "required_words is not supported in diverse_beam_search: use beam_search on one model, without a prefix")
NO_PREFIX_S = ("ValueError", "prefix is not supported in stochastic_beam_search: it samples captions from the model's own "
                             "distribution")
NO_PREFIX_C = ("ValueError", "prefix is not supported in contrastive_beam_search: it ranks the words of one deterministic "
                             "beam search by a contrast between images")
ONE_LENGTH = ("ValueError", "the prefixes of a batch must have one length (the position is one device scalar)")
COUNT_P = ("ValueError", "2 prefixes for 3 images: give one for all, or one per image")
COUNT_R = ("ValueError", "2 lists of required words for 3 images: give one for all, or one per image")
NOT_ITERABLE = ("TypeError", "'int' object is not iterable")
LEN_0D = ("TypeError", "len() of a 0-d tensor")
INT_OF_LIST = ("TypeError", "int() argument must be a string, a bytes-like object or a real number, not 'list'")


def outcomes(prefix, required, refused=None):
    """A row of the table: check_prefix's and check_required_words' outcome; the three refusals accept (`refused` None:
    refuse_required_words → None, check_stochastic_beam → its num_samples 4, check_contrast → D = 0), refuse with their
    messages (True), or are given one by one."""
    if refused is None:
        refused = (None, 4, 0)
    elif refused is True:
        refused = (REFUSED, NO_PREFIX_S, NO_PREFIX_C)
    return dict(zip(CALLS, (prefix, required) + tuple(refused)))


# what the parent commit's five functions gave, each run on its own on the CPU.  Where they disagree on a corner input
# every caller keeps its outcome:
#  * two empty lists for three images name no word, so the refusals accept them; the two checks count the lists first;
#  * a 0-d tensor where a list of ids is expected is a TypeError everywhere, worded by whichever expression met it:
#    the readers that unpack an element with tolist() iterate an int, the prefix refusals take len() of the tensor;
#  * [5, tensor(6)] is a flat list of two ids for the checks (int() takes a 0-d tensor); refuse_required_words unpacks
#    every element before it looks and fails on the tensor, the prefix refusals stop at the first word, 5, and refuse;
#  * [[5], 6] is neither flat nor nested: the checks fail on int([5]), the refusals see a word and refuse.
EXPECTED = {
    "none": outcomes(None, None),
    "empty list": outcomes(None, None),
    "empty tuple": outcomes(None, None),
    "empty lists": outcomes(None, None),
    "flat list": outcomes([[5, 6], [5, 6]], [[5, 6], [5, 6]], True),
    "flat tuple": outcomes([[5, 6], [5, 6]], [[5, 6], [5, 6]], True),
    "flat list, 3 images": outcomes([[5, 6], [5, 6], [5, 6]], [[5, 6], [5, 6], [5, 6]], True),
    "tensor 1-D": outcomes([[5, 6], [5, 6]], [[5, 6], [5, 6]], True),
    "tensor 2-D": outcomes([[5, 6], [7, 8]], [[5, 6], [7, 8]], True),
    "tensor 2-D, no columns": outcomes(None, None),
    "list of tensors": outcomes([[5, 6], [7, 8]], [[5, 6], [7, 8]], True),
    "list of tuples": outcomes([[5, 6], [7, 8]], [[5, 6], [7, 8]], True),
    "tuple of lists": outcomes([[5, 6], [7, 8]], [[5, 6], [7, 8]], True),
    "ragged": outcomes(ONE_LENGTH, [[5, -1], [6, 7]], True),
    "ragged, one empty": outcomes(ONE_LENGTH, [[-1], [5]], True),
    "2 lists for 3 images": outcomes(COUNT_P, COUNT_R, True),
    "2 empty lists for 3 images": outcomes(COUNT_P, COUNT_R),
    "tensor 2-D, 2 rows for 3 images": outcomes(COUNT_P, COUNT_R, True),
    "scalar tensor elements": outcomes(NOT_ITERABLE, NOT_ITERABLE, (NOT_ITERABLE, LEN_0D, LEN_0D)),
    "id and scalar tensor": outcomes([[5, 6], [5, 6]], [[5, 6], [5, 6]], (NOT_ITERABLE, NO_PREFIX_S, NO_PREFIX_C)),
    "list and id mixed": outcomes(INT_OF_LIST, INT_OF_LIST, True),
}


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name", INPUTS)
def test_every_reader_keeps_its_outcome_on_every_form(name, call):
    make, n_img = INPUTS[name]
    try:
        got = CALLS[call](make(), n_img)
    except Exception as e:      # noqa: BLE001  (the table holds the type and the message of whatever is raised)
        got = (type(e).__name__, str(e))
    assert got == EXPECTED[name][call]


def test_the_table_covers_every_input_and_every_reader():
    assert set(EXPECTED) == set(INPUTS) and all(set(row) == set(CALLS) for row in EXPECTED.values())


def test_the_reader_hands_out_lists_of_its_own():
    given = [[5, 6], [7, 8]]
    rows = S.per_image_word_lists(given, 2, "prefixes")
    assert rows == given and all(r is not g for r, g in zip(rows, given))
    flat = S.per_image_word_lists([5, 6], 3, "prefixes")
    assert flat == [[5, 6]] * 3 and flat[0] is not flat[1]
    assert S.per_image_word_lists(None, 2, "prefixes") is None and S.per_image_word_lists([], 2, "prefixes") == [[], []]
    with pytest.raises(ValueError) as e:
        S.per_image_word_lists([[5]], 2, "lists of nouns")
    assert str(e.value) == "1 lists of nouns for 2 images: give one for all, or one per image"


def test_the_sampling_refusals_stay_behind_the_reader():
    """Nothing named: nothing to refuse, also when drawing; something named: the refusal, before the other rules."""
    kw_p = dict(V=500, max_seq_len=12, sos_idx=SOS, eos_idx=EOS, sampling=True)
    kw_r = dict(V=500, beam_size=2, banned=None, sos_idx=SOS, eos_idx=EOS, max_seq_len=12, sampling=True)
    assert S.check_prefix([[], []], 2, **kw_p) is None and S.check_required_words([[], []], 2, **kw_r) is None
    with pytest.raises(ValueError, match="prefix applies to the deterministic searches only"):
        S.check_prefix([SOS] * 40, 2, **kw_p)
    with pytest.raises(ValueError, match="required_words applies to the deterministic beam search only"):
        S.check_required_words([SOS] * 40, 2, **kw_r)


# ------------------------------------------------------------------------------------------------- the candidate log
def stand_in_state():
    """cand_val / cand_idx / cand_pert that every step overwrites in place, as the device does."""
    return types.SimpleNamespace(cand_val=torch.zeros(2, 3), cand_idx=torch.zeros(2, 3, dtype=torch.int32),
                                 cand_pert=torch.zeros(2, 3))


def stepper(st, ran):
    def step(cons):
        ran.append(cons)
        st.cand_val.fill_(len(ran))
        st.cand_idx.fill_(10 * len(ran))
        st.cand_pert.fill_(-len(ran))
    return step


def test_without_a_list_the_step_runs_as_it_is_and_nothing_is_copied():
    st, ran = stand_in_state(), []
    step = stepper(st, ran)
    assert S.logged(step, st, None) is step              # the step itself: nothing of the state can be read or copied
    assert S.logged(step, None, None, extra=lambda: 1 / 0) is step
    S.logged(step, st, None)("cons")
    assert ran == ["cons"]


# the tuples of the searches: plain, diverse and contrastive log the candidates; required words their log-probs per row
# as well, stochastic beam the candidates' perturbed scores
ARITY = {"plain": None, "required_words": "req_logp", "stochastic": "cand_pert"}


@pytest.mark.parametrize("flavour", ARITY)
def test_with_a_list_every_step_appends_one_tuple_of_the_search_s_arity(flavour):
    st, ran, log = stand_in_state(), [], []
    extra = {None: None, "req_logp": lambda: st.cand_val[:, :1] * 2,
             "cand_pert": lambda: st.cand_pert.cpu().clone()}[ARITY[flavour]]
    step = S.logged(stepper(st, ran), st, log, extra)
    for t in range(3):
        step(None if t else "cons")
        assert len(log) == t + 1                         # once per step, after the step
    assert ran == ["cons", None, None]                   # the step gets what run_search hands it
    for t, rec in enumerate(log, start=1):               # host copies: later steps did not change the earlier tuples
        assert len(rec) == (2 if extra is None else 3)
        assert torch.equal(rec[0], torch.full((2, 3), float(t))) and rec[0] is not st.cand_val
        assert torch.equal(rec[1], torch.full((2, 3), 10 * t, dtype=torch.int32)) and rec[1] is not st.cand_idx
    if flavour == "required_words":
        assert [float(rec[2][0, 0]) for rec in log] == [2.0, 4.0, 6.0]
    if flavour == "stochastic":
        assert [float(rec[2][0, 0]) for rec in log] == [-1.0, -2.0, -3.0]
