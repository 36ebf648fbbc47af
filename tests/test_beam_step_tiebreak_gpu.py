"""odic_beam_step's tie rule: among equal totals the lowest FLAT candidate index beam·k + rank wins — not (beam, word).

The three selections share one extraction (wave_extract_best, csrc/decoder_ops.hip) and differ in the key that breaks a
tie; the group and required-words keys hold the word, the plain one must not: under sample_or_max='sample' a row's
candidates arrive in draw order, and a finished row's rule (rank 0 worth 0, the others -999) is positional.

n_img = 2, k = 3, T = 6, three steps of ops.beam_step from odic_beam_reset on hand-built candidates (dyadic values, so a
tie is a real tie).  Step 2 of either image has all of: three beams with equal cumulative scores that offer equal
values, a row whose equal-valued candidates carry descending word ids, and one finished beam.  The reference is a numpy
float32 model: total = cumul[beam] + val as one float32 add, a stable arg-sort over the flat index, and the state update
of tests/group_beam_model.py (cumulative score re-summed position by position in float32).  Every field of the state is
compared bitwise after every step.

test_the_inputs_tell_the_flat_index_from_a_beam_word_key (no GPU) confirms that on these inputs a (beam, word)-keyed
order picks differently from the flat index at steps 1 and 2 of both images — at step 2 a different SET of words, not
only another order of the rows — so the comparison can tell the two rules apart.
"""
import numpy as np
import pytest
import torch

import group_beam_model as M

DEV = "cuda:0"
N_IMG, K, T = 2, 3, 6
SOS, EOS = 3, 2
F = np.float32

# per step: rows [image·K + beam] of (values, words), in candidate (rank) order
STEPS = (
    # t = 0, seeding from row 0 of an image: image 0 seeds cumul (-1, -1, -2), image 1 (-2, -2, -2)
    [((-1, -1, -2), (7, 5, 9)), ((0, 0, 0), (20, 21, 22)), ((0, 0, 0), (20, 21, 22)),
     ((-2, -2, -2), (8, 6, 4)), ((0, 0, 0), (20, 21, 22)), ((0, 0, 0), (20, 21, 22))],
    # t = 1: image 0 ties three candidates at -1.5 (beam 0's EOS, beam 1's words 10 then 6); image 1 ties nine at -3
    [((-.5, -1, -1), (EOS, 11, 4)), ((-.5, -.5, -3), (10, 6, 12)), ((-1, -2, -3), (13, 14, 15)),
     ((-1, -1, -1), (EOS, 14, 13)), ((-1, -1, -1), (12, 5, 7)), ((-1, -1.5, -2), (9, 1, 0))],
    # t = 2: beam 0 of either image is finished (rank 0 worth 0); all three beams have one cumulative score and offer 0
    [((-1, -2, -3), (20, 21, 22)), ((0, 0, 0), (9, 8, 4)), ((0, 0, -2), (12, 11, 1)),
     ((-1, -2, -3), (20, 21, 22)), ((0, 0, 0), (7, 5, 1)), ((0, -1, -1), (10, 6, 0))],
)


def candidates():
    return [(np.array([r[0] for r in rows], F), np.array([r[1] for r in rows], np.int32)) for rows in STEPS]


def values(cv, has_eos):
    k = cv.shape[0]
    finished = np.where(np.arange(k)[None, :] == 0, F(0.0), F(-999.0)).astype(F)
    return np.where(np.asarray(has_eos, bool)[:, None], finished, cv.astype(F)).astype(F)


def select(cv, ci, cumul, has_eos, t, key=None):
    """The k picks of an image → (parent, word, lp).  key=None: the stable arg-sort over the flat index; else the order
    (total descending, key(beam, word))."""
    k = cv.shape[0]
    if t == 0:
        return np.zeros(k, np.int32), ci[0, :k].astype(np.int64), cv[0, :k].astype(F)
    val = values(cv, has_eos)
    tot = (cumul.astype(F)[:, None] + val).astype(F).reshape(-1)          # one float32 add
    if key is None:
        pick = np.argsort(-tot, kind="stable")[:k]
    else:
        pick = np.array(sorted(range(k * k), key=lambda i: (-tot[i],) + key(i // k, int(ci.reshape(-1)[i])))[:k])
    return (pick // k).astype(np.int32), ci.reshape(-1)[pick].astype(np.int64), val.reshape(-1)[pick]


def model_run():
    st, trace = M.new_state(N_IMG, K, T, SOS), []
    for cv, ci in candidates():
        st, _ = M.step(st, cv, ci, 1, K, 0.0, EOS, select=select)
        trace.append(st)
    return trace


def test_the_inputs_tell_the_flat_index_from_a_beam_word_key():
    trace = [M.new_state(N_IMG, K, T, SOS)] + model_run()
    for t, (cv, ci) in enumerate(candidates()):
        st = trace[t]
        for b in range(N_IMG):
            rows = slice(b * K, (b + 1) * K)
            args = (cv[rows], ci[rows], st["cumul"][rows], st["has_eos"][rows], t)
            flat, keyed = select(*args), select(*args, key=lambda beam, word: (beam, word))
            same = all(np.array_equal(x, y) for x, y in zip(flat, keyed))
            assert same == (t == 0), (t, b, flat, keyed)
            if t == 2:
                assert sorted(flat[1].tolist()) != sorted(keyed[1].tolist()), (b, flat, keyed)
                assert st["has_eos"][rows].tolist() == [1, 0, 0] and len(set(st["cumul"][rows].tolist())) == 1
    assert not trace[-1]["done"][0]


@pytest.mark.gpu
def test_three_steps_of_beam_step_equal_the_flat_index_model_bitwise():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops
    _hip.load()
    N = N_IMG * K
    spec = (("tokens", torch.int64, N * T), ("logprobs", torch.float32, N * T), ("anc", torch.int32, N * T),
            ("cumul", torch.float32, N), ("n_elem", torch.int32, N), ("has_eos", torch.int32, N),
            ("row_valid", torch.int32, N), ("next_tok", torch.int64, N), ("pos", torch.int32, 1), ("done", torch.int32, 1),
            ("ctr", torch.int32, 1))
    dev = {name: torch.zeros(n, dtype=dt, device=DEV) for name, dt, n in spec}
    state = _hip.BeamState(*(dev[name].data_ptr() for name, _, _ in spec))
    ops.beam_reset(state, N_IMG, K, T, SOS)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a      # noqa: E731
    for t, ((cv, ci), want) in enumerate(zip(candidates(), model_run())):
        ops.beam_step(torch.from_numpy(cv).to(DEV), torch.from_numpy(ci).to(DEV), state, N_IMG, K, T, EOS)
        torch.cuda.synchronize()
        for name in M.STATE_KEYS:
            got, ref = dev[name].cpu().numpy(), np.ascontiguousarray(want[name].reshape(-1))
            assert np.array_equal(bits(got), bits(ref)), f"step {t}: {name}\n{got}\n{ref}"
        assert int(dev["ctr"]) == 0, f"step {t}: the arrival counter is re-armed"
