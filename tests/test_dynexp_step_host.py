"""The data behind test_dynexp_step_gpu.py, checked without a GPU: the float64 step model agrees with the oracle on
materialised histories (which pins the reading of `anc`), and every case reaches the branches of the kernel it claims to
reach, at a step where the result is compared."""
import numpy as np
import pytest
import torch

import dynexp_step_model as M

torch.set_grad_enabled(False)


# ---------------------------------------------------------------------------------------------------------------------
# The shape-dependent branches of the step.  These formulas MIRROR dynexp_step_kernel and odic_dynexp_step in
# on_device_image_captioning_amd/csrc/decoder_ops.hip (block of 1024 threads): if the kernel changes how it splits its
# work, change them with it and look at the cases again — they were chosen against these numbers.
NT = 1024                # threads per block
MAX_E = 32
LDS_LIMIT = 64 * 1024


def lanes_per_key(t):
    """Lanes that share one key position in the ca / cb sums: the largest power of two <= 32 with (t+1)·LP <= 1024."""
    lp = 4
    while lp < 32 and (t + 1) * lp * 2 <= NT:
        lp *= 2
    return lp


def item_trips(t, E):
    """Trips of the dot-product loop: E + 2t + 1 items, one per 16-lane group, 64 groups."""
    return -(-(E + 2 * t + 1) // (NT // 16))


def weight_trips(t, E):
    """Trips of the strided loops over the (t+1)·E weights (the one over the t·E cached products is one shorter at most)."""
    return -(-((t + 1) * E) // NT)


def history_trips(t, E):
    return -(-(t * E) // NT)


def channel_passes(d):
    """Phase 2 handles NT/2 channels per pass, with block-wide barriers inside the loop."""
    half = NT // 2
    passes = -(-d // half)
    return passes, d - (passes - 1) * half


def shared_bytes(T, d, E):
    floats = 2 * d + 2 * T + 3 * MAX_E + 16 + 3 * T * E + 4 * T + 2 * E + NT
    return floats * 4 + T * 4


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.MODEL_CASES, ids=lambda c: c.name)
def test_step_model_agrees_with_the_oracle(case):
    """Cached form, gathered through anc, against the full recompute on materialised histories: 1e-12 of the output scale,
    float64 both (measured: a few 1e-16)."""
    plan = case.plan()
    assert any(M.step_kind(plan, t, b) != "identity" for t in range(1, case.T - 1) for b in range(case.n_img))
    sd, x, y_in = M.inputs(case)
    sd64 = {k: v.double() for k, v in sd.items()}
    x64, y64 = x.double(), y_in.double()
    lin = M.linear_rows(sd64, x64)                                            # [N, T, 5d]
    caches = M.new_caches(case.T, case.N, case.d, case.E)
    qe, be = sd64["p.query_exp_vectors.weight"], sd64["p.bias_exp_vectors.weight"]
    worst = 0.0
    for t in range(case.T):
        y = M.step_model(lin[:, t], qe, be, caches, plan.anc[t], plan.valid[t], t, y64[t])
        want = M.oracle_rows(sd64, x64, plan, t) * torch.from_numpy(plan.valid[t]).double()[:, None]
        assert bool(torch.isfinite(y).all()), f"step {t}: the model read a cache entry that was never written"
        dead = plan.valid[t] == 0
        assert torch.equal(y[dead], y64[t][dead])
        err = float((y - y64[t] - want).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, f"step {t}: {err:.3e}"
    print(f"{case.name}: worst relative error {worst:.3e}")
    assert int((plan.valid == 0).sum()) > 0, "no padded row in the case"


@pytest.mark.parametrize("case", M.CASES + M.MODEL_CASES, ids=lambda c: c.name)
def test_plan_is_a_search(case):
    """The ancestry tables follow the update of odic_beam_step, parents stay inside their image, a padded row has only
    padded descendants, and every kind of step occurs."""
    plan, T, k = case.plan(), case.T, case.beams
    assert (plan.valid[0] == 1).all() and (plan.anc[0] == M.SENTINEL).all()
    for t in range(T - 1):
        for n in range(case.N):
            q = int(plan.par[t, n])
            assert q // k == n // k
            assert (plan.anc[t + 1, n, :t] == plan.anc[t, q, :t]).all() and plan.anc[t + 1, n, t] == q
            assert (plan.anc[t + 1, n, t + 1:] == M.SENTINEL).all()
            if not plan.valid[t, q]:
                assert not plan.valid[t + 1, n]
    kinds = {M.step_kind(plan, t, b) for t in range(T - 1) for b in range(case.n_img)}
    want = {"identity", "permutation", "collapse"} | ({"duplication"} if k > 2 else set())    # (two beams: the same thing)
    assert want <= kinds, kinds
    # a beam finishes before T/2 in some image, and every image keeps a beam that never does
    assert any(t + 1 < T / 2 for t, _ in plan.finished)
    for b in range(case.n_img):
        assert plan.valid[:, b * k:(b + 1) * k].max(axis=1).all()


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_case_reaches_what_it_claims(case):
    plan, T, E, d, steps = case.plan(), case.T, case.E, case.d, case.steps
    assert steps == sorted(set(steps)) and steps[0] == 0 and steps[-1] == T - 1
    if T <= 40:
        assert steps == list(range(T))
    # lanes per key position: every class of the case at a checked step, both sides of each boundary checked
    assert {lanes_per_key(t) for t in range(T)} == set(case.lanes) == {lanes_per_key(t) for t in steps}
    for tp1 in case.boundaries:
        assert tp1 - 1 in steps
    for lo, hi in ((32, 33), (64, 65)):
        if T >= hi:
            assert lo in case.boundaries and hi in case.boundaries
            assert lanes_per_key(lo - 1) == 2 * lanes_per_key(hi - 1)
    # loop trip counts
    assert max(item_trips(t, E) for t in steps) == case.item_trips == item_trips(T - 1, E)
    assert max(weight_trips(t, E) for t in steps) == case.weight_trips == weight_trips(T - 1, E)
    assert max(history_trips(t, E) for t in steps) == case.weight_trips
    if case.weight_trips > 1:        # the steps on both sides of the first second trip are compared
        first = min(t for t in range(T) if weight_trips(t, E) > 1)
        assert first in steps and first - 1 in steps and first + 1 in steps and history_trips(first + 1, E) > 1
    assert channel_passes(d) == (case.channel_passes, case.last_pass_channels)
    # the split between the two halves of phase 2, jm = (t+1)/2: odd and even t, beyond the first lane class
    deep = [t for t in steps if t >= min(T - 2, 33)]
    assert {t % 2 for t in deep} == {0, 1}
    # re-ordering: slot[j] != n at more than half of the compared (n, j) pairs
    pairs = other = 0
    for t in steps:
        a = plan.anc[t][:, :t]
        pairs += a.size
        other += int((a != np.arange(case.N)[:, None]).sum())
    assert 2 * other > pairs, (other, pairs)
    # a padded row, a duplication and a collapse in front of a compared step (so that a compared history contains them)
    assert any((plan.valid[t] == 0).any() for t in steps)
    last = steps[-1]
    kinds = {M.step_kind(plan, t, b) for t in range(1, last) for b in range(case.n_img)}
    assert "collapse" in kinds and ("duplication" in kinds or case.beams == 2)


def test_shared_memory_formula():
    """Every case fits the 64 KB of LDS a block may ask for; the refused one does not, by less than one row of anything."""
    for c in M.CASES:
        assert shared_bytes(c.T, c.d, c.E) <= LDS_LIMIT, c.name
    big = max(M.CASES, key=lambda c: shared_bytes(c.T, c.d, c.E))
    assert big.name == "largest_lds" and shared_bytes(big.T, big.d, big.E) > 56 * 1024
    r = M.REFUSED
    assert LDS_LIMIT < shared_bytes(r["T"], r["d"], r["E"]) <= LDS_LIMIT + 4 * r["d"]
    assert r["T"] <= 128 and r["E"] in (4, 8, 16, 32) and r["d"] % 64 == 0          # refused for its size alone
