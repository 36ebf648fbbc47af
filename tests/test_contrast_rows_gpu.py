"""odic_contrast_topk on the device (`-m gpu`) against the float64 model of tests/contrast_model.py, whose
rows test_contrast_host.py proves clear.  Every operand lives in a guarded buffer (tests/guards.py): logits rows with
ldl > V, score rows with lds > V, compact top_val / top_idx / kept; the distractor rows a row does not use
(d > count[n]) hold NaN, so a read of them — like a read of the padding — would show in the scores.

Measured on an MI355X (this file's report lines): the largest |score_out − model| / bound over every shape and both
settings is 0.23."""
import numpy as np
import pytest
import torch

import contrast_model as CM
from guards import guarded, poisoned_input

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
SHAPES = CM.shapes()
IDS = [f"V{V}-k{k}-M{M}" for V, k, M in SHAPES]
PAD = 5                                        # ldl = V + PAD, lds = V + PAD + 2: odd pitches, never 16-byte rows


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


def device_rows(x: np.ndarray, count: np.ndarray, read_none: bool = False):
    """x fp32 [M, N, V] → M guarded [N, V] inputs of pitch V + PAD; distractor row d of row n is NaN where d > count[n]
    (everywhere with read_none)."""
    M, N, V = x.shape
    out = []
    for d in range(M):
        t = torch.from_numpy(x[d]).clone()
        if d > 0:
            dead = torch.from_numpy((count < d) | read_none)
            t[dead] = float("nan")
        out.append(poisoned_input(t, N, V, V + PAD, device=DEV))
    return out


def launch(ops, rows, count, args, k, want_score=True):
    """One launch in guarded outputs → (top_idx int64 [N, k], top_val [N, k], kept [N], score [N, V] or None) on the CPU."""
    N, V = rows[0].rows, rows[0].cols
    tv = guarded(N, k, k, torch.float32, DEV)
    ti = guarded(N, k, k, torch.int32, DEV)
    kept = guarded(1, N, N, torch.int32, DEV)
    score = guarded(N, V, V + PAD + 2, torch.float32, DEV) if want_score else None
    cnt = poisoned_input(torch.from_numpy(count).view(1, -1), 1, N, N, device=DEV) if len(rows) > 1 else None
    ops.contrast_topk([r.t[:, :V] for r in rows], None if cnt is None else cnt.t.view(-1), args, tv.t, ti.t, k,
                      score_out=None if score is None else score.t[:, :V], kept=kept.t.view(-1))
    torch.cuda.synchronize()
    for g, what in ((tv, "top_val"), (ti, "top_idx"), (kept, "kept"), (score, "score_out")):
        if g is not None:
            g.assert_untouched(what=what)
    return (ti.t.cpu().long(), tv.t.cpu(), kept.t.view(-1).cpu().long(),
            None if score is None else score.t[:, :V].cpu())


# ------------------------------------------------------------------------------------------------ rule 6: off
@pytest.mark.parametrize("V,k,M", SHAPES, ids=IDS)
def test_off_is_logsoftmax_topk_bit_for_bit(ops, V, k, M):
    names, x, count, _ = CM.batch(V, k, M)
    N = len(names)
    X = torch.from_numpy(x[0]).to(DEV)
    tv, ti, lp = torch.empty(N, k, device=DEV), torch.empty(N, k, dtype=torch.int32, device=DEV), torch.empty(N, V, device=DEV)
    ops.logsoftmax_topk(X, V, lp, V, tv, ti, N, V, k)
    # no weight (no distractor row may be read), and a weight with nothing to suppress
    for w, cnt, read_none in ((0.0, count, True), (0.9, np.zeros_like(count), True)):
        rows = device_rows(x, cnt, read_none=read_none)
        gi, gv, kept, score = launch(ops, rows, cnt, ops.contrast_args(w, 0.0, -20.0, k), k)
        assert torch.equal(gi, ti.cpu().long()), w
        assert torch.equal(bits(gv), bits(tv.cpu())), w
        assert torch.equal(bits(score), bits(lp.cpu())), w
        assert kept.tolist() == [V] * N


# ------------------------------------------------------------------------------------------------ rules 1-5
@pytest.mark.parametrize("V,k,M", SHAPES, ids=IDS)
def test_scores_kept_and_top_k_against_the_float64_model(ops, V, k, M):
    names, x, count, refs = CM.batch(V, k, M)
    N = len(names)
    rows = device_rows(x, count)
    for (w, pl, fl, extra), ref in zip(CM.SETTINGS, refs):
        mk = CM.min_keep_of(k, extra, V)
        gi, gv, kept, score = launch(ops, rows, count, ops.contrast_args(w, pl, fl, mk), k)
        sc = score.numpy()
        assert not np.isnan(sc).any() and not np.isnan(gv.numpy()).any()
        # kept, and the admissible set with its min_keep extension, are exact
        assert kept.tolist() == [r["kept"] for r in ref]
        worst, unclear = 0.0, 0
        for n, r in enumerate(ref):
            fin = np.isfinite(r["out"])
            assert np.array_equal(np.isfinite(sc[n]), fin), (names[n], n)
            assert (sc[n][~fin] == -np.inf).all(), (names[n], n)
            if r["kept"] < mk and not np.isinf(x[0, n]).any():
                assert int(fin.sum()) == mk, (names[n], n)                  # the cut left exactly min_keep words
            ratio = np.abs(sc[n][fin].astype(np.float64) - r["out"][fin]) / r["bound"][fin]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (names[n], n, float(ratio.max()))
            # top_val is the score of top_idx, bit for bit, in non-increasing order; no word twice
            idx = gi[n].numpy()
            assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < V
            assert np.array_equal(gv[n].numpy().view(np.int32), sc[n][idx].view(np.int32)), (names[n], n)
            with np.errstate(invalid="ignore"):
                assert not (np.diff(gv[n].numpy().astype(np.float64)) > 0).any(), (names[n], n)
            if r["clear"]:
                assert idx.tolist() == r["top"].tolist(), (names[n], n, count[n])
            else:
                assert names[n] == "dense"
                unclear += 1
            # short rows: the -inf slots are the lowest-indexed -inf words, ascending
            n_fin = int(fin.sum())
            if n_fin < k:
                assert np.isinf(gv[n].numpy()[n_fin:]).all()
                assert idx[n_fin:].tolist() == np.flatnonzero(~fin)[:k - n_fin].tolist(), (names[n], n)
        print(f"contrast_topk V={V} k={k} M={M} w={w} plausibility={pl} floor={fl}: max |score - model| / bound = {worst:.3f}, "
              f"{unclear} unclear dense rows of {CM.N_DENSE}")


def test_the_cut_falls_inside_a_level_and_short_rows_fill_by_index(ops):
    """The two rules that are easiest to get wrong, on rows small enough to read: a min_keep cut through a level of equal
    logits keeps the level's lower indices, and a row with fewer finite words than k lists the masked ones by index."""
    V, k = 17, 3
    x = np.full((2, 2, V), -3.0, dtype=np.float32)
    x[0, 0, [2, 5, 6, 9, 11, 14]] = [9.0, 4.0, 4.0, 4.0, 4.0, 4.0]     # one plausible word, then a level of five
    x[1, 0] = np.linspace(-1, 1, V, dtype=np.float32)
    x[0, 1] = -np.inf
    x[0, 1, [12, 4]] = [1.0, 2.0]                                        # two finite words, k = 3
    x[1, 1] = 0.0
    count = np.array([1, 1], dtype=np.int32)
    gi, gv, kept, score = launch(ops, device_rows(x, count), count, ops.contrast_args(0.5, 0.1, -20.0, 4), k)
    assert kept.tolist() == [1, 2]
    assert np.flatnonzero(np.isfinite(score[0].numpy())).tolist() == [2, 5, 6, 9]
    assert np.flatnonzero(np.isfinite(score[1].numpy())).tolist() == [4, 12]
    assert sorted(gi[1].tolist()[:2]) == [4, 12] and gi[1].tolist()[2] == 0 and gv[1].tolist()[2] == float("-inf")
    ref = CM.reference(x[:, 0], 1, 0.5, CM.log_alpha_of(0.1), -20.0, 4, k)
    assert ref["clear"] and gi[0].tolist() == ref["top"].tolist()


def test_without_score_out_and_kept_the_candidates_are_the_same(ops):
    V, k, M = 259, 3, 8
    names, x, count, _ = CM.batch(V, k, M)
    rows = device_rows(x, count)
    args = ops.contrast_args(0.7, 0.1, -20.0, k + 2)
    gi, gv, _, _ = launch(ops, rows, count, args, k)
    N = len(names)
    tv, ti = guarded(N, k, k, torch.float32, DEV), guarded(N, k, k, torch.int32, DEV)
    ops.contrast_topk([r.t[:, :V] for r in rows], torch.from_numpy(count).to(DEV), args, tv.t, ti.t, k)
    torch.cuda.synchronize()
    tv.assert_untouched(what="top_val")
    ti.assert_untouched(what="top_idx")
    assert torch.equal(ti.t.cpu().long(), gi) and torch.equal(bits(tv.t.cpu()), bits(gv))
