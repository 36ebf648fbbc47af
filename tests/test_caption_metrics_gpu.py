"""BLEU and ROUGE-L on the device (`-m gpu`): odic_bleu_stats and odic_lcs_pairs against the plain model of
tests/caption_metrics_model.py — integers, so equality — on the reference's recorded corpus
(tests/golden/caption_metrics.json) and on hand-made rows; containment of both launches (tests/guards.py); metrics.bleu,
metrics.rouge_l, evaluation.coco_scores and consensus_rerank(metric=) against the reference scorers' recorded scores within
cider_device_model.TOL = 1e-10; consensus_caption(metric=) end to end on the TINY synthetic checkpoint.

Every shape is the smallest at which the kernels can still go wrong: the lengths at which an n-gram order appears (0..4), the
64-bit word boundary of the LCS state (63, 64, 65) and the limits (127, 128), one query up to several blocks of waves with a
ragged last block."""
import json
import os

import numpy as np
import pytest
import torch

import caption_metrics_model as M
import guards
from cider_device_model import TOL
from conftest import cached_state_dict
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 65533
GARBAGE = 70000                      # what the token slots behind a caption's end hold: never read
UNSET = -7                           # what an output holds before the launch


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "caption_metrics.json")) as f:
        return json.load(f)


def upload(caps, width=None):
    width = max(1, max(len(c) for c in caps)) if width is None else width
    tok = np.full((len(caps), width), GARBAGE, dtype=np.int32)
    for i, c in enumerate(caps):
        tok[i, :len(c)] = c
    return torch.from_numpy(tok).to(DEV), torch.tensor([len(c) for c in caps], dtype=torch.int32, device=DEV)


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def model_query(caps, h, b, e):
    """What odic_bleu_stats documents for the query (h, [b, e)) on the rows `caps`."""
    if not 0 <= h < len(caps):
        return [0] * M.STAT_WORDS
    return M.bleu_stats(caps[h], [caps[j] for j in range(max(b, 0), min(e, len(caps)))])


def run_stats(ops, caps, queries, width=None):
    """→ (stats [Q, 12] from the device, the model's), the launch made twice and compared bit for bit."""
    tok, lens = upload(caps, width)
    ws = ops.cider_workspace(len(caps), DEV)
    ws.fill_(-1)
    ops.cider_vectorize(tok, lens, ws, default_idf=1.0)
    hyp, begin, end = (i32([q[k] for q in queries]) for k in range(3))
    stats = torch.full((len(queries), M.STAT_WORDS), UNSET, dtype=torch.int32, device=DEV)
    ops.bleu_stats(ws, lens, tok.shape[1], hyp, begin, end, stats)
    again = torch.full_like(stats, UNSET)
    ops.bleu_stats(ws, lens, tok.shape[1], hyp, begin, end, again)
    assert torch.equal(stats, again), "two runs differ"
    return stats.cpu().numpy(), np.array([model_query(caps, *q) for q in queries])


def golden_rows(golden):
    """(rows: the candidates, then every image's references; begin, end: each candidate's reference rows)"""
    rows = [list(c) for c in golden["candidates"]]
    begin, end = [], []
    for refs in golden["references"]:
        begin.append(len(rows))
        rows += [list(r) for r in refs]
        end.append(len(rows))
    return rows, begin, end


# ------------------------------------------------------------------------------------------------------------ bleu stats
def test_bleu_stats_equal_the_reference_scorer_on_the_golden_corpus(ops, golden):
    rows, begin, end = golden_rows(golden)
    H = len(golden["candidates"])
    got, want = run_stats(ops, rows, [(h, begin[h], end[h]) for h in range(H)])
    assert np.array_equal(got, want)
    g = golden["bleu"]
    assert got[:, 0:4].tolist() == g["correct"] and got[:, 4:8].tolist() == g["guess"]
    assert got[:, 8].tolist() == g["testlen"] and got[:, 9].tolist() == g["reflen"]
    assert H % 4, "a ragged last block of waves"


def test_bleu_stats_equal_the_model_on_hand_made_rows(ops):
    rng = np.random.default_rng(21)
    a = 9
    long_h, long_r = [int(v) for v in rng.integers(0, 5, 128)], [int(v) for v in rng.integers(0, 5, 128)]
    edge = [0, BIG, BIG, BIG, 0, 0, BIG, 0, BIG, BIG, BIG, BIG, 0, 0, 0, 0]        # bit 63 set: the order is unsigned
    caps = [[], [5], [5, 6], [5, 6, 7], [5, 6, 7, 8],                              # 0-4: the orders vanish one by one
            [5, 6, 7, 8, 5, 6, 7, 8, 9],                                           # 5: their reference
            long_h, long_r, long_h[:127],                                          # 6-8: the length limit
            edge, edge[1:] + [0], [BIG] * 4, [0] * 4, [32766, 32767, 32766, 32767, 0, BIG],    # 9-13
            [a] * 5, [a, a, 7], [a, a, a],                                         # 14-16: clipped at the maximum, 3
            [1, 2, 3, 4, 5], [1, 2, 3, 9], [1, 2, 3, 4, 9, 9],                     # 17-19: lengths 4 and 6 around 5
            [1, 2, 3, 4, 9, 9], [1, 2, 9, 4]]                                      # 20-21: the tie the other way round
    R = len(caps)
    queries = [(h, 5, 6) for h in range(5)] + [(5, h, h + 1) for h in range(5)]
    queries += [(6, 7, 9), (7, 6, 7), (8, 6, 9), (6, 6, 7)]
    queries += [(9, 10, 14), (10, 9, 10), (11, 9, 14), (12, 9, 14), (13, 9, 13)]
    queries += [(14, 15, 17), (14, 15, 16), (14, 16, 17), (17, 18, 20), (17, 20, 22), (17, 19, 22)]
    queries += [(17, 18, 18), (17, 19, 18), (3, 0, R)]                             # empty ranges; every row a reference
    queries += [(5, 0, 5)] * 3                                                     # one hypothesis row shared by queries
    queries += [(-1, 5, 6), (R, 5, 6), (3, -4, 2), (3, R - 1, R + 9), (3, R, R + 2), (3, -9, -2)]     # rows that do not exist
    assert len(queries) % 4
    got, want = run_stats(ops, caps, queries, width=128)
    assert np.array_equal(got, want), np.argwhere(got != want)
    at = {q: i for i, q in enumerate(queries)}
    assert got[at[(14, 15, 17)], 0] == 3 and got[at[(14, 15, 16)], 0] == 2         # the maximum over the references, not 5
    assert got[at[(17, 18, 20)], 9] == 4 and got[at[(17, 20, 22)], 9] == 4         # a tie goes to the shorter reference
    assert got[at[(17, 18, 18)]].tolist() == [0, 0, 0, 0, 5, 4, 3, 2, 5, 0, 0, 0]
    assert got[at[(-1, 5, 6)]].tolist() == [0] * 12 and got[at[(R, 5, 6)]].tolist() == [0] * 12
    assert got[at[(6, 6, 7)]].tolist() == [128, 127, 126, 125, 128, 127, 126, 125, 128, 128, 128, 128]
    assert got[at[(0, 5, 6)]].tolist() == [0] * 9 + [9, 9, 9]
    assert got[at[(11, 9, 14)], :4].tolist() == [4, 3, 2, 1]                       # BIG BIG BIG BIG is inside `edge`


def test_bleu_stats_in_the_pairwise_layout(ops):
    """N·N single-reference queries per image: every candidate against every candidate of its image."""
    rng = np.random.default_rng(22)
    B, N = 3, 5
    caps = [[int(v) for v in rng.integers(0, 4, rng.integers(1, 9))] for _ in range(B * N)]
    caps[7] = list(caps[5])
    queries = [(b * N + i, b * N + j, b * N + j + 1) for b in range(B) for i in range(N) for j in range(N)]
    got, want = run_stats(ops, caps, queries)
    assert np.array_equal(got, want)
    assert np.array_equal(got[queries.index((5, 7, 8)), :4], got[queries.index((5, 5, 6)), :4])


# -------------------------------------------------------------------------------------------------------------------- lcs
def run_lcs(ops, caps, begin, end, H, max_refs, width=None):
    tok, lens = upload(caps, width)
    out = torch.full((H, max_refs), UNSET, dtype=torch.int32, device=DEV)
    ops.lcs_pairs(tok, lens, i32(begin), i32(end), out)
    again = torch.full_like(out, UNSET)
    ops.lcs_pairs(tok, lens, i32(begin), i32(end), again)
    assert torch.equal(out, again), "two runs differ"
    want = np.zeros((H, max_refs), dtype=np.int64)
    for h in range(H):
        for s in range(max_refs):
            j = begin[h] + s
            if 0 <= j < len(caps) and j < end[h]:
                want[h, s] = M.lcs(caps[h], caps[j])
    return out.cpu().numpy(), want


def test_lcs_equals_the_reference_on_the_golden_corpus(ops, golden):
    rows, begin, end = golden_rows(golden)
    H = len(golden["candidates"])
    got, want = run_lcs(ops, rows, begin, end, H, 5)
    assert np.array_equal(got, want)
    for h, per in enumerate(golden["rouge"]["lcs"]):
        assert got[h, :len(per)].tolist() == per and np.all(got[h, len(per):] == 0)
    assert (H * 5) % 4


def test_lcs_equals_the_model_across_the_word_boundary(ops):
    rng = np.random.default_rng(23)
    lengths = [0, 1, 63, 64, 65, 127, 128]
    caps = [[int(v) for v in rng.integers(0, 3, n)] for n in lengths]                       # the hypotheses
    caps += [[int(v) for v in rng.integers(0, 3, n)] for n in lengths]                      # the references
    H = len(lengths)
    got, want = run_lcs(ops, caps, [H] * H, [2 * H] * H, H, H, width=128)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert np.all(got[0] == 0) and np.all(got[:, 0] == 0)                                   # either side empty
    assert got[6, 6] > 64 and got[6, 1] == 1 and got[1, 6] == 1


def test_lcs_on_hand_made_rows(ops):
    rng = np.random.default_rng(24)
    full = [int(v) for v in rng.integers(0, 1000, 128)]
    odd = [-5, 2 ** 31 - 1, -2 ** 31, 70000, 65534, -1, 0, 70000, -5]                       # no key, no id limit
    caps = [full, [1] * 128, [1] * 65, [2, 3, 2, 3] * 20, odd, [4, 5, 6], [7, 8, 9, 7, 8, 9, 7, 8, 9, 7],      # hypotheses
            list(full), [1] * 65, [1] * 128, [1] * 64, [4, 5] * 30, odd[::-1], odd[2:7], [0, 1, 7, 2, 9, 3, 4, 8, 5, 6, 9],
            [9, 8, 7]]
    H = 7
    begin = [7, 8, 8, 8, 12, 14, 14]
    end = [8, 11, 11, 12, 14, 16, 16]
    got, want = run_lcs(ops, caps, begin, end, H, 4)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert got[0].tolist() == [128, 0, 0, 0]                                    # identical rows of 128
    assert got[1].tolist() == [65, 128, 64, 0] and got[2].tolist() == [65, 65, 64, 0]       # the carry crosses the words
    assert got[3].tolist() == [0, 0, 0, 0]                                      # disjoint alphabets, a 4th slot in use
    assert got[4].tolist() == [M.lcs(odd, odd[::-1]), 5, 0, 0]
    assert got[5].tolist() == [3, 0, 0, 0] and got[6].tolist() == [4, 3, 0, 0]  # shorter than its reference, and longer
    # a reference count above max_refs is cut, rows outside [0, R) are skipped
    got, want = run_lcs(ops, caps, [7, len(caps) - 1, -1], [16, len(caps) + 5, 2], 3, 2)
    assert np.array_equal(got, want) and got[1, 1] == 0 and got[2, 0] == 0 and got[2, 1] == M.lcs(caps[2], caps[0])


# ------------------------------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize("shape", ["one query", "ragged"])
def test_bleu_stats_stay_inside_their_operands(ops, shape):
    rng = np.random.default_rng(25)
    if shape == "one query":
        caps, queries = [[int(v) for v in rng.integers(0, BIG + 1, 128)]], [(0, 0, 1)]
    else:
        caps = [[int(v) for v in rng.integers(0, 4, n)] for n in (9, 128, 0, 4, 1, 127, 30, 2, 3)]
        queries = [(0, 5, 9), (1, 5, 6), (2, 6, 6), (3, 0, 9), (4, 7, 12), (8, 0, 3), (9, 0, 3)]
    R, Q, width = len(caps), len(queries), max(len(c) for c in caps)
    tok, lens = upload(caps)
    words = 2 * 512 + 5
    g_ws = guards.guarded(R, words, words + 3, torch.int64, DEV)
    ws = g_ws.t[:, :words]
    g_len = guards.poisoned_input(lens[None, :], 1, R, R + 1)
    ops.cider_vectorize(tok, g_len.t[0, :R], ws, default_idf=1.0)
    before = g_ws.raw.clone()
    g_q = [guards.poisoned_input(i32([[q[k] for q in queries]]), 1, Q, Q + 1) for k in range(3)]
    g_out = guards.guarded(Q, M.STAT_WORDS, M.STAT_WORDS + 3, torch.int32, DEV)
    # (lengths is handed over whole: the wrapper wants one length per workspace row, and the view is contiguous)
    ops.bleu_stats(ws, g_len.t[0, :R], width, g_q[0].t[0, :Q], g_q[1].t[0, :Q], g_q[2].t[0, :Q], g_out.t[:, :M.STAT_WORDS])
    g_out.assert_untouched(what="stats output")
    assert torch.equal(before, g_ws.raw), "the workspace is an input"
    want = np.array([model_query(caps, *q) for q in queries])
    assert np.array_equal(g_out.t[:, :M.STAT_WORDS].cpu().numpy(), want)


@pytest.mark.parametrize("shape", ["one pair", "ragged"])
def test_lcs_pairs_stay_inside_their_operands(ops, shape):
    """The rows use -1 as a word: a read behind a row's length (the padding is 0xFF bytes, -1) would lengthen the match."""
    rng = np.random.default_rng(26)
    if shape == "one pair":
        caps, begin, end, H, max_refs = [[-1] * 100 + [5] * 28, [-1] * 128], [1], [2], 1, 1
    else:
        caps = [[int(v) for v in rng.choice([-1, 5], n)] for n in (9, 64, 0, 65, 1, 127, 30, 2, 63)]
        begin, end, H, max_refs = [5, 5, 6, 9, 0], [9, 6, 6, 12, 5], 5, 5      # 4, 1, 0, 0 and 5 references
    R, width = len(caps), max(len(c) for c in caps)
    tok, lens = upload(caps)
    g_tok = guards.poisoned_input(tok, R, width, width + 3)
    g_len = guards.poisoned_input(lens[None, :], 1, R, R + 1)
    g_b = guards.poisoned_input(i32([begin]), 1, H, H + 1)
    g_e = guards.poisoned_input(i32([end]), 1, H, H + 1)
    g_out = guards.guarded(H, max_refs, max_refs + 2, torch.int32, DEV)
    # the rows are uploaded with GARBAGE behind their ends; put the poison there too, as behind the row
    for r, c in enumerate(caps):
        g_tok.t[r, len(c):width] = -1
    ops.lcs_pairs(g_tok.t[:, :width], g_len.t[0, :R], g_b.t[0, :H], g_e.t[0, :H], g_out.t[:, :max_refs])
    g_out.assert_untouched(what="lcs output")
    got = g_out.t[:, :max_refs].cpu().numpy()
    for h in range(H):
        for s in range(max_refs):
            j = begin[h] + s
            assert got[h, s] == (M.lcs(caps[h], caps[j]) if j < min(end[h], R) else 0), (h, s)


# ------------------------------------------------------------------------------------------------------------- the scores
def as_device_forms(golden):
    rows, begin, end = golden_rows(golden)
    H = len(golden["candidates"])
    hyp = upload(rows[:H])
    ref_tok, ref_len = upload(rows[H:])
    return hyp, (ref_tok, ref_len, torch.tensor(begin, device=DEV) - H, torch.tensor(end, device=DEV) - H)


@pytest.mark.parametrize("form", ["lists", "tensors"])
def test_bleu_and_rouge_l_match_the_reference_scorers(ops, golden, form):
    from on_device_image_captioning_amd import metrics
    cands, refs = golden["candidates"], golden["references"]
    if form == "tensors":
        cands, refs = as_device_forms(golden)
    corpus, sentence = metrics.bleu(cands, refs)
    g = golden["bleu"]
    assert sentence.is_cuda and sentence.dtype == torch.float64 and tuple(sentence.shape) == (4, len(g["testlen"]))
    assert np.abs(np.array(corpus) - np.array(g["corpus"])).max() <= TOL
    assert np.abs(sentence.cpu().numpy() - np.array(g["sentence"])).max() <= TOL
    mean, image = metrics.rouge_l(cands, refs)
    assert image.is_cuda and image.dtype == torch.float64
    assert np.abs(image.cpu().numpy() - np.array(golden["rouge"]["image"])).max() <= TOL
    assert abs(mean - golden["rouge"]["mean"]) <= TOL


def test_thin_functions_give_the_integers(ops, golden):
    from on_device_image_captioning_amd import metrics
    (tok, lens), ref_rows = as_device_forms(golden)
    stats = metrics.bleu_stats(tok, lens, ref_rows).cpu().numpy()
    _, _, want = M.bleu(golden["candidates"], golden["references"])
    assert np.array_equal(stats, np.array(want))
    lcs, len_c, len_r = metrics.lcs(tok, lens, ref_rows, max_refs=5)
    for h, (c, refs) in enumerate(zip(golden["candidates"], golden["references"])):
        n = len(refs)
        assert lcs[h, :n].tolist() == golden["rouge"]["lcs"][h] and lcs[h, n:].tolist() == [0] * (5 - n)
        assert int(len_c[h]) == len(c) and len_r[h].tolist() == [len(r) for r in refs] + [0] * (5 - n)
    with pytest.raises(ValueError, match="65533"):                                  # the ids are checked on the device
        metrics.bleu((torch.tensor([[4, 65534, 5]], device=DEV), torch.tensor([2], device=DEV)), [[[4, 5]]])
    corpus, _ = metrics.bleu((torch.tensor([[4, 5, 65534]], device=DEV), torch.tensor([2], device=DEV)), [[[4, 5]]])
    assert abs(corpus[0] - 1.0) <= 1e-8                                             # … only inside the rows' lengths
    with pytest.raises(ValueError, match="empty"):
        metrics.rouge_l((tok, lens), (ref_rows[0], torch.zeros_like(ref_rows[1]), ref_rows[2], ref_rows[3]))
    mean, image = metrics.rouge_l([[], [4, 5]], [[[4]], [[4, 5]]])
    assert image.tolist() == [0.0, 1.0] and mean == 0.5                             # an empty candidate scores 0


def test_coco_scores_fill_the_table(ops, golden):
    from on_device_image_captioning_amd import evaluation
    S, E = golden["sos_idx"], golden["eos_idx"]
    cands = [[S] + c + [E] for c in golden["candidates"]]
    refs = [[[S] + r + [E] for r in per] for per in golden["references"]]
    table = evaluation.coco_scores(cands, refs)
    assert list(table) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"]
    assert np.abs(np.array([table[f"Bleu_{k}"] for k in (1, 2, 3, 4)]) - np.array(golden["bleu"]["corpus"])).max() <= TOL
    assert abs(table["ROUGE_L"] - golden["rouge"]["mean"]) <= TOL
    assert table["CIDEr"] == evaluation.cider_d_readme(cands, refs) / evaluation.README_SCALE > 0


# -------------------------------------------------------------------------------------------------------------- consensus
@pytest.mark.parametrize("metric", ["bleu4", "rouge_l"])
def test_consensus_rerank_matches_the_reference_scorers(ops, golden, metric):
    from on_device_image_captioning_amd import reward
    c, E = golden["consensus"], golden["eos_idx"]
    index, scores = reward.consensus_rerank(c["captions"], eos_idx=E, metric=metric)
    assert tuple(scores.shape) == (4, 6) and scores.dtype == torch.float64 and index.dtype == torch.int64 and scores.is_cuda
    for b, per in enumerate(c["captions"]):
        best, want = M.consensus_from_matrix(c[metric][b])                  # the means of the recorded pairwise scores
        assert np.abs(scores[b].cpu().numpy() - want).max() <= TOL, b
        assert int(index[b]) == best == M.consensus(per, E, metric)[0], b
        rows = M.consensus_rows(per, E)
        twin = rows.index(rows[0], 1)                                       # every image holds candidate 0 twice
        assert float(scores[b, 0]) == float(scores[b, twin])                # equal to the bit


@pytest.mark.parametrize("metric", ["bleu4", "rouge_l"])
def test_duplicates_tie_and_the_tie_goes_to_the_lower_index(ops, metric):
    from on_device_image_captioning_amd import reward
    S, E = 3, 2
    a, b, c = [S, 10, 11, 12, 13, 14, E], [S, 10, 11, 12, 13, 15, E], [S, 20, 21, E]
    caps = [[c, a, b, a, [S, 10, 11, 12, 13, 14]],                          # 1, 3 and 4 (cut before EOS) are one caption
            [b, b, b, b, b],
            [c, a, c, a, b]]
    index, scores = reward.consensus_rerank(caps, eos_idx=E, metric=metric)
    assert index.tolist() == [1, 0, 1]
    assert float(scores[0, 1]) == float(scores[0, 3]) == float(scores[0, 4])
    assert float(scores[2, 1]) == float(scores[2, 3]) and float(scores[2, 0]) == float(scores[2, 2])
    assert len(set(scores[1].tolist())) == 1 and abs(float(scores[1, 0]) - 1.0) <= 1e-8
    for i, per in enumerate(caps):
        best, want = M.consensus(per, E, metric)
        assert int(index[i]) == best and np.abs(scores[i].cpu().numpy() - want).max() <= TOL
    index, scores = reward.consensus_rerank([[a], [c]], eos_idx=E, metric=metric)
    assert index.tolist() == [0, 0] and scores.tolist() == [[0.0], [0.0]]


def test_the_default_metric_is_the_existing_path(ops, golden):
    from on_device_image_captioning_amd import reward
    caps, E = golden["consensus"]["captions"], golden["eos_idx"]
    index, scores = reward.consensus_rerank(caps, eos_idx=E)
    same_index, same_scores = reward.consensus_rerank(caps, eos_idx=E, metric="cider")
    assert torch.equal(index, same_index) and torch.equal(scores.view(torch.int64), same_scores.view(torch.int64))
    other = reward.consensus_rerank(caps, eos_idx=E, metric="rouge_l")[1]
    assert not torch.equal(scores, other)


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    g = W.TINY
    m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                            output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=DEV)
    m.load_state_dict(cached_state_dict("TINY", "eos"), strict=True)
    return m.to(DEV).eval().set_precision("fp32")


def test_consensus_caption_with_rouge_l_returns_its_best_candidate(model):
    from on_device_image_captioning_amd import reward
    from on_device_image_captioning_amd.captioning_model import Captioner
    img = W.synth_images(2, W.TINY).to(DEV)
    cap = Captioner({"sos_idx": 3, "eos_idx": 2, "beam_max_seq_len": 10}, model=model)
    captions, score = cap.consensus_caption(img, [0, 0], num_candidates=4, source="sampling", temperature=1.3,
                                            metric="rouge_l")
    cands, index, scores = model.last_consensus
    assert len(captions) == 2 and len(cands) == 2 and all(len(c) == 4 for c in cands)
    want_index, want_scores = reward.consensus_rerank(cands, eos_idx=2, metric="rouge_l")
    assert torch.equal(index, want_index) and torch.equal(scores, want_scores)
    for b in range(2):
        assert captions[b] == cands[b][int(index[b])] and captions[b][0] == 3
        _, s = M.consensus(cands[b], 2, "rouge_l")
        assert np.abs(scores[b].cpu().numpy() - s).max() <= TOL
        assert abs(float(score[b]) - s.max()) <= TOL                       # the best under the model, whatever its index
