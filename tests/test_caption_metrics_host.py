"""BLEU and ROUGE-L on the device, the part that needs no GPU: the plain model of the kernels
(tests/caption_metrics_model.py) against the reference scorers' recorded values (tests/golden/caption_metrics.json,
tools/make_golden_metrics.py); the C boundary and its refusals; the Python layer's refusals."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import caption_metrics_model as M
from cider_device_model import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "caption_metrics.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_model_components_equal_the_golden_ones(golden):
    g = golden["bleu"]
    lengths = set()
    for i, (c, refs) in enumerate(zip(golden["candidates"], golden["references"])):
        s = M.bleu_stats(c, refs)
        assert s[0:4] == g["correct"][i] and s[4:8] == g["guess"][i], i
        assert s[8] == g["testlen"][i] and s[9] == g["reflen"][i], i
        assert s[10] == min(len(r) for r in refs) and s[11] == sum(len(r) for r in refs)
        assert [M.lcs(r, c) for r in refs] == golden["rouge"]["lcs"][i] == [M.lcs(c, r) for r in refs], i
        lengths.add(len(c))
    assert {1, 2, 3} <= lengths and {len(r) for r in golden["references"]} == {1, 2, 3, 4, 5}


def test_model_scores_reproduce_the_golden_scores(golden):
    corpus, sentence, _ = M.bleu(golden["candidates"], golden["references"])
    g = golden["bleu"]
    assert np.abs(np.array(corpus) - np.array(g["corpus"])).max() <= TOL
    assert np.abs(np.array(sentence) - np.array(g["sentence"])).max() <= TOL
    rouge = np.array([M.rouge_l(c, refs) for c, refs in zip(golden["candidates"], golden["references"])])
    assert np.abs(rouge - np.array(golden["rouge"]["image"])).max() <= TOL
    assert abs(float(np.mean(rouge)) - golden["rouge"]["mean"]) <= TOL
    assert 0.3 < g["corpus"][3] < g["corpus"][0] < 1 and min(g["sentence"][3]) < 1e-3 < max(g["sentence"][3])


@pytest.mark.parametrize("metric", ["bleu4", "rouge_l"])
def test_model_reproduces_the_golden_consensus_block(golden, metric):
    c = golden["consensus"]
    assert len(c["captions"]) == 4 and all(len(per) == 6 for per in c["captions"])
    for per, want in zip(c["captions"], c[metric]):
        got = M.pairwise(per, golden["eos_idx"], metric)
        assert np.abs(got - np.array(want)).max() <= TOL
        # the block was chosen so that only exact duplicates come closer than 1e-6: the best index is no matter of rounding
        best, s = M.consensus_from_matrix(want)
        rows = M.consensus_rows(per, golden["eos_idx"])
        for i in range(6):
            for j in range(i):
                assert abs(s[i] - s[j]) > 1e-6 or (rows[i] == rows[j] and s[i] == s[j])
        assert M.consensus(per, golden["eos_idx"], metric)[0] == best


def test_model_on_the_quirks():
    a, b = 7, 8
    assert M.bleu_stats([a] * 5, [[a, a, b], [a, a, a]])[0] == 3                   # the maximum over the references, not 5
    assert M.bleu_stats([1, 2, 3, 4, 5], [[9] * 4, [9] * 6])[9] == 4               # a tie goes to the shorter reference
    assert M.bleu_stats([1, 2], [])[:4] == [0] * 4 and M.bleu_stats([1, 2], [])[9:] == [0, 0, 0]
    assert M.bleu_stats([1, 2], [[1, 2]])[4:8] == [2, 1, 0, 0]
    assert M.lcs([1] * 128, [1] * 65) == 65 and M.lcs([1, 2, 3, 4], [2, 4, 1, 3]) == 2 and M.lcs([], [1]) == 0
    # precision and recall are maximised separately: P from the short reference, R from the long one
    f = M.rouge_l([1, 2, 3, 4], [[1, 2], [1, 2, 3, 4, 5, 6, 7, 8]])
    assert abs(f - (1 + 1.44) * 1.0 * 1.0 / (1.0 + 1.44 * 1.0)) <= TOL
    assert M.rouge_l([], [[1]]) == 0.0 and M.rouge_l([5], [[6]]) == 0.0


def test_header_and_binding_agree_and_the_abi_is_still_26(lib):
    from on_device_image_captioning_amd import _hip, metrics
    text = open(os.path.join(ROOT, "include", "odic_hip.h")).read()
    assert "#define ODIC_ABI_VERSION 27" in text and lib.odic_abi_version() == 27 == _hip.ABI_VERSION
    for name, n_args in (("odic_bleu_stats", 12), ("odic_lcs_pairs", 12)):
        assert name in _hip.EXPORTED_SYMBOLS
        assert name in re.search(r"Pure additions since.*?\*/", text, flags=re.S).group(0)
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
        assert len(decl.split(",")) == n_args == len(getattr(lib, name).argtypes)
    words = int(re.search(r"#define ODIC_BLEU_STAT_WORDS (\d+)", text).group(1))
    assert words == _hip.BLEU_STAT_WORDS == metrics.STAT_WORDS == M.STAT_WORDS == 12
    assert (metrics.TINY, metrics.SMALL, metrics.BETA) == (M.TINY, M.SMALL, M.BETA)
    assert "caption_metrics.hip" in open(os.path.join(ROOT, "on_device_image_captioning_amd", "csrc", "Makefile")).read()


def test_the_library_refuses_bad_arguments_without_a_gpu(lib):
    from on_device_image_captioning_amd import _hip
    W = _hip.CIDER_ROW_WORDS

    def stats(ws=16, ldw=W, lengths=16, R=8, max_len=128, hyp=16, begin=16, end=16, Q=4, out=16, lds=12):
        return lib.odic_bleu_stats(ws, ldw, lengths, R, max_len, hyp, begin, end, Q, out, lds, None)

    for arg in ("ws", "lengths", "hyp", "begin", "end", "out"):
        assert stats(**{arg: None}) == -2, arg
    assert stats(Q=0) == -1 and stats(Q=-1) == -1 and stats(R=0) == -1 and stats(R=-2) == -1
    assert stats(ldw=W - 1) == -1 and stats(lds=11) == -1
    assert stats(max_len=129) == -1 and stats(max_len=-1) == -1

    def pairs(tokens=16, ld=128, lengths=16, R=8, max_len=128, begin=16, end=16, H=4, max_refs=5, out=16, ldl=5):
        return lib.odic_lcs_pairs(tokens, ld, lengths, R, max_len, begin, end, H, max_refs, out, ldl, None)

    for arg in ("tokens", "lengths", "begin", "end", "out"):
        assert pairs(**{arg: None}) == -2, arg
    assert pairs(H=0) == -1 and pairs(R=0) == -1 and pairs(H=9) == -1            # the hypotheses are rows of `tokens`
    assert pairs(max_refs=0) == -1 and pairs(ldl=4) == -1
    assert pairs(max_len=129, ld=129) == -1 and pairs(max_len=-1) == -1
    assert pairs(max_len=20, ld=19) == -1                                        # rows shorter than the permitted length


def test_the_python_layer_refuses_what_it_cannot_score():
    from on_device_image_captioning_amd import evaluation, metrics, reward
    with pytest.raises(ValueError, match="65533"):
        metrics.bleu([[1, 65534]], [[[1, 2]]])
    with pytest.raises(ValueError, match="65533"):
        metrics.bleu([[1, 2]], [[[1, 2], [-1]]])
    for fn in (metrics.bleu, metrics.rouge_l):
        with pytest.raises(ValueError, match="128"):
            fn([[1] * 129], [[[1, 2]]])
        with pytest.raises(ValueError, match="128"):
            fn([[1, 2]], [[[1] * 129]])
        with pytest.raises(ValueError, match="128"):
            fn((torch.zeros(1, 129, dtype=torch.int32), torch.ones(1, dtype=torch.int32)), [[[1, 2]]])
        with pytest.raises(ValueError, match="at least one reference"):
            fn([[1, 2], [3]], [[[1, 2]], []])
        with pytest.raises(ValueError, match="at least one reference"):
            fn([[1, 2], [3]], [[[1, 2]]])
    with pytest.raises(ValueError, match="empty"):
        metrics.rouge_l([[1, 2]], [[[1, 2], []]])
    with pytest.raises(ValueError, match="one candidate per image"):
        evaluation.coco_scores([[3, 1, 2]], [])
    corpus = reward.CiderCorpus([[[4, 5]]], 2, "cpu")
    caps = [[[3, 4, 2], [3, 5, 2]]]
    for metric in ("bleu4", "rouge_l"):
        with pytest.raises(ValueError, match="corpus"):
            reward.consensus_rerank(caps, corpus=corpus, eos_idx=2, metric=metric)
        with pytest.raises(ValueError, match="65533"):
            reward.consensus_rerank([[[3, 70000, 2], [3, 1, 2]]], eos_idx=2, metric=metric)
    with pytest.raises(ValueError, match="metric"):
        reward.consensus_rerank(caps, eos_idx=2, metric="meteor")


def test_the_metrics_have_no_cpu_fallback():
    from on_device_image_captioning_amd import metrics, reward
    tok, lens = torch.tensor([[4, 5, 6]], dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    refs = (tok, lens, torch.tensor([0]), torch.tensor([1]))
    for call in (lambda: metrics.bleu((tok, lens), [[[4, 5]]]), lambda: metrics.rouge_l((tok, lens), [[[4, 5]]]),
                 lambda: metrics.bleu([[4, 5]], [[[4, 5]]], device="cpu"), lambda: metrics.bleu_stats(tok, lens, refs),
                 lambda: metrics.lcs(tok, lens, refs, max_refs=1),
                 lambda: metrics.pairwise(tok, lens, 1, 1, "bleu4"), lambda: metrics.pairwise(tok, lens, 1, 1, "rouge_l")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_metric_defaults_to_cider():
    from on_device_image_captioning_amd import reward
    from on_device_image_captioning_amd.captioning_model import Captioner, CaptioningModel
    for fn in (reward.consensus_rerank, CaptioningModel.consensus_caption, Captioner.consensus_caption):
        p = inspect.signature(fn).parameters["metric"]
        assert p.default == "cider" and p.kind is inspect.Parameter.KEYWORD_ONLY
