"""CIDEr-D on the device, the part that needs no GPU: the numpy model of the kernels (tests/cider_device_model.py) against
the reference's recorded scores and rewards (tests/golden/reinforce_cider.json, tools/make_golden_reward.py) and against
cider.CiderD; reference encoding; the C boundary and the Python layer's refusals."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import cider_device_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "reinforce_cider.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def corpus(golden):
    """(references as id lists with EOS appended, the model's table)"""
    from on_device_image_captioning_amd import language_utils as LU, reward
    word2idx, _ = LU.load_vocab()
    enc = reward.encode_references(golden["references"], word2idx)
    refs = [[r + [golden["eos_idx"]] for r in per] for per in enc]
    return refs, M.Table(refs)


@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_model_reproduces_the_golden_scores(golden, corpus):
    refs, table = corpus
    got = [M.score(h[1:], refs[i], table, table.default_idf) for h, i in zip(golden["hyp"], golden["hyp_image"])]
    diff = np.abs(np.array(got) - np.array(golden["hyp_score"]))
    print("model vs golden scores: max difference", diff.max(), "scores up to", max(golden["hyp_score"]))
    assert max(golden["hyp_score"]) > 5 and min(golden["hyp_score"]) == 0
    assert diff.max() <= M.TOL


@pytest.mark.parametrize("base", ["mean", "given"])
def test_model_reproduces_the_golden_rewards(golden, corpus, base):
    refs, table = corpus
    g = golden["reward"]
    lp = np.array(g["logprob"], dtype=np.float32)
    loss, r, b = M.reward(g["pred"], lp, g["image_idx"], refs, table, g["base"] if base == "given" else None)
    want = g[base]
    assert np.abs(r - np.array(want["reward"])).max() <= M.TOL
    assert np.abs(b - np.array(want["reward_base"])).max() <= M.TOL
    assert abs(loss - want["reward_loss"]) <= M.TOL * abs(want["reward_loss"])


def test_model_reproduces_cider_d(golden_dir):
    """cider.CiderD builds its document frequencies from the references it is given; on such a corpus (ids stand for the
    words) the model's scores are its per-image scores."""
    from on_device_image_captioning_amd.cider import CiderD
    rng = np.random.default_rng(5)
    ids = list(range(9000, 9040)) + [0, 65533]
    gts, res, refs, hyps = {}, {}, [], []
    for i in range(25):
        rs = [[int(rng.choice(ids[:12 if rng.random() < 0.7 else 42])) for _ in range(rng.integers(1, 12))]
              for _ in range(rng.integers(1, 5))]
        h = list(rs[0]) if i % 3 else [int(rng.choice(ids)) for _ in range(rng.integers(1, 12))]
        if i % 3 == 1:
            h[len(h) // 2] = ids[3]
        refs.append(rs)
        hyps.append(h)
        gts[i] = [" ".join(f"w{t}" for t in r) for r in rs]
        res[i] = [" ".join(f"w{t}" for t in h)]
    _, want = CiderD().compute_score(gts, res)
    table = M.Table(refs)
    got = np.array([M.score(h, rs, table, table.default_idf) for h, rs in zip(hyps, refs)])
    assert want.max() > 5
    assert np.abs(got - want).max() <= M.TOL


def test_keys_pack_orders_apart_and_sort_unsigned():
    k = M.pack_keys([0, 65533, 65533, 65533])
    assert list(M.key_order(k)) == [0, 0, 0, 0, 1, 1, 1, 2, 2, 3]
    assert int(k[0]) == 1 and int(k[-1]) == 1 | (65534 << 16) | (65534 << 32) | (65534 << 48)
    assert int(k[-1]) >> 63 == 1                                    # an id >= 32767 in the fourth field sets bit 63
    v = M.vectorize([0, 65533, 65533, 65533])
    assert np.all(v["keys"][:-1] < v["keys"][1:]) and int(v["keys"][-1]) == int(k[-1])
    assert list(M.key_order(v["keys"])) == sorted(M.key_order(v["keys"]))     # sorted keys are grouped by order


def test_encode_references_keeps_unknown_words_distinct():
    from on_device_image_captioning_amd import language_utils as LU, reward
    word2idx, idx2word = LU.load_vocab()
    enc = reward.encode_references([["A dog zorblax, a Dog flumph.", "zorblax!"], ["the flumph snarfle"]], word2idx)
    d, a = word2idx["dog"], word2idx["a"]
    z, f = enc[0][0][2], enc[0][0][5]
    assert enc[0][0] == [a, d, z, a, d, f] and enc[0][1] == [z]
    assert enc[1][0] == [word2idx["the"], f, enc[1][0][2]]
    private = {z, f, enc[1][0][2]}
    assert len(private) == 3 and min(private) >= len(word2idx)
    # no SOS, no EOS
    assert word2idx["EOS"] not in sum(sum(enc, []), []) and word2idx["SOS"] not in sum(sum(enc, []), [])


def test_header_and_binding_agree_and_the_abi_is_still_26(lib):
    from on_device_image_captioning_amd import _hip
    text = open(os.path.join(ROOT, "include", "odic_hip.h")).read()
    assert "#define ODIC_ABI_VERSION 27" in text and lib.odic_abi_version() == 27 == _hip.ABI_VERSION
    for name, n_args in (("odic_cider_vectorize", 13), ("odic_cider_pairs", 10)):
        assert name in _hip.EXPORTED_SYMBOLS
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
        assert len(decl.split(",")) == n_args == len(getattr(lib, name).argtypes)
    consts = dict(re.findall(r"#define ODIC_CIDER_(MAX_LEN|MAX_KEYS|MAX_ID|ROW_WORDS) (\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {"MAX_LEN": _hip.CIDER_MAX_LEN, "MAX_KEYS": _hip.CIDER_MAX_KEYS,
                                                      "MAX_ID": _hip.CIDER_MAX_ID, "ROW_WORDS": _hip.CIDER_ROW_WORDS}
    assert (M.MAX_LEN, M.MAX_KEYS, M.MAX_ID) == (_hip.CIDER_MAX_LEN, _hip.CIDER_MAX_KEYS, _hip.CIDER_MAX_ID)


def test_the_library_refuses_bad_arguments_without_a_gpu(lib):
    from on_device_image_captioning_amd import _hip
    W = _hip.CIDER_ROW_WORDS

    def vec(tokens=16, ld=128, lengths=16, R=3, max_len=128, max_id=65533, keys=None, idf=None, n_table=0, default=1.0,
            ws=16, ldw=W):
        return lib.odic_cider_vectorize(tokens, ld, lengths, R, max_len, max_id, keys, idf, n_table, default, ws, ldw, None)

    assert vec(tokens=None) == -2 and vec(lengths=None) == -2 and vec(ws=None) == -2
    assert vec(n_table=4, keys=16) == -2 and vec(n_table=4, idf=16) == -2        # half a table
    assert vec(R=0) == -1 and vec(R=-1) == -1
    assert vec(max_len=129, ld=129) == -1                                        # a length limit above 128
    assert vec(max_len=20, ld=19) == -1                                          # rows shorter than the permitted length
    assert vec(max_id=65534) == -1 and vec(max_id=-1) == -1                      # ids the key cannot hold
    assert vec(ldw=W - 1) == -1 and vec(n_table=-1) == -1

    def pairs(ws=16, ldw=W, R=8, begin=16, end=16, H=4, max_refs=5, sim=16, lds=5):
        return lib.odic_cider_pairs(ws, ldw, R, begin, end, H, max_refs, sim, lds, None)

    assert pairs(ws=None) == -2 and pairs(begin=None) == -2 and pairs(end=None) == -2 and pairs(sim=None) == -2
    assert pairs(H=0) == -1 and pairs(R=0) == -1 and pairs(H=9) == -1            # the hypotheses are rows of the workspace
    assert pairs(max_refs=0) == -1 and pairs(lds=4) == -1 and pairs(ldw=W - 1) == -1


def test_the_python_layer_refuses_what_the_key_cannot_hold():
    from on_device_image_captioning_amd import reward
    with pytest.raises(ValueError, match="65533"):
        reward.CiderCorpus([[[1, 65534]]], 2, "cpu")
    with pytest.raises(ValueError, match="127"):
        reward.CiderCorpus([[[1] * 128]], 2, "cpu")
    with pytest.raises(ValueError, match="at least one"):
        reward.CiderCorpus([[[1]], []], 2, "cpu")
    corpus = reward.CiderCorpus([[[1] * 127, [4, 5]], [[6]]], 2, "cpu")            # 127 words + EOS is the limit
    assert corpus.max_len == 128 and corpus.max_refs == 2 and corpus.ref_offsets.tolist() == [0, 2, 3]
    assert corpus.ref_tokens[1, :4].tolist() == [4, 5, 2, 0] and corpus.ref_len.tolist() == [128, 3, 2]
    rew = reward.ReinforceCiderReward(corpus, 2, 2, "cpu")
    lp = torch.zeros(1, 2, 4)
    with pytest.raises(ValueError, match="65533"):
        rew.compute_reward([[[3, 70000, 2], [3, 1, 2]]], lp, [0])
    with pytest.raises(ValueError, match="128"):
        rew.compute_reward([[[3] + [1] * 129, [3, 1, 2]]], lp, [0])
    with pytest.raises(ValueError, match="exactly 2"):
        rew.compute_reward([[[3, 1, 2], [3, 1, 2], [3, 1, 2]]], lp, [0])          # S = 3 where 2 were announced
    with pytest.raises(ValueError, match="exactly 2"):
        rew.compute_reward([[[3, 1, 2], [3, 1, 2]], [[3, 1, 2]]], lp, [0, 1])     # ragged
    with pytest.raises(ValueError, match="expected 2"):
        rew.compute_reward((torch.zeros(1, 3, 5, dtype=torch.int64), torch.ones(1, 3, dtype=torch.int64)), lp, [0])
    with pytest.raises(ValueError, match="same number"):
        reward.consensus_rerank([[[3, 1, 2]], [[3, 1, 2], [3, 4, 2]]], eos_idx=2)
    with pytest.raises(ValueError, match="65533"):
        reward.consensus_rerank([[[3, 70000, 2], [3, 1, 2]]], eos_idx=2)
    # and the table the corpus uploads is the model's
    table = M.Table([[r + [2] for r in per] for per in [[[1] * 127, [4, 5]], [[6]]]])
    assert np.array_equal(corpus.table_keys_host, table.keys) and np.array_equal(corpus.table_idf_host, table.idf)


def test_the_reward_has_no_cpu_fallback():
    from on_device_image_captioning_amd import reward
    rew = reward.ReinforceCiderReward([[[4, 5]], [[6]]], 2, 2, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rew.compute_reward([[[3, 4, 2], [3, 5, 2]]], torch.zeros(1, 2, 3), [0])
