"""Generate tests/golden/reinforce_cider.json by running the REAL reference on the CPU (build container only).

    python tools/make_golden_reward.py

The reference's ReinforceCiderScorer (eval/cider/reinforce_cider_scorer.py) and ReinforceCiderReward.compute_reward
(losses/reward.py, rank='cpu') are run on a seeded synthetic corpus: 40 images with 1-5 reference strings each, made of
COCO-vocabulary words, a few words outside the vocabulary, capitals and punctuation for the cleaner.  Recorded, data only:
  references   the raw reference strings, per image
  eos_idx, sos_idx
  hyp          hypotheses as id lists (SOS … EOS), copies of references with words changed, dropped or repeated, and free ones
  hyp_image    the image each is scored against;  hyp_score  the reference scorer's CIDEr-D of each
  reward.*     one SCST batch: image_idx [B], pred [B][S] and base [B][S] id lists, logprob [B][S][T], and reward, reward_base
               and reward_loss of compute_reward for the mean base (`mean`) and for the given base (`given`)
The log-probs are fp32 multiples of 1/256 in (-3, 0]: a row of them sums exactly in fp32 in any order, so the recorded loss
does not carry the summation order of the CPU the reference ran on.
"""
from __future__ import annotations

import json
import os
import random
import sys

sys.dont_write_bytecode = True

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import REF                                   # noqa: E402
from on_device_image_captioning_amd import language_utils as LU     # noqa: E402

sys.path.insert(0, REF)
from eval.cider.reinforce_cider import ReinforceCider                # noqa: E402
from losses.reward import ReinforceCiderReward                       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reinforce_cider.json")
N_IMAGES, B, S = 40, 6, 5
OOV = ["zorblax", "quixotry", "flumph", "snarfle"]


def main():
    rng = random.Random(20240)
    word2idx, idx2word = LU.load_vocab()
    sos_idx, eos_idx = word2idx["SOS"], word2idx["EOS"]
    plain = [w for w in idx2word[100:3000] if w.isalpha() and w.islower()]
    common = plain[:25]

    def words(lo=3, hi=14):
        return [rng.choice(common if rng.random() < 0.6 else plain) for _ in range(rng.randint(lo, hi))]

    references = []
    for i in range(N_IMAGES):
        refs = []
        for _ in range(1 + i % 5):
            w = words()
            if rng.random() < 0.25:
                w[rng.randrange(len(w))] = rng.choice(OOV)
            s = " ".join(w)
            if rng.random() < 0.5:
                s = s.capitalize() + rng.choice([".", " .", "!", ",  ", " "])
            if rng.random() < 0.2:
                s = s.replace(" ", ", ", 1)
            refs.append(s)
        references.append(refs)

    rew = ReinforceCiderReward(references, "EOS", S, "cpu")
    cleaned = [[c.split()[:-1] for c in refs] for refs in rew.training_references]

    def hypothesis(img):
        """word list (in-vocabulary) between SOS and EOS"""
        mode = rng.random()
        ref = [w for w in rng.choice(cleaned[img]) if w in word2idx]
        if mode < 0.2 or not ref:
            w = words(1, 16)
        else:
            w = list(ref)
            for _ in range(rng.randint(0, 3)):
                w[rng.randrange(len(w))] = rng.choice(common)
            if mode < 0.4:
                w = w[:max(1, len(w) - rng.randint(1, 4))]
            elif mode < 0.5:
                w = w + [w[-1]] * rng.randint(1, 3)
        return ["SOS"] + w + ["EOS"]

    def ids(caption):
        return [word2idx[w] for w in caption]

    scorer = ReinforceCider(rew.training_references)
    hyp, hyp_image = [], []
    for img in range(N_IMAGES):
        for _ in range(2):
            hyp.append(hypothesis(img))
            hyp_image.append(img)
    hyp += [["SOS", "EOS"], ["SOS", plain[5], "EOS"], ["SOS", plain[5], plain[6], "EOS"]]
    hyp_image += [0, 1, 2]
    _, hyp_score = scorer.compute_score(hypo=[" ".join(h[1:]) for h in hyp],
                                        refs=[rew.training_references[i] for i in hyp_image])

    image_idx = rng.sample(range(N_IMAGES), B)
    pred = [[hypothesis(i) for _ in range(S)] for i in image_idx]
    base = [[hypothesis(i) for _ in range(S)] for i in image_idx]
    T = max(len(c) for per in pred for c in per)
    g = torch.Generator().manual_seed(7)
    logprob = -torch.randint(0, 768, (B, S, T), generator=g).float() / 256.0
    for b in range(B):
        for s in range(S):
            logprob[b, s, len(pred[b][s]):] = 0.0
            logprob[b, s, 0] = 0.0
    out = {"references": references, "sos_idx": sos_idx, "eos_idx": eos_idx,
           "hyp": [ids(h) for h in hyp], "hyp_image": hyp_image, "hyp_score": [float(v) for v in hyp_score],
           "reward": {"image_idx": image_idx, "pred": [[ids(c) for c in per] for per in pred],
                      "base": [[ids(c) for c in per] for per in base], "logprob": logprob.tolist()}}
    for name, given in (("mean", None), ("given", base)):
        loss, r, rb = rew.compute_reward(pred, logprob, image_idx, given)
        out["reward"][name] = {"reward": r.tolist(), "reward_base": rb.tolist(), "reward_loss": float(loss)}
    with open(OUT, "w") as f:
        json.dump(out, f)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes;", len(hyp), "hypotheses, scores", min(hyp_score), "…", max(hyp_score))
    if size > 100 * 1024:
        raise SystemExit("the fixture exceeds 100 KB")


if __name__ == "__main__":
    main()
