"""Generate tests/golden/caption_metrics.json by running the REAL reference scorers on the CPU (build container only).

    python tools/make_golden_metrics.py

The reference's Bleu(4).compute_score (eval/bleu/bleu.py, bleu_scorer.py) and Rouge().compute_score (eval/rouge/rouge.py)
are run on a seeded synthetic corpus of word ids, id i spelled "w<i>": 40 images with 1-5 references each and one candidate
per image — copies of references with words changed, truncations, repeats and free ones — then three more images whose
candidates have one, two and three words.  Recorded, data only:
  references [H][n], candidates [H]         id lists, the words alone (no SOS, no EOS)
  bleu.correct, bleu.guess [H][4], bleu.testlen, bleu.reflen [H]
                                            the scorer's integer components per image (reflen: the "closest" option)
  bleu.corpus [4], bleu.sentence [4][H]     what compute_score returns
  rouge.mean, rouge.image [H], rouge.lcs [H][n]     compute_score, and my_lcs of the candidate with every reference
  consensus.*   4 images x 6 candidates as a search returns them (SOS first, EOS last unless the search was cut), with
                `bleu4` and `rouge_l` [4][6][6]: entry (i, j) is the sentence BLEU-4 / the ROUGE-L of candidate i against
                candidate j as its single reference, both scored as caption[1:] with EOS appended where it is missing.
The consensus block is drawn again until, under both metrics, no two candidates of an image have mean scores within 1e-6 of
each other unless they are exact duplicates (which every image has one pair of): the best index is then not a matter of
rounding.
"""
from __future__ import annotations

import json
import os
import random
import sys

sys.dont_write_bytecode = True

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import REF                                   # noqa: E402

sys.path.insert(0, REF)
from eval.bleu.bleu import Bleu                                      # noqa: E402
from eval.bleu.bleu_scorer import BleuScorer                         # noqa: E402
from eval.rouge.rouge import Rouge, my_lcs                           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "caption_metrics.json")
N_IMAGES, B, N = 40, 4, 6
SOS, EOS = 3, 2
COMMON = list(range(10, 35))
PLAIN = list(range(100, 3000)) + [0, 65533]


def spell(ids):
    return " ".join(f"w{int(t)}" for t in ids)


def main():
    rng = random.Random(20241)

    def words(lo=3, hi=14):
        return [rng.choice(COMMON if rng.random() < 0.6 else PLAIN) for _ in range(rng.randint(lo, hi))]

    def edited(ref, mode):
        w = list(ref)
        for _ in range(rng.randint(0, 3)):
            w[rng.randrange(len(w))] = rng.choice(COMMON)
        if mode < 0.4:
            w = w[:max(1, len(w) - rng.randint(1, 4))]
        elif mode < 0.5:
            w = w + [w[-1]] * rng.randint(1, 3)
        return w

    references, candidates = [], []
    for i in range(N_IMAGES):
        refs = [words() for _ in range(1 + i % 5)]
        mode = rng.random()
        references.append(refs)
        candidates.append(words(1, 16) if mode < 0.2 else edited(rng.choice(refs), mode))
    for n in (1, 2, 3):                                 # the orders vanish one by one
        refs = [words(4, 9) for _ in range(2)]
        references.append(refs)
        candidates.append(refs[0][:n])
    H = len(candidates)

    gts = {i: [spell(r) for r in refs] for i, refs in enumerate(references)}
    res = {i: [spell(c)] for i, c in enumerate(candidates)}
    corpus, sentence = Bleu(4).compute_score(gts, res)
    scorer = BleuScorer(n=4)
    for i in range(H):
        scorer += (res[i][0], gts[i])
    again, _ = scorer.compute_score(option="closest")
    assert again == corpus
    comps = scorer.ctest
    bleu = {"correct": [c["correct"] for c in comps], "guess": [c["guess"] for c in comps],
            "testlen": [c["testlen"] for c in comps],
            "reflen": [scorer._single_reflen(c["reflen"], "closest", c["testlen"]) for c in comps],
            "corpus": [float(v) for v in corpus], "sentence": [[float(v) for v in row] for row in sentence]}
    mean, image = Rouge().compute_score(gts, res)
    rouge = {"mean": float(mean), "image": [float(v) for v in image],
             "lcs": [[int(my_lcs(spell(r).split(" "), spell(c).split(" "))) for r in refs]
                     for c, refs in zip(candidates, references)]}

    def rows_of(per):
        return [c[1:] + ([] if len(c) > 1 and c[-1] == EOS else [EOS]) for c in per]

    def matrices(per):
        rows = rows_of(per)
        pairs = [(i, j) for i in range(N) for j in range(N)]
        g = {k: [spell(rows[j])] for k, (i, j) in enumerate(pairs)}
        r = {k: [spell(rows[i])] for k, (i, j) in enumerate(pairs)}
        _, per_sentence = Bleu(4).compute_score(g, r)
        _, per_image = Rouge().compute_score(g, r)
        return (np.array(per_sentence[3], dtype=np.float64).reshape(N, N), np.array(per_image, dtype=np.float64).reshape(N, N))

    def separated(per, m):
        rows = rows_of(per)
        s = [(m[i].sum() - m[i, i]) / (N - 1) for i in range(N)]
        return all(abs(s[i] - s[j]) > 1e-6 or rows[i] == rows[j] for i in range(N) for j in range(i))

    for attempt in range(1000):
        block = []
        for b in range(B):
            base = words(7, 12)
            per = [[SOS] + edited(base, rng.random()) + [EOS] for _ in range(N - 1)]
            if b == 1:
                per[2] = per[2][:-1]                    # a search cut before EOS
            if b == 3:
                per[4] = [SOS, EOS]                     # an empty caption: its row is EOS alone
            per.insert(rng.randrange(1, N), list(per[0]))        # an exact duplicate of candidate 0
            block.append(per)
        mats = [matrices(per) for per in block]
        if all(separated(per, m) for per, (mb, mr) in zip(block, mats) for m in (mb, mr)):
            break
    else:
        raise SystemExit("no consensus block with separated scores was found")
    consensus = {"captions": block, "bleu4": [mb.tolist() for mb, _ in mats], "rouge_l": [mr.tolist() for _, mr in mats]}

    out = {"sos_idx": SOS, "eos_idx": EOS, "references": references, "candidates": candidates, "bleu": bleu, "rouge": rouge,
           "consensus": consensus}
    with open(OUT, "w") as f:
        json.dump(out, f)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes;", H, "images, corpus BLEU", corpus, "ROUGE-L", mean, "; consensus attempt", attempt)
    if size > 100 * 1024:
        raise SystemExit("the fixture exceeds 100 KB")


if __name__ == "__main__":
    main()
