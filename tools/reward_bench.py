"""Time of the self-critical reward for one SCST batch, two routes on the same captions:

    device  reward.ReinforceCiderReward.compute_reward on device tensors: one vectorize launch, one pairs launch, the torch
            gathers and reductions around them; timed with device events
    host    what a caller had to do before: tokens .cpu(), .tolist(), a dictionary CIDEr-D in the style of cider.py over the
            id tuples, the reward tensor uploaded again; timed with a host clock around work that ends in a synchronise

Shape: B = 16 images x S = 5 samples, 5 references per image, T = 20 (the reference's SCST shape); seeded synthetic ids over
a 10000-word vocabulary, the samples perturbed copies of references so that the n-gram matching has work to do.  The two
routes alternate in one process; their rewards are compared first (1e-10).  Median, quartiles and minimum over --iters go
to stdout as one JSON line and to --out.  Needs a GPU; there is no fallback.

    python tools/reward_bench.py --iters 200 --warmup 20 --out profiles/reward_bench.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOS, EOS, VOCAB = 79, 77, 10000


def make_batch(n_images, B, S, n_refs, T, seed=0):
    rng = np.random.default_rng(seed)
    common = rng.integers(100, VOCAB, 60)

    def sentence(n):
        return [int(rng.choice(common)) if rng.random() < 0.6 else int(rng.integers(100, VOCAB)) for _ in range(n)]

    refs = [[sentence(int(rng.integers(7, T - 2))) for _ in range(n_refs)] for _ in range(n_images)]
    image_idx = [int(i) for i in rng.choice(n_images, B, replace=False)]
    pred = []
    for i in image_idx:
        per = []
        for _ in range(S):
            w = list(refs[i][int(rng.integers(n_refs))])
            for _ in range(int(rng.integers(0, 4))):
                w[int(rng.integers(len(w)))] = int(rng.choice(common))
            per.append([SOS] + w[:T - 2] + [EOS])
        pred.append(per)
    return refs, image_idx, pred


class HostCider:
    """ReinforceCiderScorer over tuples of ids: dictionaries, one hypothesis at a time (the style of cider.py)."""

    def __init__(self, refs):
        self.refs = [[self.counts(r + [EOS]) for r in per] for per in refs]
        self.df = Counter()
        for per in self.refs:
            self.df.update(set(g for r in per for g in r))
        self.log_n = math.log(float(len(refs)))
        self.ref_vecs = [[self.vec(r) for r in per] for per in self.refs]

    @staticmethod
    def counts(ids):
        c = Counter()
        for k in range(1, 5):
            for i in range(len(ids) - k + 1):
                c[tuple(ids[i:i + k])] += 1
        return c

    def vec(self, cnt):
        vec, norm, length = [dict() for _ in range(4)], [0.0] * 4, 0
        for g, tf in cnt.items():
            k = len(g) - 1
            w = tf * (self.log_n - math.log(max(1.0, self.df.get(g, 0.0))))
            vec[k][g] = w
            norm[k] += w * w
            if k == 1:
                length += tf
        return vec, [math.sqrt(v) for v in norm], length

    def score(self, hyp, image):
        hv, hn, hl = self.vec(self.counts(hyp))
        total = 0.0
        for rv, rn, rl in self.ref_vecs[image]:
            pen = math.exp(-((hl - rl) ** 2) / 72.0)
            for k in range(4):
                acc = 0.0
                for g, w in hv[k].items():
                    rw = rv[k].get(g, 0.0)
                    acc += min(w, rw) * rw
                if hn[k] != 0 and rn[k] != 0:
                    acc /= hn[k] * rn[k]
                total += acc * pen
        return total / 4.0 / len(self.ref_vecs[image]) * 10.0


def quartiles(v):
    q = np.percentile(np.asarray(v), [25, 50, 75])
    return {"median_ms": float(q[1]), "q25_ms": float(q[0]), "q75_ms": float(q[2]), "min_ms": float(np.min(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000, help="images of the corpus the document frequencies come from")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--refs", type=int, default=5)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from on_device_image_captioning_amd import reward
    if not torch.cuda.is_available():
        raise SystemExit("reward_bench needs a GPU: a CPU run says nothing about either route")
    dev = "cuda:0"
    refs, image_idx, pred = make_batch(a.images, a.batch, a.samples, a.refs, a.T)
    rew = reward.ReinforceCiderReward(refs, EOS, a.samples, dev)
    host = HostCider(refs)
    T = max(len(c) for per in pred for c in per)
    tok = torch.zeros(a.batch, a.samples, T, dtype=torch.int64)
    lens = torch.zeros(a.batch, a.samples, dtype=torch.int64)
    for b, per in enumerate(pred):
        for s, c in enumerate(per):
            tok[b, s, :len(c)] = torch.tensor(c)
            lens[b, s] = len(c)
    tok, lens = tok.to(dev), lens.to(dev)
    idx = torch.tensor(image_idx, device=dev)
    logprob = -torch.rand(a.batch, a.samples, T, device=dev)

    def device_route():
        return rew.compute_reward((tok, lens), logprob, idx)

    def host_route():
        rows, ln = tok.cpu().tolist(), lens.cpu().tolist()
        r = torch.tensor([[host.score(rows[b][s][1:ln[b][s]], image_idx[b]) for s in range(a.samples)]
                          for b in range(a.batch)], dtype=torch.float64).to(dev)
        base = (r.sum(dim=-1, keepdim=True) - r) / (a.samples - 1)
        return ((r - base) * torch.sum(-logprob.double(), dim=-1)).mean(), r, base

    ld, rd, _ = device_route()
    lh, rh, _ = host_route()
    diff = float((rd - rh).abs().max())
    if diff > 1e-10 or abs(float(ld) - float(lh)) > 1e-10 * max(1.0, abs(float(lh))):
        raise SystemExit(f"the two routes disagree: rewards by {diff:.3e}")
    for _ in range(a.warmup):
        device_route()
        host_route()
    torch.cuda.synchronize()
    t_dev, t_host = [], []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device_route()
        e1.record()
        e1.synchronize()
        t_dev.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        host_route()
        torch.cuda.synchronize()
        t_host.append((time.perf_counter() - t0) * 1e3)
    d, h = quartiles(t_dev), quartiles(t_host)
    out = {"tool": "reward_bench", "images": a.images, "batch": a.batch, "samples": a.samples, "refs": a.refs, "T": a.T,
           "iters": a.iters, "warmup": a.warmup, "mean_reward": float(rd.mean()), "max_route_difference": diff,
           "device": d, "host": h, "host_over_device": h["median_ms"] / d["median_ms"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
