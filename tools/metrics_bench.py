"""Time of BLEU-1..4 + ROUGE-L for a coco5k-shaped evaluation and of consensus reranking at N = 16.

    device (default)   metrics.bleu + metrics.rouge_l on 5000 candidates x 5 references — from device tensors, and from id
                       lists (packing and upload included) — and reward.consensus_rerank(metric=) on 16 images x 16
                       candidates; a host clock around calls that end in a read-back or a synchronise.  Needs a GPU.
    --reference DIR    the reference's own scorers (DIR/eval/bleu, DIR/eval/rouge) on the same seeded corpus spelled as
                       strings, on this machine's CPU: Bleu(4).compute_score + Rouge().compute_score, and the N·N pairwise
                       sentence scores of the consensus block.  Needs no GPU.

Each mode writes its section ("device" / "reference_cpu", with the machine's name) into --out and leaves the other one as
it found it.  Median, quartiles and minimum over --iters.

    python tools/metrics_bench.py --iters 20 --out profiles/metrics_bench.json
    python tools/metrics_bench.py --reference /path/to/reference --iters 3 --out profiles/metrics_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOS, EOS, VOCAB = 79, 77, 10000


def make_corpus(n_images, n_refs, seed=0):
    rng = np.random.default_rng(seed)
    common = rng.integers(100, VOCAB, 60)

    def sentence(n):
        return [int(rng.choice(common)) if rng.random() < 0.6 else int(rng.integers(100, VOCAB)) for _ in range(n)]

    refs = [[sentence(int(rng.integers(7, 18))) for _ in range(n_refs)] for _ in range(n_images)]
    cands = []
    for per in refs:
        w = list(per[int(rng.integers(n_refs))])
        for _ in range(int(rng.integers(0, 4))):
            w[int(rng.integers(len(w)))] = int(rng.choice(common))
        cands.append(w[:int(rng.integers(5, 18))])
    return cands, refs


def make_consensus(B, N, seed=1):
    cands, _ = make_corpus(B, 1, seed)
    rng = np.random.default_rng(seed)
    block = []
    for base in cands:
        per = []
        for _ in range(N):
            w = list(base)
            for _ in range(int(rng.integers(0, 4))):
                w[int(rng.integers(len(w)))] = int(rng.integers(100, 160))
            per.append([SOS] + w + [EOS])
        block.append(per)
    return block


def summary(times):
    t = np.sort(np.array(times)) * 1e3
    return {"median_ms": round(float(np.median(t)), 3), "q1_ms": round(float(np.percentile(t, 25)), 3),
            "q3_ms": round(float(np.percentile(t, 75)), 3), "min_ms": round(float(t[0]), 3), "iters": len(times)}


def timed(fn, iters, warmup, sync=None):
    out = []
    for i in range(warmup + iters):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        if i >= warmup:
            out.append(time.perf_counter() - t0)
    return summary(out)


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def run_device(args, cands, refs, block):
    import torch
    from on_device_image_captioning_amd import metrics, reward
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU (or --reference DIR for the CPU scorers); there is no fallback")
    dv = torch.device("cuda:0")
    hyp = tuple(torch.from_numpy(a).to(dv) for a in reward._pack(cands))
    counts = torch.tensor([len(per) for per in refs])
    end = torch.cumsum(counts, 0)
    ref_rows = tuple(torch.from_numpy(a).to(dv) for a in reward._pack([r for per in refs for r in per])) + \
        ((end - counts).to(dv), end.to(dv))
    a, b = metrics.bleu(hyp, ref_rows), metrics.bleu(cands, refs)
    assert a[0] == b[0] and torch.equal(a[1], b[1]), "the two input forms disagree"
    sync = torch.cuda.synchronize
    out = {"machine": torch.cuda.get_device_name(0), "bleu_corpus": a[0], "rouge_l_mean": metrics.rouge_l(hyp, ref_rows)[0]}
    out["eval_from_tensors"] = timed(lambda: (metrics.bleu(hyp, ref_rows), metrics.rouge_l(hyp, ref_rows)), args.iters,
                                     args.warmup, sync)
    out["eval_from_lists"] = timed(lambda: (metrics.bleu(cands, refs), metrics.rouge_l(cands, refs)), max(3, args.iters // 4),
                                   1, sync)
    for metric in ("cider", "bleu4", "rouge_l"):
        out[f"consensus_{metric}"] = timed(lambda: reward.consensus_rerank(block, eos_idx=EOS, metric=metric), args.iters,
                                           args.warmup, sync)
    return "device", out


def run_reference(args, cands, refs, block):
    sys.path.insert(0, args.reference)
    from eval.bleu.bleu import Bleu
    from eval.rouge.rouge import Rouge

    def spell(ids):
        return " ".join(f"w{t}" for t in ids)

    gts = {i: [spell(r) for r in per] for i, per in enumerate(refs)}
    res = {i: [spell(c)] for i, c in enumerate(cands)}
    out = {"machine": cpu_name()}
    out["bleu_corpus"], out["rouge_l_mean"] = Bleu(4).compute_score(gts, res)[0], float(Rouge().compute_score(gts, res)[0])
    out["eval"] = timed(lambda: (Bleu(4).compute_score(gts, res), Rouge().compute_score(gts, res)), args.iters, 1)
    rows = [[c[1:] for c in per] for per in block]
    g = {(b, i, j): [spell(per[j])] for b, per in enumerate(rows) for i in range(len(per)) for j in range(len(per))}
    r = {(b, i, j): [spell(per[i])] for b, per in enumerate(rows) for i in range(len(per)) for j in range(len(per))}
    out["consensus_bleu4"] = timed(lambda: Bleu(4).compute_score(g, r), args.iters, 1)
    out["consensus_rouge_l"] = timed(lambda: Rouge().compute_score(g, r), args.iters, 1)
    return "reference_cpu", out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference project: time its CPU scorers instead")
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--refs", type=int, default=5)
    ap.add_argument("--consensus", type=int, nargs=2, default=[16, 16], metavar=("B", "N"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cands, refs = make_corpus(args.images, args.refs)
    block = make_consensus(*args.consensus)
    key, section = (run_reference if args.reference else run_device)(args, cands, refs, block)
    section["shape"] = {"images": args.images, "refs": args.refs, "consensus": args.consensus}
    print(json.dumps({key: section}))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc[key] = section
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
