"""Time caption scoring: the whole-sequence pass (score_captions' decoder side) against the step-replay route to the
same numbers (forward_dec(apply_log_softmax=True) + gather at the targets), FULL decoder geometry on fixed encoder
memory so that the encoder is outside the timing.

    python tools/score_bench.py [--pairs 20] [--shapes 48x19,80x73] [--profile] [--once NxT] [--out FILE]

The two paths are timed interleaved in one process, HIP events around each call, median and spread over the pairs;
peak extra device memory of one call (torch.cuda.max_memory_allocated deltas) at every shape.  Prints one JSON line.
Both timed calls start from the encoder memory: each includes its cross-attention K/V projection (per image in the new
path, per caption row in the step replay).
--profile adds the launch count of one call of either path (ops.profile).  --once NxT runs a warm-up call and then one
whole-sequence call, for a kernel trace; --trace-stats TRACE.csv OUT.csv reduces a rocprofv3 kernel trace of such a run
to the statistics of that LAST call alone (its K/V projection, then everything from the last odic_dec_embed_seq launch on).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from on_device_image_captioning_amd import ops, weights as W                      # noqa: E402
from on_device_image_captioning_amd.End_ExpansionNet_v2 import make_drop_args     # noqa: E402
from on_device_image_captioning_amd.ExpansionNet_v2 import ExpansionNet_v2         # noqa: E402

DEV = "cuda:0"
PER_IMAGE = {48: 3, 80: 5}


def build():
    g, fd = W.FULL, 1536
    m = ExpansionNet_v2(d_model=g.d_model, N_enc=g.N_enc, N_dec=g.N_dec, ff=g.ff, num_heads=g.num_heads,
                        num_exp_enc_list=list(g.num_exp_enc_list), num_exp_dec=g.num_exp_dec,
                        output_word2idx={i: i for i in range(g.vocab_size)}, output_idx2word=list(range(g.vocab_size)),
                        max_seq_len=g.max_seq_len, drop_args=make_drop_args(), img_feature_dim=fd, rank=DEV)
    m.load_state_dict(W.synth_state_dict(g, end_to_end=False, img_feature_dim=fd, variant="eos", eos_idx=77), strict=True)
    return m.to(DEV).eval(), g, fd


def case(m, g, fd, N, T):
    per = PER_IMAGE.get(N, 1)
    n_img = N // per
    eng = m._captioner_engine()
    mem = m.forward_enc(W.synth_features(n_img, 144, fd).to(DEV), [0] * n_img)
    gen = torch.Generator().manual_seed(N * 1000 + T)
    y = torch.randint(4, g.vocab_size, (N, T + 1), generator=gen)
    lens = torch.randint(max(2, T // 2), T + 2, (N,), generator=gen).clamp(max=T + 1)
    lens[0] = T + 1
    dec, tgt = y[:, :-1].contiguous().to(DEV), y[:, 1:].contiguous().to(DEV)
    dec_len = (lens - 1).to(torch.int32).to(DEV)
    pads = (T - (lens - 1)).tolist()
    enc_len = m._enc_lens(n_img, 144, [0] * n_img)
    mem_rows = mem.repeat_interleave(per, 0)

    def new():          # the K/V projection is part of the call on both sides: once per image here, once per row in old()
        return eng.decode_sequence(dec, dec_len, eng.project_kv(mem), enc_len, n_img, targets=tgt)["logp"]

    def old():
        lp = m.forward_dec(mem_rows, [0] * N, dec, pads, apply_log_softmax=True)
        return lp.gather(-1, tgt[..., None])[..., 0]
    return new, old, dec_len


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del out
    return p


def launches(fn):
    with ops.profile() as recs:
        fn()
        n = len(recs)
    torch.cuda.synchronize()
    return n


def trace_stats(trace_csv, out_csv):
    """Per-kernel statistics of the last score call in a rocprofv3 kernel trace (columns as rocprofv3 --stats writes them)."""
    import csv
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    last = max(i for i, r in enumerate(rows) if "dec_embed_seq_kernel" in r["Kernel_Name"])
    first = last - 1 if last > 0 and "gemm_f32" in rows[last - 1]["Kernel_Name"] else last      # the K/V projection
    agg = {}
    for r in rows[first:]:
        agg.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(v) for v in agg.values())
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
        for name, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(v), sum(v), round(sum(v) / len(v), 1), round(100.0 * sum(v) / total, 2), min(v), max(v)])
        w.writerow(["(all kernels of the call)", sum(len(v) for v in agg.values()), total, "", 100.0, "", ""])
        w.writerow(["(first launch to last end, ns)", "", int(rows[-1]["End_Timestamp"]) - int(rows[first]["Start_Timestamp"]),
                    "", "", "", ""])


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--trace-stats":
        return trace_stats(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--shapes", default="48x19,80x73")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    m, g, fd = build()
    if a.once:
        N, T = (int(v) for v in a.once.split("x"))
        new, _, _ = case(m, g, fd, N, T)
        new()
        torch.cuda.synchronize()
        new()
        torch.cuda.synchronize()
        return
    res = {"metric": "score_captions_decoder_ms", "geometry": "FULL decoder, fixed encoder memory", "pairs": a.pairs,
           "shapes": []}
    for sh in a.shapes.split(","):
        N, T = (int(v) for v in sh.split("x"))
        new, old, dec_len = case(m, g, fd, N, T)
        ln, lo = new(), old()
        real = torch.arange(T, device=DEV)[None, :] < dec_len[:, None]
        diff = float((ln - lo)[real].abs().max())
        for _ in range(2):
            new(), old()
        tn, to = [], []
        for _ in range(a.pairs):
            tn.append(timed(new))
            to.append(timed(old))
        ratios = sorted(o / n for o, n in zip(to, tn))
        rec = {"N": N, "T": T, "new_ms_median": statistics.median(tn), "new_ms_min": min(tn), "new_ms_max": max(tn),
               "old_ms_median": statistics.median(to), "old_ms_min": min(to), "old_ms_max": max(to),
               "pair_diff_ms_min": min(o - n for o, n in zip(to, tn)),
               "pair_diff_ms_spread": max(o - n for o, n in zip(to, tn)) - min(o - n for o, n in zip(to, tn)),
               "ratio_median": statistics.median(ratios), "ratio_min": ratios[0], "ratio_max": ratios[-1],
               "max_abs_logprob_diff": diff,
               "peak_extra_bytes_new": peak(new), "peak_extra_bytes_old": peak(old)}
        if a.profile:
            rec["launches_new"], rec["launches_old"] = launches(new), launches(old)
        res["shapes"].append(rec)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
