#!/usr/bin/env python3
"""Per-step time of the decode chain (decoder → log-softmax / top-k → selection) for a search form, alone on the chip:
FULL geometry, features-only model, 16 images, fp32, HIP events around the step loop of one search (19 steps, no `done`
poll), median and spread over the runs.  The loop is captured into one hipGraph and replayed (as CaptionPipeline runs
it: the figure is the device's, free of host launch jitter); --eager times the plain enqueue loop instead.

    python3 tools/search_step_bench.py [--runs 7] [--images 16] [--eager] beam:3 beam:9 diverse:3x3 cbeam:3 cbeam:9 cbeam:3:1 pbeam:3:6 rbeam:3:2 sample:3 sample:3:20:0.9:0.8 poolbeam:3

cbeam:K is beam:K under constraints: no_repeat_ngram_size=2, min_length=5 and 8 banned words; the step then
holds one launch more (odic_topk_rows_constrained) and the top-k launch writes the log-prob rows.
pbeam:K:P is beam:K behind a prefix of P words: one whole-sequence pass over the prefix that fills the step
caches (CaptionerEngine.seed_prefix) and max_len - 1 - P steps; compare its time per SEARCH with beam:K's.
rbeam:K:C is the search for captions that contain C required words: 2^C banks of K beams per image (words
300 .. 300+C-1 for every image); the top-k launch writes the log-prob rows and the selection is odic_require_beam_step.  Compare
it with diverse:GxK' at the same number of rows per image.
sample:K[:topk:topp:temp] is the step of beam_search(sample_or_max='sample') with K beams: the decoder, the k draws per row
and the beam bookkeeping.  sample:K draws with odic_logsoftmax_sample; with the three controls given, e.g.
sample:3:20:0.9:0.8, with odic_logsoftmax_sample_filtered: the difference of the two is the cost of the filter per step.
sbeam:K is the step of stochastic_beam_search(num_samples=K): K + 1 rows per image, the decoder, the scored
draws (odic_logsoftmax_sample_scored) and odic_stochastic_beam_step.  Compare it with beam:K+1, the same rows per image.
cbeam:K:D (two numbers) is the step of contrastive_beam_search with K beams and D distractor images per image
(image i against images i+1 .. i+D of the batch): 1 + D decoder passes on one shared beam state, one odic_contrast_topk launch
and odic_beam_step.  Compare it with beam:K.  A second line times the row launch alone against the composition the library
could already form — 1 + D odic_logsoftmax_topk launches that write their log-prob rows, an elementwise combine (torch) and
odic_topk_rows — on the same logits, alternating the two, HIP events around 200 launches each.
poolbeam:K is the step of pool_beam_search(beam_size=K): the decoder, the top-k launch that writes the log-prob
rows, odic_topk_rows_constrained with EOS inadmissible and odic_pool_beam_step, length_penalty 1, no early stopping (the graph
holds all 19 steps; a closed image's block only arrives).  Compare it with cbeam:K, the same launches with odic_beam_step.  A
second line counts the steps an eager search runs until the device raises `done` (looked at after every step), with
early_stopping off and on.
A form this build does not have (diverse on a build before ABI 25, cbeam before ABI 26, pbeam before seed_prefix, rbeam
before odic_require_beam_step, sbeam before odic_stochastic_beam_step, poolbeam before odic_pool_beam_step) is reported as
absent.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import bench
    from on_device_image_captioning_amd import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=20)
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("forms", nargs="+")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    model, _, g = bench.build_model(dev, "fp32", "features48")
    eng = model._captioner_engine()
    feats = torch.randn(a.images, 144, g.final_swin_dim, device=dev, generator=torch.Generator(dev).manual_seed(1))
    mem = model.forward_enc(feats, [0] * a.images)
    kv = eng.project_kv(mem)
    enc_len = model._enc_lens(a.images, mem.shape[1], [0] * a.images)
    steps, T = a.max_len - 1, a.max_len
    for form in a.forms:
        kind, shape = form.split(":", 1)
        P = 0
        if kind == "pbeam":
            shape, P = shape.split(":")
            P = int(P)
            if not hasattr(eng, "seed_prefix"):
                print(f"{form}: not in this build")
                continue
        if kind == "sample":
            shape, *ctl = shape.split(":")
            R, flt = int(shape), None
            if ctl:
                if len(ctl) != 3 or not hasattr(ops, "logsoftmax_sample_filtered"):
                    print(f"{form}: not in this build" if len(ctl) == 3 else f"{form}: give topk:topp:temp, or none of them")
                    continue
                flt = ops.sample_filter(float(ctl[2]), int(ctl[0]), float(ctl[1]))
            V = eng.g.vocab_size

            def one(st, flt=flt, V=V, R=R):
                eng.step_logits(st)
                if flt is None:
                    ops.logsoftmax_sample(st.logits, V, None, 0, st.cand_val, st.cand_idx, st.N, V, R, 7, st.pos)
                else:
                    ops.logsoftmax_sample_filtered(st.logits, V, None, 0, st.cand_val, st.cand_idx, None, st.N, V, R, flt, 7,
                                                   st.pos)
                ops.beam_step(st.cand_val, st.cand_idx, st.beam_state, st.n_img, st.beams, st.T, bench.EOS)
        elif kind == "rbeam":
            shape, C = shape.split(":")
            kb, C = int(shape), int(C)
            if not hasattr(eng, "require_beam_step"):
                print(f"{form}: not in this build")
                continue
            R = kb << C
            req = torch.arange(300, 300 + C, device=dev).repeat(a.images, 1)
            one = lambda st: eng.require_beam_step(st, bench.EOS, req, kb)         # noqa: E731
        elif kind == "sbeam":
            if not hasattr(eng, "stochastic_beam_step"):
                print(f"{form}: not in this build")
                continue
            R = int(shape) + 1
            one = lambda st: eng.stochastic_beam_step(st, bench.EOS, 7)            # noqa: E731
        elif kind == "poolbeam":
            if not hasattr(eng, "pool_beam_step"):
                print(f"{form}: not in this build")
                continue
            R = int(shape)
        elif kind == "cbeam" and ":" in shape:
            shape, D = shape.split(":")
            R, D = int(shape), int(D)
            if not hasattr(eng, "contrast_beam_step") or not 0 <= D <= 7 or D >= a.images:
                print(f"{form}: not in this build" if not hasattr(eng, "contrast_beam_step") else f"{form}: D must lie in [0, 7] and below --images")
                continue
            kind = "contrast"
        elif kind == "diverse":
            G, kg = (int(v) for v in shape.split("x"))
            if not hasattr(eng, "group_beam_step"):
                print(f"{form}: not in this build")
                continue
            R = G * kg
            one = lambda st: eng.group_beam_step(st, bench.EOS, G, a.penalty)      # noqa: E731
        else:
            R = int(shape)
            one = lambda st: eng.beam_step(st, bench.EOS)                          # noqa: E731
        if kind == "cbeam" and not hasattr(eng, "search_constraints"):
            print(f"{form}: not in this build")
            continue
        st = eng.new_state(a.images, R, T, kv, enc_len)
        if kind == "cbeam":
            cons = eng.search_constraints(st, bench.EOS, no_repeat_ngram=2, min_words=5,
                                          banned=[w for w in range(100, 110) if w not in (bench.SOS, bench.EOS)][:8])
            one = lambda st: eng.beam_step(st, bench.EOS, constraints=cons)        # noqa: E731
        pool = None
        if kind == "poolbeam":
            pool = ops.Pool(a.images, R, T, 1.0, 0, False, dev)
            pcons = eng.pool_constraints(st, bench.EOS)
            one = lambda st: eng.pool_beam_step(st, pool, bench.EOS, pcons)        # noqa: E731
        if kind == "contrast":
            from on_device_image_captioning_amd import search as _search
            states = [st]
            for d in range(D):
                idx = (torch.arange(a.images, device=dev) + 1 + d) % a.images
                states.append(eng.new_state(a.images, R, T, kv.index_select(0, idx).contiguous(), enc_len.index_select(0, idx)))
            _search.share_beam_state(states)
            count = torch.full((st.N,), D, dtype=torch.int32, device=dev)
            cargs = ops.contrast_args(0.5, 0.1, -20.0, R)
            one = lambda st: eng.contrast_beam_step(states, count, cargs, bench.EOS)   # noqa: E731
        prefix = torch.arange(200, 200 + P, device=dev).repeat(a.images, 1) if P else None

        def search():
            if P:
                eng.seed_prefix(st, prefix, bench.SOS)
            else:
                ops.beam_reset(st.beam_state, a.images, R, T, bench.SOS, emb=None if kind in ("sample", "contrast") else st.emb)
            if pool is not None:
                ops.pool_reset(pool.args, a.images)
            for _ in range(steps - P):
                one(st)

        graph = None
        if not a.eager:
            side = torch.cuda.Stream(dev)
            with torch.cuda.stream(side):
                search()                                                           # warm-up outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                search()
        times = []
        for run in range(a.runs + 2):                                              # two warm-up searches
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay() if graph is not None else search()
            e1.record()
            torch.cuda.synchronize()
            if run >= 2:
                times.append(e0.elapsed_time(e1) * 1000.0 / steps)
        print(f"{form} ({'eager' if a.eager else 'graph'}): rows/image {R}, {steps - P} steps, per step median {statistics.median(times):.1f} us, "
              f"min {min(times):.1f}, max {max(times):.1f} ({a.runs} runs); per search median "
              f"{statistics.median(times) * steps:.0f} us", flush=True)
        if kind == "contrast":
            rows_alone(ops, states, count, cargs, R, form)
        if kind == "poolbeam":
            ran = {}
            for early in (False, True):
                pool = ops.Pool(a.images, R, T, 1.0, 0, early, dev)
                ops.beam_reset(st.beam_state, a.images, R, T, bench.SOS, emb=st.emb)
                ops.pool_reset(pool.args, a.images)
                n = 0
                while n < steps and not int(st.done.item()):
                    one(st)
                    n += 1
                ran[early] = (n, int((pool.closed != 0).sum().item()))
            print(f"{form} steps until done (eager, of {steps}): early_stopping off {ran[False][0]} ({ran[False][1]} of {a.images} images "
                  f"closed), on {ran[True][0]} ({ran[True][1]} closed)", flush=True)


def rows_alone(ops, states, count, cargs, k, form, reps=200, rounds=5):
    """The fused row launch against (1 + D) odic_logsoftmax_topk + combine + odic_topk_rows on the states' last logits."""
    import torch
    lg = [s.logits for s in states]
    N, V = lg[0].shape
    D = len(lg) - 1
    tv, ti = states[0].cand_val, states[0].cand_idx
    lp = [torch.empty_like(x) for x in lg]
    w, floor, la = cargs.weight, cargs.floor, cargs.log_alpha

    def fused():
        ops.contrast_topk(lg, count, cargs, tv, ti, k)

    def composed():
        for x, o in zip(lg, lp):
            ops.logsoftmax_topk(x, V, o, V, tv, ti, N, V, k)
        if D:
            s = lp[1] if D == 1 else torch.logsumexp(torch.stack(lp[1:]), 0) - math.log(D)
            out = lp[0] - w * s.clamp_(min=floor)
        else:
            out = lp[0]
        out = out.masked_fill(lg[0] - lg[0].max(-1, keepdim=True).values < la, float("-inf"))
        ops.topk_rows(out, tv, ti, k)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / reps

    for fn in (fused, composed):
        timed(fn)                                                                  # warm-up
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(timed(fused))
        tc.append(timed(composed))
    byt = 4.0 * (1 + D) * N * V
    print(f"{form} rows alone (eager, {N} rows x {V} words, {1 + D} logits rows each): fused median {statistics.median(tf):.1f} us "
          f"(min {min(tf):.1f}, max {max(tf):.1f}; {byt / statistics.median(tf) / 1e3:.1f} GB/s of logits read), composed "
          f"{statistics.median(tc):.1f} us (min {min(tc):.1f}, max {max(tc):.1f}; {2 + D + (3 if D else 1) + (2 if D > 1 else 0)}+ launches)",
          flush=True)


if __name__ == "__main__":
    main()
