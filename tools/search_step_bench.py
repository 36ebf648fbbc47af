#!/usr/bin/env python3
"""Per-step time of the decode chain (decoder → log-softmax / top-k → selection) for a search form, alone on the chip:
FULL geometry, features-only model, 16 images, fp32, HIP events around the step loop of one search (19 steps, no `done`
poll), median and spread over the runs.  The loop is captured into one hipGraph and replayed (as CaptionPipeline runs
it: the figure is the device's, free of host launch jitter); --eager times the plain enqueue loop instead.

    python3 tools/search_step_bench.py [--runs 7] [--images 16] [--eager] beam:3 beam:9 diverse:3x3 cbeam:3 cbeam:9 pbeam:3:6 rbeam:3:2 sample:3 sample:3:20:0.9:0.8

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
A form this build does not have (diverse on a build before ABI 25, cbeam before ABI 26, pbeam before seed_prefix, rbeam
before odic_require_beam_step, sbeam before odic_stochastic_beam_step) is reported as absent.
"""
import argparse
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
        prefix = torch.arange(200, 200 + P, device=dev).repeat(a.images, 1) if P else None

        def search():
            if P:
                eng.seed_prefix(st, prefix, bench.SOS)
            else:
                ops.beam_reset(st.beam_state, a.images, R, T, bench.SOS, emb=None if kind == "sample" else st.emb)
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


if __name__ == "__main__":
    main()
