#!/usr/bin/env python3
"""Timing of the tail of a search step — odic_logsoftmax_topk and odic_beam_step (with the embedding tail) — against k
(beams) and V, back to back inside one hipGraph (the beam state re-armed by odic_beam_reset before every step pair)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from on_device_image_captioning_amd import _hip, ops

s = torch.cuda.Stream()


def graph_time(fn, reps=32):
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        g.replay()
        st.record()
        for _ in range(5):
            g.replay()
        en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) * 1e3 / (5 * reps)


def beam_state(n_img, k, T):
    N = n_img * k
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device="cuda")      # noqa: E731
    t = dict(tokens=z(n_img, k, T, dt=torch.int64), logprobs=z(n_img, k, T), anc=z(N, T, dt=torch.int32), cumul=z(N),
             n_elem=z(N, dt=torch.int32), has_eos=z(N, dt=torch.int32), row_valid=z(N, dt=torch.int32),
             next_tok=z(N, dt=torch.int64), pos=z(1, dt=torch.int32), done=z(1, dt=torch.int32), ctr=z(1, dt=torch.int32))
    st = _hip.BeamState(*(t[n].data_ptr() for n in ("tokens", "logprobs", "anc", "cumul", "n_elem", "has_eos",
                                                    "row_valid", "next_tok", "pos", "done", "ctr")))
    return t, st


def main():
    n_img, T, d = 16, 74, 512
    for V in (10000, 2000):
        for k in (1, 2, 3, 5, 8):
            N = n_img * k
            lg = torch.randn(N, V, device="cuda")
            cv, ci = torch.zeros(N, k, device="cuda"), torch.zeros(N, k, dtype=torch.int32, device="cuda")
            t_topk = graph_time(lambda: ops.logsoftmax_topk(lg, V, None, 0, cv, ci, N, V, k))
            t, st = beam_state(n_img, k, T)
            embed, ptab, y = torch.randn(V, d, device="cuda"), torch.randn(T, d, device="cuda"), torch.zeros(N, d, device="cuda")
            emb = ops.embed_args(embed, ptab, y, d, d, 1.0)

            def steps(n):           # reset, then n steps: position 0 (one row per image seeds), position 1 (k rows per image)
                ops.beam_reset(st, n_img, k, T, 3, emb=emb)
                for _ in range(n):
                    ops.logsoftmax_topk(lg, V, None, 0, cv, ci, N, V, k)
                    ops.beam_step(cv, ci, st, n_img, k, T, 4, emb=emb)

            t0, t1, t2 = (graph_time(lambda n=n: steps(n)) for n in (0, 1, 2))
            print(f"V={V:5d} k={k}: logsoftmax_topk ({N} rows) {t_topk:6.2f} us | reset {t0:5.2f} | topk + beam_step at pos 0 "
                  f"{t1 - t0:6.2f}, at pos 1 {t2 - t1:6.2f}", flush=True)


if __name__ == "__main__":
    main()
