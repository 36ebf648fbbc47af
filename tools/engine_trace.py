#!/usr/bin/env python3
"""Every odic_gemm call the engines make, argument by argument, and what they return, as text that two builds can be compared
by (cmp).  odic_gemm on the loaded library object is replaced by a wrapper that records every non-pointer field of
odic_gemm_args and p / - (NULL) for every pointer, then calls the real one; after each run the calls are printed in order
as numbers, a distinct argument list being spelled out once, where it first appears (`gN = ...`).
Two geometries — TINY (fp32; TINY64 for bf16 and x3), and the same with 29 expansion queries and, for the engine-level
calls, 37 encoder tokens, so that no padded size equals its unpadded one: SwinEngine.forward, encode with want_bf16_mem off and on, project_kv, decode_sequence with targets and with
want_logits, one beam search and one prefixed beam search (the prefill pass).  After each run: the SHA-256 of every returned
tensor.  Only public methods are called, so the same file runs on an older build.  The LayerNorm-reading Swin products pick
their tile by a timed race, so they are switched off here, and the tile candidates are pinned as in swin_trace.py.

    python3 tools/engine_trace.py > trace.txt
"""
import ctypes as C
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ODIC_FUSE_BACKBONE_LN_READ", "0")
os.environ.setdefault("ODIC_TILE_CANDIDATES", "1")
os.environ.setdefault("ODIC_X3_TILE_CANDIDATES", "0")

SOS, EOS, N_IMG, MAX_LEN, T_SEQ = 3, 2, 2, 6, 5


def main():
    import torch

    from on_device_image_captioning_amd import _hip
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    from on_device_image_captioning_amd.engine import CaptionerEngine, SwinEngine

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _hip.load()
    real = lib.odic_gemm

    calls, ids = [], {}

    def recording(argref, stream):
        a = argref._obj
        calls.append(" ".join(("-" if not getattr(a, n) else "p") if t is C.c_void_p else repr(getattr(a, n))
                              for n, t in a._fields_))
        return real(argref, stream)

    def flush_calls():
        """The calls since the last flush, in order, as numbers; an argument list is spelled out where it first appears."""
        for c in calls:
            if c not in ids:
                ids[c] = len(ids) + 1
                print(f"g{ids[c]} = {c}")
        seq = [str(ids[c]) for c in calls]
        for i in range(0, len(seq), 40):
            print("calls", " ".join(seq[i:i + 40]))
        calls.clear()

    lib.odic_gemm = recording
    print("# gN =", " ".join(n for n, _ in _hip.GemmArgs._fields_), "(pointers: p, or - for NULL)")

    def sha(name, t):
        t = t.detach().cpu().contiguous()
        print(name, str(t.dtype), tuple(t.shape), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest(), flush=True)

    def run(title, call):
        print("==", title)
        out = call()
        torch.cuda.synchronize()
        flush_calls()
        if isinstance(out, dict):
            for k in sorted(out):
                sha(k, out[k])
        else:
            for i, t in enumerate(out if isinstance(out, (tuple, list)) else (out,)):
                sha(f"out{i}", t)
        return out

    # (the bf16 / split-fp16 products want K % 64 / 32 == 0: those precisions run TINY64, whose Swin widths are 128·2^s)
    geometries = [(f"{n}{tag}", p, dataclasses.replace(g, **kw), S_feat)
                  for tag, kw, S_feat in (("", {}, None), (" nq=29 S=37", {"num_exp_enc_list": (8, 16, 5)}, 37))
                  for n, g, p in (("TINY", W.TINY, ("fp32",)), ("TINY64", W.TINY64, ("bf16", "x3")))]
    for gname, precisions, g, S_feat in geometries:
        sd = W.synth_state_dict(g, seed=0, variant="eos", eos_idx=EOS)
        img = W.synth_images(N_IMG, g).to(dev)
        tokens = (torch.arange(2 * N_IMG * T_SEQ, dtype=torch.int64, device=dev).view(2 * N_IMG, T_SEQ) * 7 + 5) % g.vocab_size
        targets = (tokens * 3 + 1) % g.vocab_size
        dec_len = torch.tensor([T_SEQ, 3, 1, T_SEQ - 1], dtype=torch.int32, device=dev)
        for precision in precisions:
            tag = f"{gname} {precision}:"
            swin, cap = SwinEngine(sd, g, dev, precision), CaptionerEngine(sd, g, dev, precision)
            feats = run(f"{tag} SwinEngine.forward", lambda: swin.forward(img, out_dtype=cap.cdt))
            inputs = [("", feats)]
            if S_feat is not None:
                inputs.append((f" S={S_feat}", W.synth_features(N_IMG, S_feat, g.final_swin_dim, seed=5).to(dev)))
            for stag, x in inputs:
                S = x.shape[1]
                enc_len = torch.tensor([S, S - 3], dtype=torch.int32, device=dev)
                mem = run(f"{tag} encode{stag}", lambda: cap.encode(x, enc_len))
                run(f"{tag} encode{stag} want_bf16_mem", lambda: cap.encode(x, enc_len, want_bf16_mem=True))
                kv = run(f"{tag} project_kv{stag}", lambda: cap.project_kv(mem))
                run(f"{tag} decode_sequence{stag} targets",
                    lambda: cap.decode_sequence(tokens, dec_len, kv, enc_len, N_IMG, targets=targets))
                run(f"{tag} decode_sequence{stag} want_logits",
                    lambda: cap.decode_sequence(tokens, dec_len, kv, enc_len, N_IMG, want_logits=True, row_chunk=8))
            model = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                                        output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=dev)
            model.load_state_dict(sd, strict=True)
            model = model.to(dev).eval().set_precision(precision)
            beam = dict(sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=2, max_seq_len=MAX_LEN)
            for title, kw in (("beam_search", {}), ("beam_search prefix", {"prefix": [5, 6]})):
                print("==", f"{tag} {title}")
                toks, lps = model.beam_search(img, [0] * N_IMG, **beam, **kw)
                torch.cuda.synchronize()
                flush_calls()
                print("tokens", toks)
                sha("logprobs", lps)
            del swin, cap, model


if __name__ == "__main__":
    main()
