#!/usr/bin/env python3
"""What every search flavour enqueues and returns, as text that two builds can be compared by (diff): TINY geometry, the
synthetic "eos" checkpoint, four synthetic images, fp32, max_seq_len 12.  For each flavour: the (family, detail) of every
launch ops.profile() records (repeated blocks — the steps — written once with their count, a start shared with an earlier
flavour named; both without loss), the token lists, and the SHA-256 of the log-prob tensor's bytes (consensus_caption: of
its scores; word_attention: of its maps).  Only public methods are called, so the same file runs on an older build.

    python3 tools/search_trace.py > trace.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOS, EOS, N_IMG, MAX_LEN = 3, 2, 4, 12


def fold(lines):
    """The lines with every immediate repetition of a block written once, as "r x [" block "]" (at each line the period
    that saves most; blocks fold again inside).  Nothing is lost: equal lists give equal text and unequal lists unequal."""
    out, i = [], 0
    while i < len(lines):
        saved, period, reps = 0, 1, 1
        for p in range(1, (len(lines) - i) // 2 + 1):
            r = 1
            while lines[i + r * p:i + (r + 1) * p] == lines[i:i + p]:
                r += 1
            if p * (r - 1) > saved:
                saved, period, reps = p * (r - 1), p, r
        if reps > 1:
            out += [f"{reps} x ["] + ["  " + line for line in fold(lines[i:i + period])] + ["]"]
        else:
            out.append(lines[i])
        i += period * reps
    return out


def print_launches(launches, earlier):
    """A flavour's launch lines, short enough to read: a start shared with an earlier flavour (the encoder pass, mostly)
    is named, not repeated — the earlier flavour with the longest common start, the first of them — and the rest folded."""
    name, n = None, 0
    for other, lines in earlier.items():
        k = next((j for j, (a, b) in enumerate(zip(launches, lines)) if a != b), min(len(launches), len(lines)))
        if k > n:
            name, n = other, k
    if n >= 8:
        print(f"the first {n} launches of '{name}'")
    else:
        n = 0
    for line in fold(launches[n:]):
        print(line)


def generated_word_attention(captioner, img):
    """word_attention on captions it generates itself, in the (tokens, tensor) shape of the searches: the tensor is the maps."""
    wa = captioner.word_attention(img)
    return wa.tokens, wa.maps


def main():
    import torch

    from on_device_image_captioning_amd import ops
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.captioning_model import Captioner
    from on_device_image_captioning_amd.End_ExpansionNet_v2 import End_ExpansionNet_v2, make_drop_args
    from on_device_image_captioning_amd.ensemble_captioning_model import EsembleCaptioningModel

    torch.set_grad_enabled(False)
    dev = "cuda:0"
    g = W.TINY

    def build(seed):
        m = End_ExpansionNet_v2(**g.model_kwargs(), output_word2idx={i: i for i in range(g.vocab_size)},
                                output_idx2word=list(range(g.vocab_size)), drop_args=make_drop_args(), rank=dev)
        m.load_state_dict(W.synth_state_dict(g, seed=seed, variant="eos", eos_idx=EOS), strict=True)
        m = m.to(dev).eval().set_precision("fp32")
        m.sampling_seed = 7
        return m

    model = build(0)
    ens = EsembleCaptioningModel([model, build(1)], rank=dev)
    img = W.synth_images(N_IMG, g).to(dev)
    pads = [0] * N_IMG
    beam = dict(sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=2, max_seq_len=MAX_LEN)
    cons = dict(no_repeat_ngram_size=2, min_length=5)
    args = dict(sos_idx=SOS, eos_idx=EOS, beam_size=3, how_many_outputs=2, beam_max_seq_len=MAX_LEN, sample_max_seq_len=MAX_LEN,
                num_groups=3, group_size=3)
    flavours = [
        ("beam 3", lambda: model.beam_search(img, pads, **beam)),
        ("beam 3, sample", lambda: model.beam_search(img, pads, sample_or_max="sample", **beam)),
        ("diverse 3x3", lambda: model.diverse_beam_search(img, pads, sos_idx=SOS, eos_idx=EOS, num_groups=3, group_size=3,
                                                          max_seq_len=MAX_LEN)),
        ("beam 3, constrained", lambda: model.beam_search(img, pads, **beam, **cons)),
        ("ensemble of 2, beam 3", lambda: ens.ensemble_beam_search(img, pads, **beam)),
        ("ensemble of 2, beam 3, constrained", lambda: ens.ensemble_beam_search(img, pads, **beam, **cons)),
        ("ensemble of 2, beam 3, sample", lambda: ens.ensemble_beam_search(img, pads, sample_or_max="sample", **beam)),
        ("mode=sampling", lambda: model(enc_x=img, enc_x_num_pads=pads, mode="sampling", **args)),
        ("forward(mode=beam_search)", lambda: model(enc_x=img, enc_x_num_pads=pads, mode="beam_search", **args)),
        ("forward(mode=beam_search), constrained", lambda: model(enc_x=img, enc_x_num_pads=pads, mode="beam_search", **args,
                                                                 **cons)),
        ("forward(mode=diverse_beam_search)", lambda: model(enc_x=img, enc_x_num_pads=pads, mode="diverse_beam_search",
                                                            **args)),
        ("ensemble forward(mode=beam_search)", lambda: ens(enc_x=img, enc_x_num_pads=pads, mode="beam_search", **args)),
        ("Captioner beam_search", lambda: Captioner(args, model=model)(img, enc_x_num_pads=pads, mode="beam_search")),
        ("Captioner sampling", lambda: Captioner(args, model=model)(img, enc_x_num_pads=pads, mode="sampling")),
        ("Captioner diverse_beam_search, constrained",
         lambda: Captioner(dict(args, **cons), model=model)(img, enc_x_num_pads=pads, mode="diverse_beam_search")),
        ("beam 3, prefix", lambda: model.beam_search(img, pads, prefix=[7, 9], **beam)),
        ("beam 2, two required words", lambda: model.beam_search(img, pads, sos_idx=SOS, eos_idx=EOS, beam_size=2,
                                                                 how_many_outputs=2, max_seq_len=MAX_LEN,
                                                                 required_words=[11, 23])),
        ("diverse 3x3, prefix", lambda: model.diverse_beam_search(img, pads, sos_idx=SOS, eos_idx=EOS, num_groups=3,
                                                                  group_size=3, max_seq_len=MAX_LEN,
                                                                  prefix=[[7, 9], [9, 7], [5, 6], [6, 5]])),
        ("stochastic beam 4, seed 11", lambda: model.stochastic_beam_search(img, pads, sos_idx=SOS, eos_idx=EOS, num_samples=4,
                                                                            max_seq_len=MAX_LEN, seed=11)),
        ("contrastive 3, others", lambda: model.contrastive_beam_search(img, pads, distractors="others", **beam)),
        ("contrastive 3, others, constrained", lambda: model.contrastive_beam_search(img, pads, distractors="others", **beam,
                                                                                     **cons)),
        ("ensemble of 2, beam 3, prefix", lambda: ens.ensemble_beam_search(img, pads, prefix=[7, 9], **beam)),
        ("consensus of 4, stochastic_beam, seed 11",
         lambda: model.consensus_caption(img, pads, num_candidates=4, source="stochastic_beam", seed=11, sos_idx=SOS,
                                         eos_idx=EOS, max_seq_len=MAX_LEN)),
        ("Captioner word_attention, captions=None", lambda: generated_word_attention(Captioner(args, model=model), img)),
    ]
    seen = {}
    for name, call in flavours:
        with ops.profile() as recs:
            toks, lps = call()
        torch.cuda.synchronize()
        print(f"== {name}: {len(recs)} launches")
        seen[name] = [f"{r[0]} {r[5]}".rstrip() for r in recs]
        print_launches(seen[name], {k: v for k, v in seen.items() if k != name})
        print("tokens", toks)
        lp = lps.detach().cpu().contiguous()
        print("logprobs", tuple(lp.shape), hashlib.sha256(lp.numpy().tobytes()).hexdigest(), flush=True)


if __name__ == "__main__":
    main()
