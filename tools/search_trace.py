#!/usr/bin/env python3
"""What every search flavour enqueues and returns, as text that two builds can be compared by (diff): TINY geometry, the
synthetic "eos" checkpoint, four synthetic images, fp32, max_seq_len 12.  For each flavour: the (family, detail) of every
launch ops.profile() records, the token lists, and the SHA-256 of the log-prob tensor's bytes.  Only public methods are
called, so the same file runs on an older build.

    python3 tools/search_trace.py > trace.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOS, EOS, N_IMG, MAX_LEN = 3, 2, 4, 12


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
    ]
    for name, call in flavours:
        with ops.profile() as recs:
            toks, lps = call()
        torch.cuda.synchronize()
        print(f"== {name}")
        for r in recs:
            print(f"{r[0]} {r[5]}".rstrip())
        print("tokens", toks)
        lp = lps.detach().cpu().contiguous()
        print("logprobs", tuple(lp.shape), hashlib.sha256(lp.numpy().tobytes()).hexdigest(), flush=True)


if __name__ == "__main__":
    main()
