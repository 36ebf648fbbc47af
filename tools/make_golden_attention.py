"""Generate tests/golden/tiny_attention.npz by running the REAL reference on the CPU (build container only).

    python tools/make_golden_attention.py

The reference's legacy models are run teacher-forced as in tools/make_golden_scoring.py, with a forward pre-hook on the
cross attention of every decoder layer (`decoders[i].mha`).  The hook sees the module's own inputs (q, k, mask); from those
and the module's own Wq / Wk the softmax of the masked scores is recomputed exactly as MultiHeadAttention.forward
(layers.py:236-250) computes it — the module itself never returns it.  Recorded, data only:
  e2e.*   TINY xavier, the tokens and pads of tiny_scoring.npz `xavier.fresh.*` (3 images x 2 captions, lengths 2 … 24):
          the head-mean maps of every layer, fp32 [6, N_dec, 23, 144]; the per-head maps of captions 0 and 2; the peak
          position and the top-1/top-2 margin of the layer- and head-mean map.  (The `eos` checkpoint only rescales
          vocab_linear, which the maps do not see.)
  feat.*  the features-only TINY model with the inputs and ragged encoder pads of tiny_features.npz, one caption per input
          (the first four of make_golden_scoring.fresh_captions): head-mean maps of every layer.  The reference's own maps
          are asserted to be exactly 0 at padded keys.
Rows behind a caption's end are stored as zeros.  Printed for every set, and the set is refused otherwise:
  * the largest difference between the recorded fp32 maps and an fp64 restatement from oracle.expansionnet_ref pieces;
  * the share of real positions whose top-1/top-2 margin on the layer- and head-mean map is at most twice the bound of the
    GPU tests, 2·2e-4·max(map) (where the peak position is not compared); above 1 % the set is refused.
"""
from __future__ import annotations

import math
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from on_device_image_captioning_amd import weights as W          # noqa: E402
from oracle import expansionnet_ref as R                          # noqa: E402
from oracle import make_golden as MG                              # noqa: E402
from tools import make_golden_scoring as MS                       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tiny_attention.npz")
MAP_BOUND = 2e-4                  # of scale: LP_BOUND["xavier"], tests/test_scoring_gpu.py
MARGIN_CAP = 0.01
RESTATEMENT_BOUND = 1e-6
PER_HEAD_CAPTIONS = (0, 2)
FEAT_DIM, FEAT_LEN, FEAT_PADS = 64, 20, [0, 3, 7, 1]       # oracle/make_golden.py, the tiny_features.npz set


def hooked_maps(ref, n_dec, **fwd):
    """Run the reference forward; → [N, n_dec, H, T, S] fp32, the softmax each decoders[i].mha computed inside."""
    got, handles = {}, []

    def make(i):
        def pre(mod, args, kwargs):
            q, k, mask = kwargs["q"], kwargs["k"], kwargs["mask"]
            B, T, _ = q.shape
            S = k.size(1)
            kp = mod.Wk(k).view(B, S, mod.num_heads, mod.d_k).transpose(2, 1)
            qp = mod.Wq(q).view(B, T, mod.num_heads, mod.d_k).transpose(2, 1)
            s = torch.matmul(qp, kp.transpose(3, 2)) / mod.d_k ** 0.5
            s = s.masked_fill(mask.unsqueeze(1).repeat(1, mod.num_heads, 1, 1) == 0, value=-1e4)
            got[i] = torch.softmax(s, dim=-1)
        return pre

    for i in range(n_dec):
        handles.append(ref.decoders[i].mha.register_forward_pre_hook(make(i), with_kwargs=True))
    try:
        ref(**fwd, apply_log_softmax=False, mode="forward")
    finally:
        for h in handles:
            h.remove()
    return torch.stack([got[i] for i in range(n_dec)], 1)


def restated_maps(sd, g, mem, tokens, dec_pads, enc_pads):
    """The same probabilities in fp64 from the oracle's pieces (decoder_forward with the softmax kept): [N, L, H, T, S]."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    mem = mem.double()
    N, T = tokens.shape
    S, H = mem.shape[1], g.num_heads
    dk = g.d_model // H
    causal, allow = R._dec_masks(N, T, S, dec_pads, enc_pads)
    y = sd["out_embedder.embed.weight"][tokens] * math.sqrt(g.d_model) + sd["pos_encoder.weight"][:T]
    maps = []
    for i in range(g.N_dec):
        p = f"decoders.{i}"
        y = y + R.dynamic_expansion(sd, p + ".dyn_exp", R._ln(sd, p + ".norm_1", y), g.num_exp_dec, causal.double())
        x2 = R._ln(sd, p + ".norm_2", y)
        q = R._linear(sd, p + ".mha.Wq", x2).view(N, T, H, dk).transpose(1, 2)
        k = R._linear(sd, p + ".mha.Wk", mem).view(N, S, H, dk).transpose(1, 2)
        s = (torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dk)).masked_fill(allow[:, None] == 0, -1e4)
        maps.append(torch.softmax(s, -1))
        y = y + R.cross_attention(sd, p + ".mha", x2, mem, H, allow)
        y = y + R.feed_forward(sd, p + ".ff", R._ln(sd, p + ".norm_3", y))
    return torch.stack(maps, 1)


def record(store, name, maps, oracle, y, pads, enc_pads, per_head_rows=()):
    """maps [N, L, H, T, S] fp32 from the reference, oracle the fp64 restatement."""
    N, Ty = y.shape
    S = maps.shape[-1]
    real = torch.arange(Ty - 1)[None, :] < (Ty - 1 - torch.tensor(pads))[:, None]
    diff = float((maps.double() - oracle)[real[:, None, None, :, None].expand_as(maps)].abs().max())
    print(f"{name}: recorded fp32 maps vs the fp64 restatement, max difference {diff:.3e}")
    if diff > RESTATEMENT_BOUND:
        raise SystemExit(f"{name}: the restatement differs by {diff:.3e}; set refused")
    key_ok = torch.arange(S)[None, :] < (S - torch.tensor(enc_pads))[:, None]             # [N, S]
    dead = maps.permute(0, 3, 1, 2, 4)[real]                                              # [rows, L, H, S] of real rows
    dead_keys = (~key_ok)[:, None, :].expand(N, Ty - 1, S)[real][:, None, None, :].expand_as(dead)
    assert float(dead[dead_keys].abs().max() if dead_keys.any() else 0.0) == 0.0, "a padded key got a non-zero probability"
    maps = maps * real[:, None, None, :, None]                                           # rows behind the end: zeros
    mean = maps.double().mean((1, 2))                                                     # [N, T, S]
    top2 = mean.topk(min(2, S), -1).values
    margin = top2[..., 0] - top2[..., -1]
    thr = 2 * MAP_BOUND * float(mean[real].max())
    excluded = float(((margin <= thr) & real).sum()) / float(real.sum())
    print(f"{name}: {int(real.sum())} real positions, maps peak at {float(mean[real].max(-1).values.min()):.4f} … "
          f"{float(mean[real].max()):.4f} (uniform {1 / S:.4f}), smallest margin {float(margin[real].min()):.3e}, threshold "
          f"{thr:.3e}, excluded by the margin rule {100 * excluded:.2f} %")
    if excluded > MARGIN_CAP:
        raise SystemExit(f"{name}: {100 * excluded:.2f} % of the positions are near-ties; set refused")
    k = name + "."
    store[k + "tokens"] = y.numpy()
    store[k + "pads"] = np.array(pads)
    store[k + "enc_pads"] = np.array(enc_pads)
    store[k + "head_mean"] = maps.double().mean(2).float().numpy()                        # [N, L, T, S]
    store[k + "peak"] = mean.argmax(-1).numpy().astype(np.int32)
    store[k + "margin"] = margin.float().numpy()
    if per_head_rows:
        store[k + "per_head_rows"] = np.array(per_head_rows)
        store[k + "per_head"] = maps[list(per_head_rows)].numpy()                         # [rows, L, H, T, S]


def main():
    E2E, FEAT, _ = MG._import_reference()
    g = W.TINY
    store = {}
    with torch.no_grad():
        # ---- end to end, TINY xavier, the fresh captions of tiny_scoring.npz
        sd = W.synth_state_dict(g, variant="xavier", eos_idx=MG.TINY_EOS)
        ref = MG.build_ref_e2e(E2E, g, sd)
        fx = np.load(os.path.join(ROOT, "tests", "golden", "tiny_scoring.npz"))
        y = torch.from_numpy(fx["xavier.fresh.tokens"]).long()
        pads = [int(p) for p in fx["xavier.fresh.pads"]]
        per = int(fx["xavier.fresh.per_image"])
        img = W.synth_images(3, g)
        enc = img.repeat_interleave(per, 0)
        N = y.shape[0]
        maps = hooked_maps(ref, g.N_dec, enc_x=enc, dec_x=y[:, :-1], enc_x_num_pads=[0] * N, dec_x_num_pads=pads)
        mem = R.forward_enc({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, g, img.double(),
                            [0] * 3).repeat_interleave(per, 0)
        record(store, "e2e", maps, restated_maps(sd, g, mem, y[:, :-1], pads, [0] * N), y, pads, [0] * N,
               PER_HEAD_CAPTIONS)
        # ---- features only, ragged encoder pads
        sd = W.synth_state_dict(g, end_to_end=False, img_feature_dim=FEAT_DIM, variant="eos", eos_idx=MG.TINY_EOS)
        ref = MG.build_ref_feat(FEAT, g, sd, FEAT_DIM)
        feats = W.synth_features(len(FEAT_PADS), FEAT_LEN, FEAT_DIM)
        y, pads = MS.fresh_captions(g, seed=11)
        y, pads = y[:len(FEAT_PADS)], pads[:len(FEAT_PADS)]
        maps = hooked_maps(ref, g.N_dec, enc_x=feats, dec_x=y[:, :-1], enc_x_num_pads=FEAT_PADS, dec_x_num_pads=pads)
        mem = R.forward_enc({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, g, feats.double(),
                            FEAT_PADS, end_to_end=False)
        record(store, "feat", maps, restated_maps(sd, g, mem, y[:, :-1], pads, FEAT_PADS), y, pads, FEAT_PADS)
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    if size > 200 * 1024:
        raise SystemExit("the fixture exceeds 200 KB")


if __name__ == "__main__":
    main()
