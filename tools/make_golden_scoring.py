"""Generate tests/golden/tiny_scoring.npz by running the REAL reference on the CPU (build container only).

    python tools/make_golden_scoring.py

For the TINY checkpoints (xavier, eos) the reference's legacy model is run teacher-forced as test.py:119-125 does
(`forward(enc_x, dec_y[:, :-1], dec_x_num_pads = pads of dec_y)`) and its own LabelSmoothingLoss
(losses/loss.py:15-39) is evaluated on those logits.  Recorded, data only: tokens, pads, per-position target log-probs,
Σ_v log-prob, arg-max, top-1/top-2 margins and the loss values.  Two input sets per checkpoint:
  teacher  the teacher tokens of tiny_<variant>.npz (3 images, one caption each)
  fresh    3 images x 2 captions, ragged lengths from 2 tokens up to max_seq_len
The arg-max of a position is only compared where the top-1/top-2 margin exceeds twice the log-prob bound of the GPU
tests (2e-4 xavier / 1e-3 eos); the share of real positions this excludes is printed for every set and a set above 1 %
is refused.  The reference's `divide_by_non_zeros=True` branch casts to a CUDA tensor type and cannot run on the CPU;
that value is recorded as its `False` result divided by the number of non-ignored targets, which is all the branch does.
"""
from __future__ import annotations

import importlib.util
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

OUT = os.path.join(ROOT, "tests", "golden", "tiny_scoring.npz")
PAD = 0
LP_BOUND = {"xavier": 2e-4, "eos": 1e-3}      # tests/test_hip_ops.py::test_tiny_teacher_forced_logits
SMOOTHINGS = (0.0, 0.1, 1.0)
MARGIN_CAP = 0.01


def _reference_loss():
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(MG.REF, "losses", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LabelSmoothingLoss


def fresh_captions(g, seed: int):
    """3 images x 2 captions: lengths 2 (a start token and one more), max_seq_len (full) and four in between."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    lens = [2, g.max_seq_len, 7, 13, 5, 18]
    Ty = max(lens)
    y = np.full((len(lens), Ty), PAD, dtype=np.int64)
    for i, n in enumerate(lens):
        y[i, :n] = rng.integers(4, g.vocab_size, size=n)
        y[i, 0] = MG.TINY_SOS
        y[i, n - 1] = MG.TINY_EOS
    return torch.from_numpy(y), [Ty - n for n in lens]


def record(store, report, name, variant, ref, sd, g, img, y, pads, per_image, Loss):
    N, Ty = y.shape
    enc = img.repeat_interleave(per_image, 0)
    dec, tgt = y[:, :-1], y[:, 1:]
    logits = ref(enc_x=enc, dec_x=dec, enc_x_num_pads=[0] * N, dec_x_num_pads=pads, apply_log_softmax=False,
                 mode="forward")
    lp = torch.log_softmax(logits.double(), -1)
    real = torch.arange(Ty - 1)[None, :] < (Ty - 1 - torch.tensor(pads))[:, None]
    top2 = lp.topk(2, -1).values
    margin = (top2[..., 0] - top2[..., 1])
    excluded = float(((margin <= 2 * LP_BOUND[variant]) & real).sum()) / float(real.sum())
    print(f"{variant}/{name}: {int(real.sum())} real positions, smallest margin {float(margin[real].min()):.4f}, "
          f"excluded by the margin rule {100 * excluded:.2f} %")
    if excluded > MARGIN_CAP:
        raise SystemExit(f"{variant}/{name}: {100 * excluded:.2f} % of the positions are near-ties; set refused")
    oracle = R.forward_teacher(sd, g, enc, dec, [0] * N, pads, log_softmax=True)
    report[f"{variant}/{name}/oracle_vs_reference_logp"] = float((oracle.double() - lp).abs().max())
    k = f"{variant}.{name}."
    store[k + "tokens"] = y.numpy()
    store[k + "pads"] = np.array(pads)
    store[k + "per_image"] = np.array(per_image)
    store[k + "logp_target"] = lp.gather(-1, tgt[..., None])[..., 0].float().numpy()
    store[k + "sum_logp"] = lp.sum(-1).float().numpy()
    store[k + "argmax"] = lp.argmax(-1).numpy().astype(np.int32)
    store[k + "margin"] = margin.float().numpy()
    # the ignore index follows the padding (test.py:129); a second run ignores nothing (index outside the vocabulary)
    for tag, ign in (("pad", PAD), ("none", -1)):
        n_keep = float((tgt != ign).sum())
        vals = []
        for s in SMOOTHINGS:
            v = float(Loss(s, rank="cpu")(logits, tgt, ign, divide_by_non_zeros=False))
            vals.append([v, v / n_keep])
        store[k + f"loss_ignore_{tag}"] = np.array(vals, dtype=np.float64)      # [smoothing][sum, per kept target]


def main():
    E2E, _, _ = MG._import_reference()
    Loss = _reference_loss()
    store, report = {"smoothings": np.array(SMOOTHINGS)}, {}
    g = W.TINY
    with torch.no_grad():
        for variant in ("xavier", "eos"):
            sd = W.synth_state_dict(g, variant=variant, eos_idx=MG.TINY_EOS)
            ref = MG.build_ref_e2e(E2E, g, sd)
            img = W.synth_images(3, g)
            old = np.load(os.path.join(ROOT, "tests", "golden", f"tiny_{variant}.npz"))
            y = torch.from_numpy(old["teacher.tokens"]).long().clone()
            pads = [int(p) for p in old["teacher.pads"]]
            for i, p in enumerate(pads):                       # behind a caption's end: the pad token, as a data loader gives
                if p:
                    y[i, y.shape[1] - p:] = PAD
            record(store, report, "teacher", variant, ref, sd, g, img, y, pads, 1, Loss)
            y, pads = fresh_captions(g, seed=11)
            record(store, report, "fresh", variant, ref, sd, g, img, y, pads, 2, Loss)
    for k, v in report.items():
        print(f"{k}: {v:.3e}")
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
