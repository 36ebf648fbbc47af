#!/usr/bin/env python3
"""What one SwinEngine.forward enqueues and returns for every precision and every ODIC_FUSE_* setting, as text that two
builds can be compared by (diff): Swin-L with two blocks per stage (every block form of the real backbone, a third of its
launches), the synthetic "xavier" backbone weights of seed 0, synthetic images of seed 93.  For each configuration: the
(family, detail) of every launch ops.profile() records and the SHA-256 of the feature tensor's bytes.  Only the
constructor, forward and the environment are used, so the same file runs on an older build.  The tile candidates are pinned
to one configuration per family, so that no timed choice can differ between two runs.

    python3 tools/swin_trace.py > trace.txt
"""
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("ODIC_TILE_CANDIDATES", "1")
os.environ.setdefault("ODIC_X3_TILE_CANDIDATES", "0")

FLAGS = ("ODIC_FUSE_BACKBONE_LN_READ", "ODIC_FUSE_QKV_ATTENTION", "ODIC_FUSE_QKV_ATTENTION_TILED",
         "ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C", "ODIC_FUSE_MLP", "ODIC_SWIN_CHUNKS")
#: (precision, environment, images)
CONFIGS = [("fp32", {}, 1), ("x3", {}, 1), ("x3", {"ODIC_FUSE_BACKBONE_LN_READ": "x3"}, 1), ("fp8", {}, 1), ("bf16", {}, 1),
           ("bf16", {"ODIC_FUSE_BACKBONE_LN_READ": "0"}, 1), ("bf16", {"ODIC_FUSE_QKV_ATTENTION": "0"}, 1),
           ("bf16", {"ODIC_FUSE_QKV_ATTENTION_TILED": "0"}, 1), ("bf16", {"ODIC_FUSE_MLP": "0"}, 1),
           ("bf16", {"ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C": "384"}, 1), ("bf16", {"ODIC_SWIN_CHUNKS": "2,2"}, 2)]


def main():
    import torch

    from on_device_image_captioning_amd import ops
    from on_device_image_captioning_amd import weights as W
    from on_device_image_captioning_amd.engine import SwinEngine

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    g = dataclasses.replace(W.FULL, swin_depths=(2, 2, 2, 2))
    sd = {name: W.synth_tensor(name, shape, kind, g, 0) for name, shape, kind in W.state_dict_spec(g)
          if name.startswith("swin_transf.")}
    for precision, env, n_img in CONFIGS:
        for k in FLAGS:
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = SwinEngine(sd, g, dev, precision)
        img = W.synth_images(n_img, g, seed=93).to(dev)
        eng.forward(img)                                                     # code load, the a_ln tile choice
        with ops.profile() as recs:
            out = eng.forward(img)
        torch.cuda.synchronize()
        print("==", " ".join([precision] + [f"{k}={v}" for k, v in env.items()] + [f"B={n_img}"]))
        for r in recs:
            print(f"{r[0]} {r[5]}".rstrip())
        out = out.detach().cpu().contiguous()
        print("features", tuple(out.shape), hashlib.sha256(out.numpy().tobytes()).hexdigest(), flush=True)
        del eng


if __name__ == "__main__":
    main()
