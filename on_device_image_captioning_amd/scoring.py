"""Host-side pieces of caption scoring: packing ragged captions, the result object and the closed-form
label-smoothing loss (losses/loss.py:15-39 evaluated from per-position statistics instead of an [N, T, V] tensor).

Nothing here touches the GPU; the arithmetic over the vocabulary is CaptionerEngine.decode_sequence.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch


@dataclass
class CaptionScores:
    """Result of `score_captions`.  Row n is caption n (image-major with `captions_per_image`)."""
    logprobs: torch.Tensor      # fp32 [N, Tmax-1]: log-prob of token t+1 given tokens 0..t; 0 at padded positions
    lengths: torch.Tensor       # int64 [N]: scored tokens per caption (its length minus the start token)
    sum: torch.Tensor           # fp32 [N]: Σ of the caption's log-probs
    mean: torch.Tensor          # fp32 [N]: sum / lengths
    argmax: torch.Tensor        # int32 [N, Tmax-1]: the model's most likely token at each position; -1 at padded positions
    sum_logp_vocab: torch.Tensor  # fp32 [N, Tmax-1]: Σ_v log-prob(v) at each position (label smoothing); 0 at padded positions


def pack_captions(captions, dec_x_num_pads=None, *, pad_idx: Optional[int] = None, max_seq_len: Optional[int] = None
                  ) -> Tuple[torch.Tensor, List[int]]:
    """Ragged token-id lists (SOS … EOS), or a padded int64 tensor with its pad counts → (tokens int64 [N, Tmax] on
    the host, positions behind a caption's end set to 0; lengths).  A padded tensor without pad counts is measured
    with `pad_idx` (trailing pads).  A caption shorter than 2 tokens or longer than `max_seq_len` is an error."""
    if isinstance(captions, torch.Tensor):
        if captions.dim() != 2:
            raise ValueError("a caption tensor must be [N, Tmax]")
        t = captions.detach().to("cpu", torch.int64)
        N, Tm = t.shape
        if dec_x_num_pads is not None:
            pads = [int(p) for p in (dec_x_num_pads.tolist() if isinstance(dec_x_num_pads, torch.Tensor) else dec_x_num_pads)]
            if len(pads) != N:
                raise ValueError(f"expected {N} pad counts, got {len(pads)}")
            lens = [Tm - p for p in pads]
        elif pad_idx is not None:
            lens = []
            for row in t.tolist():
                n = Tm
                while n > 0 and row[n - 1] == pad_idx:
                    n -= 1
                lens.append(n)
        else:
            lens = [Tm] * N
        rows = [t[i, :max(0, lens[i])].tolist() for i in range(N)]
    else:
        if dec_x_num_pads is not None:
            raise ValueError("dec_x_num_pads goes with a padded caption tensor, not with ragged lists")
        rows = [[int(v) for v in c] for c in captions]
        lens = [len(r) for r in rows]
    if not rows:
        raise ValueError("no captions")
    for i, n in enumerate(lens):
        if n < 2:
            raise ValueError(f"caption {i} has {n} tokens; a caption needs at least a start token and one more")
        if max_seq_len is not None and n > max_seq_len:
            raise ValueError(f"caption {i} has {n} tokens, more than max_seq_len = {max_seq_len}")
    Tm = max(lens)
    out = torch.zeros(len(rows), Tm, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return out, lens


def label_smoothing_loss(logp_target: torch.Tensor, sum_logp: torch.Tensor, ignored: torch.Tensor, num_classes: int,
                         smoothing: float = 0.0, divide_by_non_zeros: bool = False) -> torch.Tensor:
    """LabelSmoothingLoss.forward (losses/loss.py:15-39) from per-position statistics: `logp_target` = log-prob of the
    target, `sum_logp` = Σ_v log-prob(v), `ignored` = target == ignore_index.  With u = smoothing/(V-1) and
    c = 1 - smoothing the KL divergence of a kept position is
        c·log c + (V-1)·u·log u − c·lp_t − u·(Σ_v lp_v − lp_t)
    where a term with a zero coefficient is 0 (as nn.KLDivLoss treats a zero target probability).  Summed in fp64."""
    if not 0.0 <= smoothing <= 1.0:
        raise ValueError("smoothing must lie in [0, 1]")
    V = int(num_classes)
    u, c = smoothing / (V - 1), 1.0 - smoothing
    lp = logp_target.detach().to(torch.float64)
    sl = sum_logp.detach().to(torch.float64)
    const = (c * math.log(c) if c > 0 else 0.0) + ((V - 1) * u * math.log(u) if u > 0 else 0.0)
    per = torch.full_like(lp, const)
    if c > 0:
        per = per - c * lp
    if u > 0:
        per = per - u * (sl - lp)
    keep = ~ignored.to(torch.bool)
    tot = torch.where(keep, per, torch.zeros_like(per)).sum()
    if divide_by_non_zeros:
        tot = tot / keep.sum().to(torch.float64)
    return tot.to(torch.float32)
