"""Host-side pieces of word grounding: the result object of `word_attention` (per-word cross-attention maps over the
encoder positions), the parsing of its `layers` / `heads` arguments, and the way back from a grid cell to a box of the
source image (`source_box`) for `Captioner.caption_regions`.

Nothing here touches the GPU; the probabilities come from CaptionerEngine.decode_sequence(attn=...)
(odic_cross_attn_probs).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import torch


def parse_layers(layers, n_dec: int) -> Tuple[List[int], bool]:
    """`layers` of word_attention → (decoder layer indices, reduce to their mean).  "mean": all layers averaged; "all":
    all layers, one map each; an int or a list of ints (negative = from the end): those layers, one map each."""
    if isinstance(layers, str):
        if layers == "mean":
            return list(range(n_dec)), True
        if layers == "all":
            return list(range(n_dec)), False
        raise ValueError(f"layers must be 'mean', 'all', an int or a list of ints, not {layers!r}")
    if isinstance(layers, bool):
        raise ValueError("layers must be 'mean', 'all', an int or a list of ints, not a bool")
    if isinstance(layers, int):
        layers = [layers]
    try:
        idx = [int(i) for i in layers]
        exact = all(int(i) == i for i in layers)
    except (TypeError, ValueError):
        raise ValueError(f"layers must be 'mean', 'all', an int or a list of ints, not {layers!r}") from None
    if not idx or not exact:
        raise ValueError(f"layers must be 'mean', 'all', an int or a non-empty list of ints, not {layers!r}")
    out = []
    for i in idx:
        if not -n_dec <= i < n_dec:
            raise ValueError(f"decoder layer {i} is out of range: the model has {n_dec} decoder layers")
        out.append(i % n_dec)
    if len(set(out)) != len(out):
        raise ValueError(f"layers names a decoder layer twice: {layers!r}")
    return out, False


def parse_heads(heads) -> bool:
    """`heads` of word_attention → per_head."""
    if isinstance(heads, str) and heads in ("mean", "all"):
        return heads == "all"
    raise ValueError(f"heads must be 'mean' or 'all', not {heads!r}")


def source_box(box, from_size: Union[int, Tuple[int, int]],
               image_size: Union[int, Tuple[int, int]]) -> Tuple[float, float, float, float]:
    """A (x0, y0, x1, y1) box in an image of `from_size` — what `WordAttention.cell_box(idx, from_size)` returns for the
    model's input size — as the float (l, t, r, b) box of the same area in the source image of `image_size` (sizes are an
    int, or (height, width)): the box `DevicePreprocessor.resize_regions` and `Captioner.caption_regions` take.
    "Caption what word t of caption n looked at", for `images = pre.decode_jpeg(blobs)` and their batch
    `x = pre.from_jpeg_bytes(blobs)`:

        wa = captioner.word_attention(x)
        box = source_box(wa.cell_box(wa.peak_cells()[n, t], pre.S), pre.S, images[n].shape[:2])
        tokens = captioner.caption_regions(pre, images, [(n, box)])[n][0].tokens
    """
    fh, fw = (from_size, from_size) if isinstance(from_size, int) else (int(from_size[0]), int(from_size[1]))
    H, W = (image_size, image_size) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
    x0, y0, x1, y1 = (float(v) for v in box)
    if fh <= 0 or fw <= 0 or H <= 0 or W <= 0 or not (0 <= x0 < x1 <= fw and 0 <= y0 < y1 <= fh):
        raise ValueError(f"box {tuple(box)!r} does not lie in a {fw} x {fh} image")
    return (x0 * W / fw, y0 * H / fh, x1 * W / fw, y1 * H / fh)


@dataclass
class RegionCaption:
    """One region of `Captioner.caption_regions`: its position in the `regions` argument, its box, the captions the
    search returned for it (best first) and their per-token log-probabilities [how_many_outputs, Tmax]."""
    region: int
    box: Tuple[float, float, float, float]
    tokens: List[List[int]]
    logprobs: torch.Tensor


@dataclass
class WordAttention:
    """Result of `word_attention`.  Row n is caption n (image-major with `captions_per_image`)."""
    tokens: List[List[int]]        # the captions, SOS … EOS
    maps: torch.Tensor             # fp32 [N, Tmax-1, S] | [N, L', Tmax-1, S] | [N, L', H, Tmax-1, S] ([N, H, Tmax-1, S]:
    #                                layers="mean" with heads="all"); maps[n, …, t, :] is the attention of the step that
    #                                predicted tokens[n][t+1]; 0 at padded positions t >= lengths[n]
    lengths: torch.Tensor          # int64 [N] = len(caption) - 1
    enc_lengths: torch.Tensor      # int64 [N] valid encoder positions of the caption's image
    grid: Optional[Tuple[int, int]]  # (12, 12) for the end-to-end model, None for features-only

    def word_maps(self, n: int) -> torch.Tensor:
        """The maps of caption n without its padded positions: [..., lengths[n], S] (a view)."""
        return self.maps[n][..., :int(self.lengths[n]), :]

    def mean_maps(self) -> torch.Tensor:
        """[N, Tmax-1, S]: the maps averaged over whatever layer and head axes they carry."""
        m = self.maps
        while m.dim() > 3:
            m = m.mean(1)
        return m

    def peak_cells(self) -> torch.Tensor:
        """int64 [N, Tmax-1]: the encoder position the layer- and head-mean map of each word peaks at (ties → the lower
        index); -1 at padded positions."""
        m = self.mean_maps()
        # (the first maximum, on every device: torch.argmax does not promise which of several equal maxima it returns)
        top = m.max(-1, keepdim=True).values
        idx = torch.arange(m.shape[-1], device=m.device).expand_as(m)
        peak = torch.where(m == top, idx, torch.full_like(idx, m.shape[-1])).min(-1).values
        real = torch.arange(m.shape[1], device=m.device)[None, :] < self.lengths.to(m.device)[:, None]
        return torch.where(real, peak, torch.full_like(peak, -1))

    def _need_grid(self) -> Tuple[int, int]:
        if self.grid is None:
            raise ValueError("these maps have no grid: a features-only model does not know where its inputs lie in an image")
        return self.grid

    def cell_box(self, idx: int, image_size: Union[int, Tuple[int, int]]) -> Tuple[int, int, int, int]:
        """Encoder position `idx` → its (x0, y0, x1, y1) pixel box in an image of `image_size` (an int, or (height,
        width)).  Positions are row-major on `grid`, the token order of SwinEngine.forward's output."""
        gh, gw = self._need_grid()
        idx = int(idx)
        if not 0 <= idx < gh * gw:
            raise ValueError(f"position {idx} is outside the {gh} x {gw} grid")
        H, W = (image_size, image_size) if isinstance(image_size, int) else (int(image_size[0]), int(image_size[1]))
        r, c = divmod(idx, gw)
        return (c * W // gw, r * H // gh, (c + 1) * W // gw, (r + 1) * H // gh)

    def heatmaps(self, size: Union[int, Tuple[int, int]]) -> torch.Tensor:
        """[N, Tmax-1, H, W]: the layer- and head-mean maps on the grid, bilinearly resized to `size` (an int, or
        (height, width))."""
        gh, gw = self._need_grid()
        m = self.mean_maps()
        if m.shape[-1] != gh * gw:
            raise ValueError(f"{m.shape[-1]} encoder positions do not fill a {gh} x {gw} grid")
        size = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
        return torch.nn.functional.interpolate(m.reshape(m.shape[0], m.shape[1], gh, gw), size=size, mode="bilinear",
                                               align_corners=False)
