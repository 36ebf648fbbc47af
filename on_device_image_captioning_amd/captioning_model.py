"""Search / API layer.

Two call shapes of the reference are served:
  * legacy:      model(enc_x, dec_x, enc_x_num_pads, dec_x_num_pads, apply_log_softmax, mode=..., **kw)
                 and model.beam_search(...)            — legacy_models/captioning_model.py:24-57,111-241
                 (what demo.py:124-129 and test.py:209-214 call)
  * refactored:  Captioner(beam_search_args, model=...)(enc_x, enc_x_num_pads=..., mode="beam_search")
                                                       — models/captioning_model.py:40-110

The search itself runs on the GPU: one incremental decoder step per new token (engine.py) and the
beam bookkeeping of captioning_model.py:172-223 in odic_beam_step.  The host loop only enqueues
steps; it looks at the device-side `done` flag every few steps (the all-beams-finished state is a
fixed point of the step, so running a few extra steps cannot change the result).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import engine as _engine
from . import ops
from . import grounding as _grounding
from . import scoring as _scoring
from . import search as _search
from .search import _DONE_POLL      # noqa: F401  (the sampling loop below; importers of this module)


class CaptioningModel(nn.Module):
    """Base class: mode dispatch + GPU search.  Subclasses provide `_engines()`, `forward_enc`,
    `_cross_kv(mem)` and set `self.rank` (legacy_models/captioning_model.py:11-16)."""

    def __init__(self, apply_log_softmax: bool = False):
        super().__init__()
        self.rank = None
        self.apply_log_softmax = apply_log_softmax
        self._eng_cache = None
        self.precision = "fp32"
        self.encoder_precision = None       # None = follow `precision`
        self.calibration_images = None      # fp8 mode: images the static activation scales are calibrated on
        self.sampling_seed = 0              # Philox key of the device-side draws ('sample' / 'sampling' modes)
        self._sampling_calls = 0
        self._draw_log = None               # list → every sampled-beam-search draw is appended (tests)
        self._cand_log = None               # list → every deterministic search step's (cand_val, cand_idx) is appended (tests)
        self.last_stochastic_beam = None    # after stochastic_beam_search: the samples' perturbed scores, kappa and log-probs
        self.last_required_satisfied = None  # after a beam_search with required_words: per image, does output 0 hold them all
        self.last_pool_scores = None        # after pool_beam_search: the outputs' scores sum / len^alpha, fp32 [B, how_many_outputs],
        self.last_pool_counts = None        # the hypotheses every image's pool held, int32 [B], and
        self.last_pool_closed = None        # whether the image closed before the steps ran out, bool [B] (all on the host)

    # ------------------------------------------------------------------ engine cache plumbing
    def check_required_attributes(self):
        if self.rank is None:
            raise NotImplementedError("Subclass must assign the rank integer according to the GPU group")

    def set_precision(self, precision: str, encoder_precision: Optional[str] = None,
                      calibration_images: Optional[torch.Tensor] = None) -> "CaptioningModel":
        """'fp32' (default; exact-fp32 MFMA, parity mode), 'bf16' (backbone GEMMs + window attention in bf16 with
        fp32 accumulation and an fp32 residual stream; expansion-encoder products in bf16 too unless
        `encoder_precision='fp32'`) or 'fp8' (BASELINE.json configs[4]: Swin-block GEMMs qkv / fc1 / fc2 on the fp8
        MFMA with statically calibrated scales, fp16 qkv / attention activations, everything else as 'bf16'), or
        'x3' — the near-exact fast mode: every backbone / encoder contraction on split-fp16 operands (hi + lo pairs,
        22 significand bits, three fp16 MFMAs per product with fp32 accumulation; 'bf16x3' is accepted as an alias
        for the name the technique usually goes by), fp32 residual streams, exact-erf GELU — the mode that reproduces
        the fp32 (= reference) captions at several times the exact-fp32 MFMA rate.  The decoder is always fp32.
        `calibration_images` (fp8 only; fp32 [n,3,H,W], preprocessed like the inputs): the images the static per-tensor
        activation scales are measured on (amax x 1.25 → the e4m3 maximum).  Default: two synthetic noise images —
        fine for synthetic benchmarks, NOT for real photographs, whose LayerNorm / GELU ranges differ; the fp8 casts
        saturate silently at ±448, so calibrate on a sample of the deployment distribution and check
        `fp8_saturation_report(images)` on held-out images."""
        if precision == "bf16x3":
            precision = "x3"
        if encoder_precision == "bf16x3":
            encoder_precision = "x3"
        if precision not in ("fp32", "bf16", "fp8", "x3") or (encoder_precision or "bf16") not in ("fp32", "bf16", "x3"):
            raise ValueError("precision must be 'fp32', 'bf16', 'fp8' or 'x3' (encoder_precision 'fp32', 'bf16' or 'x3')")
        if calibration_images is not None and precision != "fp8":
            raise ValueError("calibration_images only applies to precision='fp8'")
        same_cal = (calibration_images is None and self.calibration_images is None) or \
            (calibration_images is not None and self.calibration_images is not None and
             calibration_images.shape == self.calibration_images.shape and
             bool(torch.equal(calibration_images.detach().cpu(), self.calibration_images)))
        if (precision, encoder_precision) != (self.precision, self.encoder_precision) or not same_cal:
            self.precision, self.encoder_precision = precision, encoder_precision
            self.calibration_images = None if calibration_images is None else calibration_images.detach().float().cpu().clone()
            self._eng_cache = None
        return self

    def fp8_saturation_report(self, images: torch.Tensor) -> dict:
        """fp8 mode: how the activation ranges of `images` compare with the calibrated scales — per quantised tensor
        (LayerNorm outputs and GELU hidden of every Swin block) the ratio observed amax / representable range; a ratio
        above 1 means the static cast clips there (End_ExpansionNet_v2 only)."""
        if self.precision != "fp8":
            raise RuntimeError("fp8_saturation_report needs set_precision('fp8')")
        swin = self._engines()[0]
        return swin.fp8_saturation(images.to(swin.device, torch.float32))

    def _search_constraint_args(self, *, no_repeat_ngram_size=0, min_length=0, banned_words=None, sos_idx, eos_idx, max_seq_len,
                                rows_per_image, sampling=False) -> Optional[dict]:
        """The constraint keywords of the search methods, checked on the host before any device work: None when none is
        active (the search then launches exactly what it always did), else the keywords of
        CaptionerEngine.search_constraints."""
        return _search.check_constraints(no_repeat_ngram_size, min_length, banned_words, V=self._vocab_size,
                                         max_seq_len=max_seq_len, rows_per_image=rows_per_image, sos_idx=sos_idx,
                                         eos_idx=eos_idx, sampling=sampling)

    def _search_prefix_arg(self, prefix, enc_input, *, sos_idx, eos_idx, max_seq_len, sampling=False):
        """The `prefix` keyword of the search methods, checked on the host before any device work (search.check_prefix):
        None for no prefix, else one id list per image."""
        if prefix is None:
            return None
        return _search.check_prefix(prefix, len(enc_input), V=self._vocab_size, max_seq_len=max_seq_len, sos_idx=sos_idx,
                                    eos_idx=eos_idx, sampling=sampling)

    def _search_required_arg(self, required_words, enc_input, *, beam_size, banned_words, sos_idx, eos_idx, max_seq_len,
                             sampling=False):
        """The `required_words` keyword of beam_search, checked on the host before any device work
        (search.check_required_words): None for nothing required, else one padded id list per image."""
        if required_words is None:
            return None
        return _search.check_required_words(required_words, len(enc_input), V=self._vocab_size, beam_size=beam_size,
                                            banned=banned_words, sos_idx=sos_idx, eos_idx=eos_idx, max_seq_len=max_seq_len,
                                            sampling=sampling)

    def _check_rows_fit(self, rows: int, what: str = "rows") -> None:
        """A search of `rows` rows per image takes that many distinct words of a row: ValueError past the vocabulary."""
        if rows > self._vocab_size():
            raise ValueError(f"{rows} {what} per image exceed the vocabulary ({self._vocab_size()} words)")

    def _open_search(self, mem, enc_input_num_pads, rows: int, max_seq_len: int):
        """A search of `rows` rows per image on the encoder memory `mem` → (the engine, the DecodeState still to be
        armed, steps): positions 0 .. steps-1 are fed, the state holds steps + 1 (a prefix reaches that far)."""
        eng = self._captioner_engine()
        B, S, _ = mem.shape
        steps = max(1, max_seq_len - 1)
        st = eng.new_state(B, rows, steps + 1, eng.project_kv(mem), self._enc_lens(B, S, enc_input_num_pads))
        return eng, st, steps

    def _next_sampling_seed(self) -> int:
        """A fresh Philox key per sampling call (so repeated calls differ), reproducible from `sampling_seed`."""
        self._sampling_calls += 1
        return (int(self.sampling_seed) * 0x9E3779B97F4A7C15 + self._sampling_calls) & 0xFFFFFFFFFFFFFFFF

    def _apply(self, fn, *a, **k):
        self._eng_cache = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._eng_cache = None
        return super().load_state_dict(*a, **k)

    def _device(self) -> torch.device:
        """GPU the HIP engines of this model live on.  A module moved with `.to('cuda:N')` runs there.  A module
        left on the host — demo.py:68-104 builds the model with rank='cpu', loads the checkpoint and never calls
        `.to()` — keeps its nn.Parameters on the host and the engines pack their own copy of the weights onto
        `rank` if that names a GPU, else cuda:0; inputs are moved there, results come back on the input's
        device.  Arithmetic is HIP in every case: without a GPU this raises (there is no CPU fallback)."""
        dv = next(self.parameters()).device
        if dv.type == "cuda":
            return dv
        if not torch.cuda.is_available():
            raise RuntimeError("the HIP path needs a GPU and none is visible; there is no CPU fallback in this package")
        r = self.rank
        if isinstance(r, int) and not isinstance(r, bool):
            return torch.device("cuda", r)
        if isinstance(r, torch.device) and r.type == "cuda":
            return r
        if isinstance(r, str) and r.startswith("cuda"):
            return torch.device(r)
        return torch.device("cuda", 0)

    # ------------------------------------------------------------------ to be provided
    def forward_enc(self, enc_input, enc_input_num_pads):
        raise NotImplementedError

    def _captioner_engine(self) -> "_engine.CaptionerEngine":
        raise NotImplementedError

    def _enc_lens(self, n: int, S: int, enc_input_num_pads) -> torch.Tensor:
        raise NotImplementedError

    # ------------------------------------------------------------------ decoder API
    def forward_dec(self, cross_input, enc_input_num_pads, dec_input, dec_input_num_pads,
                    apply_log_softmax: bool = False):
        """(N,T) token ids → (N,T,V) logits / log-probs, teacher forced (End_ExpansionNet_v2.py:103-138).
        Runs the incremental step T times; padded positions reproduce the reference's masked rows."""
        eng = self._captioner_engine()
        dv = eng.device
        cross_input = cross_input.to(dv, torch.float32)
        dec_input = dec_input.to(dv, torch.int64)
        N, T = dec_input.shape
        S = cross_input.shape[1]
        enc_len = self._enc_lens(N, S, enc_input_num_pads)
        kv = eng.project_kv(cross_input)
        st = eng.new_state(N, 1, T + 1, kv, enc_len)
        st.anc.copy_(torch.arange(N, dtype=torch.int32, device=dv)[:, None].expand(N, T + 1))
        dec_len = torch.as_tensor([T - int(p) for p in _as_list(dec_input_num_pads, N)], device=dv)
        V = eng.g.vocab_size
        out = torch.empty(N, T, V, dtype=torch.float32, device=dv)
        for t in range(T):
            st.pos.fill_(t)
            st.next_tok.copy_(dec_input[:, t])
            st.row_valid.copy_((dec_len > t).to(torch.int32))
            eng.step_logits(st)
            if apply_log_softmax:
                ops.logsoftmax_topk(st.logits, V, out[:, t], T * V, st.cand_val, st.cand_idx, N, V, 1)
            else:
                out[:, t].copy_(st.logits)
        return out

    # ------------------------------------------------------------------ scoring given captions
    def _sequence_stats(self, enc_x, enc_x_num_pads, n_img: int, dec: torch.Tensor, dec_len: torch.Tensor,
                        targets: torch.Tensor, row_chunk: Optional[int] = None) -> dict:
        """Encoder once per image + one whole-sequence decoder pass → per-position statistics [N, T] on the device
        (CaptionerEngine.decode_sequence).  The ensemble overrides this."""
        eng = self._captioner_engine()
        dv = eng.device
        mem = self.forward_enc(enc_x, enc_x_num_pads)
        S = mem.shape[1]
        return eng.decode_sequence(dec.to(dv), dec_len.to(dv), eng.project_kv(mem), self._enc_lens(n_img, S, enc_x_num_pads),
                                   n_img, targets=targets.to(dv), row_chunk=row_chunk)

    def _vocab_size(self) -> int:
        return self.geometry.vocab_size          # (the module's own geometry: argument checks need no GPU)

    def _max_seq_len(self) -> int:
        return self.geometry.max_seq_len

    def _packed_captions(self, n_img: int, captions, enc_x_num_pads, captions_per_image: int, pad_idx, dec_x_num_pads):
        """The checked operands of score_captions / word_attention: (tokens int64 [N, Tm] SOS … EOS, the lengths, the
        decoder lengths int32 [N] = length - 1, enc_x_num_pads with its default)."""
        toks, lens = _scoring.pack_captions(captions, dec_x_num_pads, pad_idx=pad_idx, max_seq_len=self._max_seq_len())
        N = toks.shape[0]
        if captions_per_image < 1 or N != n_img * captions_per_image:
            raise ValueError(f"{N} captions for {n_img} inputs x {captions_per_image} captions per image")
        V = self._vocab_size()
        if int(toks.min()) < 0 or int(toks.max()) >= V:
            raise ValueError(f"token ids must lie in [0, {V})")
        if enc_x_num_pads is None:
            enc_x_num_pads = [0] * n_img
        return toks, lens, torch.tensor([n - 1 for n in lens], dtype=torch.int32), enc_x_num_pads

    def score_captions(self, enc_x, captions, enc_x_num_pads=None, *, captions_per_image: int = 1, pad_idx=None,
                       dec_x_num_pads=None, row_chunk: Optional[int] = None) -> "_scoring.CaptionScores":
        """Log-probability of given captions under the model, in one whole-sequence decoder pass (what test.py:84-138
        does with forward + log_softmax + gather).  `captions`: token-id lists (SOS … EOS, ragged), or a padded int64
        tensor with `dec_x_num_pads` (or `pad_idx` to measure trailing pads).  With `captions_per_image = R` the rows
        are image-major — captions[i·R : (i+1)·R] belong to image i — and the encoder runs once per image.
        Returns scoring.CaptionScores: logprobs[n, t] = log p(token t+1 | tokens 0..t), 0 behind the caption's end."""
        n_img = enc_x.shape[0]
        toks, lens, dec_len, enc_x_num_pads = self._packed_captions(n_img, captions, enc_x_num_pads, captions_per_image,
                                                                    pad_idx, dec_x_num_pads)
        Tm = toks.shape[1]
        st = self._sequence_stats(enc_x, enc_x_num_pads, n_img, toks[:, :-1].contiguous(), dec_len,
                                  toks[:, 1:].contiguous(), row_chunk)
        dv = st["logp"].device
        real = torch.arange(Tm - 1, device=dv)[None, :] < dec_len.to(dv)[:, None]
        lp = torch.where(real, st["logp"], torch.zeros_like(st["logp"]))
        lengths = dec_len.to(dv, torch.int64)
        tot = lp.sum(-1)
        out_dv = enc_x.device if isinstance(enc_x, torch.Tensor) else dv
        res = _scoring.CaptionScores(
            logprobs=lp, lengths=lengths, sum=tot, mean=tot / lengths.to(torch.float32),
            argmax=torch.where(real, st["argmax"], torch.full_like(st["argmax"], -1)),
            sum_logp_vocab=torch.where(real, st["sum_logp"], torch.zeros_like(st["sum_logp"])))
        for k in ("logprobs", "lengths", "sum", "mean", "argmax", "sum_logp_vocab"):
            setattr(res, k, getattr(res, k).to(out_dv))
        return res

    # ------------------------------------------------------------------ where the model looked for each word
    def _attention_grid(self, S: int) -> Optional[Tuple[int, int]]:
        """The (rows, columns) the S encoder positions lie on in the image, or None when the model cannot know."""
        return None

    def word_attention(self, enc_x, captions=None, enc_x_num_pads=None, *, captions_per_image: int = 1, pad_idx=None,
                       dec_x_num_pads=None, layers="mean", heads="mean", sos_idx=None, eos_idx=None, beam_size: int = 3,
                       max_seq_len: int = 20) -> "_grounding.WordAttention":
        """Per-word cross-attention maps: for every word of a caption, how the decoder's cross attention spread over the
        S encoder positions when it predicted that word — in one whole-sequence decoder pass (the softmax of
        layers.py:244-250 kept instead of discarded; odic_cross_attn_probs).  `captions`, `captions_per_image`, `pad_idx`
        and `dec_x_num_pads` are those of score_captions, with the same errors.  With `captions=None` the best caption
        of every input is generated first (`beam_search(..., how_many_outputs=1)` with `sos_idx`, `eos_idx`, `beam_size`,
        `max_seq_len`) and then grounded: the encoder then runs twice, once for the search and once for the maps.
        layers: "mean" (the mean over the decoder layers), "all", an int or a list of ints (negative = from the end);
        heads: "mean" or "all".  Returns grounding.WordAttention: maps[n, …, t, :] belongs to the step that predicted
        token t+1 of caption n and sums to 1 over the S positions; rows behind a caption's end are 0.  The decoder is
        fp32 in every precision mode, so the method works in all of them."""
        a_layers, a_reduce = _grounding.parse_layers(layers, self.geometry.N_dec)
        a_heads = _grounding.parse_heads(heads)
        n_img = enc_x.shape[0]
        if captions is None:
            if sos_idx is None or eos_idx is None:
                raise ValueError("word_attention without captions generates them and needs sos_idx and eos_idx")
            if captions_per_image != 1:
                raise ValueError("word_attention without captions grounds one generated caption per input")
            best, _ = self.beam_search(enc_x, [0] * n_img if enc_x_num_pads is None else enc_x_num_pads, sos_idx=sos_idx,
                                       eos_idx=eos_idx, beam_size=beam_size, how_many_outputs=1, max_seq_len=max_seq_len)
            captions, pad_idx, dec_x_num_pads = [per[0] for per in best], None, None
        toks, lens, dec_len, enc_x_num_pads = self._packed_captions(n_img, captions, enc_x_num_pads, captions_per_image,
                                                                    pad_idx, dec_x_num_pads)
        N, Tm = toks.shape
        eng = self._captioner_engine()
        dv = eng.device
        mem = self.forward_enc(enc_x, enc_x_num_pads)
        S = mem.shape[1]
        enc_len = self._enc_lens(n_img, S, enc_x_num_pads)
        st = eng.decode_sequence(toks[:, :-1].contiguous().to(dv), dec_len.to(dv), eng.project_kv(mem), enc_len, n_img,
                                 attn={"layers": a_layers, "per_head": a_heads, "reduce_layers": a_reduce})
        maps = st["attn"]                                                       # [N, (L',) (H,) Tm-1, S]
        real = torch.arange(Tm - 1, device=dv)[None, :] < dec_len.to(dv)[:, None]
        real = real.view([N] + [1] * (maps.dim() - 3) + [Tm - 1, 1])
        maps = torch.where(real, maps, torch.zeros_like(maps))
        out_dv = enc_x.device if isinstance(enc_x, torch.Tensor) else dv
        return _grounding.WordAttention(
            tokens=[toks[i, :n].tolist() for i, n in enumerate(lens)], maps=maps.to(out_dv),
            lengths=dec_len.to(out_dv, torch.int64),
            enc_lengths=enc_len.to(out_dv, torch.int64).repeat_interleave(captions_per_image),
            grid=self._attention_grid(S))

    def caption_loss(self, enc_x, dec_y, enc_x_num_pads, dec_y_num_pads, ignore_index, smoothing: float = 0.0,
                     divide_by_non_zeros: bool = False) -> torch.Tensor:
        """The evaluation loss of test.py:119-131: LabelSmoothingLoss(smoothing)(forward(enc_x, dec_y[:, :-1]),
        dec_y[:, 1:], ignore_index, divide_by_non_zeros) — computed from the per-position statistics of one
        whole-sequence pass in closed form (scoring.label_smoothing_loss); no [N, T, V] tensor exists."""
        dec_y = dec_y.detach().to("cpu", torch.int64)
        if dec_y.dim() != 2:
            raise ValueError("dec_y must be [N, Ty]")
        N, Ty = dec_y.shape
        if enc_x.shape[0] != N:
            raise ValueError(f"{N} target rows for {enc_x.shape[0]} inputs")
        if Ty < 2:
            raise ValueError("dec_y needs at least two columns")
        pads = _as_list(dec_y_num_pads, N)
        V = self._vocab_size()
        dec = dec_y[:, :-1].contiguous()
        tgt = dec_y[:, 1:].contiguous()
        ignored = tgt == ignore_index
        if int(dec.min()) < 0 or int(dec.max()) >= V or bool(((tgt < 0) | (tgt >= V))[~ignored].any()):
            raise ValueError(f"token ids must lie in [0, {V})")
        # as the reference, the decoder sees Ty - 1 positions with the pad counts of the Ty-long rows (test.py:121-123)
        dec_len = torch.tensor([max(0, Ty - 1 - p) for p in pads], dtype=torch.int32)
        st = self._sequence_stats(enc_x, enc_x_num_pads, N, dec, dec_len, tgt.masked_fill(ignored, 0))
        loss = _scoring.label_smoothing_loss(st["logp"].cpu(), st["sum_logp"].cpu(), ignored, V, smoothing,
                                             divide_by_non_zeros)
        return _to_input_device(loss, enc_x)

    def forward(self, enc_x, dec_x=None, enc_x_num_pads=[0], dec_x_num_pads=[0], apply_log_softmax=False,
                mode="forward", **kwargs):
        if mode == "forward":
            x = self.forward_enc(enc_x, enc_x_num_pads)
            y = self.forward_dec(x, enc_x_num_pads, dec_x, dec_x_num_pads, apply_log_softmax)
            return _to_input_device(y, enc_x)
        assert ("sos_idx" in kwargs.keys() or "eos_idx" in kwargs.keys()), \
            "sos and eos must be provided in case of batch sampling or beam search"
        return _search.dispatch(self, mode, kwargs, enc_x, enc_x_num_pads)

    def get_batch_multiple_sampled_prediction(self, enc_input, enc_input_num_pads, num_outputs, sos_idx, eos_idx,
                                              max_seq_len, *, temperature=1.0, top_k=0, top_p=1.0):
        """mode='sampling' (legacy_models/captioning_model.py:59-109): `num_outputs` ancestral samples per
        image.  Each step runs the incremental decoder and ONE kernel that normalises the row and draws the
        next word on the device (odic_logsoftmax_sample, Philox noise keyed by `self.sampling_seed`, the row and
        the position) — no host round trip, no ATen launch.  The draws cannot be those of the reference's CPU
        generator; what IS checkable — and tested — is that every reported log-prob equals the teacher-forced
        log-prob of the returned sequence, and that the draw frequencies follow the distribution.
        `temperature`, `top_k`, `top_p`: the draws come from softmax(logits / temperature), cut to its
        top_k best words (0 = all) and to the nucleus of mass top_p (1 = all) on the device
        (odic_logsoftmax_sample_filtered); the returned log-probs stay the model's own.  With the defaults the call
        launches exactly what it launches without them."""
        flt = _search.check_sampling_filter(temperature, top_k, top_p)
        eng = self._captioner_engine()
        dv = eng.device
        mem = self.forward_enc(enc_input, enc_input_num_pads)
        bs, S, _ = mem.shape
        N = bs * num_outputs
        V = eng.g.vocab_size
        enc_len = self._enc_lens(bs, S, enc_input_num_pads)
        st = eng.new_state(bs, num_outputs, max_seq_len + 1, eng.project_kv(mem), enc_len)
        st.anc.copy_(torch.arange(N, dtype=torch.int32, device=dv)[:, None].expand(N, max_seq_len + 1))
        st.next_tok.fill_(sos_idx)
        st.row_valid.fill_(1)
        draw_val = torch.empty(N, 1, dtype=torch.float32, device=dv)
        draw_idx = torch.empty(N, 1, dtype=torch.int32, device=dv)
        toks = torch.full((N, max_seq_len + 1), sos_idx, dtype=torch.int64, device=dv)
        lps = torch.zeros(N, max_seq_len + 1, dtype=torch.float32, device=dv)
        where_eos = torch.full((N,), max_seq_len, dtype=torch.int64, device=dv)
        finished = torch.zeros(N, dtype=torch.bool, device=dv)
        seed = self._next_sampling_seed()
        t = 0
        while t < max_seq_len:
            st.pos.fill_(t)
            eng.step_logits(st)
            _search.draw_candidates(st.logits, draw_val, draw_idx, N, V, 1, seed, st.pos, flt)
            nxt = draw_idx[:, 0].long()
            toks[:, t + 1] = nxt
            lps[:, t + 1] = draw_val[:, 0]
            t += 1
            hit = nxt == eos_idx
            where_eos = torch.minimum(where_eos, torch.where(hit, torch.full_like(where_eos, t), where_eos))
            finished |= hit
            st.next_tok.copy_(nxt)
            if t % _DONE_POLL == 0 and bool(finished.all()):
                break
        toks_h, eos_h = toks.cpu(), where_eos.cpu()
        res = [[toks_h[i * num_outputs + j, :int(eos_h[i * num_outputs + j]) + 1].tolist()
                for j in range(num_outputs)] for i in range(bs)]
        # the reference stops at the step every sequence has finished (:96-97) and pads to the longest one: the
        # host only looks every _DONE_POLL steps, so trim the columns the extra steps added
        width = int(eos_h.max()) + 1
        ar = torch.arange(width, device=dv)[None, :]
        probs = lps[:, :width].masked_fill(ar > where_eos[:, None], 0.0).reshape(bs, num_outputs, -1)
        return res, _to_input_device(probs, enc_input)

    # ------------------------------------------------------------------ search
    def beam_search(self, enc_input, enc_input_num_pads, sos_idx, eos_idx, beam_size=3, how_many_outputs=1,
                    max_seq_len=20, sample_or_max="max", *, no_repeat_ngram_size=0, min_length=0, banned_words=None,
                    prefix=None, required_words=None, temperature=1.0, top_k=0, top_p=1.0):
        """The reference's beam search.  Keyword-only controls over what it may choose, applied on the
        device inside the step: `no_repeat_ngram_size` = n > 0: no caption holds an n-gram twice; `min_length`: at least
        that many words between SOS and EOS; `banned_words`: word ids that never appear.  With the defaults the search
        launches exactly what it launches without them.
        `prefix`: words every caption starts with — one list of word ids for all images, or one list per
        image, all of one length P <= max_seq_len - 2.  The returned token lists are [sos, prefix…, continuation…] and the
        log-probs include the prefix words' own, so a prefixed result agrees with score_captions like any other;
        max_seq_len, min_length and the n-gram rule count the prefix words (a prefix may hold banned words).  One
        whole-sequence decoder pass over the prefix replaces its P steps.
        `required_words`: word ids every caption must contain — one list for all images, or one list per
        image (ragged lists allowed), C <= 4 words at most.  The search then keeps `beam_size` beams PER BANK, a bank for
        every subset of the C words (2^C·beam_size <= 16 rows per image), and a caption may take EOS only once it holds all
        its words (odic_require_beam_step).  Output j of an image is the j-th best caption that holds them all;
        `self.last_required_satisfied` says per image whether there was one (else the outputs are the best captions the
        search still had).  Composes with the three controls above; not with `prefix` or sample_or_max='sample'.  None, [] or
        nothing but empty lists: exactly the search without the keyword.
        `temperature`, `top_k`, `top_p`, with sample_or_max='sample' only: every beam's candidates are
        drawn from softmax(logits / temperature) cut to its top_k best words (0 = all) and to the nucleus of mass top_p
        (1 = all), never fewer than beam_size words; the log-probs and the ranking stay the model's own."""
        assert (how_many_outputs <= beam_size), "requested output per sequence must be lower than beam width"
        assert (sample_or_max == "max" or sample_or_max == "sample"), \
            "argument must be chosen between 'max' and 'sample'"
        sampling = sample_or_max == "sample"
        flt = _search.check_sampling_filter(temperature, top_k, top_p, sampling=sampling)
        self.last_required_satisfied = None
        required = self._search_required_arg(required_words, enc_input, beam_size=beam_size, banned_words=banned_words,
                                             sos_idx=sos_idx, eos_idx=eos_idx, max_seq_len=max_seq_len, sampling=sampling)
        rows_per_image = beam_size << len(required[0]) if required else beam_size
        cons = self._search_constraint_args(no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                            banned_words=banned_words, sos_idx=sos_idx, eos_idx=eos_idx,
                                            max_seq_len=max_seq_len, rows_per_image=rows_per_image, sampling=sampling)
        prefix = self._search_prefix_arg(prefix, enc_input, sos_idx=sos_idx, eos_idx=eos_idx, max_seq_len=max_seq_len,
                                         sampling=sampling)
        if required and prefix:
            raise ValueError("required_words together with prefix is not supported")
        if required:
            self._check_rows_fit(rows_per_image)
        mem = self.forward_enc(enc_input, enc_input_num_pads)
        if required:
            toks, lp = self._required_search_from_memory(mem, enc_input_num_pads, sos_idx, eos_idx, beam_size,
                                                         how_many_outputs, max_seq_len, required, cons)
        else:
            toks, lp = self._search_from_memory(mem, enc_input_num_pads, sos_idx, eos_idx, beam_size, how_many_outputs,
                                                max_seq_len, sample=sampling, constraints=cons, prefix=prefix,
                                                sample_filter=flt)
        return toks, _to_input_device(lp, enc_input)

    def _required_search_from_memory(self, mem, enc_input_num_pads, sos_idx, eos_idx, bank_beams, how_many_outputs,
                                     max_seq_len, required: List[List[int]], constraints: Optional[dict]):
        """beam_search with required words (check_required_words' lists): 2^C banks of bank_beams rows per image."""
        R = bank_beams << len(required[0])
        eng, st, steps = self._open_search(mem, enc_input_num_pads, R, max_seq_len)
        req = torch.tensor(required, dtype=torch.int64, device=eng.device)

        def req_logp():                          # the log: the candidates and the required words' log-probs per row
            logp_h, req_h = st.logp.cpu(), req.cpu().repeat_interleave(R, dim=0)
            return torch.where(req_h >= 0, logp_h.gather(1, req_h.clamp(min=0)), torch.tensor(float("-inf")))

        def pick(order, score):
            rows, self.last_required_satisfied = _search.required_outputs(
                order.cpu().tolist(), st.cumul.view(st.n_img, R).cpu().tolist(), required, bank_beams, how_many_outputs)
            return rows

        step = lambda cons: eng.require_beam_step(st, eos_idx, req, bank_beams, constraints=cons)      # noqa: E731
        return _search.run_search(eng, st, eos_idx, steps, how_many_outputs, constraints=constraints, pick=pick,
                                  step=_search.logged(step, st, self._cand_log, req_logp),
                                  arm=lambda: _search.arm_state(eng, st, sos_idx, emb=st.emb))

    def _search_from_memory(self, mem, enc_input_num_pads, sos_idx, eos_idx, beam_size, how_many_outputs,
                            max_seq_len, sample: bool = False, constraints: Optional[dict] = None,
                            prefix: Optional[List[List[int]]] = None, sample_filter=None
                            ) -> Tuple[List[List[List[int]]], torch.Tensor]:
        eng, st, steps = self._open_search(mem, enc_input_num_pads, beam_size, max_seq_len)
        seed = self._next_sampling_seed() if sample else 0

        def draw_step(cons):
            # 'sample' variant (captioning_model.py:128-131,166-168): the k candidates of every beam are drawn
            # without replacement from its distribution instead of being its top-k — on the device
            eng.step_logits(st)
            _search.draw_candidates(st.logits, st.cand_val, st.cand_idx, st.N, eng.g.vocab_size, beam_size, seed, st.pos,
                                    sample_filter)
            if self._draw_log is not None:                        # test hook: the draws, for replay in the oracle
                self._draw_log.append(st.cand_idx.cpu().clone())
            ops.beam_step(st.cand_val, st.cand_idx, st.beam_state, st.n_img, st.beams, st.T, eos_idx)

        step = _search.logged(lambda cons: eng.beam_step(st, eos_idx, constraints=cons), st, self._cand_log)
        # (a prefix never comes with `sample`: check_prefix; the log-probs are on the engine's device, beam_search moves them)
        return _search.run_search(eng, st, eos_idx, steps - (len(prefix[0]) if prefix else 0), how_many_outputs,
                                  constraints=constraints, step=draw_step if sample else step,
                                  arm=lambda: _search.arm_state(eng, st, sos_idx, prefix, emb=None if sample else st.emb))

    def diverse_beam_search(self, enc_input, enc_input_num_pads, sos_idx, eos_idx, num_groups=3, group_size=3,
                            diversity_penalty=0.5, how_many_outputs=None, max_seq_len=20, *, no_repeat_ngram_size=0,
                            min_length=0, banned_words=None, prefix=None, required_words=None):
        """Diverse (group) beam search (Vijayakumar et al.): `num_groups` groups of `group_size` beams per image.
        Within a step the groups choose one after the other, and a group pays `diversity_penalty` for every earlier
        group that appended the same word at this step (odic_group_beam_step).  The penalty only steers
        the choice: the returned log-probs and the ranking (sum of log-probs / length) are the model's own.
        Output j of an image is the best beam of group j (ties → the lower row), in group order — output 0 is what
        beam_search(beam_size=group_size) returns, group 0 never being penalised.  `how_many_outputs` defaults to
        num_groups and may not exceed it.  Returns what beam_search returns: a token list per image and output, and
        the padded per-token log-probs [B, how_many_outputs, longest].
        `no_repeat_ngram_size`, `min_length`, `banned_words`: as in beam_search; every group's caption keeps them (the
        words are removed before the ranking the penalty works on).  `prefix`: as in beam_search; every group starts
        behind it, and the groups part at the first free word as they part at the first word without it.
        `required_words`: beam_search's; anything but nothing required is refused here."""
        if how_many_outputs is None:
            how_many_outputs = num_groups
        _search.refuse_required_words(required_words, "in diverse_beam_search")
        if num_groups < 1 or group_size < 1 or num_groups * group_size > 16:
            raise ValueError("diverse_beam_search needs num_groups >= 1, group_size >= 1 and num_groups·group_size <= 16")
        if not 1 <= how_many_outputs <= num_groups:
            raise ValueError("requested outputs per image must lie in [1, num_groups]: a group yields one caption")
        penalty = float(diversity_penalty)
        if not (0.0 <= penalty < float("inf")):
            raise ValueError("diversity_penalty must be finite and >= 0")
        constraints = self._search_constraint_args(no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                                   banned_words=banned_words, sos_idx=sos_idx, eos_idx=eos_idx,
                                                   max_seq_len=max_seq_len, rows_per_image=num_groups * group_size)
        prefix = self._search_prefix_arg(prefix, enc_input, sos_idx=sos_idx, eos_idx=eos_idx, max_seq_len=max_seq_len)
        mem = self.forward_enc(enc_input, enc_input_num_pads)
        G, kg = int(num_groups), int(group_size)
        self._check_rows_fit(G * kg, "beams")
        eng, st, steps = self._open_search(mem, enc_input_num_pads, G * kg, max_seq_len)

        def pick(order, score):                                   # output j of an image: the best row of group j
            best = score.view(st.n_img, G, kg).cpu().argmax(dim=2)     # (first maximum: ties go to the lower row)
            return (torch.arange(G)[None, :] * kg + best)[:, :how_many_outputs]

        step = lambda cons: eng.group_beam_step(st, eos_idx, G, penalty, constraints=cons)              # noqa: E731
        res_tok, lp = _search.run_search(eng, st, eos_idx, steps - (len(prefix[0]) if prefix else 0), how_many_outputs,
                                         constraints=constraints, step=_search.logged(step, st, self._cand_log), pick=pick,
                                         arm=lambda: _search.arm_state(eng, st, sos_idx, prefix, emb=st.emb, group_beams=kg))
        return res_tok, _to_input_device(lp, enc_input)

    def stochastic_beam_search(self, enc_input, enc_input_num_pads, sos_idx, eos_idx, num_samples=5, max_seq_len=20,
                               seed=None, *, prefix=None, required_words=None, no_repeat_ngram_size=0, min_length=0,
                               banned_words=None, temperature=1.0, top_k=0, top_p=1.0):
        """Stochastic beam search (Kool, van Hoof & Welling, ICML 2019): `num_samples` captions per image
        sampled from the model WITHOUT replacement — always distinct, the first an exact sample from the model, the set a
        Plackett-Luce sample over whole captions.  Every step is the decoder, one launch that draws every row's words with
        their Gumbel-perturbed scores (odic_logsoftmax_sample_scored) and one that keeps the rows with the largest
        perturbed scores (odic_stochastic_beam_step).  Returns what beam_search(how_many_outputs=num_samples) returns;
        output j is row j, in sampling order (descending perturbed score), and the log-probs are the model's own.
        The search runs num_samples + 1 rows, so 1 <= num_samples <= 15.  It sets
          self.last_stochastic_beam = {"gumbel": fp32 [B, num_samples], "kappa": fp32 [B], "sum_logprob": fp32 [B, num_samples]}
        on the device: the samples' perturbed scores, the perturbed score of the extra row (-inf when the image had no
        further caption to offer) and the samples' log-probs phi.  Given kappa, sample s was included with probability
        1 − exp(−exp(phi_s − kappa)): what a without-replacement REINFORCE estimator weighs it by (not computed here).
        `seed`: the Philox key of the noise; None draws one from torch's default generator (torch.manual_seed governs it),
        and leaves `sampling_seed`'s call counter alone.
        prefix, required_words, no_repeat_ngram_size, min_length, banned_words, temperature / top_k / top_p: accepted so
        that a call that names them fails loudly — anything but their defaults raises ValueError: they change the
        distribution that is sampled."""
        n = _search.check_stochastic_beam(num_samples, prefix=prefix, required_words=required_words,
                                          no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                          banned_words=banned_words, temperature=temperature, top_k=top_k, top_p=top_p)
        R = n + 1
        self._check_rows_fit(R)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        mem = self.forward_enc(enc_input, enc_input_num_pads)
        eng, st, steps = self._open_search(mem, enc_input_num_pads, R, max_seq_len)
        B = st.n_img

        def pick(order, score):                                   # the rows are in sampling order already
            return torch.arange(n)[None, :].expand(B, n)

        step = _search.logged(lambda cons: eng.stochastic_beam_step(st, eos_idx, seed), st, self._cand_log,
                              lambda: st.cand_pert.cpu().clone())
        res_tok, lp = _search.run_search(eng, st, eos_idx, steps, n, step=step, pick=pick,
                                         arm=lambda: _search.arm_state(eng, st, sos_idx, emb=st.emb))
        g = st.gscore.view(B, R)
        self.last_stochastic_beam = {"gumbel": g[:, :n].clone(), "kappa": g[:, n].clone(),
                                     "sum_logprob": st.cumul.view(B, R)[:, :n].clone()}
        return res_tok, _to_input_device(lp, enc_input)

    def pool_beam_search(self, enc_input, enc_input_num_pads, sos_idx, eos_idx, beam_size=3, how_many_outputs=1,
                         max_seq_len=20, length_penalty=1.0, early_stopping=False, no_repeat_ngram_size=0, min_length=0,
                         banned_words=None, *, prefix=None, required_words=None, sample_or_max="max"):
        """Beam search with a pool of finished captions: a beam that takes EOS leaves the beam for a
        per-image pool of at most `beam_size` finished captions scored by (sum of log-probs) / length^`length_penalty`
        (length counts SOS and EOS; 1.0 is the final ranking of beam_search, 0 ranks by the raw sum, larger values favour
        longer captions), so all `beam_size` rows keep exploring, and an image stops once its pool is full and no live
        row can still beat the pool's worst entry — or, with `early_stopping`, as soon as the pool is full.  Rows still
        unfinished when the steps run out join the pool as they are.  Every step is the decoder, the constrained row
        selection with EOS inadmissible and odic_pool_beam_step.
        Returns what beam_search returns: output j of an image is the j-th best caption of its pool, with the model's own
        per-token log-probs.  `self.last_pool_scores` (fp32 [B, how_many_outputs]) holds their scores,
        `self.last_pool_counts` (int32 [B]) the captions each pool held and `self.last_pool_closed` (bool [B]) whether the
        image closed before the steps ran out (every caption of such an image ends in EOS).  A pool holds fewer than
        how_many_outputs captions only when every candidate of the image died (-inf rows): the missing outputs are then
        the EMPTY caption [sos, eos] with log-probs [0, -inf] and score -inf.
        how_many_outputs <= beam_size <= 15.  `no_repeat_ngram_size`, `min_length`, `banned_words`: as in beam_search.
        prefix, required_words and sample_or_max='sample' are accepted so that a call that names them fails loudly:
        ValueError, like length_penalty < 0 or not finite."""
        alpha = _search.check_pool_beam(beam_size, how_many_outputs, length_penalty, prefix=prefix,
                                        required_words=required_words, sample_or_max=sample_or_max)
        k, n_out = int(beam_size), int(how_many_outputs)
        cons = self._search_constraint_args(no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                            banned_words=banned_words, sos_idx=sos_idx, eos_idx=eos_idx,
                                            max_seq_len=max_seq_len, rows_per_image=k) or {}
        self._check_rows_fit(k + 1, "beams and EOS")
        mem = self.forward_enc(enc_input, enc_input_num_pads)
        eng, st, steps = self._open_search(mem, enc_input_num_pads, k, max_seq_len)
        pool = ops.Pool(st.n_img, k, st.T, alpha, cons.get("min_words", 0), bool(early_stopping), eng.device)
        dev_cons = eng.pool_constraints(st, eos_idx, no_repeat_ngram=cons.get("no_repeat_ngram", 0),
                                        banned=cons.get("banned"))

        def arm():
            _search.arm_state(eng, st, sos_idx, emb=st.emb)
            ops.pool_reset(pool.args, st.n_img)

        def finish():
            closed = pool.closed.cpu() != 0                       # (before the finalize marks every image)
            toks, lp, self.last_pool_scores, self.last_pool_counts = _search.read_pool(st, pool, n_out, sos_idx, eos_idx)
            self.last_pool_closed = closed
            return toks, lp

        step = _search.logged(lambda _: eng.pool_beam_step(st, pool, eos_idx, dev_cons), st, self._cand_log,
                              lambda: st.logp[:, eos_idx].cpu().clone())
        res_tok, lp = _search.run_search(eng, st, eos_idx, steps, n_out, arm=arm, step=step, finish=finish)
        return res_tok, _to_input_device(lp, enc_input)

    def contrastive_beam_search(self, enc_input, enc_input_num_pads, sos_idx, eos_idx, distractors, beam_size=3,
                                how_many_outputs=1, max_seq_len=20, *, contrast=0.5, plausibility=0.1,
                                suppressor_floor=-20.0, no_repeat_ngram_size=0, min_length=0, banned_words=None,
                                prefix=None, required_words=None, sample_or_max="max"):
        """Distinctive captions: the emitter–suppressor beam search of Vedantam et al. (CVPR 2017) with
        the plausibility cut of contrastive decoding (Li et al. 2022).  `distractors`: for every image a sequence of
        0..7 distinct indices of OTHER images of this batch (ragged lists allowed), or 'others' for all of them
        (B - 1 <= 7).  At every step a word of an image's beam is ranked by
            log p(word | image) − contrast · max(log mean_d p(word | distractor d), suppressor_floor)
        among the words whose probability under the image itself is at least `plausibility` times its best word's (0 = no
        cut; never fewer than the words the step needs), so the caption says what tells the image apart from its
        distractors without leaving what the model finds sayable.  The encoder and the K/V projection run once per
        batch; a distractor is the same beam prefix decoded against another image's memory, so a step costs about
        1 + D decoder passes, D the longest distractor list, and one launch for the scores (odic_contrast_topk).
        An image without distractors, and every image at contrast = 0 with plausibility = 0, gets beam_search's captions.
        Returns what beam_search returns; the per-word values are the CONTRASTIVE scores the search ranked by (they can
        be positive), not log-probs: score_captions gives the model's own log-probs of the returned captions.
        `no_repeat_ngram_size`, `min_length`, `banned_words`: as in beam_search.  prefix, required_words and
        sample_or_max='sample' are accepted so that a call that names them fails loudly: ValueError."""
        assert (how_many_outputs <= beam_size), "requested output per sequence must be lower than beam width"
        B = enc_input.shape[0]
        c = _search.check_contrast(distractors, B, contrast=contrast, plausibility=plausibility,
                                   suppressor_floor=suppressor_floor, prefix=prefix, required_words=required_words,
                                   sample_or_max=sample_or_max)
        cons = self._search_constraint_args(no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                            banned_words=banned_words, sos_idx=sos_idx, eos_idx=eos_idx,
                                            max_seq_len=max_seq_len, rows_per_image=beam_size)
        self._check_rows_fit(beam_size, "beams")
        mem = self.forward_enc(enc_input, enc_input_num_pads)
        k = int(beam_size)
        eng, st, steps = self._open_search(mem, enc_input_num_pads, k, max_seq_len)
        dv = eng.device
        states = [st]
        for d in range(c["D"]):      # distractor d of every image: its memory rows (an unused slot: the image's own; count masks it)
            idx = torch.tensor([r[d] if d < len(r) else i for i, r in enumerate(c["lists"])], dtype=torch.int64, device=dv)
            states.append(eng.new_state(B, k, st.T, st.kv.index_select(0, idx).contiguous(), st.enc_len.index_select(0, idx)))
        _search.share_beam_state(states)
        count = torch.tensor([len(r) for r in c["lists"]], dtype=torch.int32, device=dv).repeat_interleave(k).contiguous()
        # under constraints a row can lose n_banned + T words (odic_topk_rows_constrained): beam_size finite ones remain
        min_keep = k + (len(cons["banned"]) + st.T if cons else 0)
        args = ops.contrast_args(c["contrast"], c["plausibility"], c["suppressor_floor"], min_keep)
        step = lambda dev_cons: eng.contrast_beam_step(states, count, args, eos_idx, constraints=dev_cons)     # noqa: E731
        res_tok, lp = _search.run_search(eng, st, eos_idx, steps, how_many_outputs, constraints=cons,
                                         step=_search.logged(step, st, self._cand_log),
                                         arm=lambda: _search.arm_state(eng, st, sos_idx, emb=None))
        return res_tok, _to_input_device(lp, enc_input)

    def consensus_caption(self, enc_x, enc_x_num_pads=[0], *, num_candidates, source="sampling", sos_idx, eos_idx,
                          max_seq_len=20, corpus=None, metric="cider", **search_args):
        """One caption per image by consensus: draw `num_candidates` candidates, score each against the
        others under CIDEr-D on the device (reward.consensus_rerank) and return the one that agrees most with the rest.
        source='sampling': get_batch_multiple_sampled_prediction(num_outputs=num_candidates, **search_args) — temperature,
        top_k, top_p; source='diverse': diverse_beam_search(num_groups=num_candidates, **search_args) — group_size (default
        1), diversity_penalty and the search controls; source='stochastic_beam': stochastic_beam_search(num_samples=
        num_candidates, **search_args) — `seed`; the candidates are distinct, so no pair is scored twice.  `corpus`: a reward.CiderCorpus whose IDF table weighs the n-grams
        (default: every n-gram counts 1).  `metric`: 'cider', or 'bleu4' / 'rouge_l' for the pairwise sentence BLEU-4 or
        ROUGE-L F as the utility (§4.20; no corpus with them).  → (captions: one token list per image, scores fp64 [B]: its
        mean utility against the other candidates).  `self.last_consensus` keeps (candidates, best_index [B], scores [B, N])."""
        from . import reward as _reward
        if num_candidates < 1:
            raise ValueError("consensus_caption needs num_candidates >= 1")
        if source == "sampling":
            cands, _ = self.get_batch_multiple_sampled_prediction(enc_x, enc_x_num_pads, num_candidates, sos_idx, eos_idx,
                                                                  max_seq_len, **search_args)
        elif source == "diverse":
            search_args.setdefault("group_size", 1)
            cands, _ = self.diverse_beam_search(enc_x, enc_x_num_pads, sos_idx, eos_idx, num_groups=num_candidates,
                                                max_seq_len=max_seq_len, **search_args)
        elif source == "stochastic_beam":
            cands, _ = self.stochastic_beam_search(enc_x, enc_x_num_pads, sos_idx, eos_idx, num_samples=num_candidates,
                                                   max_seq_len=max_seq_len, **search_args)
        else:
            raise ValueError("source must be 'sampling', 'diverse' or 'stochastic_beam'")
        index, scores = _reward.consensus_rerank(cands, corpus=corpus, eos_idx=eos_idx, metric=metric)
        self.last_consensus = (cands, index, scores)
        best = index.tolist()
        return [cands[b][best[b]] for b in range(len(cands))], scores.gather(1, index[:, None])[:, 0]


def _as_list(pads, n: int) -> List[int]:
    if isinstance(pads, torch.Tensor):
        pads = pads.tolist()
    pads = list(pads)
    if len(pads) != n:
        raise RuntimeError(f"expected {n} pad counts, got {len(pads)}")
    return [int(p) for p in pads]


def _to_input_device(x: torch.Tensor, enc_input) -> torch.Tensor:
    """A result goes back on the device its input came from; an input that is no tensor leaves it on the engine's."""
    return x.to(enc_input.device) if isinstance(enc_input, torch.Tensor) else x


# =================================================================================================
# refactored API  (models/captioning_model.py:40-110, models/End_ExpansionNet_v2.py:311-354)
# =================================================================================================
class Captioner:
    def __init__(self, beam_search_args, model=None, split_encoder=False, apply_log_softmax=False, encoder=None,
                 decoder=None):
        self.rank = None
        self.split_encoder = split_encoder
        if self.split_encoder:
            self.encoder, self.decoder = encoder, decoder
            if self.encoder is None or self.decoder is None:
                raise ValueError("Both encoder and decoder must be supplied in Split Encoder mode")
            raise NotImplementedError("split encoder/decoder modules exist for the reference's FX int8 "
                                      "quantisation route, which is out of scope (SURVEY §2 row 21)")
        self.model = model
        if self.model is None:
            raise ValueError("An Encoder-Decoder model must be provided")
        self.beam_search_args = beam_search_args
        self.apply_log_softmax = apply_log_softmax

    def __call__(self, enc_x, dec_x=None, enc_x_num_pads=[0], dec_x_num_pads=[0], mode="beam_search"):
        assert ("sos_idx" in self.beam_search_args.keys() or "eos_idx" in self.beam_search_args.keys()), \
            "sos and eos must be provided in case of batch sampling or beam search"
        self.apply_log_softmax = True
        return _search.dispatch(self.model, mode, self._dispatch_args(), enc_x, enc_x_num_pads)

    def _dispatch_args(self, **more) -> dict:
        """`beam_search_args` (and `more`) as search.dispatch takes them; sos_idx and eos_idx are required here (KeyError;
        forward() has -999)."""
        a = self.beam_search_args
        return dict(a, sos_idx=a["sos_idx"], eos_idx=a["eos_idx"], **more)

    def _fill_search_defaults(self, k: dict, *names) -> None:
        """Every keyword of `names` the call left out takes its value from `beam_search_args`, where that has one
        (max_seq_len is its beam_max_seq_len)."""
        for name in names:
            key = "beam_max_seq_len" if name == "max_seq_len" else name
            if key in self.beam_search_args:
                k.setdefault(name, self.beam_search_args[key])

    def forward_enc(self, enc_input, enc_input_num_pads):
        return self.model.forward_enc(enc_input, enc_input_num_pads)

    def forward_dec(self, cross_input, enc_input_num_pads, dec_input, dec_input_num_pads):
        return self.model.forward_dec(cross_input, enc_input_num_pads, dec_input, dec_input_num_pads,
                                      self.apply_log_softmax)

    def beam_search(self, *a, **k):
        return self.model.beam_search(*a, **k)

    def diverse_beam_search(self, *a, **k):
        return self.model.diverse_beam_search(*a, **k)

    def stochastic_beam_search(self, *a, **k):
        return self.model.stochastic_beam_search(*a, **k)

    def contrastive_beam_search(self, *a, **k):
        return self.model.contrastive_beam_search(*a, **k)

    def pool_beam_search(self, *a, **k):
        return self.model.pool_beam_search(*a, **k)

    def consensus_caption(self, enc_x, enc_x_num_pads=[0], *, metric="cider", **k):
        """CaptioningModel.consensus_caption with this object's `beam_search_args` (sos_idx, eos_idx, beam_max_seq_len)
        unless the call names its own."""
        k["metric"] = metric
        self._fill_search_defaults(k, "sos_idx", "eos_idx", "max_seq_len")
        return self.model.consensus_caption(enc_x, enc_x_num_pads, **k)

    def score_captions(self, *a, **k):
        return self.model.score_captions(*a, **k)

    def caption_loss(self, *a, **k):
        return self.model.caption_loss(*a, **k)

    def word_attention(self, enc_x, captions=None, *a, **k):
        """CaptioningModel.word_attention; the generated-caption form (`captions=None`) searches with this object's
        `beam_search_args` (sos_idx, eos_idx, beam_size, beam_max_seq_len) unless the call names its own."""
        self._fill_search_defaults(k, "sos_idx", "eos_idx", "beam_size", "max_seq_len")
        return self.model.word_attention(enc_x, captions, *a, **k)

    def caption_regions(self, preprocessor, images, regions, distinctive=False, **contrast_args):
        """Captions of parts of pictures that live on the device: `preprocessor.resize_regions(images, regions)` (a
        DevicePreprocessor of the model's input size; images: uint8 (H,W,3) device tensors as its `decode_jpeg` returns
        them; regions: sequence of (image index, (l, t, r, b)), the box as PIL's `resize(..., box=)` takes it), then
        this object's encode and search on that batch (`__call__`).  Returns one list per input image,
        holding a grounding.RegionCaption for each of its regions in the order they were given; an image without a
        region gets an empty list.
        `distinctive=True`: the search is contrastive_beam_search with, for every region, the OTHER
        regions of the same source image as its distractors, so sibling crops stop sharing one caption; `contrast_args`
        (contrast, plausibility, suppressor_floor) go to it, the rest comes from `beam_search_args` as in `__call__`
        with mode='contrastive_beam_search'.  A region without siblings gets beam_search's caption; more than 7 siblings is
        a ValueError.  The RegionCaption's `logprobs` are then the contrastive scores."""
        regions = [(int(i), tuple(float(v) for v in box)) for i, box in regions]
        per_image = [[] for _ in images]
        if not regions:
            return per_image
        if not distinctive and contrast_args:
            raise ValueError(f"{sorted(contrast_args)} apply to distinctive=True only")
        if distinctive:
            siblings = [[m for m, (j, _) in enumerate(regions) if j == i and m != n] for n, (i, _) in enumerate(regions)]
            most = max(len(r) for r in siblings)
            if most > _search.MAX_DISTRACTORS:
                raise ValueError(f"a region with {most} sibling regions: distinctive captions take at most "
                                 f"{_search.MAX_DISTRACTORS} distractors per region")
        batch = preprocessor.resize_regions(images, regions)
        if distinctive:
            toks, lps = _search.dispatch(self.model, "contrastive_beam_search",
                                         self._dispatch_args(distractors=siblings, **contrast_args), batch, [0] * len(regions))
        else:
            toks, lps = self(batch, enc_x_num_pads=[0] * len(regions))
        for n, (i, box) in enumerate(regions):
            per_image[i].append(_grounding.RegionCaption(region=n, box=box, tokens=toks[n], logprobs=lps[n]))
        return per_image
