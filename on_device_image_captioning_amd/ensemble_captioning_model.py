"""Ensemble beam search (reference models/ensemble_captioning_model.py:5-291, same class
name and call shape: `EsembleCaptioningModel(models_list, rank)`, `forward(..., mode='beam_search')`).

Every member encodes and decodes on its own step engine; the per-step distribution is
log(mean_m softmax(logits_m)) (`odic_ensemble_logprobs`), its row-wise top-k (`odic_topk_rows`) feeds the
same on-device beam bookkeeping (`odic_beam_step`) as the single-model search.  The members share ONE beam
state (tokens, ancestor table, positions, finished flags) — only their caches and logits are private, so
the incremental decoding stays exact for each of them.
"""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn

from . import ops
from . import search as _search
from .captioning_model import CaptioningModel


class EsembleCaptioningModel(CaptioningModel):
    def __init__(self, models_list, rank):
        super().__init__()
        self.num_models = len(models_list)
        self.models_list = models_list
        self.rank = rank
        self.dummy_linear = nn.Linear(1, 1)                       # reference :13 (keeps .parameters() non-empty)
        for model in self.models_list:
            model.eval()

    def forward(self, enc_x, dec_x=None, enc_x_num_pads=[0], dec_x_num_pads=[0], apply_log_softmax=False,
                mode="beam_search", **kwargs):
        assert mode == "beam_search", "this class supports only beam search."
        return _search.dispatch(self, mode, kwargs, enc_x, enc_x_num_pads)

    def forward_enc(self, enc_input, enc_input_num_pads):
        return [m.forward_enc(enc_input, enc_input_num_pads) for m in self.models_list]

    # ------------------------------------------------------------------ scoring (CaptioningModel.score_captions)
    def _vocab_size(self) -> int:
        sizes = {m._vocab_size() for m in self.models_list}
        if len(sizes) != 1:
            raise ValueError(f"the members of an ensemble must share one vocabulary (sizes {sorted(sizes)})")
        return sizes.pop()

    def _max_seq_len(self) -> int:
        return min(m._max_seq_len() for m in self.models_list)

    def _sequence_stats(self, enc_x, enc_x_num_pads, n_img, dec, dec_len, targets, row_chunk=None) -> dict:
        """Per member the whole-sequence logits of a row chunk, averaged as the search averages a step
        (odic_ensemble_logprobs), then the same odic_token_stats as the single model: its log-sum-exp of an already
        normalised row is ~0, and there is one code path.
        `row_chunk` here bounds the logits rows held at once over ALL members (each member's [rows, V] tensor plus the
        average): the captions are processed in groups of whole images of about row_chunk / (members + 1) rows, each group
        one decode_sequence(want_logits=True) call per member (whose own vocabulary product then fits one chunk)."""
        V = self._vocab_size()
        engs = [m._captioner_engine() for m in self.models_list]
        dv = engs[0].device
        N, T = dec.shape
        dec, dec_len, tg = dec.to(dv), dec_len.to(dv), targets.to(dv).contiguous().view(-1)
        per_img = N // n_img
        # whole captions-of-an-image groups per chunk, so that every chunk is a decode_sequence call of its own
        imgs_per_chunk = max(1, (row_chunk or engs[0].vocab_row_chunk()) // (per_img * T * (len(engs) + 1)))
        kvs, lens = [], []
        for m, eng, mem in zip(self.models_list, engs, self.forward_enc(enc_x, enc_x_num_pads)):
            kvs.append(eng.project_kv(mem))
            lens.append(m._enc_lens(n_img, mem.shape[1], enc_x_num_pads))
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dv)      # noqa: E731
        logp, sum_logp, max_logp = f(N * T), f(N * T), f(N * T)
        argmax = torch.empty(N * T, dtype=torch.int32, device=dv)
        status = torch.zeros(1, dtype=torch.int32, device=dv)
        for i0 in range(0, n_img, imgs_per_chunk):
            i1 = min(n_img, i0 + imgs_per_chunk)
            r0, r1 = i0 * per_img, i1 * per_img
            lg = [eng.decode_sequence(dec[r0:r1], dec_len[r0:r1], kv[i0:i1], ln[i0:i1], i1 - i0, want_logits=True)
                  .view(-1, V) for eng, kv, ln in zip(engs, kvs, lens)]
            avg = f((r1 - r0) * T, V)
            ops.ensemble_logprobs(lg, avg)
            a, b = r0 * T, r1 * T
            ops.token_stats(avg, V, tg[a:b], logp[a:b], sum_logp[a:b], argmax[a:b], max_logp[a:b], status, b - a, V)
        return {"logp": logp.view(N, T), "sum_logp": sum_logp.view(N, T), "argmax": argmax.view(N, T),
                "max_logp": max_logp.view(N, T), "status": status}

    def word_attention(self, *a, **k):
        raise NotImplementedError("an ensemble has no single set of attention maps: call word_attention on one of its "
                                  "member models (models_list[i])")

    def diverse_beam_search(self, *a, **k):
        raise NotImplementedError("diverse beam search runs on a single model: call it on one of the ensemble's member "
                                  "models (models_list[i])")

    def stochastic_beam_search(self, *a, **k):
        raise NotImplementedError("stochastic beam search runs on a single model: call it on one of the ensemble's member "
                                  "models (models_list[i])")

    def pool_beam_search(self, *a, beam_size=3, how_many_outputs=1, length_penalty=1.0, **k):
        """Refused (search.check_pool_beam): the pooled search runs on a single model."""
        _search.check_pool_beam(beam_size, how_many_outputs, length_penalty, ensemble=True)

    def contrastive_beam_search(self, *a, **k):
        raise NotImplementedError("contrastive beam search runs on a single model: call it on one of the ensemble's member "
                                  "models (models_list[i])")

    def ensemble_beam_search(self, enc_input, enc_input_num_pads, sos_idx, eos_idx, beam_size=3, how_many_outputs=1,
                             max_seq_len=20, sample_or_max="max", *, no_repeat_ngram_size=0, min_length=0,
                             banned_words=None, prefix=None, required_words=None, temperature=1.0, top_k=0, top_p=1.0
                             ) -> Tuple[List[List[List[int]]], torch.Tensor]:
        """`no_repeat_ngram_size`, `min_length`, `banned_words`: as in CaptioningModel.beam_search; the constrained
        selection (odic_topk_rows_constrained) then replaces odic_topk_rows on the averaged log-probs.
        `prefix`: as in CaptioningModel.beam_search; every member fills its caches in one pass over the prefix and the
        prefix words' log-probs are the averaged distribution's (search.ensemble_seed_prefix).
        `required_words`: CaptioningModel.beam_search's; anything but nothing required is refused here.
        `temperature`, `top_k`, `top_p`: as in CaptioningModel.beam_search, on the averaged distribution."""
        assert (how_many_outputs <= beam_size), "requested output per sequence must be lower than beam width"
        assert (sample_or_max == "max" or sample_or_max == "sample"), \
            "argument must be chosen between 'max' and 'sample'"
        sample = sample_or_max == "sample"
        flt = _search.check_sampling_filter(temperature, top_k, top_p, sampling=sample)
        _search.refuse_required_words(required_words, "in ensemble_beam_search")
        constraints = self._search_constraint_args(no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                                   banned_words=banned_words, sos_idx=sos_idx, eos_idx=eos_idx,
                                                   max_seq_len=max_seq_len, rows_per_image=beam_size, sampling=sample)
        prefix = self._search_prefix_arg(prefix, enc_input, sos_idx=sos_idx, eos_idx=eos_idx, max_seq_len=max_seq_len,
                                         sampling=sample)
        # 'sample' (reference models/ensemble_captioning_model.py:123-130,174-183): the k candidates of every beam are drawn
        # without replacement from the averaged distribution — odic_logsoftmax_sample on rows that already are
        # log-probabilities (its normalisation is then the identity up to rounding), keyed by the lead member's seed
        seed = self.models_list[0]._next_sampling_seed() if sample else None
        mems = self.forward_enc(enc_input, enc_input_num_pads)
        engs, states = [], []
        for m, mem in zip(self.models_list, mems):
            eng, st, steps = m._open_search(mem, enc_input_num_pads, beam_size, max_seq_len)
            engs.append(eng)
            states.append(st)
        lead = _search.share_beam_state(states)
        avg = torch.empty(lead.N, engs[0].g.vocab_size, dtype=torch.float32, device=engs[0].device)
        # (the log-probs stay on the engine's device, unlike beam_search's, which go to the input's)
        return _search.run_search(
            engs[0], lead, eos_idx, steps - (len(prefix[0]) if prefix else 0), how_many_outputs, constraints=constraints,
            arm=lambda: _search.arm_state(     # (emb: the members embed for themselves in step_logits)
                engs[0], lead, sos_idx, prefix, emb=None,
                seed_prefix=lambda p: _search.ensemble_seed_prefix(engs, states, p, sos_idx)),
            step=lambda cons: _search.ensemble_step(engs, states, avg, eos_idx, sample_seed=seed, constraints=cons,
                                                    sample_filter=flt))

    def beam_search(self, *a, **k):
        """ensemble_beam_search, with its arguments, under the name the mode dispatch (search.dispatch) calls; the
        single-model beam_search this overrides could not run on a list of encoder memories."""
        return self.ensemble_beam_search(*a, **k)
