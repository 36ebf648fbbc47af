"""CIDEr-D on the device: the self-critical (SCST) reward and consensus reranking.

The reference rewards every sampled caption with `ReinforceCiderReward.compute_reward` (losses/reward.py,
eval/cider/reinforce_cider_scorer.py): CIDEr-D against the image's training references, document frequencies from the whole
training corpus — Python dictionaries over strings.  Here captions stay what the sampler produces, rows of word ids on the
device: one launch turns hypotheses and references into sorted TF-IDF n-gram vectors (ops.cider_vectorize), one takes the
clipped cosine of every (hypothesis, reference) pair (ops.cider_pairs); row means and the loss are plain torch on the
device.  Only the document-frequency table is built on the host, once per corpus.

The reference's quirks are kept (cider.py's docstring lists them): IDF = log(images) − log(max(1, df)), an n-gram the corpus
never saw weighs log(images); the "length" of the Gaussian penalty is the number of bigram tokens; similarity sums
min(hyp, ref)·ref over the hypothesis's n-grams.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip, language_utils, ops

MAX_ID = _hip.CIDER_MAX_ID
MAX_LEN = _hip.CIDER_MAX_LEN


def encode_references(references: Sequence[Sequence[str]], word2idx: Dict[str, int]) -> List[List[List[int]]]:
    """Reference strings (per image, per reference) → word-id lists without SOS and EOS, cleaned as the reference's
    ReinforceCiderReward.__init__ cleans them (lowercase, symbols spaced out, punctuation dropped, split on white space).
    A word outside the vocabulary gets a private id >= len(word2idx), one per distinct word: it stays distinct from every
    other such word, as distinct strings do, and can never equal a word the model emits."""
    private: Dict[str, int] = {}
    base = len(word2idx)
    out = []
    for refs in references:
        ids = []
        for caption in refs:
            s = language_utils.lowercase_and_clean_trailing_spaces([caption])
            s = language_utils.add_space_between_non_alphanumeric_symbols(s)
            s = language_utils.remove_punctuations(s)
            row = []
            for w in s[0].split():
                i = word2idx.get(w)
                if i is None:
                    i = private.setdefault(w, base + len(private))
                row.append(int(i))
            ids.append(row)
        out.append(ids)
    return out


def ngram_keys(ids: Sequence[int]) -> np.ndarray:
    """The uint64 keys of a caption's n-grams of orders 1..4, in no particular order: Σ_j (id_j + 1) << (16·j)."""
    a = np.asarray(ids, dtype=np.uint64) + np.uint64(1)
    L = a.size
    keys = []
    for k in range(1, 5):
        if L >= k:
            v = np.zeros(L - k + 1, dtype=np.uint64)
            for j in range(k):
                v |= a[j:L - k + 1 + j] << np.uint64(16 * j)
            keys.append(v)
    return np.concatenate(keys) if keys else np.zeros(0, dtype=np.uint64)


def _check_ids(rows, what: str) -> None:
    for r in rows:
        if len(r) and (min(r) < 0 or max(r) > MAX_ID):
            raise ValueError(f"{what}: word ids must lie in [0, {MAX_ID}] (the n-gram key packs id + 1 into 16 bits)")


def _pack(rows: Sequence[Sequence[int]], width: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """id lists → (int32 [n, width] zero-padded, int32 [n] lengths) on the host."""
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    width = max(1, int(lens.max()) if len(rows) else 1) if width is None else width
    tok = np.zeros((len(rows), width), dtype=np.int32)
    for i, r in enumerate(rows):
        tok[i, :len(r)] = r
    return tok, lens


class CiderCorpus:
    """The training references of a corpus on the device, with the document-frequency table of their n-grams.

    references: list[n_images][n_refs] of word-id lists WITHOUT SOS and EOS (encode_references); EOS is appended here, as the
    reference appends its eos_token.  The table is built once, on the host: the unique keys of every image over all its
    references, their counts over the images, idf = log(n_images) − log(max(1, df)) in fp64."""

    def __init__(self, references: Sequence[Sequence[Sequence[int]]], eos_idx: int, device):
        self.device = torch.device(device)
        self.eos_idx = int(eos_idx)
        self.n_images = len(references)
        if self.n_images == 0 or any(len(refs) == 0 for refs in references):
            raise ValueError("CiderCorpus needs at least one image and at least one reference per image")
        rows, counts = [], []
        for refs in references:
            counts.append(len(refs))
            for r in refs:
                if len(r) > MAX_LEN - 1:
                    raise ValueError(f"a reference of {len(r)} words exceeds the limit of {MAX_LEN - 1} (EOS is appended)")
                rows.append([int(t) for t in r] + [self.eos_idx])
        _check_ids(rows, "CiderCorpus")
        per_image, at = [], 0
        for c in counts:
            per_image.append(np.unique(np.concatenate([ngram_keys(r) for r in rows[at:at + c]])))
            at += c
        keys, df = np.unique(np.concatenate(per_image), return_counts=True)
        self.log_images = float(np.log(float(self.n_images)))
        idf = self.log_images - np.log(np.maximum(1.0, df.astype(np.float64)))
        tok, lens = _pack(rows)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.max_refs = int(max(counts))
        self.max_len = tok.shape[1]
        self.max_id = int(tok.max())
        self.table_keys_host, self.table_idf_host = keys, idf
        dv = self.device
        self.df_keys = torch.from_numpy(keys.view(np.int64)).to(dv)         # the uint64 bits
        self.df_idf = torch.from_numpy(idf).to(dv)
        self.ref_tokens = torch.from_numpy(tok).to(dv)
        self.ref_len = torch.from_numpy(lens).to(dv)
        self.ref_offsets = torch.from_numpy(offsets).to(dv)                 # int64 [n_images + 1]
        self.ref_counts = torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dv)


def cider_d(hyp_tokens: torch.Tensor, hyp_len: torch.Tensor, *, ref_rows, corpus: Optional[CiderCorpus] = None,
            samples_per_image: int = 1, max_refs: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """CIDEr-D of H hypotheses against their references: one vectorize launch over hypotheses and references together, one
    pairs launch.  → (sim fp64 [H, max_refs], the similarity to every reference with unused slots 0; n_refs int64 [H]).
    A hypothesis's score is sim.sum(1) / n_refs.

    hyp_tokens: int [H, T] on the device, hyp_len [H]; the words scored are hyp_tokens[h, :hyp_len[h]].
    With a corpus: `ref_rows` is the corpus image index of every GROUP of samples_per_image consecutive hypotheses (a device
    tensor, or a list that is uploaded), H = len(ref_rows)·samples_per_image; an image's references are vectorised once
    and shared by its samples, and the IDF comes from the corpus table.
    Without one: `ref_rows` = (ref_tokens int [Rr, L], ref_len [Rr], ref_begin [H], ref_end [H]): hypothesis h is scored
    against the given rows [ref_begin[h], ref_end[h]), max_refs (required) bounds their number, and every n-gram has IDF 1."""
    dv = hyp_tokens.device
    H, T = hyp_tokens.shape
    if T > MAX_LEN:
        raise ValueError(f"captions of {T} tokens exceed the limit of {MAX_LEN}")
    if corpus is not None:
        img = torch.as_tensor(ref_rows, dtype=torch.int64, device=dv).reshape(-1)
        G, M = img.numel(), corpus.max_refs
        if G * samples_per_image != H:
            raise ValueError(f"{H} hypotheses are not {samples_per_image} per image of {G} images")
        # the images' reference blocks, padded to M slots each: a fixed shape, so nothing is read back to size it
        slot = torch.arange(M, device=dv)[None, :]
        count = corpus.ref_counts[img]
        src = (corpus.ref_offsets[img][:, None] + torch.minimum(slot, count[:, None] - 1)).reshape(-1)
        ref_tokens = corpus.ref_tokens[src]
        ref_len = corpus.ref_len[src]
        begin = (H + torch.arange(G, device=dv) * M).repeat_interleave(samples_per_image)
        n_refs = count.repeat_interleave(samples_per_image)
        end = begin + n_refs
        table = dict(df_keys=corpus.df_keys, df_idf=corpus.df_idf, default_idf=corpus.log_images)
    else:
        if max_refs is None:
            raise ValueError("cider_d without a corpus needs max_refs")
        ref_tokens, ref_len, begin, end = ref_rows
        M = int(max_refs)
        begin = begin.to(dv, torch.int64) + H
        end = end.to(dv, torch.int64) + H
        n_refs = (end - begin).clamp(max=M)
        table = dict(default_idf=1.0)
    if ref_tokens.shape[1] > MAX_LEN:
        raise ValueError(f"references of {ref_tokens.shape[1]} tokens exceed the limit of {MAX_LEN}")
    Rr, width = ref_tokens.shape[0], max(T, ref_tokens.shape[1])
    tokens = torch.zeros(H + Rr, width, dtype=torch.int32, device=dv)
    tokens[:H, :T] = hyp_tokens
    tokens[H:, :ref_tokens.shape[1]] = ref_tokens
    lengths = torch.cat([hyp_len.reshape(-1).to(dv, torch.int32), ref_len.reshape(-1).to(dv, torch.int32)])
    ws = ops.cider_workspace(H + Rr, dv)
    ops.cider_vectorize(tokens, lengths, ws, **table)
    sim = torch.empty(H, M, dtype=torch.float64, device=dv)
    ops.cider_pairs(ws, begin.to(torch.int32), end.to(torch.int32), sim)
    return sim, n_refs


def _scored_rows(captions, n_per_image: Optional[int], what: str, device) -> Tuple[torch.Tensor, torch.Tensor, int, int]:
    """The sampler's captions (SOS … EOS) → (int32 [B·S, T − 1] without SOS, int32 [B·S] lengths, B, S).  `captions` is
    list[B][S] of id lists, or (tokens int [B, S, T] on the device, lengths [B, S] counting SOS and EOS)."""
    if isinstance(captions, (tuple, list)) and len(captions) == 2 and isinstance(captions[0], torch.Tensor):
        tok, lens = captions
        if tok.dim() != 3 or tuple(lens.shape) != tuple(tok.shape[:2]):
            raise ValueError(f"{what}: expected tokens [B, S, T] and lengths [B, S]")
        B, S, T = tok.shape
        if n_per_image is not None and S != n_per_image:
            raise ValueError(f"{what}: {S} captions per image, expected {n_per_image}")
        if T - 1 > MAX_LEN:
            raise ValueError(f"{what}: captions of {T - 1} words exceed the limit of {MAX_LEN}")
        return (tok.to(device)[:, :, 1:].reshape(B * S, T - 1).to(torch.int32),
                (lens.to(device).reshape(-1) - 1).clamp(min=0).to(torch.int32), B, S)
    B = len(captions)
    S = len(captions[0]) if n_per_image is None else n_per_image
    if B == 0 or any(len(c) != S for c in captions):
        raise ValueError(f"{what}: every image needs exactly {S} captions")
    rows = [[int(t) for t in cap[1:]] for per in captions for cap in per]
    if any(len(r) > MAX_LEN for r in rows):
        raise ValueError(f"{what}: a caption exceeds the limit of {MAX_LEN} words")
    _check_ids(rows, what)
    tok, lens = _pack(rows)
    return torch.from_numpy(tok).to(device), torch.from_numpy(lens).to(device), B, S


class ReinforceCiderReward:
    """The reference's losses/reward.py on the device.  training_references: list[n_images][n_refs] of word-id lists without
    SOS and EOS (encode_references maps the reference's strings), or a CiderCorpus built from them."""

    def __init__(self, training_references, eos_idx: int, num_sampled_captions: int, rank):
        self.rank = rank
        self.num_sampled_captions = int(num_sampled_captions)
        self.corpus = training_references if isinstance(training_references, CiderCorpus) else \
            CiderCorpus(training_references, eos_idx, rank)

    def _scores(self, captions, image_idx, what: str):
        tok, lens, B, S = _scored_rows(captions, self.num_sampled_captions, what, self.corpus.device)
        sim, n_refs = cider_d(tok, lens, ref_rows=image_idx, corpus=self.corpus, samples_per_image=S)
        return (sim.sum(dim=1) / n_refs).view(B, S)

    def compute_reward(self, pred_captions, logprob: torch.Tensor, image_idx, base_captions=None):
        """→ (reward_loss, reward [B, S] fp64, reward_base [B, S] fp64), all on the device.  pred_captions: what the sampler
        returns, list[B][S] of id lists with SOS and EOS (uploaded), or (tokens [B, S, T], lengths [B, S]) on the device
        (nothing touches the host); the caption scored is caption[1:], SOS dropped and EOS kept.  reward_base is the mean of
        the other samples, (Σ − r) / (S − 1), or the CIDEr-D of `base_captions` (same forms) when given.
        reward_loss = mean((reward − reward_base) · Σ_t −logprob)."""
        reward = self._scores(pred_captions, image_idx, "pred_captions")
        if base_captions is None:
            reward_base = (reward.sum(dim=-1, keepdim=True) - reward) / (reward.shape[1] - 1)
        else:
            reward_base = self._scores(base_captions, image_idx, "base_captions")
        # (the log-probs are summed in fp64; the reference sums them in their own fp32 before the fp64 product)
        loss = ((reward - reward_base) * torch.sum(-logprob.to(reward.device, torch.float64), dim=-1)).mean()
        return loss, reward, reward_base


def consensus_rerank(captions, *, corpus: Optional[CiderCorpus] = None, eos_idx: int, metric: str = "cider"):
    """Minimum-Bayes-risk selection under CIDEr-D: of the N candidates of every image, the one that agrees most with the
    other N − 1.  captions: list[B][N] of id lists as the sampler and the searches return them (SOS first); a candidate is
    scored as caption[1:], with EOS appended where the search was cut before it.  Without a corpus every n-gram has IDF 1 (a
    clipped term-frequency cosine; a corpus of this one image would give every n-gram IDF 0); with one, its table weighs
    them.  → (best_index int64 [B], scores fp64 [B, N]) on the device; ties go to the lower index, N = 1 gives index 0 and
    score 0, duplicate candidates are legal.
    metric 'bleu4' or 'rouge_l' takes the pairwise sentence BLEU-4, or the pairwise ROUGE-L F, of candidate i against
    candidate j as its single reference in place of CIDEr-D (metrics.pairwise); neither has an IDF, so a
    corpus with them is refused."""
    if metric not in ("cider", "bleu4", "rouge_l"):
        raise ValueError("metric must be 'cider', 'bleu4' or 'rouge_l'")
    if metric != "cider" and corpus is not None:
        raise ValueError(f"metric {metric!r} has no IDF: it takes no corpus")
    B = len(captions)
    N = len(captions[0]) if B else 0
    if B == 0 or N == 0 or any(len(c) != N for c in captions):
        raise ValueError("consensus_rerank needs the same number (>= 1) of candidates for every image")
    eos_idx = int(eos_idx)
    full = [[[int(t) for t in c] + ([] if len(c) > 1 and c[-1] == eos_idx else [eos_idx]) for c in per] for per in captions]
    dv = corpus.device if corpus is not None else torch.device("cuda")
    tok, lens, _, _ = _scored_rows(full, N, "captions", dv)
    H = B * N
    if N == 1:
        return torch.zeros(B, dtype=torch.int64, device=dv), torch.zeros(B, 1, dtype=torch.float64, device=dv)
    if metric != "cider":
        from . import metrics
        sim = metrics.pairwise(tok, lens, B, N, metric)
    else:
        ws = ops.cider_workspace(H, dv)
        if corpus is not None:
            ops.cider_vectorize(tok, lens, ws, df_keys=corpus.df_keys, df_idf=corpus.df_idf, default_idf=corpus.log_images)
        else:
            ops.cider_vectorize(tok, lens, ws, default_idf=1.0)
        begin = (torch.arange(B, device=dv, dtype=torch.int32) * N).repeat_interleave(N)
        sim = torch.empty(H, N, dtype=torch.float64, device=dv)
        ops.cider_pairs(ws, begin, begin + N, sim)
        sim = sim.view(B, N, N)
    off_diagonal = ~torch.eye(N, dtype=torch.bool, device=dv)
    # summed in ascending order (the similarities are >= 0, the dropped diagonal sorts first): candidates that are equal
    # get scores equal to the bit wherever they stand, so their tie is a tie
    scores = (sim * off_diagonal).sort(dim=2).values.sum(dim=2) / (N - 1)
    at_best = scores == scores.max(dim=1, keepdim=True).values
    index = torch.where(at_best, torch.arange(N, device=dv)[None, :], N).min(dim=1).values
    return index, scores
