"""BLEU-1..4 and ROUGE-L on the device: the two COCOEvalCap metrics next to CIDEr that need no Java.

The reference scores with pure-Python dictionaries over strings (eval/bleu/bleu_scorer.py, eval/rouge/rouge.py).  Here the
captions are rows of word ids on the device: ops.bleu_stats counts the clipped n-gram matches on the term-frequency rows
ops.cider_vectorize writes, ops.lcs_pairs takes the longest common subsequence of every (candidate, reference) pair; both
give integers.  The scores are the reference's own expressions on those integers, in fp64.

The reference's quirks are kept: an n-gram count is clipped against the MAXIMUM over the references; the brevity penalty
compares with the closest reference length, a tie going to the shorter one; `tiny` = 1e-15 and `small` = 1e-9 smooth every
ratio, so a sentence without a 4-gram still has a (minute) BLEU-4; ROUGE-L takes the maximum precision and the maximum recall
SEPARATELY over the references, β = 1.2.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch

from . import _hip, ops
from .reward import MAX_ID, MAX_LEN, _check_ids, _pack

STAT_WORDS = _hip.BLEU_STAT_WORDS
TINY, SMALL = 1e-15, 1e-9                       # bleu_scorer.compute_score
BETA = 1.2                                      # rouge.Rouge


def _is_tensors(x, n: int) -> bool:
    return isinstance(x, (tuple, list)) and len(x) == n and isinstance(x[0], torch.Tensor)


def _gather(candidates, references, what: str, device=None, check_ids: bool = False, empty_refs: bool = True):
    """Candidates and references in either form → (hyp_tokens int32 [H, T], hyp_len int32 [H], ref_rows = (ref_tokens int32
    [Rr, L], ref_len [Rr], ref_begin [H], ref_end [H]), max_refs or None, ids_checked), the operands of bleu_stats and lcs.
    candidates: list[H] of id lists, or (tokens [H, T], lengths [H]) on the device.  references: list[H][n] of id lists, or
    (ref_tokens, ref_len, ref_begin, ref_end) on the device as reward.cider_d takes them.  Lists are checked on the host —
    lengths, at least one reference per candidate, with check_ids the ids — and uploaded; every ValueError comes before
    the device is touched."""
    hyp, refs, max_refs, ids_checked = candidates, references, None, check_ids
    if _is_tensors(candidates, 2):
        if hyp[0].dim() != 2 or hyp[1].numel() != hyp[0].shape[0]:
            raise ValueError(f"{what}: expected candidate tokens [H, T] and lengths [H]")
        if hyp[0].shape[1] > MAX_LEN:
            raise ValueError(f"{what}: candidates of {hyp[0].shape[1]} words exceed the limit of {MAX_LEN}")
        device = hyp[0].device if device is None else device
        ids_checked = False
    else:
        rows = [[int(t) for t in c] for c in candidates]
        if not rows:
            raise ValueError(f"{what}: no candidates")
        if any(len(r) > MAX_LEN for r in rows):
            raise ValueError(f"{what}: a candidate exceeds the limit of {MAX_LEN} words")
        if check_ids:
            _check_ids(rows, what)
        hyp = tuple(torch.from_numpy(a) for a in _pack(rows))
    H = hyp[0].shape[0]
    if _is_tensors(references, 4):
        if refs[0].dim() != 2 or refs[0].shape[1] > MAX_LEN:
            raise ValueError(f"{what}: expected reference tokens [Rr, L] with L <= {MAX_LEN}")
        device = refs[0].device if device is None else device
        ids_checked = False
    else:
        if len(references) != H or any(len(per) == 0 for per in references):
            raise ValueError(f"{what}: every candidate needs at least one reference")
        rows = [[int(t) for t in r] for per in references for r in per]
        if any(len(r) > MAX_LEN for r in rows):
            raise ValueError(f"{what}: a reference exceeds the limit of {MAX_LEN} words")
        if not empty_refs and any(len(r) == 0 for r in rows):
            raise ValueError(f"{what}: a reference is empty")
        if check_ids:
            _check_ids(rows, what)
        counts = torch.tensor([len(per) for per in references], dtype=torch.int64)
        end = torch.cumsum(counts, 0)
        refs = tuple(torch.from_numpy(a) for a in _pack(rows)) + (end - counts, end)
        max_refs = int(counts.max())
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("caption metrics run on the GPU only and none is available; there is no CPU fallback")
        device = torch.device("cuda")
    return (hyp[0].to(device, torch.int32), hyp[1].reshape(-1).to(device, torch.int32), tuple(t.to(device) for t in refs),
            max_refs, ids_checked)


def _stack(hyp_tokens, hyp_len, ref_rows):
    """Hypotheses and references as ONE block of rows, hypotheses first, as reward.cider_d lays them out: → (tokens int32
    [H + Rr, width], lengths int32 [H + Rr], ref_begin int32 [H], ref_end int32 [H], both counted in the block's rows)."""
    ref_tokens, ref_len, begin, end = ref_rows
    dv = hyp_tokens.device
    ops._need_cuda(hyp_tokens, hyp_len, ref_tokens, ref_len, begin, end)
    H, T = hyp_tokens.shape
    if T > MAX_LEN or ref_tokens.shape[1] > MAX_LEN:
        raise ValueError(f"captions of {max(T, ref_tokens.shape[1])} tokens exceed the limit of {MAX_LEN}")
    Rr, width = ref_tokens.shape[0], max(1, T, ref_tokens.shape[1])
    tokens = torch.zeros(H + Rr, width, dtype=torch.int32, device=dv)
    tokens[:H, :T] = hyp_tokens
    tokens[H:, :ref_tokens.shape[1]] = ref_tokens
    lengths = torch.cat([hyp_len.reshape(-1).to(dv, torch.int32), ref_len.reshape(-1).to(dv, torch.int32)])
    return tokens, lengths, (begin.to(dv, torch.int64) + H).to(torch.int32), (end.to(dv, torch.int64) + H).to(torch.int32)


def _ids_fit_the_key(tokens: torch.Tensor, lengths: torch.Tensor) -> None:
    """One boolean is read back: the words of every row (positions behind its length are not looked at) lie in [0, MAX_ID]."""
    live = torch.arange(tokens.shape[1], device=tokens.device)[None, :] < lengths[:, None]
    if bool((((tokens < 0) | (tokens > MAX_ID)) & live).any()):
        raise ValueError(f"BLEU: word ids must lie in [0, {MAX_ID}] (the n-gram key packs id + 1 into 16 bits)")


def bleu_stats(hyp_tokens: torch.Tensor, hyp_len: torch.Tensor, ref_rows, *, check_ids: bool = True) -> torch.Tensor:
    """The integer BLEU components of H hypotheses, int32 [H, 12] on the device: correct_1..4, guess_1..4, the hypothesis
    length, the closest, the shortest and the summed reference length (include/odic_hip.h, odic_bleu_stats).  One vectorize
    launch over hypotheses and references together, one stats launch.
    hyp_tokens int [H, T] on the device, hyp_len [H]; ref_rows = (ref_tokens int [Rr, L], ref_len [Rr], ref_begin [H],
    ref_end [H]): hypothesis h is scored against the given rows [ref_begin[h], ref_end[h]) — reward.cider_d's form without a
    corpus.  check_ids reads one boolean back and refuses ids outside [0, 65533] with ValueError; without it such ids are
    clamped, as odic_cider_vectorize clamps them."""
    tokens, lengths, begin, end = _stack(hyp_tokens, hyp_len, ref_rows)
    if check_ids:
        _ids_fit_the_key(tokens, lengths)
    H = hyp_tokens.shape[0]
    ws = ops.cider_workspace(tokens.shape[0], tokens.device)
    ops.cider_vectorize(tokens, lengths, ws, default_idf=1.0)
    stats = torch.empty(H, STAT_WORDS, dtype=torch.int32, device=tokens.device)
    ops.bleu_stats(ws, lengths, tokens.shape[1], torch.arange(H, dtype=torch.int32, device=tokens.device), begin, end, stats)
    return stats


def lcs(hyp_tokens: torch.Tensor, hyp_len: torch.Tensor, ref_rows, *, max_refs: int):
    """Longest-common-subsequence lengths of H hypotheses with their references, the operands as in bleu_stats (the ids may
    be any int32).  → (lcs int32 [H, max_refs] with unused slots 0, len_c int32 [H], len_r int32 [H, max_refs] with unused
    slots 0), all on the device; one launch."""
    tokens, lengths, begin, end = _stack(hyp_tokens, hyp_len, ref_rows)
    H, dv = hyp_tokens.shape[0], tokens.device
    out = torch.empty(H, int(max_refs), dtype=torch.int32, device=dv)
    ops.lcs_pairs(tokens, lengths, begin, end, out)
    lengths = lengths.clamp(0, tokens.shape[1])
    row = begin[:, None].to(torch.int64) + torch.arange(int(max_refs), device=dv)[None, :]
    used = (row < end[:, None]) & (row >= 0) & (row < tokens.shape[0])
    len_r = torch.where(used, lengths[row.clamp(0, tokens.shape[0] - 1)], 0)
    return out, lengths[:H], len_r


def sentence_bleu(stats: torch.Tensor) -> torch.Tensor:
    """bleu_scorer.compute_score's per-sentence list from stats [..., 12], in torch fp64 where the stats are: → [..., 4]."""
    s = stats.to(torch.float64)
    out, prod = [], torch.ones_like(s[..., 0])
    for k in range(4):
        prod = prod * ((s[..., k] + TINY) / (s[..., 4 + k] + SMALL))
        out.append(prod ** (1.0 / (k + 1)))
    ratio = (s[..., 8] + TINY) / (s[..., 9] + SMALL)
    penalty = torch.where(ratio < 1, torch.exp(1 - 1 / ratio), torch.ones_like(ratio))
    return torch.stack(out, dim=-1) * penalty[..., None]


def corpus_bleu(totals: Sequence[int]) -> List[float]:
    """bleu_scorer.compute_score's corpus score from the stats summed over the corpus (12 integers), on the host."""
    bleus, bleu = [], 1.0
    for k in range(4):
        bleu *= float(totals[k] + TINY) / (totals[4 + k] + SMALL)
        bleus.append(bleu ** (1.0 / (k + 1)))
    ratio = (totals[8] + TINY) / (totals[9] + SMALL)
    if ratio < 1:
        bleus = [b * math.exp(1 - 1 / ratio) for b in bleus]
    return bleus


def bleu(candidates, references, *, device=None) -> Tuple[List[float], torch.Tensor]:
    """BLEU-1..4 as Bleu(4).compute_score gives them (the "closest" reference length): → (the corpus scores, 4 floats; the
    per-sentence scores fp64 [4, H] on the device).  candidates: list[H] of id lists (the words alone, no SOS or EOS), or
    (tokens [H, T], lengths [H]) on the device; references: list[H][n >= 1] of id lists, or reward.cider_d's (ref_tokens,
    ref_len, ref_begin, ref_end).  The stats are summed over the corpus on the device as int64 and that one row of 12
    integers is read back.  ValueError: an id outside [0, 65533], a caption above 128 words, a candidate without reference."""
    hyp_tokens, hyp_len, ref_rows, _, ids_checked = _gather(candidates, references, "bleu", device, check_ids=True)
    stats = bleu_stats(hyp_tokens, hyp_len, ref_rows, check_ids=not ids_checked)
    totals = stats.to(torch.int64).sum(dim=0).tolist()
    return corpus_bleu(totals), sentence_bleu(stats).t().contiguous()


def rouge_f(lcs_len: torch.Tensor, len_c: torch.Tensor, len_r: torch.Tensor) -> torch.Tensor:
    """rouge.Rouge.calc_score from the integers: lcs_len and len_r [..., M] (an unused slot holds 0 in both), len_c [...].
    precision = lcs / len_c and recall = lcs / len_r, the maximum of each taken separately over the slots;
    F = (1 + β²)·P·R / (R + β²·P), 0 where either maximum is 0 (an empty candidate scores 0).  fp64 where the operands are."""
    l, c, r = lcs_len.to(torch.float64), len_c.to(torch.float64)[..., None], len_r.to(torch.float64)
    zero = torch.zeros_like(l)
    prec = torch.where((c > 0) & (r > 0), l / c, zero).max(dim=-1).values
    rec = torch.where(r > 0, l / r, zero).max(dim=-1).values
    b2 = BETA ** 2
    hit = (prec != 0) & (rec != 0)
    return torch.where(hit, ((1 + b2) * prec * rec) / torch.where(hit, rec + b2 * prec, torch.ones_like(rec)), torch.zeros_like(rec))


def rouge_l(candidates, references, *, device=None) -> Tuple[float, torch.Tensor]:
    """ROUGE-L as Rouge().compute_score gives it: → (the mean, a float; the per-image scores fp64 [H] on the device).
    Operands as in bleu (ids may be any int32); the device form of the references needs every range within `max_refs` =
    the widest range, which is read back.  ValueError: an empty reference (the reference's split(" ") would make it one
    empty word, which has no meaning on ids), a candidate without reference, a caption above 128 words."""
    hyp_tokens, hyp_len, ref_rows, max_refs, _ = _gather(candidates, references, "rouge_l", device, empty_refs=False)
    ops._need_cuda(hyp_tokens, *ref_rows)
    if max_refs is None:
        max_refs = max(1, int((ref_rows[3] - ref_rows[2]).max()))
    lcs_len, len_c, len_r = lcs(hyp_tokens, hyp_len, ref_rows, max_refs=max_refs)
    slot = torch.arange(max_refs, device=lcs_len.device)[None, :]
    n_refs = (ref_rows[3] - ref_rows[2]).to(lcs_len.device)[:, None]
    if bool(((n_refs <= 0) | ((slot < n_refs) & (len_r <= 0))).any()):
        raise ValueError("rouge_l: every candidate needs at least one reference and no reference may be empty")
    score = rouge_f(lcs_len, len_c, len_r)
    return float(score.mean()), score


def pairwise(tokens: torch.Tensor, lengths: torch.Tensor, B: int, N: int, metric: str) -> torch.Tensor:
    """The utility matrix of consensus reranking, fp64 [B, N, N] on the device: entry (b, i, j) is the sentence BLEU-4
    (metric 'bleu4') or the ROUGE-L F ('rouge_l') of candidate i of image b against candidate j as its single reference.
    tokens int32 [B·N, T], lengths int32 [B·N]: the candidates, image after image."""
    dv = tokens.device
    first = (torch.arange(B, device=dv, dtype=torch.int32) * N).repeat_interleave(N)          # [B·N]: the image's first row
    if metric == "bleu4":
        ws = ops.cider_workspace(B * N, dv)
        ops.cider_vectorize(tokens, lengths, ws, default_idf=1.0)
        hyp = torch.arange(B * N, device=dv, dtype=torch.int32).repeat_interleave(N)           # query (b, i, j): row b·N + i
        ref = (first[:, None] + torch.arange(N, device=dv, dtype=torch.int32)[None, :]).reshape(-1)        # … against b·N + j
        stats = torch.empty(B * N * N, STAT_WORDS, dtype=torch.int32, device=dv)
        ops.bleu_stats(ws, lengths, tokens.shape[1], hyp, ref, ref + 1, stats)
        return sentence_bleu(stats)[:, 3].view(B, N, N)
    if metric == "rouge_l":
        out = torch.empty(B * N, N, dtype=torch.int32, device=dv)
        ops.lcs_pairs(tokens, lengths, first, first + N, out)
        lens = lengths.clamp(0, tokens.shape[1]).view(B, N)
        return rouge_f(out.view(B, N, N, 1), lens[:, :, None].expand(B, N, N), lens[:, None, :, None].expand(B, N, N, 1))
    raise ValueError("metric must be 'cider', 'bleu4' or 'rouge_l'")
