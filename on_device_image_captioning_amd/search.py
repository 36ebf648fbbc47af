"""The host side of a search, once, for beam_search, diverse_beam_search, ensemble_beam_search and the ensemble step of
CaptionPipeline: argument rules, mode dispatch, the members of an ensemble on one beam state, and
run_search — arm, constraints, the step loop with its look at the device's `done` flag, ranking, row pick, read-out — which
every search method calls with its own way to arm, its step and its rows.  Plain functions over a DecodeState (engine.py);
the device side of a step is ops.beam_step / ops.group_beam_step / ops.require_beam_step / ops.stochastic_beam_step /
ops.pool_beam_step, five rules on one extraction (wave_extract_best, csrc/beam_step.h); contrastive_beam_search changes what
ops.beam_step is fed, not the step (ops.contrast_topk).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

from . import ops

_DONE_POLL = 4      # host looks at the device `done` flag every this many steps


def _constraint_kwargs(args) -> dict:
    """The constraint keywords present in a forward(**kwargs) / beam_search_args mapping (absent = the default)."""
    return {k: args[k] for k in ("no_repeat_ngram_size", "min_length", "banned_words") if k in args}


def check_constraints(n: int, m: int, banned, *, V, max_seq_len: int, rows_per_image: int, sos_idx, eos_idx,
                      sampling: bool = False) -> Optional[dict]:
    """The rules of a constrained search (no-repeat n-gram size `n`, `m` words at least, the `banned` word ids) for a
    vocabulary of V words (an int, or a callable that is asked only when the rule is reached), captions of max_seq_len
    positions and rows_per_image candidates per row.  None when no constraint is active, else the keywords of
    CaptionerEngine.search_constraints; ValueError for what cannot work."""
    banned = [] if banned is None else sorted({int(w) for w in banned})
    n, m = int(n), int(m)
    if n < 0 or m < 0:
        raise ValueError("no_repeat_ngram_size and min_length must be >= 0")
    if n == 0 and m == 0 and not banned:
        return None
    if sampling:
        raise ValueError("no_repeat_ngram_size / min_length / banned_words apply to the deterministic searches only: "
                         "drawing under constraints (sample_or_max='sample', mode='sampling') is not supported")
    T = max(1, max_seq_len - 1) + 1
    if m > max_seq_len - 2:
        raise ValueError(f"min_length {m} > max_seq_len - 2 = {max_seq_len - 2}: no caption could end")
    if sos_idx in banned or eos_idx in banned:
        raise ValueError("the SOS and EOS ids cannot be banned (min_length is the control over where a caption ends)")
    V = V() if callable(V) else V
    if len(banned) + T + rows_per_image > V:
        raise ValueError(f"{len(banned)} banned words + {T} positions + {rows_per_image} candidates per row exceed the "
                         f"vocabulary ({V} words): a row could run out of admissible words")
    if len(banned) > 1024:
        raise ValueError("at most 1024 banned words")
    return dict(no_repeat_ngram=n, min_words=m, banned=banned)


def per_image_word_lists(value, n_img: int, noun: str) -> Optional[List[List[int]]]:
    """"One word list for all images, or one per image", read once for `prefix` and `required_words`.  `value`: None, a
    1-D or 2-D tensor, a flat sequence of word ids (one list for all images), or a sequence whose elements are all lists,
    tuples or tensors (one per image; `noun` names them in the count error).  → None for None, else n_img lists of ints."""
    if value is None:
        return None
    value = list(value.tolist() if isinstance(value, torch.Tensor) else value)
    if not value or not all(isinstance(r, (list, tuple, torch.Tensor)) for r in value):
        return [[int(w) for w in value] for _ in range(n_img)]
    rows = [[int(w) for w in (r.tolist() if isinstance(r, torch.Tensor) else r)] for r in value]
    if len(rows) != n_img:
        raise ValueError(f"{len(rows)} {noun} for {n_img} images: give one for all, or one per image")
    return rows


def names_a_word(value) -> bool:
    """Does a `prefix` / `required_words` value the caller will refuse hold any word (per_image_word_lists' forms, read
    without the image count)."""
    if isinstance(value, torch.Tensor):
        value = value.tolist()
    return value is not None and any(len(p) if isinstance(p, (list, tuple, torch.Tensor)) else 1 for p in value)


def check_prefix(prefix, n_img: int, *, V, max_seq_len: int, sos_idx, eos_idx, sampling: bool = False
                 ) -> Optional[List[List[int]]]:
    """The rules of a search that starts behind given words.  `prefix`: one sequence of word ids used
    for every image, or one sequence per image, all of the same length.  None for no prefix (None, or nothing but empty
    sequences: the search then launches exactly what it launches without the keyword), else the n_img id lists;
    ValueError, before any device work, for what cannot work."""
    rows = per_image_word_lists(prefix, n_img, "prefixes") or []
    P = len(rows[0]) if rows else 0
    if any(len(r) != P for r in rows):
        raise ValueError("the prefixes of a batch must have one length (the position is one device scalar)")
    if P == 0:
        return None
    if sampling:
        raise ValueError("prefix applies to the deterministic searches only: drawing behind a prefix "
                         "(sample_or_max='sample', mode='sampling') is not supported")
    if P > max_seq_len - 2:
        raise ValueError(f"a prefix of {P} words > max_seq_len - 2 = {max_seq_len - 2}: the caption could not go on and end")
    V = V() if callable(V) else V
    for r in rows:
        for w in r:
            if not 0 <= w < V:
                raise ValueError(f"prefix word id {w} lies outside the vocabulary [0, {V})")
            if w == sos_idx or w == eos_idx:
                raise ValueError("the SOS and EOS ids cannot be part of a prefix")
    return rows


def _filter_kwargs(args) -> dict:
    """The sampling-control keywords present in a forward(**kwargs) / beam_search_args mapping (absent = the default)."""
    return {k: args[k] for k in ("temperature", "top_k", "top_p") if k in args}


def check_sampling_filter(temperature=1.0, top_k=0, top_p=1.0, *, sampling: bool = True, where: str = "sample_or_max='max'"):
    """The rules of the sampling controls: the draws come from softmax(logits / temperature) cut to its
    `top_k` best words (0 = all) and to the nucleus of mass `top_p` (1 = all).  None when all three are at their defaults
    (the search then launches exactly what it launches without them: odic_logsoftmax_sample), else the odic_sample_filter of
    odic_logsoftmax_sample_filtered; ValueError for what cannot work.  `sampling`: whether the search draws at all; one
    that does not (`where` names it) takes the defaults only."""
    t, p = float(temperature), float(top_p)
    if isinstance(top_k, bool) or int(top_k) != top_k:
        raise ValueError(f"top_k must be an integer, not {top_k!r}")
    k = int(top_k)
    if not (0.0 < t < float("inf")):
        raise ValueError(f"temperature must be finite and > 0, not {temperature!r}")
    if k < 0:
        raise ValueError(f"top_k must be >= 0 (0 = off), not {top_k!r}")
    if not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must lie in (0, 1] (1 = off), not {top_p!r}")
    flt = ops.sample_filter(t, k, p)
    if t == 1.0 and k == 0 and p == 1.0:
        return None
    if not (0.0 < flt.inv_temperature < float("inf")):
        raise ValueError(f"temperature {temperature!r}: its reciprocal is not a positive finite fp32 number")
    if not (0.0 < flt.top_p <= 1.0):
        raise ValueError(f"top_p {top_p!r} is not a positive fp32 number")
    if not sampling:
        raise ValueError(f"temperature / top_k / top_p shape the draws of the sampling searches (sample_or_max='sample', "
                         f"mode='sampling'): {where} draws nothing")
    return flt


def draw_candidates(logits, cand_val, cand_idx, N: int, V: int, k: int, seed: int, pos, flt=None) -> None:
    """k draws without replacement per logits row into cand_val / cand_idx: odic_logsoftmax_sample, or under `flt`
    (check_sampling_filter's) odic_logsoftmax_sample_filtered."""
    if flt is None:
        ops.logsoftmax_sample(logits, V, None, 0, cand_val, cand_idx, N, V, k, seed, pos)
    else:
        ops.logsoftmax_sample_filtered(logits, V, None, 0, cand_val, cand_idx, None, N, V, k, flt, seed, pos)


MAX_REQUIRED = 4    # required words per image (odic_require_beam_step: 2^C banks of beams, 16 rows per image at most)


def check_required_words(required, n_img: int, *, V, beam_size: int, banned, sos_idx, eos_idx, max_seq_len: int,
                         sampling: bool = False) -> Optional[List[List[int]]]:
    """The rules of a search whose captions must contain given words.  `required`: one sequence of word
    ids for all images, or one sequence per image (ragged lists allowed).  None for nothing required (None, or nothing
    but empty sequences: the search then launches exactly what it launches without the keyword), else n_img lists of C ids,
    C the longest list, the shorter ones padded with -1; ValueError, before any device work, for what cannot work.
    `beam_size` is the beams per bank: an image searches 2^C·beam_size rows."""
    rows = per_image_word_lists(required, n_img, "lists of required words") or []
    C = max((len(r) for r in rows), default=0)
    if C == 0:
        return None
    if sampling:
        raise ValueError("required_words applies to the deterministic beam search only: drawing under it "
                         "(sample_or_max='sample', mode='sampling') is not supported")
    if C > MAX_REQUIRED:
        raise ValueError(f"{C} required words for one image: at most {MAX_REQUIRED}")
    if (1 << C) * beam_size > 16:
        raise ValueError(f"{C} required words take 2^{C} banks of beam_size = {beam_size} beams, more than 16 rows per "
                         f"image: beam_size may be {16 >> C} at most")
    if C == 1 and beam_size == 1:
        raise ValueError("one required word needs beam_size >= 2: a row must keep a candidate besides that word and EOS")
    if C > max_seq_len - 2:
        raise ValueError(f"{C} required words > max_seq_len - 2 = {max_seq_len - 2}: no caption could hold them and end")
    V = V() if callable(V) else V
    banned = set() if banned is None else {int(w) for w in banned}
    for r in rows:
        if len(set(r)) != len(r):
            raise ValueError(f"required words {r}: an image's words must be distinct")
        for w in r:
            if not 0 <= w < V:
                raise ValueError(f"required word id {w} lies outside the vocabulary [0, {V})")
            if w == sos_idx or w == eos_idx:
                raise ValueError("the SOS and EOS ids cannot be required words")
            if w in banned:
                raise ValueError(f"word id {w} is both required and banned")
    return [r + [-1] * (C - len(r)) for r in rows]


def refuse_required_words(required, where: str) -> None:
    """For the searches that do not take required words: ValueError unless `required` is None or holds no word.
    (Not names_a_word: this reader unpacks every element before it looks, that one stops at the first word, so where a
    0-d tensor stands for a list of ids the two raise differently — [5, tensor(6)]: TypeError here, a word there.)"""
    if required is None:
        return
    if isinstance(required, torch.Tensor):
        required = required.tolist()
    flat = [w for r in required for w in (r if isinstance(r, (list, tuple)) else r.tolist() if isinstance(r, torch.Tensor)
                                          else [r])]
    if flat:
        raise ValueError(f"required_words is not supported {where}: use beam_search on one model, without a prefix")


MAX_STOCHASTIC_SAMPLES = 15     # stochastic_beam_search runs num_samples + 1 rows per image, 16 at most


def check_stochastic_beam(num_samples, *, prefix=None, required_words=None, no_repeat_ngram_size=0, min_length=0,
                          banned_words=None, temperature=1.0, top_k=0, top_p=1.0) -> int:
    """The rules of stochastic_beam_search → num_samples as an int.  Everything that would change the
    distribution the captions are sampled from is refused, in the wording of refuse_required_words: the samples, their
    perturbed scores and the inclusion probabilities derived from them are those of the model itself."""
    where = "in stochastic_beam_search"
    if isinstance(num_samples, bool) or int(num_samples) != num_samples or not 1 <= int(num_samples) <= MAX_STOCHASTIC_SAMPLES:
        raise ValueError(f"num_samples must be an integer in [1, {MAX_STOCHASTIC_SAMPLES}] (the search runs num_samples + 1 "
                         f"rows per image, 16 at most), not {num_samples!r}")
    refuse_required_words(required_words, where)
    tail = "it samples captions from the model's own distribution"
    if names_a_word(prefix):
        raise ValueError(f"prefix is not supported {where}: {tail}")
    if int(no_repeat_ngram_size) != 0:
        raise ValueError(f"no_repeat_ngram_size is not supported {where}: {tail}")
    if int(min_length) != 0:
        raise ValueError(f"min_length is not supported {where}: {tail}")
    if banned_words is not None and len(list(banned_words)):
        raise ValueError(f"banned_words is not supported {where}: {tail}")
    if float(temperature) != 1.0 or top_k != 0 or float(top_p) != 1.0:
        raise ValueError(f"temperature / top_k / top_p are not supported {where}: {tail}")
    return int(num_samples)


MAX_POOL_BEAMS = 15             # odic_pool_beam_step ranks beam_size·(beam_size + 1) candidates, 256 at most


def check_pool_beam(beam_size, how_many_outputs, length_penalty, *, prefix=None, required_words=None, sample_or_max="max",
                    ensemble: bool = False) -> float:
    """The rules of pool_beam_search → length_penalty as a float.  What the pooled rule has no form for is
    refused, in the wording of check_stochastic_beam."""
    where = "in pool_beam_search"
    tail = "it keeps one pool of finished captions per image beside one deterministic beam of one model"
    if ensemble:
        raise ValueError(f"an ensemble is not supported {where}: {tail}")
    if isinstance(beam_size, bool) or int(beam_size) != beam_size or not 1 <= int(beam_size) <= MAX_POOL_BEAMS:
        raise ValueError(f"beam_size must be an integer in [1, {MAX_POOL_BEAMS}] (the step ranks beam_size·(beam_size + 1) "
                         f"candidates, 256 at most), not {beam_size!r}")
    if isinstance(how_many_outputs, bool) or int(how_many_outputs) != how_many_outputs or \
            not 1 <= int(how_many_outputs) <= int(beam_size):
        raise ValueError(f"how_many_outputs must be an integer in [1, beam_size] (the pool holds beam_size captions), not "
                         f"{how_many_outputs!r}")
    refuse_required_words(required_words, where)
    if names_a_word(prefix):
        raise ValueError(f"prefix is not supported {where}: {tail}")
    if sample_or_max != "max":
        raise ValueError(f"sample_or_max={sample_or_max!r} is not supported {where}: {tail}")
    a = float(length_penalty)
    if not (0.0 <= a < float("inf")):
        raise ValueError(f"length_penalty must be finite and >= 0 (0 = rank by the sum of log-probs), not {length_penalty!r}")
    return a


MAX_DISTRACTORS = 7             # odic_contrast_topk takes the target's row and seven more


def check_contrast(distractors, n_img: int, *, contrast=0.5, plausibility=0.1, suppressor_floor=-20.0, prefix=None,
                   required_words=None, sample_or_max="max") -> dict:
    """The rules of contrastive_beam_search.  `distractors`: one sequence per image of 0..7 distinct
    indices into the same batch, never the image itself (ragged lists allowed), or 'others' for every other image
    (n_img - 1 <= 7), or None for none.  → dict(lists: n_img lists of ints, D: the longest list, contrast, plausibility,
    suppressor_floor as floats); ValueError, before any device work, for what cannot work.  prefix, required_words and
    sample_or_max='sample' are refused, in the wording of check_stochastic_beam."""
    where = "in contrastive_beam_search"
    refuse_required_words(required_words, where)
    tail = "it ranks the words of one deterministic beam search by a contrast between images"
    if names_a_word(prefix):
        raise ValueError(f"prefix is not supported {where}: {tail}")
    if sample_or_max != "max":
        raise ValueError(f"sample_or_max={sample_or_max!r} is not supported {where}: {tail}")
    w, a, fl = float(contrast), float(plausibility), float(suppressor_floor)
    if not (0.0 <= w <= 3.0e38):
        raise ValueError(f"contrast must be finite and >= 0 (0 = off), not {contrast!r}")
    if not (0.0 <= a <= 1.0):
        raise ValueError(f"plausibility must lie in [0, 1] (0 = off), not {plausibility!r}")
    if not (-3.0e38 <= fl <= 0.0):
        raise ValueError(f"suppressor_floor must be finite and <= 0, not {suppressor_floor!r}")
    if distractors is None:
        lists = [[] for _ in range(n_img)]
    elif isinstance(distractors, str):
        if distractors != "others":
            raise ValueError(f"distractors must be 'others' or one sequence of image indices per image, not {distractors!r}")
        if n_img - 1 > MAX_DISTRACTORS:
            raise ValueError(f"distractors='others' with {n_img} images: an image takes at most {MAX_DISTRACTORS} distractors")
        lists = [[j for j in range(n_img) if j != i] for i in range(n_img)]
    else:
        if isinstance(distractors, torch.Tensor):
            distractors = distractors.tolist()
        lists = []
        for r in distractors:
            r = r.tolist() if isinstance(r, torch.Tensor) else r
            if not isinstance(r, (list, tuple)):
                raise ValueError("distractors must hold one sequence of image indices per image")
            if any(isinstance(j, bool) or int(j) != j for j in r):
                raise ValueError(f"distractors {list(r)}: the indices must be integers")
            lists.append([int(j) for j in r])
        if len(lists) != n_img:
            raise ValueError(f"{len(lists)} lists of distractors for {n_img} images: give one per image")
    for i, r in enumerate(lists):
        if len(r) > MAX_DISTRACTORS:
            raise ValueError(f"{len(r)} distractors for image {i}: at most {MAX_DISTRACTORS}")
        if len(set(r)) != len(r):
            raise ValueError(f"distractors {r} of image {i}: an image's distractors must be distinct")
        for j in r:
            if not 0 <= j < n_img:
                raise ValueError(f"distractor index {j} of image {i} lies outside the batch [0, {n_img})")
            if j == i:
                raise ValueError(f"image {i} cannot be its own distractor")
    return dict(lists=lists, D=max((len(r) for r in lists), default=0), contrast=w, plausibility=a, suppressor_floor=fl)


def required_outputs(order, cumul, required: List[List[int]], bank_beams: int, how_many_outputs: int):
    """The rows a required-words search returns.  order: odic_beam_finalize's [B, R] (host integers), cumul [B, R] (host
    floats), required: check_required_words' lists.  Output j of an image is the j-th live row (cumul > -inf) of its
    accepting bank in finalize order; an image whose accepting bank holds no live row falls back to the finalize order
    over all its live rows.  Fewer live rows than outputs: the remaining outputs go on with the image's other live rows,
    then repeat the last.  → (rows [B, how_many_outputs] int64, satisfied: a bool per image)."""
    rows, satisfied = [], []
    for b, req in enumerate(required):
        accept = sum(1 << c for c, w in enumerate(req) if w >= 0)
        live = []
        for i in (int(v) for v in order[b]):
            if i not in live and float(cumul[b][i]) > float("-inf"):
                live.append(i)
        inside = [i for i in live if i // bank_beams == accept]
        satisfied.append(bool(inside))
        pick = (inside + [i for i in live if i not in inside]) if inside else live
        pick = (pick or [0])[:how_many_outputs]
        rows.append(pick + [pick[-1]] * (how_many_outputs - len(pick)))
    return torch.tensor(rows, dtype=torch.int64), satisfied


def dispatch(model, mode: str, args, enc_x, enc_x_num_pads):
    """mode='beam_search' | 'sampling' | 'diverse_beam_search' | 'stochastic_beam_search' | 'contrastive_beam_search' |
    'pool_beam_search' with the keys of `args` (a forward(**kwargs) or
    beam_search_args mapping; an absent key takes the reference's default) → the call of the model's method."""
    ends = dict(sos_idx=args.get("sos_idx", -999), eos_idx=args.get("eos_idx", -999))
    cons, flt = _constraint_kwargs(args), _filter_kwargs(args)
    pre = {k: args[k] for k in ("prefix", "required_words") if k in args}       # (absent = the default, as the constraints)
    if mode == "sampling":
        ends["max_seq_len"] = args.get("sample_max_seq_len", 20)
        model._search_constraint_args(**cons, **ends, rows_per_image=1, sampling=True)
        if pre.get("prefix") is not None:
            model._search_prefix_arg(pre["prefix"], enc_x, **ends, sampling=True)
        if pre.get("required_words") is not None:
            model._search_required_arg(pre["required_words"], enc_x, beam_size=1, banned_words=None, **ends, sampling=True)
        return model.get_batch_multiple_sampled_prediction(enc_x, enc_x_num_pads, num_outputs=args.get("how_many_outputs", 1),
                                                           **ends, **flt)
    # the deterministic searches: the ends and the length, the prefix / required words and the constraints go to all four
    common = dict(ends, max_seq_len=args.get("beam_max_seq_len", 20), **pre, **cons)
    beam = dict(beam_size=args.get("beam_size", 5), how_many_outputs=args.get("how_many_outputs", 1),
                sample_or_max=args.get("sample_or_max", "max"))
    if mode == "beam_search":
        return model.beam_search(enc_x, enc_x_num_pads, **beam, **common, **flt)
    if mode == "diverse_beam_search":
        check_sampling_filter(**flt, sampling=False, where="diverse_beam_search")
        return model.diverse_beam_search(enc_x, enc_x_num_pads, num_groups=args.get("num_groups", 3),
                                         group_size=args.get("group_size", 3),
                                         diversity_penalty=args.get("diversity_penalty", 0.5),
                                         how_many_outputs=args.get("how_many_outputs", None), **common)
    if mode == "stochastic_beam_search":
        return model.stochastic_beam_search(enc_x, enc_x_num_pads, num_samples=args.get("num_samples", 5),
                                            seed=args.get("seed", None), **common, **flt)
    if mode == "contrastive_beam_search":
        check_sampling_filter(**flt, sampling=False, where="contrastive_beam_search")
        knobs = {k: args[k] for k in ("contrast", "plausibility", "suppressor_floor") if k in args}
        return model.contrastive_beam_search(enc_x, enc_x_num_pads, distractors=args.get("distractors", "others"), **beam,
                                             **knobs, **common)
    if mode == "pool_beam_search":
        check_sampling_filter(**flt, sampling=False, where="pool_beam_search")
        knobs = {k: args[k] for k in ("length_penalty", "early_stopping") if k in args}
        return model.pool_beam_search(enc_x, enc_x_num_pads, **beam, **knobs, **common)
    raise ValueError(f"unknown mode {mode!r}")


def run_steps(lead_state, steps: int, step_fn: Callable[[int], None]) -> None:
    """Enqueue step_fn(0) .. step_fn(steps - 1); the host looks at the device's `done` flag after every _DONE_POLL-th
    step (never after the last) and stops there once it is set.  All beams finished is a fixed point of the step, so the
    steps run between two looks cannot change the result."""
    for t in range(steps):
        step_fn(t)
        if t >= 1 and (t + 1) % _DONE_POLL == 0 and t + 1 < steps and int(lead_state.done.item()):
            return


def rank_beams(st) -> Tuple[torch.Tensor, torch.Tensor]:
    """odic_beam_finalize: (order int32 [B, k] — the rows of every image, best first; score fp32 [B, k] by row)."""
    order = torch.empty(st.n_img, st.beams, dtype=torch.int32, device=st.tokens.device)
    score = torch.empty_like(order, dtype=torch.float32)
    ops.beam_finalize(st.beam_state, order, score, st.n_img, st.beams)
    return order, score


def read_captions(state, rows: torch.Tensor, how_many_outputs: int) -> Tuple[List[List[List[int]]], torch.Tensor]:
    """Rows `rows[b, j]` (host integers [B, how_many_outputs], row within image b) of the beam state → the token lists
    per image and output, cut at the row's length, and their log-probs [B, how_many_outputs, longest chosen row],
    zero-padded, on the state's device."""
    B = state.n_img
    n_elem_h = state.n_elem.view(B, state.beams).cpu()
    tokens_h = state.tokens.cpu()
    res_tok, lp_rows = [], []
    for b in range(B):
        per = []
        for j in range(how_many_outputs):
            i = int(rows[b, j])
            n = int(n_elem_h[b, i])
            per.append(tokens_h[b, i, :n].tolist())
            lp_rows.append(state.logprobs[b, i, :n])
        res_tok.append(per)
    return res_tok, torch.nn.utils.rnn.pad_sequence(lp_rows, batch_first=True).view(B, how_many_outputs, -1)


def read_pool(st, pool, how_many_outputs: int, sos_idx: int, eos_idx: int):
    """odic_pool_beam_finalize on the pool of the search on `st`, then its best hypotheses → (token lists per image and
    output, log-probs [B, how_many_outputs, longest] zero-padded on the state's device, scores fp32 [B, how_many_outputs],
    counts int32 [B] — both on the host).  Output j of an image is the j-th best hypothesis of its pool; an image with
    fewer than how_many_outputs hypotheses (every candidate died) fills the rest with the EMPTY caption [sos, eos], log-probs
    [0, -inf], score -inf."""
    B, P, dv = st.n_img, st.beams, st.tokens.device
    order = torch.empty(B, P, dtype=torch.int32, device=dv)
    score = torch.empty(B, P, dtype=torch.float32, device=dv)
    ops.pool_beam_finalize(pool.args, st.beam_state, order, score, B, P, st.T)
    order_h, len_h, tok_h = order.cpu(), pool.len.cpu(), pool.tokens.cpu()
    empty_lp = torch.tensor([0.0, float("-inf")], dtype=torch.float32, device=dv)
    res_tok, lp_rows = [], []
    for b in range(B):
        per = []
        for j in range(how_many_outputs):
            i = int(order_h[b, j])
            if i < 0:
                per.append([int(sos_idx), int(eos_idx)])
                lp_rows.append(empty_lp)
                continue
            n = int(len_h[b, i])
            per.append(tok_h[b, i, :n].tolist())
            lp_rows.append(pool.logprobs[b, i, :n])
        res_tok.append(per)
    lp = torch.nn.utils.rnn.pad_sequence(lp_rows, batch_first=True).view(B, how_many_outputs, -1)
    return res_tok, lp, score[:, :how_many_outputs].cpu(), pool.count.cpu()


def arm_state(eng, st, sos_idx: int, prefix: Optional[List[List[int]]] = None, *, emb, group_beams: Optional[int] = None,
              seed_prefix: Optional[Callable[[torch.Tensor], None]] = None) -> None:
    """Bring the built (lead) state to its first position, the arm() of every search.  Behind `prefix` (check_prefix's
    lists): eng.seed_prefix on `st`, the rows in groups of `group_beams` — or seed_prefix(prefix tensor), the ensemble's
    way (ensemble_seed_prefix).  Without one: odic_beam_reset, which with `emb` (st.emb) also embeds the start token as
    the input of position 0; None where the step embeds for itself (step_logits: the draws, the contrast, the ensemble)."""
    if prefix:
        p = prefix_tensor(prefix, eng.device)
        seed_prefix(p) if seed_prefix else eng.seed_prefix(st, p, sos_idx, group_beams=group_beams)
    else:
        ops.beam_reset(st.beam_state, st.n_img, st.beams, st.T, sos_idx, emb=emb)


def logged(step: Callable[[object], None], st, log: Optional[list], extra: Optional[Callable[[], torch.Tensor]] = None):
    """The test hook of the deterministic searches, once: `step` itself when `log` (a model's _cand_log) is None, else
    step followed by log.append((cand_val, cand_idx[, extra()])) — host copies of what the step chose from, for replay in
    the tests' models."""
    if log is None:
        return step

    def logged_step(cons):
        step(cons)
        log.append((st.cand_val.cpu().clone(), st.cand_idx.cpu().clone()) + ((extra(),) if extra else ()))
    return logged_step


def run_search(eng, st, eos_idx: int, steps: int, how_many_outputs: int, *, arm: Callable[[], None],
               step: Callable[[object], None], pick: Optional[Callable] = None, constraints: Optional[dict] = None,
               finish: Optional[Callable[[], tuple]] = None):
    """A whole search on the built (lead) state `st`, once for every search: arm() brings the state to its first position
    (beam_reset, seed_prefix, ensemble_seed_prefix); `constraints` (check_constraints' keywords, or None) become the
    device's on `eng`; step(cons) enqueues one step under them and feeds the caller's log hook, `steps` times at most
    (run_steps); pick(order, score) takes rank_beams' device tensors to the output rows [B, how_many_outputs] (host
    integers; default: the first of the finalize order).  → read_captions: the log-probs are on the state's device.
    `finish` (the pooled search, whose captions do not lie in the beam state): called in place of the ranking and the
    read-out, → what run_search returns."""
    arm()
    cons = eng.search_constraints(st, eos_idx, **constraints) if constraints else None
    run_steps(st, steps, lambda t: step(cons))
    if finish is not None:
        return finish()
    order, score = rank_beams(st)
    return read_captions(st, pick(order, score) if pick else order.cpu()[:, :how_many_outputs], how_many_outputs)


def share_beam_state(states):
    """One beam state for all members of an ensemble: every state reads the lead's (states[0]) ancestor table, finished
    flags, next words and position; only caches and logits stay private.  → the lead state."""
    lead = states[0]
    for st in states[1:]:
        st.anc, st.row_valid, st.next_tok, st.pos = lead.anc, lead.row_valid, lead.next_tok, lead.pos
    return lead


def prefix_tensor(prefix: List[List[int]], device) -> torch.Tensor:
    """check_prefix's id lists → int64 [n_img, P] on the device."""
    return torch.tensor(prefix, dtype=torch.int64, device=device)


def ensemble_seed_prefix(engines, states, prefix: torch.Tensor, sos_idx: int) -> None:
    """seed_prefix for an ensemble on share_beam_state(states): every member fills its own caches in a whole-sequence pass
    over the prefix; the prefix words' log-probs are those of the averaged distribution (odic_ensemble_logprobs on the
    members' logits rows, read by odic_token_stats as the ensemble's score_captions reads them); one
    odic_beam_reset_prefix on the shared lead state (the members embed for themselves in step_logits)."""
    lead = states[0]
    n_img, P = prefix.shape
    V = engines[0].g.vocab_size
    dv = prefix.device
    lg = [eng.prefill(st, prefix, sos_idx, want_logits=True).view(-1, V) for eng, st in zip(engines, states)]
    avg = torch.empty(n_img * P, V, dtype=torch.float32, device=dv)
    ops.ensemble_logprobs(lg, avg)
    logp, sum_logp, max_logp = (torch.empty(n_img * P, dtype=torch.float32, device=dv) for _ in range(3))
    argmax = torch.empty(n_img * P, dtype=torch.int32, device=dv)
    status = torch.zeros(1, dtype=torch.int32, device=dv)
    ops.token_stats(avg, V, prefix.contiguous().view(-1), logp, sum_logp, argmax, max_logp, status, n_img * P, V)
    ops.beam_reset_prefix(lead.beam_state, prefix.contiguous(), logp.view(n_img, P), lead.n_img, lead.beams, lead.beams,
                          lead.T, sos_idx, emb=None)


def ensemble_step(engines, states, avg: torch.Tensor, eos_idx: int, *, sample_seed: Optional[int] = None,
                  constraints=None, sample_filter=None) -> None:
    """One search step of an ensemble on share_beam_state(states): a decoder pass per member, avg [N, V] =
    log(mean_m softmax(logits_m)), the lead's k candidates per row from it — its top-k, under `constraints` the
    admissible top-k, with `sample_seed` k draws without replacement (odic_logsoftmax_sample on rows that already are
    log-probabilities: its normalisation is then the identity up to rounding; under `sample_filter`, check_sampling_filter's,
    the filtered draws) — and the beam bookkeeping."""
    lead = states[0]
    for eng, st in zip(engines, states):
        eng.step_logits(st)                                      # private caches, shared next_tok / pos / ancestors
    ops.ensemble_logprobs([st.logits for st in states], avg)
    if sample_seed is not None:
        draw_candidates(avg, lead.cand_val, lead.cand_idx, lead.N, avg.shape[1], lead.beams, sample_seed, lead.pos,
                        sample_filter)
    elif constraints is not None:
        engines[0].constrained_candidates(lead, constraints, logp=avg)
    else:
        ops.topk_rows(avg, lead.cand_val, lead.cand_idx, lead.beams)
    ops.beam_step(lead.cand_val, lead.cand_idx, lead.beam_state, lead.n_img, lead.beams, lead.T, eos_idx)
