"""A float32 numpy model of one step of the required-words beam search, and of the choice of its outputs.

Written from the semantics in include/odic_hip.h (odic_require_beam_step) and DESIGN.md §4.16, not from the kernel:

  * an image has C required word ids (-1 = unused slot, an id >= V counts as -1); its R = 2^C·kb rows are 2^C banks of kb
    rows, bank m (a bit mask over the slots) being rows m·kb .. m·kb+kb-1; the accepting bank is the mask of the used slots;
  * the live rows are those with cumul > -inf; target bank m keeps its kb best of
      stay:  from a live row of bank m — finished: its rank-0 candidate at 0; growing: every candidate whose word is
             neither a required word with its bit clear in m nor EOS outside the accepting bank;
      enter: for slot c set in m (used), from a live growing row of bank m ^ (1 << c): the word required[c] at the value
             of the row's log-prob row;
  * total = cumul + v (one float32 addition); at t = 0 only row 0 offers, total = v;
  * order: total descending, source row ascending, word ascending;
  * a slot without a finite total left is an empty row: parent = itself (row 0 at t = 0), word = EOS, stored -inf;
  * the update is odic_beam_step's (group_beam_model.step's), the stored value the word's own.

Operates on the state arrays of group_beam_model (STATE_KEYS, new_state).  Not a conftest and not a test module: import it
(`import required_words_model as RM`).
"""
from __future__ import annotations

import numpy as np

from group_beam_model import STATE_KEYS, new_state  # noqa: F401  (the same state)

F = np.float32
NEG = F(-np.inf)


def used_slots(req, V: int):
    """The ids of one image as the kernel sees them: -1 for an unused slot or an id outside [0, V)."""
    return [int(w) if 0 <= int(w) < V else -1 for w in req]


def accepting_bank(req) -> int:
    return sum(1 << c for c, w in enumerate(req) if w >= 0)


def select_image(cv, ci, req_lp, req, cumul, has_eos, t: int, kb: int, eos: int):
    """The selection of one image.  cv / ci [R, ncand]: the candidates of its rows (value descending, then word
    ascending); req_lp [R, C]: the log-prob of required word c in row r; req: used_slots(...); cumul / has_eos [R].
    → parent (row within the image), word, lp (the stored value), empty — each [R] — and a dict of the events met."""
    C = len(req)
    R = kb << C
    assert cv.shape[0] == R
    accept = accepting_bank(req)
    parent, word, lp, empty = np.zeros(R, np.int32), np.zeros(R, np.int64), np.zeros(R, F), np.zeros(R, bool)
    ev = dict(required_is_rank0=False, required_outside_candidates=False, eos_rank0_refused=False, tie_across_rows=False,
              tie_within_row=False, entered=False, empty_slot=False, finished_stays=False)

    def live(row):
        return row == 0 if t == 0 else bool(cumul[row] > NEG)

    def fin(row):
        return t > 0 and bool(has_eos[row])

    for m in range(1 << C):
        cands = []                                   # (total, row, word, stored value, entered)
        for row in range(m * kb, m * kb + kb):
            if not live(row):
                continue
            if fin(row):
                cands.append((F(cumul[row]) + F(0.0), row, int(ci[row, 0]), F(0.0), False))
                ev["finished_stays"] = True
                continue
            for c in range(cv.shape[1]):
                w = int(ci[row, c])
                if w == eos and m != accept:
                    ev["eos_rank0_refused"] |= c == 0
                    continue
                if any(w == req[q] and not (m >> q) & 1 for q in range(C)):
                    ev["required_is_rank0"] |= c == 0
                    continue
                v = F(cv[row, c])
                cands.append((v if t == 0 else F(F(cumul[row]) + v), row, w, v, False))
        for q in range(C):
            if not (m >> q) & 1 or req[q] < 0:
                continue
            src = m ^ (1 << q)
            for row in range(src * kb, src * kb + kb):
                if not live(row) or fin(row):
                    continue
                v = F(req_lp[row, q])
                if req[q] not in [int(x) for x in ci[row]]:
                    ev["required_outside_candidates"] = True
                cands.append((v if t == 0 else F(F(cumul[row]) + v), row, req[q], v, True))
        cands = sorted((x for x in cands if x[0] > NEG), key=lambda x: (-float(x[0]), x[1], x[2]))
        for r in range(kb):
            slot = m * kb + r
            if r < len(cands):
                best = cands[r]
                tied = [x for x in cands[r + 1:] if x[0] == best[0]]
                ev["tie_across_rows"] |= any(x[1] != best[1] for x in tied)
                ev["tie_within_row"] |= any(x[1] == best[1] for x in tied)
                ev["entered"] |= best[4]
                parent[slot], word[slot], lp[slot] = best[1], best[2], best[3]
            else:
                parent[slot], word[slot], lp[slot], empty[slot] = (0 if t == 0 else slot), eos, NEG, True
                ev["empty_slot"] = True
    return parent, word, lp, empty, ev


def apply_choice(st: dict, b: int, parent, word, lp, eos: int, emb: dict | None, new: dict) -> bool:
    """odic_beam_step's update of image b for the chosen (parent, word, lp); → does a row of it keep the search alive."""
    n_img, R, T = st["tokens"].shape
    t = int(st["pos"][0])
    alive = False
    with np.errstate(invalid="ignore"):
        for r in range(R):
            par = int(parent[r])
            n = b * R + r
            new["tokens"][b, r, :t + 1] = st["tokens"][b, par, :t + 1]
            new["logprobs"][b, r, :t + 1] = st["logprobs"][b, par, :t + 1]
            new["anc"][n, :t] = st["anc"][b * R + par, :t]
            new["anc"][n, t] = b * R + par
            new["tokens"][b, r, t + 1] = word[r]
            new["logprobs"][b, r, t + 1] = lp[r]
            cs = F(0.0)
            for j in range(t + 1):
                cs = F(cs + st["logprobs"][b, par, j])
            new["cumul"][n] = F(cs + lp[r])
            pe = 0 if t == 0 else int(st["has_eos"][b * R + par])
            ne = 1 if t == 0 else int(st["n_elem"][b * R + par])
            new["n_elem"][n] = ne + (0 if pe else 1)
            new["has_eos"][n] = 1 if (pe or int(word[r]) == eos) else 0
            new["row_valid"][n] = 0 if pe else 1
            new["next_tok"][n] = word[r]
            alive |= not pe
            if emb is not None and t + 2 < T and t + 1 < emb["pos_table"].shape[0]:
                emb["y"][n, :] = F(emb["embed"][int(word[r])] * F(emb["scale"])) + emb["pos_table"][t + 1]
    return alive


def step(st: dict, cand_val, cand_idx, req_logp, required, kb: int, eos: int, V: int, emb: dict | None = None):
    """One step on every image.  st: the arrays of STATE_KEYS; cand_val / cand_idx [n_img·R, ncand]; req_logp [n_img·R, C];
    required [n_img, C] (-1 = unused).  emb: as in group_beam_model.step.  → (new state, per-image event dicts, each with
    parent / word / empty)."""
    n_img, R, T = st["tokens"].shape
    required = np.asarray(required, np.int64).reshape(n_img, -1)
    C = required.shape[1]
    assert R == kb << C
    t = int(st["pos"][0])
    new = {k: v.copy() for k, v in st.items()}
    if t + 1 >= T:
        return new, []
    events, alive_any = [], False
    for b in range(n_img):
        rows = slice(b * R, (b + 1) * R)
        req = used_slots(required[b], V)
        rl = np.asarray(req_logp, F).reshape(n_img * R, C)[rows] if C else np.zeros((R, 0), F)
        parent, word, lp, empty, ev = select_image(np.asarray(cand_val)[rows], np.asarray(cand_idx)[rows], rl, req,
                                                   st["cumul"][rows], st["has_eos"][rows], t, kb, eos)
        alive_any |= apply_choice(st, b, parent, word, lp, eos, emb, new)
        events.append(dict(ev, parent=parent, word=word, empty=empty))
    new["pos"][0] = t + 1
    if not alive_any:
        new["done"][0] = 1
    return new, events


def live_rows(st: dict) -> np.ndarray:
    return st["cumul"] > NEG


def finalize_order(st: dict, b: int):
    """odic_beam_finalize's order over the LIVE rows of image b: score = cumul / n_elem descending, the lower row first."""
    R = st["tokens"].shape[1]
    sc = [(F(st["cumul"][b * R + r]) / F(st["n_elem"][b * R + r]), r) for r in range(R) if st["cumul"][b * R + r] > NEG]
    return [r for _, r in sorted(sc, key=lambda x: (-float(x[0]), x[1]))]


def outputs(st: dict, required, kb: int, how_many: int, V: int):
    """The rows beam_search(required_words=…) returns: per image the first `how_many` live rows of the accepting bank in
    finalize order; none there → the finalize order over all live rows.  Short lists go on with the other live rows, then
    repeat the last.  → (rows [n_img][how_many], satisfied [n_img])."""
    n_img = st["tokens"].shape[0]
    rows, sat = [], []
    for b in range(n_img):
        accept = accepting_bank(used_slots(np.asarray(required).reshape(n_img, -1)[b], V))
        order = finalize_order(st, b)
        inside = [r for r in order if r // kb == accept]
        sat.append(bool(inside))
        pick = (inside + [r for r in order if r not in inside]) if inside else order
        pick = (pick or [0])[:how_many]
        rows.append(pick + [pick[-1]] * (how_many - len(pick)))
    return rows, sat


def caption(st: dict, b: int, r: int):
    """(tokens, log-probs) of row r of image b, cut at its length."""
    R = st["tokens"].shape[1]
    n = int(st["n_elem"][b * R + r])
    return st["tokens"][b, r, :n].tolist(), st["logprobs"][b, r, :n].copy()
