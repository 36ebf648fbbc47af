"""A float32 numpy model of one step of diverse (group) beam search: the group selection and the state update.

Written from the semantics in include/odic_hip.h (odic_group_beam_step) and DESIGN.md §4.13, not from the kernel:

  * rows g·kg .. g·kg+kg-1 of an image are group g; the groups choose in order;
  * count[w] = number of picks of earlier groups AT THIS STEP that appended w to a beam that had not finished before;
  * a growing beam j offers word w at v = logp_j(w) - penalty·count[w], total = cumul_j + v (three float32 operations);
  * a finished beam offers its rank-0 candidate at 0 and every other one at -999, never penalised;
  * a total of -inf is never ranked (a dead beam, cumul = -inf, offers nothing; nor does a candidate of value -inf);
  * a group keeps its kg best: total descending, then beam in group ascending, then word ascending — among the -999
    fillers of one finished beam, rank ascending (the flat index of odic_beam_step);
  * a slot for which no total above -inf is left becomes an EMPTY row: parent = the slot's own row, word = EOS, stored
    value -inf, not growing (it is never counted by a later group);
  * at t = 0 group g draws from its own first row, total = v;
  * what is stored is the candidate's own value; cumul is the float32 sum, in position order, of the parent's per-token
    log-probs plus the new one.

Not a conftest and not a test module: import it (`import group_beam_model as M`).
"""
from __future__ import annotations

import numpy as np

F = np.float32
STATE_KEYS = ("tokens", "logprobs", "anc", "cumul", "n_elem", "has_eos", "row_valid", "next_tok", "pos", "done")


def new_state(n_img: int, R: int, T: int, sos: int, fill: int = 0) -> dict:
    """What odic_beam_reset leaves, the arrays it does not touch holding `fill`."""
    N = n_img * R
    st = dict(tokens=np.full((n_img, R, T), fill, np.int64), logprobs=np.full((n_img, R, T), fill, F),
              anc=np.full((N, T), fill, np.int32), cumul=np.full(N, fill, F), n_elem=np.full(N, fill, np.int32),
              has_eos=np.full(N, fill, np.int32), row_valid=np.ones(N, np.int32), next_tok=np.full(N, sos, np.int64),
              pos=np.zeros(1, np.int32), done=np.zeros(1, np.int32))
    st["tokens"][:, :, 0] = sos
    st["logprobs"][:, :, 0] = 0
    return st


def select_image(cv, ci, cumul, has_eos, t: int, G: int, kg: int, lam: float, eos: int | None = None):
    """The selection of one image.  cv / ci: [R, C] candidates of its R = G·kg rows, every row sorted by value descending,
    then word ascending (C = R for the kernel; any C >= 1 here, the whole vocabulary included).  cumul / has_eos: [R].
    eos: the word of an EMPTY row (needed only where a group runs out of totals above -inf).
    Returns parent (row within the image), word, lp (the stored value), grow — each [R] — and a dict of the events met."""
    R = G * kg
    lam = F(lam)
    parent, word, lp, grow = (np.zeros(R, np.int32), np.zeros(R, np.int64), np.zeros(R, F), np.zeros(R, np.int32))
    count: dict = {}
    ev = dict(same_word_wanted=False, tie_across_beams=False, tie_within_beam_after_penalty=False)
    for g in range(G):
        rows = [g * kg] if t == 0 else list(range(g * kg, g * kg + kg))
        cands = []                    # (total, beam in group, word, stored value, row, count, plain total, tie key)
        for j, row in enumerate(rows):
            fin = t > 0 and bool(has_eos[row])
            for c in range(cv.shape[1]):
                w = int(ci[row, c])
                if fin:
                    v, cnt, stored = F(0.0) if c == 0 else F(-999.0), 0, F(0.0) if c == 0 else F(-999.0)
                else:
                    cnt = count.get(w, 0)
                    pen = F(lam * F(cnt))
                    v, stored = F(F(cv[row, c]) - pen), F(cv[row, c])
                total = v if t == 0 else F(F(cumul[row]) + v)
                plain = stored if t == 0 else F(F(cumul[row]) + stored)
                if total > -np.inf:                                    # (a NaN is not ranked either)
                    cands.append((float(total), j, w, stored, row, cnt, float(plain), c if fin else w))
        by_plain = sorted(cands, key=lambda x: (-x[6], x[1], x[2]))[:kg]
        if any(x[5] > 0 for x in by_plain):
            ev["same_word_wanted"] = True
        left = sorted(cands, key=lambda x: (-x[0], x[1], x[7]))
        for r in range(kg):
            q = g * kg + r
            if not left:
                assert eos is not None, "fewer finite totals than beams: the EMPTY row needs eos"
                parent[q], word[q], lp[q], grow[q] = q, eos, F(-np.inf), 0
                continue
            best = left[0]
            tied = [x for x in left[1:] if x[0] == best[0]]
            if any(x[1] != best[1] for x in tied):
                ev["tie_across_beams"] = True
            if any(x[1] == best[1] and (x[5] > 0 or best[5] > 0) for x in tied):
                ev["tie_within_beam_after_penalty"] = True
            left = left[1:]
            fin = t > 0 and bool(has_eos[best[4]])
            parent[q], word[q], lp[q], grow[q] = best[4], best[2], best[3], 0 if fin else 1
        for q in range(g * kg, g * kg + kg):
            if grow[q]:
                count[int(word[q])] = count.get(int(word[q]), 0) + 1
    return parent, word, lp, grow, ev


def step(st: dict, cand_val, cand_idx, G: int, kg: int, lam: float, eos: int, emb: dict | None = None, select=None):
    """One step on every image.  st: the arrays of STATE_KEYS; cand_val / cand_idx: [n_img·R, C].  emb: None or
    dict(embed [V, d], pos_table [rows, d], scale, y [n_img·R, d]) — y is updated in place as the embedding tail does.
    `select(cv, ci, cumul, has_eos, t) -> (parent, word, lp)`: another selection in place of select_image (G = 1), for
    the state update alone.  Returns (new state, per-image event dicts)."""
    n_img, R, T = st["tokens"].shape
    assert R == G * kg
    t = int(st["pos"][0])
    new = {k: v.copy() for k, v in st.items()}
    if t + 1 >= T:
        return new, []
    events, alive_any = [], False
    for b in range(n_img):
        rows = slice(b * R, (b + 1) * R)
        if select is None:
            parent, word, lp, grow, ev = select_image(np.asarray(cand_val)[rows], np.asarray(cand_idx)[rows],
                                                      st["cumul"][rows], st["has_eos"][rows], t, G, kg, lam, eos)
        else:
            parent, word, lp = select(np.asarray(cand_val)[rows], np.asarray(cand_idx)[rows], st["cumul"][rows],
                                      st["has_eos"][rows], t)
            grow, ev = [0 if t > 0 and st["has_eos"][b * R + int(q)] else 1 for q in parent], {}
        ev = dict(ev, parent=parent, word=word, grow=grow)
        for r in range(R):
            par = int(parent[r])
            n = b * R + r
            assert par // kg == r // kg, "a beam's parent is in its own group"
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
            alive_any |= not pe
            if emb is not None and t + 2 < T and t + 1 < emb["pos_table"].shape[0]:
                emb["y"][n, :] = F(emb["embed"][int(word[r])] * F(emb["scale"])) + emb["pos_table"][t + 1]
        ev["finished_now"] = [r for r in range(R) if new["has_eos"][b * R + r] and grow[r]]
        ev["all_finished"] = bool(new["has_eos"][rows].all())
        events.append(ev)
    new["pos"][0] = t + 1
    if not alive_any:
        new["done"][0] = 1
    return new, events


def single_group_rule(cv, ci, cumul, has_eos, t: int):
    """A direct transcription of the existing step's selection (odic_beam_step; k beams, the k x k table): candidate
    (j, c) is worth cumul_j + (has_eos_j ? (c == 0 ? 0 : -999) : cv[j][c]); k rounds take the largest, the lowest flat
    index j·k + c winning a tie; at t = 0 the k candidates of row 0 in order."""
    k = cv.shape[0]
    if t == 0:
        return np.zeros(k, np.int32), ci[0, :k].astype(np.int64), cv[0, :k].astype(F)
    val = np.empty((k, k), F)
    for j in range(k):
        for c in range(k):
            val[j, c] = (F(0.0) if c == 0 else F(-999.0)) if has_eos[j] else F(cv[j, c])
    tot = (cumul.astype(F)[:, None] + val).astype(F).reshape(-1)
    parent, word, lp = np.zeros(k, np.int32), np.zeros(k, np.int64), np.zeros(k, F)
    for r in range(k):
        i = int(np.argmax(tot))                      # first occurrence of the maximum = lowest flat index
        parent[r], word[r], lp[r] = i // k, ci[i // k, i % k], val.reshape(-1)[i]
        tot[i] = -np.inf
    return parent, word, lp
