"""Float32 numpy models of the beam bookkeeping on DEAD rows, and the inputs that reach them.

Written from include/odic_hip.h (odic_beam_step, odic_group_beam_step, odic_beam_finalize(_best)), not from the kernels:

  * a row with cumul = -inf is dead and offers nothing; a candidate of value -inf is never ranked; a finished row (has_eos)
    offers its rank-0 candidate at 0 and the others at -999; total = cumul + value, one rounded fp32 addition;
  * the k largest totals above -inf are taken, the lowest flat index row·k + rank winning a tie;
  * a slot for which no total above -inf is left becomes an EMPTY row: parent = the slot itself, word = EOS, stored
    log-prob -inf.  The update (group_beam_model.step: cumulative scores re-summed in position order) then leaves it with
    cumul = -inf and has_eos = 1, so it never offers anything again;
  * finalize: score = cumul / n_elem, order = the rows by score descending, a tie (-inf against -inf too) to the lower
    row — always a permutation; finalize_best emits row order[0], cut at its n_elem and padded.

Also here, shared with tests/test_hip_ops.py: the candidate tables and the list-based restatement of the reference's
search loop that test_beam_step_direct_against_the_search_loop compares the device with (SearchLoop).

Not a conftest and not a test module: import it (`import beam_dead_rows_model as D`).
"""
from __future__ import annotations

import functools

import numpy as np

import group_beam_model as M

F = np.float32
NEG = F(-np.inf)

N_IMG, T, DIM, V = 4, 8, 8, 24
SOS, EOS = 3, 2
T0 = 2                       # the position the cases start at (prefix length 3)
N_STEPS = 3
SCALE = 4.0
PENALTY = 0.5
CONTROL = N_IMG - 1          # the all-finite image of every batch
BEAMS = (1, 2, 3, 16)
GROUP_SHAPES = ((1, 3), (2, 2), (4, 4), (3, 1))


# ------------------------------------------------------------------------------------------------- the plain step
def plain_select(cv, ci, cumul, has_eos, t: int, eos: int):
    """The selection of odic_beam_step for one image: cv / ci [k, k], cumul / has_eos [k] → parent, word, lp, each [k]."""
    k = cv.shape[0]
    if t == 0:
        return np.zeros(k, np.int32), ci[0, :k].astype(np.int64), cv[0, :k].astype(F)
    val = np.empty((k, k), F)
    for j in range(k):
        for c in range(k):
            val[j, c] = (F(0.0) if c == 0 else F(-999.0)) if has_eos[j] else F(cv[j, c])
    with np.errstate(invalid="ignore"):
        tot = (np.asarray(cumul, F)[:, None] + val).astype(F).reshape(-1)
    left = [i for i in range(k * k) if tot[i] > NEG]                       # (a NaN is not ranked either)
    left.sort(key=lambda i: (-float(tot[i]), i))
    parent, word, lp = np.zeros(k, np.int32), np.zeros(k, np.int64), np.zeros(k, F)
    for r in range(k):
        if r < len(left):
            i = left[r]
            parent[r], word[r], lp[r] = i // k, ci[i // k, i % k], val.reshape(-1)[i]
        else:
            parent[r], word[r], lp[r] = r, eos, NEG
    return parent, word, lp


def plain_step(st: dict, cand_val, cand_idx, eos: int, emb: dict | None = None):
    """One odic_beam_step on every image (the update half is group_beam_model.step's)."""
    k = st["tokens"].shape[1]
    sel = lambda cv, ci, cumul, has_eos, t: plain_select(cv, ci, cumul, has_eos, t, eos)      # noqa: E731
    with np.errstate(invalid="ignore"):
        return M.step(st, cand_val, cand_idx, 1, k, 0.0, eos, emb=emb, select=sel)


def group_step(st: dict, cand_val, cand_idx, G: int, kg: int, lam: float, eos: int, emb: dict | None = None):
    with np.errstate(invalid="ignore"):
        return M.step(st, cand_val, cand_idx, G, kg, lam, eos, emb=emb)


def empty_rows(st: dict, eos: int) -> np.ndarray:
    """[n_img, R] bool: the rows that are EMPTY after a step (dead, finished, the last word EOS at log-prob -inf)."""
    n_img, R, _ = st["tokens"].shape
    t = int(st["pos"][0])
    return ((st["cumul"].reshape(n_img, R) == NEG) & (st["has_eos"].reshape(n_img, R) == 1) &
            (st["tokens"][:, :, t] == eos) & (st["logprobs"][:, :, t] == NEG))


# ------------------------------------------------------------------------------------------------- finalize
def finalize(cumul, n_elem, n_img: int, k: int):
    """→ (order int32 [n_img, k], score fp32 [n_img, k])."""
    with np.errstate(divide="ignore", invalid="ignore"):
        score = (np.asarray(cumul, F) / np.asarray(n_elem).astype(F)).astype(F).reshape(n_img, k)
    order = np.array([sorted(range(k), key=lambda j: (-float(score[b, j]), j)) for b in range(n_img)], np.int32)
    return order.reshape(n_img, k), score


def finalize_best(tokens, cumul, n_elem, n_img: int, k: int, pad: int):
    """→ (order, score, out_tok int32 [n_img, T], out_len int32 [n_img])."""
    order, score = finalize(cumul, n_elem, n_img, k)
    T_ = tokens.shape[-1]
    tok = np.asarray(tokens).reshape(n_img, k, T_)
    ne = np.asarray(n_elem).reshape(n_img, k)
    out_tok, out_len = np.full((n_img, T_), pad, np.int32), np.zeros(n_img, np.int32)
    for b in range(n_img):
        best = int(order[b, 0])
        n = int(ne[b, best])
        out_tok[b, :n] = tok[b, best, :n]
        out_len[b] = n
    return order, score, out_tok, out_len


#: hand-made (cumul, n_elem) rows for the finalize kernels, one image each; k = len
FINALIZE_ROWS = (
    ("dead_live_dead", [NEG, -2.0, NEG], [3, 4, 3]),
    ("all_dead", [NEG, NEG, NEG, NEG], [2, 3, 4, 5]),
    ("equal_finite", [-3.0, -6.0, -1.5, -4.5], [2, 4, 1, 3]),
    ("tie_next_to_dead", [NEG, -3.0, NEG, -1.5, -8.0, NEG], [3, 4, 3, 2, 4, 5]),
    ("one_dead", [NEG], [3]),
    ("one_live", [-2.5], [5]),
    ("sixteen_dead_at_both_ends", [NEG, NEG] + [-(1.0 + (j * 5) % 7) for j in range(11)] + [NEG, NEG, NEG],
     [3 + j % 4 for j in range(16)]),
    ("sixteen_all_dead", [NEG] * 16, [2 + j % 5 for j in range(16)]),
)


# ------------------------------------------------------------------------------------------------- the cases
def tables():
    rng = np.random.default_rng(5)
    embed = (rng.integers(-16, 17, size=(V, DIM)) / 8.0).astype(F)
    pos_table = (rng.integers(-16, 17, size=(T, DIM)) / 8.0).astype(F)
    return embed, pos_table


def _row(rng, R, nf, first=None, low=False):
    """One candidate row: R distinct words, the first nf values finite (multiples of 1/2 in [-4, 0], or <= -10 behind a
    given first word at 0 when `low`), the rest -inf; value descending, then word ascending (the short-row rule)."""
    pool = [w for w in range(V) if w != EOS and w != first]
    words = rng.choice(pool, size=R - (first is not None), replace=False)
    vals = -rng.integers(0, 9, size=len(words)) * 32
    if first is not None:
        words = np.concatenate([[first], words])
        vals = np.concatenate([[0], (-640 - rng.integers(0, 5, size=R - 1) * 32) if low else np.minimum(vals, -32)])
    order = np.lexsort((words, -vals))
    words, vals = words[order], (vals[order] / 64.0).astype(F)
    vals[nf:] = NEG
    words[nf:] = np.sort(words[nf:])
    return vals, words.astype(np.int32)


def _image(rng, R, status, nf, firsts=None):
    """status[r] in {'live', 'dead', 'fin', 'empty'} → the image's slice of the state at position T0 and its first
    candidate table.  dead: a real prefix with cumul = -inf (what odic_beam_reset_prefix leaves); fin: a live finished
    row; empty: the EMPTY row of a step before."""
    L = T0 + 1
    tok = np.zeros((R, T), np.int64); lp = np.zeros((R, T), F)
    cumul, ne, he = np.zeros(R, F), np.zeros(R, np.int32), np.zeros(R, np.int32)
    cv, ci = np.empty((R, R), F), np.empty((R, R), np.int32)
    for r in range(R):
        tok[r, 0] = SOS
        tok[r, 1:L] = rng.choice([w for w in range(V) if w != EOS], size=L - 1)
        lp[r, 1:L] = -rng.integers(0, 257, size=L - 1) / 64.0
        ne[r] = L
        if status[r] in ("fin", "empty"):
            tok[r, L - 1] = EOS
            he[r] = 1
            if status[r] == "fin" and rng.uniform() < 0.5:               # finished one position earlier: frozen length
                tok[r, L - 2], lp[r, L - 1], ne[r] = EOS, 0.0, L - 1
            if status[r] == "empty":
                lp[r, L - 1] = NEG
        cs = F(0.0)
        with np.errstate(invalid="ignore"):
            for j in range(L):
                cs = F(cs + lp[r, j])
        cumul[r] = NEG if status[r] == "dead" else cs
        cv[r], ci[r] = _row(rng, R, nf[r], first=None if firsts is None else firsts[r])
    return dict(tok=tok, lp=lp, cumul=cumul, ne=ne, he=he, cv=cv, ci=ci, status=list(status), nf=list(nf))


def _tie(img, a, b):
    """Make rank 0 of rows a and b the image's best total, exactly equal."""
    for r in range(len(img["cumul"])):                                  # (a shift keeps every row sorted)
        img["cv"][r] = np.where(img["cv"][r] > NEG, img["cv"][r] - F(0.5), NEG)
    img["cv"][a, 0] = img["cv"][b, 0] = F(0.0)
    top =F(max(img["cumul"][a], img["cumul"][b]))
    for r in (a, b):                                                    # move the prefix so that both cumuls are `top`
        img["lp"][r, 1] = F(img["lp"][r, 1] + (top - img["cumul"][r]))
        cs = F(0.0)
        for j in range(T0 + 1):
            cs = F(cs + img["lp"][r, j])
        img["cumul"][r] = cs
    assert img["cumul"][a] == img["cumul"][b]
    others = [r for r in range(len(img["cumul"])) if r not in (a, b)]
    for r in others:                                                    # nobody else reaches it
        img["lp"][r, 2] = F(img["lp"][r, 2] - 8.0)
        if img["cumul"][r] > NEG:
            img["cumul"][r] = F(F(F(0.0) + img["lp"][r, 1]) + img["lp"][r, 2])
    return img


def _plain_images(rng, R):
    """class name → image, the patterns over the whole image (classes 1 to 4)."""
    k, mid, last = R, R // 2, R - 1
    one = lambda at, st="live": [st if r == at else "dead" for r in range(k)]            # noqa: E731
    out = {}
    for name, at in (("c1_live_first", 0), ("c1_live_middle", mid), ("c1_live_last", last)):
        out[name] = _image(rng, R, one(at), [k] * k)
    out["c2_dead_interleaved"] = _image(rng, R, ["live" if r % 2 == 0 else "dead" for r in range(k)], [k] * k)
    out["c2_short_rows"] = _image(rng, R, ["live"] * k, [max(1, k - 1 - r % 3) for r in range(k)])
    tie_st = ["live", "dead", "live"] + ["dead" if r % 2 else "live" for r in range(3, k)] if k >= 3 else ["live"] * k
    out["c2_tie_across_dead"] = _image(rng, R, tie_st, [max(1, k - r % 2) for r in range(k)])
    if k >= 2:
        _tie(out["c2_tie_across_dead"], 0, 2 if k >= 3 else 1)
    out["c3_k_minus_1"] = _image(rng, R, one(mid), [k - 1] * k)
    out["c3_one"] = _image(rng, R, one(min(1, last)), [1] * k)
    out["c3_zero"] = _image(rng, R, one(0), [0] * k)
    out["c4_finished_among_dead"] = _image(rng, R, one(mid, "fin"), [k] * k)
    out["c4_empty_beside_live"] = _image(rng, R, ["empty"] + ["live"] * (k - 1), [k] * k)
    out["c4_finished_empty_dead"] = _image(rng, R, (["fin", "empty"] + ["dead"] * k)[:k], [max(0, k - 2)] * k)
    return out


def _group_images(rng, G, kg):
    """Class 5: classes 3 and 4 inside ONE group (the last, or a middle one), the other groups healthy."""
    R = G * kg
    out = {}

    def build(gs, st_in, nf_in, firsts=None):
        status, nf = ["live"] * R, [R] * R
        status[gs * kg:(gs + 1) * kg], nf[gs * kg:(gs + 1) * kg] = st_in, nf_in
        return _image(rng, R, status, nf, firsts)

    one = lambda at, st="live": [st if j == at else "dead" for j in range(kg)]           # noqa: E731
    gl, gm = G - 1, G // 2
    out["c5_k_minus_1"] = build(gl, one(kg - 1), [kg - 1] * kg)
    out["c5_one"] = build(gm, one(0), [1] * kg)
    out["c5_zero"] = build(gl, ["dead"] * kg, [R] * kg)
    out["c5_finished_among_dead"] = build(gm, one(kg // 2, "fin"), [R] * kg)
    out["c5_empty_beside_live"] = build(gl, ["empty"] + ["live"] * (kg - 1), [R] * kg)
    # the only finite candidate of the last group is the word group 0 takes first: penalised, finite, chosen
    w = 7
    firsts = [None] * R
    firsts[0] = firsts[gl * kg] = w
    img = build(gl, one(0), [1] * kg, firsts)
    img["cv"][0, 0] = F(0.0)
    img["lp"][0, 1:T0 + 1] = 0.0                                        # row 0 leads its group: (row 0, w) is pick 0
    img["cumul"][0] = F(0.0)
    assert img["ci"][0, 0] == w and img["ci"][gl * kg, 0] == w and img["cv"][gl * kg, 0] > NEG
    out["c5_penalised_only_one_left"] = img
    return out


def _later_tables(rng, R, step, control_rows):
    """The candidate tables of the second and third step: the control image all finite; elsewhere a row loses a random
    tail to -inf.  At the second step EOS comes first and far ahead (rows finish; `done` can rise at the third)."""
    N = N_IMG * R
    cv, ci = np.empty((N, R), F), np.empty((N, R), np.int32)
    for n in range(N):
        nf = R if n in control_rows else int(rng.integers(0, R + 1))
        if step == 1:
            cv[n], ci[n] = _row(rng, R, nf, first=EOS, low=True)
        else:
            cv[n], ci[n] = _row(rng, R, nf)
    return cv, ci


@functools.lru_cache(maxsize=None)
def batches(G: int, kg: int):
    """The batches of (G, kg): [dict(state, cands [(cv, ci)] * N_STEPS, classes [N_IMG names])].  Every batch holds three
    case images and the control image (all rows live, every candidate finite) at index CONTROL.  Candidate rows are sorted
    as the group step wants them, so every batch serves both kernels (the plain one with k = G·kg)."""
    R = G * kg
    rng = np.random.default_rng(4000 + 100 * G + kg)
    images = _plain_images(rng, R)
    if G > 1:
        images.update(_group_images(rng, G, kg))
    names = list(images)
    out = []
    for i in range(0, len(names), N_IMG - 1):
        group = names[i:i + N_IMG - 1]
        imgs = [images[n] for n in group] + [_image(rng, R, ["live"] * R, [R] * R)]
        st = M.new_state(N_IMG, R, T, SOS)
        st["anc"][:] = 0
        for b, im in enumerate(imgs):
            rows = slice(b * R, (b + 1) * R)
            st["tokens"][b], st["logprobs"][b] = im["tok"], im["lp"]
            st["cumul"][rows], st["n_elem"][rows], st["has_eos"][rows] = im["cumul"], im["ne"], im["he"]
            st["anc"][rows, :T0] = b * R + rng.integers(0, R, size=(R, T0))
            st["next_tok"][rows] = im["tok"][:, T0]
        st["pos"][0] = T0
        control_rows = set(range(CONTROL * R, (CONTROL + 1) * R))
        cands = [(np.concatenate([im["cv"] for im in imgs]), np.concatenate([im["ci"] for im in imgs]))]
        cands += [_later_tables(rng, R, s, control_rows) for s in range(1, N_STEPS)]
        out.append(dict(state=st, cands=cands, classes=group + ["control"], images=imgs))
    return out


def run(batch, G: int, kg: int, plain: bool, only_image: int | None = None):
    """The model over the N_STEPS steps of a batch → [(state, y, events)] after every step.  plain: odic_beam_step with
    k = G·kg; else odic_group_beam_step.  only_image: that image alone, as a batch of one."""
    R = G * kg
    embed, pos_table = tables()
    st = {k: v.copy() for k, v in batch["state"].items()}
    cands = batch["cands"]
    if only_image is not None:
        b, rows = only_image, slice(only_image * R, (only_image + 1) * R)
        st = {k: (v[b:b + 1] if k in ("tokens", "logprobs") else v if k in ("pos", "done") else v[rows]).copy()
              for k, v in st.items()}
        st["anc"] = st["anc"] - b * R
        cands = [(cv[rows], ci[rows]) for cv, ci in cands]
    y = np.zeros((st["cumul"].shape[0], DIM), F)
    emb = dict(embed=embed, pos_table=pos_table, scale=SCALE, y=y)
    trace = []
    for cv, ci in cands:
        st, ev = plain_step(st, cv, ci, EOS, emb) if plain else group_step(st, cv, ci, G, kg, PENALTY, EOS, emb)
        trace.append((st, y.copy(), ev))
    return trace


def finite_totals(im, rows=None) -> int:
    """Totals above -inf among the first-step candidates of an image (of the rows given: a group)."""
    n = 0
    for r in (range(len(im["cumul"])) if rows is None else rows):
        if im["cumul"][r] > NEG:
            n += len(im["nf"]) if im["he"][r] else int((im["cv"][r] > NEG).sum())
    return n


# ------------------------------------------------------------------------------------------------- the old search loop
def search_loop_candidates(rng, N: int, k: int, step: int, eos: int):
    """The candidate tables of test_beam_step_direct_against_the_search_loop: log-probs on a coarse grid (→ exact ties
    across beams), sorted descending per row; EOS is frequent from step 3 on so that every beam finishes well before T."""
    cv = -np.sort(rng.integers(1, 6, size=(N, k)).astype(np.float32) * 0.25, axis=1)
    cw = rng.integers(10, 40, size=(N, k)).astype(np.int32)
    if step >= 3:
        cw[rng.random((N, k)) < 0.45] = eos
    return cv, cw


class SearchLoop:
    """A plain restatement of captioning_model.py:117-241 on Python lists: EXACT ties in the k·k selection (lowest flat
    index wins, the scan order of torch.topk on sorted input), finished beams (0.0 / −999 masking, frozen length),
    re-summed cumulative scores, the ancestor table.  It knows nothing of dead rows."""

    def __init__(self, n_img: int, k: int, T_: int, sos: int, eos: int):
        self.n_img, self.k, self.eos = n_img, k, eos
        self.toks = [[[sos] for _ in range(k)] for _ in range(n_img)]
        self.lps = [[[np.float32(0.0)] for _ in range(k)] for _ in range(n_img)]
        self.n_elem = [[1] * k for _ in range(n_img)]
        self.anc = np.zeros((n_img * k, T_), dtype=np.int64)

    def advance(self, cv, cw, step: int):
        """One step → (row_valid, next_tok) as flat lists; toks / lps / n_elem / anc move on."""
        n_img, k, eos, toks, lps, n_elem, anc = self.n_img, self.k, self.eos, self.toks, self.lps, self.n_elem, self.anc
        new_toks, new_lps, new_ne, valid, nxt = [], [], [], [], []
        new_anc = anc.copy()
        for b in range(n_img):
            if step == 0:
                sel = [(0, c) for c in range(k)]
                val = {(0, c): cv[b * k, c] for c in range(k)}
            else:
                tot, val = [], {}
                for j in range(k):
                    dn = eos in toks[b][j]
                    cu = np.float32(0.0)
                    for x in lps[b][j]:
                        cu = np.float32(cu + x)
                    for c in range(k):
                        v = (np.float32(0.0) if c == 0 else np.float32(-999.0)) if dn else cv[b * k + j, c]
                        val[(j, c)] = v
                        tot.append((np.float32(cu + v), j, c))
                sel = []
                for _ in range(k):
                    bi = max(range(len(tot)), key=lambda i: (tot[i][0], -i))        # ties → lowest flat index
                    sel.append((tot[bi][1], tot[bi][2]))
                    tot[bi] = (np.float32(-np.inf), 0, 0)
            rt, rl, rn = [], [], []
            for r, (j, c) in enumerate(sel):
                had = (eos in toks[b][j]) if step > 0 else False
                w = int(cw[b * k + j, c])
                rt.append(toks[b][j] + [w])
                rl.append(lps[b][j] + [val[(j, c)]])
                rn.append((n_elem[b][j] if step > 0 else 1) + (0 if had else 1))
                valid.append(0 if had else 1)
                nxt.append(w)
                new_anc[b * k + r, :step] = anc[b * k + j, :step]
                new_anc[b * k + r, step] = b * k + j
            new_toks.append(rt); new_lps.append(rl); new_ne.append(rn)
        self.toks, self.lps, self.n_elem, self.anc = new_toks, new_lps, new_ne, new_anc
        return valid, nxt

    def cumul(self):
        cum = [[np.float32(0.0)] * self.k for _ in range(self.n_img)]
        for b in range(self.n_img):
            for j in range(self.k):
                c = np.float32(0.0)
                for x in self.lps[b][j]:
                    c = np.float32(c + x)
                cum[b][j] = c
        return cum
