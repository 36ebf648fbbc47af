"""A numpy model of one step of stochastic beam search (odic_stochastic_beam_step), its error band, its invariants and the
cases its tests use (no tests here).

Written from the semantics in include/odic_hip.h and DESIGN.md §4.21, not from the kernel:

  * row j of an image has phi_j = cumul[j] and G_j = gscore[j]; a live row has cumul > -inf; at t = 0 only row 0 offers, with
    phi = G = 0;
  * a live growing row offers every candidate r with cand_val > -inf at
        d = pert_r - pert_0;  d == 0: G~ = G_j exactly;
        else u = (G_j - phi_j) - pert_r, v = u + log1mexp(d), G~ = G_j - max(v, 0) - log1p(exp(-|v|));
    a live finished row offers itself (the word of its rank-0 slot, stored log-prob 0) at G~ = G_j;
  * the `beams` best offers are the new rows: G~ descending, then source row, then rank, ascending;
  * a slot without an offer is an empty row: parent = itself (row 0 at t = 0), word = EOS, stored -inf, gscore -inf;
  * the update is odic_beam_step's (required_words_model.apply_choice), the stored value the word's own log-prob.

The transform is evaluated in float64 on the fp32 inputs.  The noise of the scored draw comes from sample_filter_model
(noise_bits, gumbel).

The band.  What the device may differ from the model's G~ by, from the fp32 operations of the transform (eps = 2^-24, the
relative error of one rounded operation; the library functions expm1f, logf, expf, log1pf are taken at 2 ulp = 4·eps relative):
    d   = pert_r - pert_0              eps·|d|
    w   = G - phi                      eps·|w|
    u   = w - pert_r                   eps·|u| + eps·|w|
    L   = log1mexp(d)                  |dL/dd|·eps·|d| <= eps  (|d| / (e^|d| - 1) <= 1)
                                       + 4·eps: the inner function (-expm1(d) or exp(d), at most 1/2) is 4·eps relative, and the
                                         outer logarithm turns a relative error of its argument into an absolute one of that
                                         size (log1p(-e) with 1/(1 - e) <= 2 and e <= 1/2: the same 4·eps)
                                       + 4·eps·|L|: the outer function's own error
    v   = u + L                        eps·|v| + the errors of u and L
    s   = max(v, 0) + log1p(exp(-|v|)) the error of v (the slope of softplus is at most 1) + 4·eps (exp, at most 1, through
                                       log1p's slope <= 1) + 4·eps·ln 2 (log1p's own, its value at most ln 2)
    G~  = (G - max(v, 0)) - log1p(..)  eps·(|G| + |v|) + eps·(|G| + |v| + ln 2)
  band = eps·(3·|v| + 2·|w| + |u| + 4·|L| + 2·|G| + 12.5)
With S = max(1, |G|, |phi|, |pert|): |w| <= 2S, |u| <= 3S, |v| <= 3S + |L|, so band <= eps·(18·S + 7·|L| + 12.5) — it scales with
S, and with |L| = |log(1 - e^d)|, which is large only where two perturbed scores nearly tie.  An offer with d == 0 and a
finished row's offer copy an fp32 input: their band is 0.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import required_words_model as RM
import sample_filter_model as SF
from group_beam_model import STATE_KEYS, new_state  # noqa: F401  (the same state)

F = np.float32
NEG = F(-np.inf)
EPS = 2.0 ** -24
LN2 = math.log(2.0)


def log1mexp(d: float) -> float:
    return math.log(-math.expm1(d)) if d > -LN2 else math.log1p(-math.exp(d))


def child(G, phi, pert, pert0):
    """fp32 inputs → (G~ in float64, band, exact: the value is a copy of G)."""
    G, phi, pert, pert0 = float(G), float(phi), float(pert), float(pert0)
    d = pert - pert0
    if d == 0.0:
        return G, 0.0, True
    w = G - phi
    u = w - pert
    L = log1mexp(d)
    v = u + L
    g = G - max(v, 0.0) - math.log1p(math.exp(-abs(v)))
    band = EPS * (3 * abs(v) + 2 * abs(w) + abs(u) + 4 * abs(L) + 2 * abs(G) + 12.5)
    return g, band, False


def offers_of_image(cv, ci, cp, cumul, has_eos, gscore, t: int):
    """Every offer of one image, best first: dicts g (float64), band, exact, row, rank, word, lp (the stored fp32 value)."""
    k = cv.shape[0]
    out = []
    for j in range(k):
        live = j == 0 if t == 0 else bool(cumul[j] > NEG)
        if not live:
            continue
        G, phi = (F(0), F(0)) if t == 0 else (F(gscore[j]), F(cumul[j]))
        if t > 0 and has_eos[j]:
            out.append(dict(g=float(G), band=0.0, exact=True, row=j, rank=0, word=int(ci[j, 0]), lp=F(0)))
            continue
        for r in range(cv.shape[1]):
            if not cv[j, r] > NEG:
                continue
            g, band, exact = child(G, phi, cp[j, r], cp[j, 0])
            out.append(dict(g=g, band=band, exact=exact, row=j, rank=r, word=int(ci[j, r]), lp=F(cv[j, r])))
    return sorted(out, key=lambda o: (-o["g"], o["row"], o["rank"]))


def select_image(offers, k: int, t: int, eos: int):
    """→ parent, word, lp, g (float64), band — each [k]; empty slots by the convention above."""
    parent, word, lp = np.zeros(k, np.int32), np.zeros(k, np.int64), np.zeros(k, F)
    g, band = np.full(k, -np.inf), np.zeros(k)
    for r in range(k):
        if r < len(offers):
            o = offers[r]
            parent[r], word[r], lp[r], g[r], band[r] = o["row"], o["word"], o["lp"], o["g"], o["band"]
        else:
            parent[r], word[r], lp[r] = (0 if t == 0 else r), eos, NEG
    return parent, word, lp, g, band


def is_clear(offers, k: int, slack=None) -> bool:
    """The device's choice AND its order are determined: every two neighbours among the first k + 1 offers are either
    both exact copies of fp32 inputs (their order is then that of the inputs and the key) or further apart than twice the
    larger band.  slack [k]: what the device's G of every source row may already differ from the model's by (a chained
    replay; G~ moves with G at a slope of at most 1), added to the band of that row's offers."""
    head = offers[:k + 1]
    unc = lambda o: o["band"] + (float(slack[o["row"]]) if slack is not None else 0.0)      # noqa: E731
    for a, b in zip(head, head[1:]):
        if a["exact"] and b["exact"]:
            continue
        if not a["g"] - b["g"] > 2.0 * max(unc(a), unc(b)):
            return False
    return True


def step(st: dict, gscore, cand_val, cand_idx, cand_pert, eos: int, emb: dict | None = None):
    """One step on every image.  st: the arrays of STATE_KEYS; gscore fp32 [n_img·k]; cand_* [n_img·k, k].
    → (new state, new gscore float64 [n_img·k], band [n_img·k], per-image offer lists)."""
    n_img, k, T = st["tokens"].shape
    t = int(st["pos"][0])
    new = {key: v.copy() for key, v in st.items()}
    gnew, band = np.asarray(gscore, np.float64).copy(), np.zeros(n_img * k)
    if t + 1 >= T:
        return new, gnew, band, []
    alive, every = False, []
    for b in range(n_img):
        rows = slice(b * k, (b + 1) * k)
        offers = offers_of_image(np.asarray(cand_val)[rows], np.asarray(cand_idx)[rows], np.asarray(cand_pert)[rows],
                                 st["cumul"][rows], st["has_eos"][rows], np.asarray(gscore)[rows], t)
        parent, word, lp, g, bd = select_image(offers, k, t, eos)
        alive |= RM.apply_choice(st, b, parent, word, lp, eos, emb, new)
        gnew[rows], band[rows] = g, bd
        every.append(offers)
    new["pos"][0] = t + 1
    if not alive:
        new["done"][0] = 1
    return new, gnew, band, every


# ---------------------------------------------------------------------------------------------------------- invariants
def check_invariants(before: dict, g_before, after: dict, g_after, what: str = "") -> None:
    """The four invariants of a step, from the states on both sides of it alone (a new row's parent is anc[n][t])."""
    n_img, k, T = before["tokens"].shape
    t = int(before["pos"][0])
    assert int(after["pos"][0]) == t + 1, what
    g_before, g_after = np.asarray(g_before, F), np.asarray(g_after, F)
    for b in range(n_img):
        rows = np.arange(b * k, (b + 1) * k)
        ga = g_after[rows]
        assert np.all(ga[:-1] >= ga[1:]), f"{what}: gscore of image {b} is not sorted: {ga}"
        live = after["cumul"][rows] > NEG
        assert np.all(np.isneginf(ga[~live])), f"{what}: an empty row of image {b} has a finite gscore"
        best_child = {}
        for r in np.flatnonzero(live):
            par = int(after["anc"][b * k + r, t])
            assert b * k <= par < (b + 1) * k, f"{what}: parent outside the image"
            Gp = F(0) if t == 0 else g_before[par]
            assert ga[r] <= Gp, f"{what}: image {b} row {r}: child {ga[r]} above its parent's {Gp}"
            best_child[par] = max(best_child.get(par, NEG), ga[r])
        for par, gmax in best_child.items():
            Gp = F(0) if t == 0 else g_before[par]
            assert np.array_equal(np.asarray(gmax, F).view(np.int32), np.asarray(Gp, F).view(np.int32)), \
                f"{what}: image {b}: the best child of row {par} has {gmax}, its parent {Gp}"
        seen = {tuple(after["tokens"][b, r, :t + 2].tolist()) for r in np.flatnonzero(live)}
        assert len(seen) == int(live.sum()), f"{what}: image {b} holds a prefix twice"


# --------------------------------------------------------------------------------------------------------------- cases
V, SOS, EOS, D = 64, 3, 2, 8
SCALE = 4.0
N_IMGS, BEAMS, TS = (1, 3), (1, 2, 5, 16), (2, 6, 128)
KINDS = ("seed", "mixed", "all_finished", "few_offers", "tie", "ln2", "large", "full")


def tables(T: int):
    rng = np.random.default_rng(5)
    return (rng.integers(-16, 17, size=(V, D)) / 8.0).astype(F), (rng.integers(-16, 17, size=(T, D)) / 8.0).astype(F)


def applicable(kind: str, k: int, T: int) -> bool:
    if kind in ("seed", "full"):
        return True
    if T == 2:                                   # position 0 is the only one that steps
        return False
    if kind in ("tie", "ln2", "mixed"):
        return k >= 2
    return True


def _build(kind: str, n_img: int, k: int, T: int, salt: int) -> dict:
    rng = np.random.default_rng([sum(map(ord, kind)), n_img, k, T, salt])
    N = n_img * k
    t = 0 if kind == "seed" else T - 1 if kind == "full" else min(T - 2, 100 if kind == "large" else 3)
    per_tok = 7.0 if kind == "large" else 1.0   # 100 words at about -7 each: a 74-word caption's scale and beyond
    st = new_state(n_img, k, T, SOS)
    st["pos"][0] = t
    gscore = np.zeros(N, F)
    if t > 0:
        for b in range(n_img):
            for r in range(k):
                n = b * k + r
                fin = {"mixed": r % 2 == 1, "all_finished": True}.get(kind, False) and t >= 3
                length = int(rng.integers(3, t + 2)) if fin else t + 1          # tokens incl. SOS (and EOS when finished)
                words = rng.integers(4, V, size=t + 1)
                words[0] = SOS
                words[1] = 4 + (r % (V - 4))                                   # the rows of an image differ in their first word
                lps = -(rng.integers(1, 17, size=t + 1) / 8.0 * per_tok).astype(F)
                lps[0] = 0
                if fin:
                    words[length - 1:] = EOS
                    lps[length:] = 0
                st["tokens"][b, r, :t + 1], st["logprobs"][b, r, :t + 1] = words, lps
                cs = F(0)
                for v in lps:
                    cs = F(cs + v)
                st["cumul"][n], st["n_elem"][n], st["has_eos"][n] = cs, length, int(fin)
                st["row_valid"][n] = 0 if fin and length < t + 1 else 1
                st["next_tok"][n] = words[t]
                st["anc"][n, :t] = rng.integers(b * k, (b + 1) * k, size=t)
            # perturbed scores: phi + Gumbel noise, the rows sorted by them as a step leaves them
            rows = slice(b * k, (b + 1) * k)
            g = (st["cumul"][rows].astype(np.float64) + rng.gumbel(size=k)).astype(F)
            order = np.argsort(-g, kind="stable")
            for key in ("tokens", "logprobs"):
                st[key][b] = st[key][b][order]
            for key in ("cumul", "n_elem", "has_eos", "row_valid", "next_tok", "anc"):
                st[key][rows] = st[key][rows][order]
            gscore[rows] = g[order]
    # candidates: k distinct words per row, log-probs and Gumbel noise, by perturbed score descending
    cv, ci, cp = np.zeros((N, k), F), np.zeros((N, k), np.int32), np.zeros((N, k), F)
    for n in range(N):
        words = rng.choice(np.arange(V), size=k, replace=False)
        lp = -(rng.uniform(0.05, 6.0, size=k) * per_tok).astype(F)
        pert = (lp.astype(np.float64) + rng.gumbel(size=k)).astype(F)
        if kind == "tie" and k >= 2:
            pert[1] = pert[0] = max(pert[0], pert[1])                           # rank 1 ties rank 0 exactly
        if kind == "ln2" and k >= 2:
            top = pert.max()
            gaps = np.array([0.0, LN2 - 1e-3, LN2 + 1e-3, 0.1, 5.0, 20.0])[:k]   # d on both sides of -ln 2, near 0, far
            pert[:len(gaps)] = (top - gaps).astype(F)
            pert[len(gaps):] = np.minimum(pert[len(gaps):], top - F(25.0))
        order = np.argsort(-pert, kind="stable")
        cv[n], ci[n], cp[n] = lp[order], words[order], pert[order]
        if kind == "few_offers":                                                # a row with one finite word; the rest masked
            cv[n, 1:], cp[n, 1:] = NEG, NEG
    if kind == "few_offers" and t > 0:                                          # image 0 keeps one live row: k - 1 empty rows
        st["cumul"][1:k] = NEG
        st["logprobs"][0, 1:, t] = NEG
        st["has_eos"][1:k] = 1
        gscore[1:k] = NEG
    return dict(kind=kind, n_img=n_img, k=k, T=T, t=t, st=st, gscore=gscore, cv=cv, ci=ci, cp=cp)


@functools.lru_cache(maxsize=None)
def case(kind: str, n_img: int, k: int, T: int):
    """The first salt whose case is clear (the model alone decides; test_stochastic_beam_host.py asserts that every case is),
    with the model's result: dict(..., new, gnew, band, offers)."""
    for salt in range(64):
        c = _build(kind, n_img, k, T, salt)
        embed, pos_table = tables(T)
        y = np.zeros((n_img * k, D), F)
        c["emb"] = dict(embed=embed, pos_table=pos_table, scale=SCALE, y=y)
        c["new"], c["gnew"], c["band"], c["offers"] = step(c["st"], c["gscore"], c["cv"], c["ci"], c["cp"], EOS, emb=c["emb"])
        if all(is_clear(o, k) for o in c["offers"]):
            return c
    raise AssertionError(f"no clear case for {kind} n_img={n_img} k={k} T={T}")


CASES = [(kind, n, k, T) for kind in KINDS for n in N_IMGS for k in BEAMS for T in TS if applicable(kind, k, T)]


# ------------------------------------------------------------------------------------------------- the scored row draw
def scored_draw(x: np.ndarray, k: int, seed: int, pos: int):
    """odic_logsoftmax_sample_scored on fp32 rows x [N, V]: the fp32 sum x + Gumbel the device ranks by (noise in float64
    from the device's bits, rounded once), the draw order, and → (top_idx [N, k], top_pert float64 [N, k] from the exact
    noise and log-sum-exp, gumbel [N, V], lse [N]).  Rows with fewer than k finite words: -inf in the remaining slots."""
    x = np.asarray(x, F)
    N, V_ = x.shape
    gum = SF.gumbel(SF.noise_bits(seed, np.arange(N), V_, pos))
    with np.errstate(invalid="ignore"):
        s = x.astype(np.float64) + gum
    m = x.max(axis=1).astype(np.float64)
    lse = m + np.log(np.exp(x.astype(np.float64) - m[:, None]).sum(axis=1))
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    pert = np.take_along_axis(s, order, 1) - lse[:, None]
    return order.astype(np.int32), pert, gum, lse
