"""A numpy float32 model of pooled beam search (include/odic_hip.h: odic_pool_beam_step,
odic_pool_beam_finalize): the step, the pool and the finalize, with the device's arithmetic — fp32 additions, the
sequential re-sum in position order, one fp32 division by the host-built table — so that every field can be compared bit
for bit.  Not a test module: tests/test_pool_beam_host.py, test_pool_beam_kernels_gpu.py and test_pool_beam_search_gpu.py
import it.

State: dict(tokens int64 [n_img, k, T], logprobs f32 [n_img, k, T], anc int32 [n_img·k, T], cumul f32, n_elem, has_eos,
row_valid int32, next_tok int64 [n_img·k], pos, done int32 [1]).  Pool: dict(tokens, logprobs [n_img, P, T]; len, sum,
score, serial [n_img, P]; count, closed [n_img]), P = k.
"""
import numpy as np

F = np.float32
NINF = F(-np.inf)
SOS, EOS, V = 1, 2, 12
STATE_KEYS = ("tokens", "logprobs", "anc", "cumul", "n_elem", "has_eos", "row_valid", "next_tok", "pos", "done")
POOL_KEYS = ("tokens", "logprobs", "len", "sum", "score", "serial", "count", "closed")


def scale_table(T: int, alpha: float) -> np.ndarray:
    """scale[L] = float32(float64(L) ** alpha), L = 0 .. T: the power in float64, then one rounding."""
    return np.array([float(L) ** float(alpha) for L in range(T + 1)], dtype=np.float64).astype(F)


def fdiv(a, b) -> np.float32:
    with np.errstate(all="ignore"):
        return F(F(a) / F(b))


def fadd(a, b) -> np.float32:
    with np.errstate(all="ignore"):
        return F(F(a) + F(b))


def resum(lp_row, t: int, v) -> np.float32:
    """The parent's per-token log-probs re-summed in position order, then + v (beam_apply's order)."""
    cs = F(0.0)
    for j in range(t + 1):
        cs = fadd(cs, lp_row[j])
    return fadd(cs, v)


def new_state(n_img: int, k: int, T: int) -> dict:
    N = n_img * k
    st = dict(tokens=np.zeros((n_img, k, T), np.int64), logprobs=np.zeros((n_img, k, T), F), anc=np.zeros((N, T), np.int32),
              cumul=np.zeros(N, F), n_elem=np.zeros(N, np.int32), has_eos=np.zeros(N, np.int32),
              row_valid=np.ones(N, np.int32), next_tok=np.full(N, SOS, np.int64), pos=np.zeros(1, np.int32),
              done=np.zeros(1, np.int32))
    st["tokens"][:, :, 0] = SOS
    return st


def new_pool(n_img: int, P: int, T: int) -> dict:
    return dict(tokens=np.zeros((n_img, P, T), np.int64), logprobs=np.zeros((n_img, P, T), F),
                len=np.zeros((n_img, P), np.int32), sum=np.zeros((n_img, P), F), score=np.zeros((n_img, P), F),
                serial=np.zeros((n_img, P), np.int32), count=np.zeros(n_img, np.int32), closed=np.zeros(n_img, np.int32))


def copy(d: dict) -> dict:
    return {k: v.copy() for k, v in d.items()}


def pool_worst(pool, b: int) -> int:
    """The worst entry of a non-empty pool: lowest score, a tie to the highest serial."""
    sc, ser = pool["score"][b], pool["serial"][b]
    w = 0
    for i in range(1, int(pool["count"][b])):
        if sc[i] < sc[w] or (sc[i] == sc[w] and ser[i] > ser[w]):
            w = i
    return w


def pool_offer(pool, b: int, sm, ln: int, scale, tok_row, lp_row) -> int:
    """One offer: appended while the pool is not full, else in place of the worst entry when STRICTLY better.  → the slot
    or -1.  tok_row / lp_row: the hypothesis's whole rows of T entries."""
    P = pool["score"].shape[1]
    T = len(scale) - 1
    sc = fdiv(sm, scale[min(max(int(ln), 0), T)])
    cnt = int(pool["count"][b])
    ser = max([int(s) + 1 for s in pool["serial"][b, :cnt]], default=0)
    if cnt < P:
        slot = cnt
        pool["count"][b] = cnt + 1
    else:
        slot = pool_worst(pool, b)
        if not sc > pool["score"][b, slot]:
            return -1
    pool["len"][b, slot], pool["sum"][b, slot], pool["score"][b, slot], pool["serial"][b, slot] = ln, F(sm), sc, ser
    pool["tokens"][b, slot], pool["logprobs"][b, slot] = tok_row, lp_row
    return slot


def walk(cumul, cv, elp, k: int, t: int, min_words: int):
    """The ranking and the walk of one image.  cumul [k], cv [k, k], elp [k] → (rows: [(parent, cand, value)] of the new
    live rows, offers: [(parent, value)] in walk order)."""
    cands = []
    for j in range(k):
        if not ((j == 0) if t == 0 else (cumul[j] > NINF)):
            continue
        for c in range(k + 1):
            if c == k and t < min_words:
                continue
            v = F(elp[j]) if c == k else F(cv[j, c])
            tot = v if t == 0 else fadd(cumul[j], v)
            if tot > NINF:                                   # (-inf and NaN are never ranked)
                cands.append((-float(tot), j * (k + 1) + c, v))
    cands.sort(key=lambda x: (x[0], x[1]))
    rows, offers = [], []
    for ex, (_, key, v) in enumerate(cands[:2 * k]):
        if len(rows) == k:
            break
        j, c = divmod(key, k + 1)
        if c == k:
            if ex < k:
                offers.append((j, v))
        else:
            rows.append((j, c, v))
    return rows, offers


def step(st: dict, pool: dict, cv, ci, elp, scale, min_words: int = 0, early: bool = False, eos: int = EOS) -> None:
    """One odic_pool_beam_step, in place.  cv f32 / ci int [n_img·k, k], elp f32 [n_img·k]: EOS's log-prob per row."""
    n_img, k, T = st["tokens"].shape
    t = int(st["pos"][0])
    if t + 1 >= T:
        return
    old = copy(st)
    alive_any = False
    for b in range(n_img):
        if pool["closed"][b] != 0:
            continue
        r0 = b * k
        rows, offers = walk(old["cumul"][r0:r0 + k], cv[r0:r0 + k], elp[r0:r0 + k], k, t, min_words)
        for j, v in offers:
            tok_row, lp_row = np.zeros(T, np.int64), np.zeros(T, F)
            tok_row[:t + 1], lp_row[:t + 1] = old["tokens"][b, j, :t + 1], old["logprobs"][b, j, :t + 1]
            tok_row[t + 1], lp_row[t + 1] = eos, v
            ln = (1 if t == 0 else int(old["n_elem"][r0 + j])) + 1
            pool_offer(pool, b, resum(old["logprobs"][b, j], t, v), ln, scale, tok_row, lp_row)
        chosen = [(j, int(ci[r0 + j, c]), v) for j, c, v in rows]
        chosen += [(0 if t == 0 else r, eos, NINF) for r in range(len(chosen), k)]          # EMPTY rows
        ncu = [resum(old["logprobs"][b, j], t, v) for j, _, v in chosen]
        closing = False
        if int(pool["count"][b]) == k:
            best = NINF
            for c in ncu:
                if c > best:
                    best = c
            closing = bool(early) or bool(pool["score"][b, pool_worst(pool, b)] >= fdiv(best, scale[T]))
        if closing:
            pool["closed"][b] = 1
        for r, (j, w, v) in enumerate(chosen):
            n = r0 + r
            st["tokens"][b, r, :t + 1], st["logprobs"][b, r, :t + 1] = old["tokens"][b, j, :t + 1], old["logprobs"][b, j, :t + 1]
            st["anc"][n, :t] = old["anc"][r0 + j, :t]
            st["anc"][n, t] = r0 + j
            st["tokens"][b, r, t + 1], st["logprobs"][b, r, t + 1] = w, v
            pe = 0 if t == 0 else int(old["has_eos"][r0 + j])
            ne = 1 if t == 0 else int(old["n_elem"][r0 + j])
            st["cumul"][n] = ncu[r]
            st["n_elem"][n] = ne + (0 if pe else 1)
            st["has_eos"][n] = 1 if (pe or w == eos) else 0
            st["row_valid"][n] = 0 if (pe or closing) else 1
            st["next_tok"][n] = w
            alive_any = alive_any or not (pe or closing)
    if not alive_any:
        st["done"][0] = 1
    st["pos"][0] = t + 1


def finalize(st: dict, pool: dict, scale):
    """odic_pool_beam_finalize, in place on the pool → (order int32 [n_img, P], score f32 [n_img, P])."""
    n_img, k, T = st["tokens"].shape
    order, score = np.full((n_img, k), -1, np.int32), np.full((n_img, k), NINF, F)
    for b in range(n_img):
        if pool["closed"][b] == 0:
            for r in range(k):
                n = b * k + r
                if not st["cumul"][n] > NINF or st["has_eos"][n] != 0:
                    continue
                ln = int(st["n_elem"][n])
                m = min(max(ln, 0), T)
                tok_row, lp_row = np.zeros(T, np.int64), np.zeros(T, F)
                tok_row[:m], lp_row[:m] = st["tokens"][b, r, :m], st["logprobs"][b, r, :m]
                pool_offer(pool, b, st["cumul"][n], ln, scale, tok_row, lp_row)
        pool["closed"][b] |= 2
        cnt = int(pool["count"][b])
        sc, ser = pool["score"][b], pool["serial"][b]
        taken = set()
        for r in range(cnt):
            bi = -1
            for j in range(cnt):
                if j not in taken and (bi < 0 or sc[j] > sc[bi] or (sc[j] == sc[bi] and ser[j] < ser[bi])):
                    bi = j
            taken.add(bi)
            order[b, r], score[b, r] = bi, sc[bi]
    return order, score


def captions(pool: dict, order, how_many: int, sos: int = SOS, eos: int = EOS):
    """The token lists a search returns from the finalized pool: [sos, eos] where the pool ran out."""
    out = []
    for b in range(order.shape[0]):
        per = []
        for j in range(how_many):
            i = int(order[b, j])
            per.append([sos, eos] if i < 0 else pool["tokens"][b, i, :int(pool["len"][b, i])].tolist())
        out.append(per)
    return out


# ------------------------------------------------------------------------------------------------- cases for the kernels
KINDS = ("all_eos", "ties", "equal_scores", "dead", "nan", "close_one", "last", "min_length", "empty", "seed")


def _random_state(rng, n_img, k, T, t, dyadic):
    """A consistent state at position t: every row live, growing, n_elem = t + 1, cumul the re-sum of its log-probs."""
    st = new_state(n_img, k, T)
    N = n_img * k
    st["tokens"][:, :, 1:t + 1] = rng.integers(3, V, size=(n_img, k, t))
    lp = -rng.integers(1, 5, size=(n_img, k, t)).astype(F) * F(0.5) if dyadic else -rng.random((n_img, k, t)).astype(F) * F(3.0)
    st["logprobs"][:, :, 1:t + 1] = lp
    st["anc"][:, :t] = (np.arange(N)[:, None] // k) * k + rng.integers(0, k, size=(N, t))
    st["cumul"][:] = [resum(st["logprobs"].reshape(N, T)[n], t, F(0.0)) for n in range(N)]
    st["n_elem"][:] = t + 1
    st["next_tok"][:] = st["tokens"].reshape(N, T)[:, t]
    st["pos"][0] = t
    if t == 0:                                                # what odic_beam_reset leaves alone holds anything
        st["cumul"][:] = np.nan
        st["n_elem"][:] = 77
        st["has_eos"][:] = 1
    return st


def _random_cands(rng, N, k, dyadic):
    if dyadic:
        cv = -np.sort(rng.integers(1, 4, size=(N, k)), axis=1).astype(F) * F(0.5)
        elp = -rng.integers(1, 4, size=N).astype(F) * F(0.5)
    else:
        cv = -np.sort(rng.random((N, k)).astype(F) * F(4.0), axis=1) - F(0.05)
        elp = -rng.random(N).astype(F) * F(4.0) - F(0.05)
    ci = np.stack([rng.permutation(np.arange(3, V + 8))[:k] for _ in range(N)]).astype(np.int32)      # never EOS
    return cv, ci, elp


def _prefill(pool, rng, b, n, scale, T, score_like=None):
    """n hypotheses of 3 tokens in the pool of image b (scores random, or all the given sum over length 3)."""
    for _ in range(n):
        sm = F(score_like) if score_like is not None else -F(rng.random() * 6.0 + 0.1)
        tok_row, lp_row = np.zeros(T, np.int64), np.zeros(T, F)
        tok_row[:3], lp_row[:3] = [SOS, 5, EOS], [0.0, sm / F(2.0), sm / F(2.0)]
        pool_offer(pool, b, sm, 3, scale, tok_row, lp_row)


def case(kind: str, n_img: int, k: int, T: int, alpha: float) -> dict:
    """→ dict(st, pool, scale, min_words, early, steps: [(cv, ci, elp), ...]): the state before the first step and the
    candidates of every chained step.  The kinds are the situations of the issue; see the kernel test's docstring."""
    rng = np.random.default_rng([KINDS.index(kind), n_img, k, T, int(alpha * 10)])
    N = n_img * k
    scale = scale_table(T, alpha)
    dyadic = kind in ("ties", "equal_scores")
    t = {"seed": 0, "last": T - 2}.get(kind, 1)
    st, pool = _random_state(rng, n_img, k, T, t, dyadic), new_pool(n_img, k, T)
    # unused pool slots hold anything: the kernels never read behind count
    pool["score"][:], pool["serial"][:], pool["sum"][:], pool["len"][:] = np.nan, 1000, np.nan, -5
    min_words, early, n_steps = 0, False, 2
    steps = [_random_cands(rng, N, k, dyadic) for _ in range(3)]
    if kind == "all_eos":                                     # k offers in one step into a pool that overflows
        for b in range(n_img):
            _prefill(pool, rng, b, max(k - 1 - b, 0), scale, T, score_like=-20.0 - b)      # (worse than any offer)
        steps[0][2][:] = -F(0.01) * (1 + rng.permutation(N)).astype(F)
    elif kind == "ties":
        st["cumul"][:] = -rng.integers(1, 3, size=N).astype(F)
    elif kind == "equal_scores":                              # rows of one history and one EOS log-prob: equal sums and lengths
        st["logprobs"][:, :, 1] = F(-1.0)
        st["cumul"][:] = F(-1.0)
        steps[0][2][:] = F(-0.5)
        for b in range(n_img):
            _prefill(pool, rng, b, k // 2, scale, T, score_like=-1.5)
    elif kind == "dead":
        dead = rng.random(N) < 0.4
        dead[::k] = False
        dead[-1] = k > 1
        st["cumul"][dead], st["has_eos"][dead] = NINF, 1
        steps[0][0][rng.random(N) < 0.3] = NINF                # rows of -inf candidates
        steps[0][2][rng.random(N) < 0.3] = NINF
    elif kind == "nan":
        steps[0][0][rng.random((N, k)) < 0.3] = np.nan
        steps[0][2][rng.random(N) < 0.5] = np.nan
        steps[1][0][:, 0] = np.nan
    elif kind == "close_one":                                 # image 0 closes by the bound at once; the others when their
        n_steps, early = 3, True                              # pools fill at the third step (early stopping)
        _prefill(pool, rng, 0, k, scale, T, score_like=-0.001)
        for s in (0, 1):
            steps[s][2][k:] = F(-30.0)                         # no EOS among the first k of the other images
        steps[2][2][:] = F(-0.001)
        steps[2][0][:] -= F(40.0)                             # every row's EOS ahead of every word
        if T < 5:
            n_steps = 1
    elif kind == "last":
        for b in range(n_img):
            _prefill(pool, rng, b, min(b, k), scale, T)
    elif kind == "min_length":
        min_words = 2
        steps[0][2][:] = F(-0.001)                            # EOS would be every row's best
    elif kind == "empty":                                     # one live row with one finite candidate: k - 1 EMPTY rows
        st["cumul"][:] = NINF
        st["has_eos"][:] = 1
        st["cumul"][::k], st["has_eos"][::k] = F(-1.0), 0
        steps[0][0][:, 1:] = NINF
    elif kind == "seed":
        steps[0][2][:] = steps[0][0][:, min(1, k - 1)]        # EOS ties with a word of row 0
    return dict(st=st, pool=pool, scale=scale, min_words=min_words, early=early, steps=steps[:n_steps])


def logp_rows(elp, eos: int = EOS) -> np.ndarray:
    """Log-prob rows [N, V] whose only defined column is EOS (the step reads nothing else of them): NaN elsewhere."""
    lp = np.full((len(elp), V), np.nan, F)
    lp[:, eos] = elp
    return lp
