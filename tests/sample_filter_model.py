"""A model of odic_logsoftmax_sample_filtered (include/odic_hip.h) in numpy, and the rows and filters its tests use: the host
tests check the model and that every row is `clear`, the GPU tests compare the kernel with it (no tests here).

  noise     Philox4x32-10 in integer arithmetic, exact, so the device's bits; u from them in fp32 as the device forms it
            (clamped below 1), the Gumbel noise g = -log(-log(u)) in float64.
  filter    in float64 on the fp32 z = x·inv_temperature: rank (larger first, ties to the lower index), K = the first top_k,
            c(v) = mass of K ranked before v / mass of K, m = #{v in K: c(v) < top_p} (top_p = 1: m = |K|),
            S = the first max(m, k) in rank order.
  clear     no c(v) lies within 1e-4·top_p of top_p, ten times the contract's band: on such a row `kept` must equal m.
"""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------- noise
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counters and keys (arrays or scalars of values < 2^32) → the four output words, uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # < 2^64: exact
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def noise_bits(seed: int, rows, V: int, pos: int) -> np.ndarray:
    """The 32 bits behind the noise of word v of row n: output v % 4 of counter (n, v / 4, pos, 0) under `seed` → [R, V]."""
    rows = np.asarray(rows, dtype=np.uint64)
    g4 = np.arange((V + 3) // 4, dtype=np.uint64)
    out = philox4x32_10(rows[:, None], g4[None, :], pos, 0, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(out, axis=-1).reshape(len(rows), -1)[:, :V]


def uniform_from_bits(b: np.ndarray) -> np.ndarray:
    """fp32, as the device: ((b >> 8) + 0.5)·2^-24, which rounds to 1 for b >> 8 = 0xFFFFFF, clamped to the float below 1."""
    u = ((b >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24))


def gumbel(b: np.ndarray) -> np.ndarray:
    return -np.log(-np.log(uniform_from_bits(b).astype(np.float64)))


# ------------------------------------------------------------------------------------------------------------ filter
def inv_temperature(t: float) -> np.float32:
    return np.float32(1.0 / float(t))


def scaled(x, temperature: float) -> np.ndarray:
    """z = x·inv_temperature in fp32, one rounding."""
    return (np.asarray(x, dtype=np.float32) * inv_temperature(temperature)).astype(np.float32)


def ranked(z: np.ndarray):
    """order [R, V]: the words of every row by (z descending, index ascending), and their masses exp(z - max z) in that
    order, float64 (a masked word: 0)."""
    z = np.asarray(z, dtype=np.float64)
    order = np.argsort(-z, axis=-1, kind="stable")
    zs = np.take_along_axis(z, order, -1)
    with np.errstate(invalid="ignore"):
        w = np.exp(zs - zs[..., :1])
    return order, w


def filter_ref(z: np.ndarray, top_k: int, top_p: float, k: int, rank=None):
    """fp32 z [R, V] → (order [R, V], m [R], c [R, kk]): m the size of top-k ∩ nucleus, c(v) of the words of K in rank order.
    The draw set of row r is order[r, :max(m[r], k)]."""
    order, w = rank if rank is not None else ranked(z)
    V = order.shape[-1]
    kk = V if top_k == 0 or top_k >= V else top_k
    wk = w[:, :kk]
    c = (np.cumsum(wk, -1) - wk) / wk.sum(-1, keepdims=True)
    m = np.full(len(order), kk) if top_p == 1.0 else (c < np.float32(top_p).astype(np.float64)).sum(-1)
    return order, m, c


def clear(c: np.ndarray, top_p: float) -> np.ndarray:
    """Per row: no c(v) within 1e-4·top_p of top_p (top_p = 1 is off: always clear)."""
    if top_p == 1.0:
        return np.ones(len(c), dtype=bool)
    p = float(np.float32(top_p))
    return (np.abs(c - p) > 1e-4 * p).all(-1)


def draw_sets(order, m, k):
    return [set(order[r, :max(int(m[r]), k)].tolist()) for r in range(len(order))]


# --------------------------------------------------------------------------------------------------- rows and filters
VS = (16, 67, 1024, 1025, 4099, 10000, 20000)       # 20000: past the 16384 words a block holds in registers, the re-read path
KS = (1, 3, 16)
SHAPES = [(V, k) for V in VS for k in KS if k <= V and (V <= 10000 or k != 3)]
TOP_KS = (1, 5, 64, 0)                     # 0 stands for V (off)
TOP_PS = (0.1, 0.5, 0.9, 0.999)
TEMPERATURES = (0.5, 1.0, 2.0)
KEPT_FILTERS = [(t, tk, tp) for t in TEMPERATURES for tk in TOP_KS for tp in TOP_PS]
DRAW_FILTERS = [(0.5, 5, 0.9), (1.0, 1, 0.5), (2.0, 64, 0.999), (1.0, 0, 0.5), (2.0, 5, 1.0), (0.5, 0, 0.1)]
SEED, POS = 90417, 5


def _gen(*key) -> torch.Generator:
    seed = 0xF117
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def crossing_words(V: int):
    """Words on both sides of the wave (64) and the thread-stride (1024) boundaries, as far as the row has them."""
    return sorted({i for i in (3, 62, 63, 64, 65, 127, 128, 1022, 1023, 1024, 1025, 2047, 2048, V - 1) if 0 <= i < V})


HEAD, TAIL = 24, -60.0


def _family(name: str, V: int, salt: int) -> torch.Tensor:
    """One row: at most HEAD live words at random places (`crossing`: at crossing_words), every other word TAIL below
    them — finite, ranked and counted, but of no visible mass, so that c(v) moves in steps a filter boundary can clear."""
    g = _gen(V, sum(map(ord, name)), salt)
    n = min(HEAD, V)
    live = torch.randperm(V, generator=g)[:n]
    x = torch.randn(V, generator=g) * 3.0 + TAIL
    h = torch.randn(n, generator=g) * 3.0
    if name == "peaked":
        h[0] = h.max() + 60.0
    elif name == "flat":                   # all equal but one: the boundary falls inside the tie, the lower indices win
        h = torch.zeros(n)
        h[1] = 0.2 + 0.01 * salt
    elif name == "levels":                 # few distinct values: ties straddle the top_k cut
        lv = torch.randint(0, 4, (n,), generator=g)
        lv[:min(7, n)] = 3                 # at least 7 words on the top level: the top_k = 5 cut falls inside it
        h = lv.float() * (0.5 + 0.01 * salt)
    elif name.startswith("crossing"):
        cw = crossing_words(V)
        live, h = torch.tensor(cw), h[:len(cw)]
        if name == "crossing_tie":
            h = torch.full((len(cw),), 1.5)
            h[0] = 1.7 + 0.01 * salt
    x[live] = h
    if name.startswith("masked"):
        dead = torch.randperm(V, generator=g)[:min(30, V // 3)]
        x[dead] = float("-inf")
    if name.startswith("offset"):
        x = x + float(name[len("offset"):])
    return x.float()


FAMILIES = ("random_a", "random_b", "peaked", "flat", "levels", "masked_a", "masked_b", "crossing", "crossing_tie",
            "offset+80", "offset-80")
REPS = 3                                   # rows per family: other live words, tie positions and wave placements
_ROWS = {}


def rows(V: int):
    """(names, X fp32 [R, V]): the row families of the `kept` and draw tests, REPS rows of each (`flat`, `flat.1`, `flat.2`).
    A family's rows are the first of its salts that are clear under every filter of KEPT_FILTERS
    (test_sample_filter_host.py asserts that all are)."""
    if V not in _ROWS:
        names, out = [], []
        for name in FAMILIES:
            found = 0
            for salt in range(200):
                x = _family(name, V, salt)
                if all_clear(x[None].numpy()):
                    names.append(name if found == 0 else f"{name}.{found}")
                    out.append(x)
                    found += 1
                    if found == REPS:
                        break
            else:
                raise AssertionError(f"fewer than {REPS} clear {name} rows at V={V}")
        _ROWS[V] = (names, torch.stack(out))
    return list(_ROWS[V][0]), _ROWS[V][1]


def all_clear(X: np.ndarray) -> bool:
    for t in TEMPERATURES:
        z = scaled(X, t)
        rk = ranked(z)
        for tk in TOP_KS:
            for tp in TOP_PS:
                if not clear(filter_ref(z, tk, tp, 1, rk)[2], tp).all():
                    return False
    return True


# Dense rows, the production case: plain randn·3 rows whose nucleus holds hundreds of words spread over every wave.  Some
# c(v) always lies near top_p on such a row, so `kept` is held to the contract's band instead: m at top_p·(1 -+ 1e-5).
DENSE_VS, DENSE_N, DENSE_K, BAND = (10000, 20000), 24, 3, 1e-5
DENSE_FILTERS = [(1.0, 0, 0.9), (0.7, 0, 0.95), (2.0, 0, 0.5), (1.0, 64, 0.9), (0.5, 0, 0.999), (1.5, 500, 0.9), (3.0, 0, 0.999)]


def dense_rows(V: int) -> torch.Tensor:
    return (torch.randn(DENSE_N, V, generator=_gen(V, 99)) * 3.0).float()


def kept_band(c: np.ndarray, top_p: float):
    """(m_lo, m_hi) per row: the words the band obliges the kernel to keep, and the most it may keep."""
    p = float(np.float32(top_p))
    return (c < p * (1.0 - BAND)).sum(-1), (c <= p * (1.0 + BAND)).sum(-1)


FREQ_V, FREQ_N = 12, 40000
FREQ_FILTERS = [(0.7, 5, 1.0), (0.7, 5, 0.8)]


def freq_row() -> torch.Tensor:
    return (torch.randn(FREQ_V, generator=_gen(7, 7)) * 1.3).float()


# The u = 1 pattern: Philox4x32-10 under HIT_SEED at counter (HIT_ROW, HIT_WORD / 4, HIT_POS, 0) gives a word HIT_WORD % 4
# whose upper 24 bits are all ones (found once by scanning positions with philox4x32_10; test_sample_filter_host.py
# checks it).  Before the clamp its noise was +inf.
HIT_SEED, HIT_ROW, HIT_POS, HIT_WORD = 90417, 1, 48894, 13
HIT_V, HIT_ROWS = 16, 4
