"""Plain data and a float64 model for odic_dynexp_step under beam re-ordering: ancestry plans, the oracle on materialised
histories, a step-by-step model of the cached form, and the cases test_dynexp_step_host.py / test_dynexp_step_gpu.py run.

Two independent references:

  * oracle_rows: the history of every slot is MATERIALISED (the rows a search that copied its caches would hold) and run
    through oracle/expansionnet_ref.py::dynamic_expansion in float64, every position valid, causal mask; the last row is
    what the step must add to y.  Nothing of the kernel's caching or re-association is imitated.
  * step_model: the contract of include/odic_hip.h (odic_dynexp_step) transcribed in float64: caches indexed [pos][slot],
    the history gathered through `anc`, caches written for row_valid = 0 rows as well, those rows contributing 0.  Written
    from the header text, not from the kernel: it forms the class vectors of every position and sums them with the backward
    weights, as the reference does.

Not a conftest and not a test module: import it (`import dynexp_step_model as M`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

SENTINEL = 2 ** 30          # anc entries at positions >= t: the contract says they are not read
NAMES = ["cond_embed", "key_linear", "class_a_embed", "class_b_embed", "selector_embed"]     # column blocks of `lin`
CACHES = ("cond", "key", "va", "vb", "wfa", "wfb", "qk")                                      # argument order of the step


# ------------------------------------------------------------------------------------------------------ ancestry
@dataclass
class Plan:
    n_img: int
    beams: int
    T: int
    par: np.ndarray          # [T-1, N]  par[t][n]: the slot at step t that slot n at step t+1 descends from (same image)
    anc: np.ndarray          # [T, N, T] anc[t]: the table the step at position t reads; entries at positions >= t = SENTINEL
    valid: np.ndarray        # [T, N]    row_valid of step t
    finished: list = field(default_factory=list)     # (t, slot): the slot whose child is the first padded row of a beam

    @property
    def N(self) -> int:
        return self.n_img * self.beams


def _derangement(rng, k: int) -> np.ndarray:
    while True:
        p = rng.permutation(k)
        if not (p == np.arange(k)).any():
            return p


def ancestry_plan(n_img: int, beams: int, T: int, seed: int) -> Plan:
    """T - 1 re-orderings of n_img x beams slots, the update of odic_beam_step (tests/group_beam_model.py):
    anc'[n, :t] = anc[par, :t]; anc'[n, t] = par, par a slot of the same image.

    The steps mix the identity, pure permutations (mostly without a fixed point), duplication (two children of one parent
    while another beam dies) and collapse (every beam of the image descends from one slot; the first step of a search is
    one, onto the image's first row).  A beam finishes at T//4 in the first image and at 3T//4 in the last one: the child of
    the finishing slot has row_valid = 0 and so has every descendant of it.  A beam only finishes while its image has two
    live ones, and a duplicated or collapsed-onto parent is a live one, so every image keeps a beam that never finishes."""
    assert beams >= 2 and T >= 8
    rng = np.random.default_rng(seed)
    N = n_img * beams
    par = np.zeros((T - 1, N), np.int32)
    anc = np.full((T, N, T), SENTINEL, np.int32)
    valid = np.ones((T, N), np.int32)
    finished = []
    for t in range(T - 1):
        for b in range(n_img):
            base = b * beams
            live = np.flatnonzero(valid[t, base:base + beams])
            fin = -1
            finishing = (t == T // 4 and b == 0) or (t == (3 * T) // 4 and b == n_img - 1)
            if t == 0:
                p = np.zeros(beams, np.int64)
            elif finishing:
                p = _derangement(rng, beams)
                if len(live) >= 2:
                    fin = int(rng.choice(live))
                    finished.append((t, base + fin))
            elif t == (11 * T) // 20 + 2 * b:
                p = np.full(beams, rng.choice(live), np.int64)
            elif t % 7 == 3 and (beams > 2 or t % 21 == 3):     # (two beams: a duplication is a collapse; keep them rare)
                p = rng.permutation(beams)
                a = int(rng.choice(live))
                c = int(rng.choice([r for r in range(beams) if r != a]))
                p[p == c] = a
            elif t == 1 or t % 11 == 5:
                p = np.arange(beams)
            else:
                p = _derangement(rng, beams) if rng.random() < 0.85 else rng.permutation(beams)
            for r in range(beams):
                n, q = base + r, base + int(p[r])
                par[t, n] = q
                anc[t + 1, n, :t] = anc[t, q, :t]
                anc[t + 1, n, t] = q
                valid[t + 1, n] = 1 if (valid[t, q] and int(p[r]) != fin) else 0
    return Plan(n_img, beams, T, par, anc, valid, finished)


def step_kind(plan: Plan, t: int, b: int) -> str:
    """What re-ordering step t (0 <= t < T-1) is for image b, read off the parent map alone."""
    k = plan.beams
    p = plan.par[t, b * k:(b + 1) * k] - b * k
    if (p == np.arange(k)).all():
        return "identity"
    children = np.bincount(p, minlength=k)
    if (children == 1).all():
        return "permutation"
    return "collapse" if children.max() == k else "duplication"


def history(x, anc_t, n: int, t: int):
    """The input sequence slot n has consumed up to and including step t: x[anc_t[n][j], j] for j < t, then x[n, t].
    x: [N, T, ...] indexed [slot][position]."""
    return torch.stack([x[int(anc_t[n][j]), j] for j in range(t)] + [x[n, t]])


# ------------------------------------------------------------------------------------------------------ references
def weights(d: int, E: int, seed: int) -> dict:
    """A DynamicExpansionBlock's parameters (float32), scaled as in test_dynexp_step_matches_full_recompute."""
    def rnd(*shape, s, scale):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + s)) * scale
    sd = {}
    for i, nm in enumerate(NAMES):
        sd[f"p.{nm}.weight"] = rnd(d, d, s=10 + i, scale=d ** -0.5)
        sd[f"p.{nm}.bias"] = rnd(d, s=20 + i, scale=0.1)
    sd["p.query_exp_vectors.weight"] = rnd(E, d, s=30, scale=0.3)
    sd["p.bias_exp_vectors.weight"] = rnd(E, d, s=31, scale=0.3)
    return sd


def linear_rows(sd64: dict, x64):
    """cond | key | class_a | class_b | selector pre-activation of every row of x64, the layout the step reads (float64)."""
    Wcat = torch.cat([sd64[f"p.{nm}.weight"] for nm in NAMES], 0)
    bcat = torch.cat([sd64[f"p.{nm}.bias"] for nm in NAMES], 0)
    return x64 @ Wcat.T + bcat


def oracle_rows(sd64: dict, x64, plan: Plan, t: int, dtype=torch.float64):
    """[N, d]: the oracle's DynamicExpansionBlock on the N materialised histories of length t + 1, last row of each.
    `dtype` float32 evaluates the same oracle in single precision (to measure what fp32 alone costs on a case)."""
    from oracle import expansionnet_ref as R
    N = plan.N
    X = torch.stack([history(x64, plan.anc[t], n, t) for n in range(N)]).to(dtype)
    causal = torch.tril(torch.ones(t + 1, t + 1, dtype=dtype))[None].expand(N, -1, -1)
    sd = {k: v.to(dtype) for k, v in sd64.items()}
    E = sd["p.query_exp_vectors.weight"].shape[0]
    return R.dynamic_expansion(sd, "p", X, E, causal)[:, -1]


def new_caches(T: int, N: int, d: int, E: int, dtype=torch.float64, device="cpu") -> dict:
    """The seven caches of include/odic_hip.h, every entry NaN: nothing may be read that no earlier step wrote."""
    shapes = dict(cond=(T, N, d), key=(T, N, d), va=(T, N, d), vb=(T, N, d), wfa=(T, N, T, E), wfb=(T, N, T, E), qk=(T, N, E))
    return {k: torch.full(shapes[k], float("nan"), dtype=dtype, device=device) for k in CACHES}


def step_model(lin, qexp, bexp, caches: dict, anc_t, row_valid, t: int, y_in, eps: float = 1e-9):
    """One odic_dynexp_step at position t in float64.  lin [N, 5d]; caches as new_caches() (updated in place, at position t
    only); anc_t [N, T]; row_valid [N]; y_in [N, d].  Returns y [N, d]."""
    N, d = y_in.shape
    E = qexp.shape[0]
    y = y_in.clone()
    for n in range(N):
        cond_t, key_t, va_t, vb_t, sel = (lin[n, i * d:(i + 1) * d] for i in range(5))
        caches["cond"][t, n], caches["key"][t, n], caches["va"][t, n], caches["vb"][t, n] = cond_t, key_t, va_t, vb_t
        caches["qk"][t, n] = qexp @ key_t
        slot = [int(anc_t[n][j]) for j in range(t)] + [n]               # position `pos` itself is always slot n
        pos = list(range(t + 1))
        cond, key, va, vb, qk = (caches[k][pos, slot] for k in ("cond", "key", "va", "vb", "qk"))     # [t+1, ...]
        # forward weights of this position's E queries over its keys 0..t (:165-176) -> cache
        z_fw = (qk + (key @ cond_t)[:, None]) / math.sqrt(d)            # [i, e] = (qexp[e] + cond_t)·key_i / sqrt(d)
        pf, nf = torch.relu(z_fw), torch.relu(-z_fw)
        caches["wfa"][t, n, :t + 1] = pf / (pf.sum(0, keepdim=True) + eps)
        caches["wfb"][t, n, :t + 1] = nf / (nf.sum(0, keepdim=True) + eps)
        # class vectors of every position j of the history, from the forward weights cached when j was processed
        A = torch.empty(t + 1, E, d, dtype=lin.dtype)
        B = torch.empty(t + 1, E, d, dtype=lin.dtype)
        for j in pos:
            A[j] = caches["wfa"][j, slot[j], :j + 1].T @ va[:j + 1] + bexp + cond[j]
            B[j] = caches["wfb"][j, slot[j], :j + 1].T @ vb[:j + 1] + bexp + cond[j]
        # backward weights of the newest key over all (j, e) (:183-200)
        z_bw = ((qexp[None] + cond[:, None]) @ key_t) / math.sqrt(d)    # [j, e]
        pb, nb = torch.relu(z_bw), torch.relu(-z_bw)
        pb, nb = pb / (pb.sum() + eps), nb / (nb.sum() + eps)
        out_a = torch.einsum("je,jec->c", pb, A)
        out_b = torch.einsum("je,jec->c", nb, B)
        if int(row_valid[n]):
            sg = torch.sigmoid(sel)
            y[n] = y_in[n] + sg * out_a + (1 - sg) * out_b
    return y


# ------------------------------------------------------------------------------------------------------ cases
def checked_steps(T: int) -> list:
    """The steps at which the oracle is evaluated: all of them up to T = 40; beyond, t <= 3, both sides of the lane-split
    boundaries (t + 1 in 31..34 and 63..66), the last two and every fifth in between.  (The cap bounds the CPU oracle's cost.)"""
    if T <= 40:
        return list(range(T))
    s = set(range(4)) | {T - 2, T - 1} | set(range(0, T, 5))
    s |= {tp1 - 1 for tp1 in (31, 32, 33, 34, 63, 64, 65, 66) if tp1 <= T}
    return sorted(s)


@dataclass(frozen=True)
class Case:
    name: str
    n_img: int
    beams: int
    T: int
    d: int
    E: int
    seed: int
    # what the case is there to reach (test_dynexp_step_host.py checks every claim against the kernel's formulas)
    lanes: tuple = (32,)             # lanes per key position in the ca / cb sums, at checked steps
    boundaries: tuple = ()           # t + 1 values on both sides of a lane-split boundary, all checked
    item_trips: int = 1              # trips of the dot-product item loop (E + 2t + 1 items over 64 groups)
    weight_trips: int = 1            # trips of the strided loops over (t+1)·E
    channel_passes: int = 1          # passes of the phase-2 channel loop (512 channels each)
    last_pass_channels: int = 0      # live channels of the last pass
    rtol: float = 5e-5               # of the output scale: the figure of test_dynexp_step_matches_full_recompute

    @property
    def N(self) -> int:
        return self.n_img * self.beams

    @property
    def steps(self) -> list:
        return checked_steps(self.T)

    def plan(self) -> Plan:
        return ancestry_plan(self.n_img, self.beams, self.T, self.seed)


# (n_img x beams, T, d, E): the smallest shapes that reach the branch named.  Measured on an MI355X, worst step of each
# case as a fraction of the output scale: 1.3e-7, 2.7e-7, 1.0e-6, 2.0e-7, 1.9e-7, 3.0e-7 (the same oracle evaluated in
# float32 on the CPU: 3e-7 .. 1.5e-6) — every case holds the 5e-5 of the existing tests.
CASES = [
    Case("lane_splits", 2, 3, 128, 64, 4, seed=1, lanes=(32, 16, 8), boundaries=(32, 33, 64, 65), item_trips=5,
         last_pass_channels=64),
    Case("largest_lds", 2, 2, 128, 64, 32, seed=2, lanes=(32, 16, 8), boundaries=(32, 33, 64, 65), item_trips=5,
         weight_trips=4, last_pass_channels=64),
    Case("half_exact", 1, 5, 40, 512, 32, seed=3, lanes=(32, 16), boundaries=(32, 33), item_trips=2, weight_trips=2,
         last_pass_channels=512),
    Case("shipped", 2, 2, 74, 512, 16, seed=4, lanes=(32, 16, 8), boundaries=(32, 33, 64, 65), item_trips=3,
         weight_trips=2, last_pass_channels=512),
    Case("partial_pass", 1, 3, 12, 576, 8, seed=5, channel_passes=2, last_pass_channels=64),
    Case("two_passes", 1, 2, 20, 1024, 4, seed=6, channel_passes=2, last_pass_channels=512),
]
REFUSED = dict(N=2, T=128, d=1024, E=32)         # 192 bytes over the 64 KB of LDS a block may ask for: ODIC_EINVAL

#: the two small cases on which step_model is held against oracle_rows without a GPU
MODEL_CASES = [Case("model_e4", 2, 3, 12, 64, 4, seed=11), Case("model_e8", 1, 4, 10, 64, 8, seed=12)]


def inputs(case: Case):
    """(sd float32, x float32 [N, T, d] indexed [slot][position], y_in float32 [T, N, d]) of a case."""
    sd = weights(case.d, case.E, 100 * case.seed)
    g = torch.Generator().manual_seed(1000 + case.seed)
    x = torch.randn(case.N, case.T, case.d, generator=g)
    y_in = torch.randn(case.T, case.N, case.d, generator=g)
    return sd, x, y_in
