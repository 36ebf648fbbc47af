"""odic_dynexp_fill_caches and odic_beam_reset_prefix on the GPU (`-m gpu`).

fill: the want is odic_dynexp_step itself, run P times on the same `lin` rows (anc[n][j] = n) and read at the two slots
the fill writes.  Every cache the fill writes sits in a guarded, poisoned buffer (tests/guards.py): what lies outside
positions < P, entries i <= t and slots 0 and 3 must still be poison afterwards.
  exact inputs (multiples of 1/8 in [-1, 1], d = 64): every dot product is exact in fp32 in any order, so cond / key / va /
  vb / qk must be BIT-EQUAL; wfa / wfb within (P + 4)·2^-23 relative (two orderings of a sum of at most P non-negative
  terms, one reciprocal, one product).
  random normal inputs (d = 512, E = 16, P = 19): 5e-5 of the output scale, the project's bound for this block
  (test_dynexp_seq_matches_the_oracle), against the step kernel and against the float64 model of tests/prefix_model.py.
reset: every state array equals tests/prefix_model.py, the -inf pattern of cumul included, for group_beams in
{beams, 1, 2}; guards intact; refused shapes write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import guards
import prefix_model as PM

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
F32 = torch.float32
CACHES = ("cond", "key", "va", "vb", "wfa", "wfb", "qk")
N_SEQ, RPI, N_CACHE = 2, 3, 6
SLOTS = [i * RPI for i in range(N_SEQ)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


def cache_widths(T, d, E):
    return dict(cond=d, key=d, va=d, vb=d, wfa=T * E, wfb=T * E, qk=E)


def guarded_caches(T, d, E):
    """One guarded buffer per cache, [T·N_CACHE rows, width]: all poison."""
    return {k: guards.guarded(T * N_CACHE, w, w, F32, DEV) for k, w in cache_widths(T, d, E).items()}


def step_caches(ops, lin, qexp, P, T, d, E):
    """The want: P calls of odic_dynexp_step from NaN caches.  lin [N_SEQ, P, 5d]; sequence i is row i·RPI of every step."""
    N = N_CACHE
    caches = {k: torch.full((T, N, w), float("nan"), dtype=F32, device=DEV) for k, w in cache_widths(T, d, E).items()}
    bexp = torch.zeros(E, d, dtype=F32, device=DEV)
    anc = torch.arange(N, dtype=torch.int32, device=DEV)[:, None].expand(N, T).contiguous()
    valid = torch.ones(N, dtype=torch.int32, device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    y_in, y = torch.zeros(N, d, dtype=F32, device=DEV), torch.empty(N, d, dtype=F32, device=DEV)
    for t in range(P):
        rows = torch.zeros(N, 5 * d, dtype=F32, device=DEV)
        rows[SLOTS] = lin[:, t]
        pos.fill_(t)
        ops.dynexp_step(rows, 5 * d, qexp, bexp, *[caches[k] for k in CACHES], anc, valid, pos, y_in, d, y, d, N, T, d, E)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in caches.items()}


def run_fill(ops, lin, qexp, P, T, d, E):
    g = guarded_caches(T, d, E)
    ops.dynexp_fill_caches(lin.view(N_SEQ * P, 5 * d), 5 * d, qexp, {k: g[k].t for k in CACHES}, N_SEQ, P, RPI, N_CACHE,
                           T, d, E)
    torch.cuda.synchronize()
    return g


def written_mask(k, P, T, d, E):
    """Boolean [T, N_CACHE, width]: the elements the header says are written."""
    m = np.zeros((T, N_CACHE, cache_widths(T, d, E)[k]), bool)
    for t in range(P):
        for s in SLOTS:
            m[t, s, :(t + 1) * E if k in ("wfa", "wfb") else None] = True
    return m


def check_containment(g, P, T, d, E):
    for k in CACHES:
        g[k].assert_untouched(what=k)
        bits = g[k].t.cpu().view(torch.int32).numpy().reshape(T, N_CACHE, -1)
        m = written_mask(k, P, T, d, E)
        stray = np.argwhere((bits != -1) & ~m)
        assert stray.size == 0, f"{k}: element (t, slot, column) = {stray[0].tolist()} was written and is not the fill's"
        missing = np.argwhere((bits == -1) & m)
        assert missing.size == 0, f"{k}: element (t, slot, column) = {missing[0].tolist()} still holds the poison"


EXACT = [(E, T, P) for E in (4, 16) for T in (12, 40) for P in (1, 2, 5, 11, 33, 38) if P < T]


@pytest.mark.parametrize("E,T,P", EXACT, ids=[f"E{E}-T{T}-P{P}" for E, T, P in EXACT])
def test_fill_equals_p_steps_on_exact_inputs(ops, E, T, P):
    d = 64
    gen = torch.Generator().manual_seed(1000 * E + 10 * T + P)
    lin = (torch.randint(-8, 9, (N_SEQ, P, 5 * d), generator=gen).float() / 8).to(DEV)
    qexp = (torch.randint(-8, 9, (E, d), generator=gen).float() / 8).to(DEV)
    want = step_caches(ops, lin, qexp, P, T, d, E)
    g = run_fill(ops, lin, qexp, P, T, d, E)
    check_containment(g, P, T, d, E)
    tol = (P + 4) * 2.0 ** -23
    worst = 0.0
    for k in CACHES:
        got = g[k].t.cpu().view(T, N_CACHE, -1)
        w = want[k].view(T, N_CACHE, -1)
        m = torch.from_numpy(written_mask(k, P, T, d, E))
        a, b = got[m], w[m]
        assert bool(torch.isfinite(b).all()), f"{k}: the step kernel left a NaN where the fill writes"
        if k in ("wfa", "wfb"):
            rel = ((a.double() - b.double()).abs() / b.double().abs().clamp_min(1e-300))
            rel[(a == b)] = 0.0
            worst = max(worst, rel.max().item())
            assert rel.max().item() <= tol, f"{k}: relative error {rel.max().item():.3e} > (P + 4)·2^-23 = {tol:.3e}"
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{k} is not bit-equal to the step kernel's"
    print(f"E={E} T={T} P={P}: wfa/wfb max relative error {worst:.3e} (bound {tol:.3e})")


def test_fill_on_random_inputs_at_the_shipped_width(ops):
    d, E, T, P = 512, 16, 24, 19
    gen = torch.Generator().manual_seed(5)
    lin = torch.randn(N_SEQ, P, 5 * d, generator=gen).to(DEV)
    qexp = torch.randn(E, d, generator=gen).to(DEV)
    want = step_caches(ops, lin, qexp, P, T, d, E)
    g = run_fill(ops, lin, qexp, P, T, d, E)
    check_containment(g, P, T, d, E)
    model = [PM.fill_caches(lin[i].cpu().numpy(), qexp.cpu().numpy(), P, d) for i in range(N_SEQ)]
    for k in CACHES:
        got = g[k].t.cpu().view(T, N_CACHE, -1)
        w = want[k].view(T, N_CACHE, -1)
        m = torch.from_numpy(written_mask(k, P, T, d, E))
        scale = w[m].abs().max().item()
        err = (got[m].double() - w[m].double()).abs().max().item()
        merr = 0.0
        for i, s in enumerate(SLOTS):
            ref = torch.from_numpy(model[i][k]).reshape(P, -1)                 # wfa: [P, P·E], zero where i > t
            mm = m[:P, s, :ref.shape[1]]
            merr = max(merr, (got[:P, s, :ref.shape[1]].double() - ref)[mm].abs().max().item())
        print(f"{k}: max err vs step {err:.3e}, vs float64 model {merr:.3e}, scale {scale:.3e}")
        assert err <= 5e-5 * scale and merr <= 5e-5 * scale, (k, err, merr, scale)
        if k in ("cond", "key", "va", "vb"):
            assert torch.equal(got[m], w[m]), f"{k}: a copied row differs"


def test_fill_refuses_bad_shapes_and_writes_nothing(ops):
    d, E, T = 64, 16, 12
    lin = torch.zeros(N_SEQ * 12, 5 * d, device=DEV)
    qexp = torch.zeros(E, d, device=DEV)
    g = guarded_caches(T, d, E)
    c = {k: g[k].t for k in CACHES}
    for kw in (dict(P=12), dict(P=0), dict(rpi=6), dict(E=12), dict(n_seq=3)):
        a = dict(n_seq=N_SEQ, P=5, rpi=RPI, E=E)
        a.update(kw)
        with pytest.raises(RuntimeError, match="EINVAL"):
            ops.dynexp_fill_caches(lin, 5 * d, qexp, c, a["n_seq"], a["P"], a["rpi"], N_CACHE, T, d, a["E"])
    torch.cuda.synchronize()
    for k in CACHES:
        g[k].assert_all_poison(what=k)


# ------------------------------------------------------------------------------------------------- odic_beam_reset_prefix
N_IMG, R, T_ST, D_EMB, V, SOS = 3, 6, 12, 64, 50, 3
I32, I64 = torch.int32, torch.int64


class DeviceState:
    def __init__(self, ops):
        from on_device_image_captioning_amd import _hip
        N = N_IMG * R
        shapes = dict(tokens=(N, T_ST, I64), logprobs=(N, T_ST, F32), anc=(N, T_ST, I32), cumul=(1, N, F32),
                      n_elem=(1, N, I32), has_eos=(1, N, I32), row_valid=(1, N, I32), next_tok=(1, N, I64),
                      pos=(1, 1, I32), done=(1, 1, I32), ctr=(1, 1, I32))
        self.g = {k: guards.guarded(r, c, c, dt, DEV) for k, (r, c, dt) in shapes.items()}
        self.state = _hip.BeamState(*(self.g[k].data_ptr() for k in shapes))
        gen = torch.Generator().manual_seed(3)
        self.embed = torch.randn(V, D_EMB, generator=gen).to(DEV)
        self.pos_table = torch.randn(T_ST, D_EMB, generator=gen).to(DEV)
        self.y = guards.guarded(N, D_EMB, D_EMB + 8, F32, DEV)
        self.emb = ops.embed_args(self.embed, self.pos_table, self.y.t, D_EMB + 8, D_EMB, 8.0)

    def everything(self):
        return list(self.g.items()) + [("y", self.y)]


@pytest.mark.parametrize("P", [1, 4, 10])
@pytest.mark.parametrize("gb", [R, 1, 2])
def test_reset_prefix_equals_the_model(ops, P, gb):
    dev = DeviceState(ops)
    gen = torch.Generator().manual_seed(10 * P + gb)
    prefix = torch.randint(4, V, (N_IMG, P), generator=gen)
    plogp = -torch.rand(N_IMG, P, generator=gen) * 6
    ops.beam_reset_prefix(dev.state, prefix.to(DEV), plogp.to(DEV), N_IMG, R, gb, T_ST, SOS, emb=dev.emb)
    torch.cuda.synchronize()
    want = PM.reset_state(N_IMG, R, T_ST, SOS, prefix.numpy(), plogp.numpy(), gb, fill=-1)
    got = {k: g.t.cpu().numpy() for k, g in dev.g.items()}
    N = N_IMG * R
    assert np.array_equal(got["tokens"], want["tokens"].reshape(N, T_ST))                  # (poison reads as -1)
    assert np.array_equal(got["logprobs"][:, :P + 1], want["logprobs"].reshape(N, T_ST)[:, :P + 1])
    assert (got["logprobs"][:, P + 1:].view(np.int32) == -1).all(), "a log-prob behind the prefix was written"
    assert np.array_equal(got["anc"], want["anc"])
    for k in ("cumul", "n_elem", "has_eos", "row_valid", "next_tok"):
        assert np.array_equal(got[k].reshape(-1), want[k]), k
    inf = np.isneginf(got["cumul"].reshape(N_IMG, R))
    assert inf.tolist() == [[r % gb != 0 for r in range(R)]] * N_IMG
    assert (int(got["pos"][0, 0]), int(got["done"][0, 0]), int(got["ctr"][0, 0])) == (P, 0, 0)
    y = PM.reset_embedding(dev.embed.cpu().numpy(), dev.pos_table.cpu().numpy(), 8.0, prefix.numpy(), R)
    assert np.allclose(dev.y.t[:, :D_EMB].cpu().numpy(), y, rtol=0, atol=2e-6 * np.abs(y).max())    # (fma or two roundings)
    for k, g in dev.everything():
        g.assert_untouched(what=k)


def test_reset_prefix_refuses_bad_shapes_and_writes_nothing(ops):
    dev = DeviceState(ops)
    prefix = torch.full((N_IMG, 11), 5, dtype=I64, device=DEV)
    plogp = torch.zeros(N_IMG, 11, device=DEV)
    for P, gb in ((11, R), (4, 4), (4, 0)):                 # P > T - 2; beams % group_beams != 0
        with pytest.raises(RuntimeError, match="EINVAL"):
            ops.beam_reset_prefix(dev.state, prefix[:, :P].contiguous(), plogp[:, :P].contiguous(), N_IMG, R, gb, T_ST, SOS,
                                  emb=dev.emb)
    torch.cuda.synchronize()
    for k, g in dev.everything():
        g.assert_all_poison(what=k)
