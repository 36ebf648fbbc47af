"""A float32 numpy model of what a search behind a given prefix starts from:

  * reset_state — what odic_beam_reset_prefix leaves, on the state dict of tests/group_beam_model.py;
  * fill_caches — what odic_dynexp_fill_caches writes, from the definitions in include/odic_hip.h: for a sequence's
    positions i <= t < P, with s = 1/sqrt(d),
        cond | key | va | vb [t] = lin columns 0..4d of row t,     qk[t][e] = qexp[e]·key_t,
        z(t, i, e) = (qexp[e]·key_i + cond_t·key_i)·s,   wfa[t][i][e] = relu(z)/(Σ_{i<=t} relu(z) + eps),   wfb: -z.

Written from the header, not from the kernels.  Not a conftest and not a test module: import it (`import prefix_model`).
"""
from __future__ import annotations

import numpy as np

import group_beam_model as M

F = np.float32


def reset_state(n_img: int, R: int, T: int, sos: int, prefix, prefix_logp, group_beams: int, fill: int = 0) -> dict:
    """prefix int [n_img, P], prefix_logp float32 [n_img, P]; the arrays the reset does not touch (positions behind P,
    ancestors from P on) hold `fill`."""
    prefix, prefix_logp = np.asarray(prefix, np.int64), np.asarray(prefix_logp, F)
    P = prefix.shape[1]
    assert prefix.shape == prefix_logp.shape == (n_img, P) and 1 <= P <= T - 2 and R % group_beams == 0
    st = M.new_state(n_img, R, T, sos, fill)
    for b in range(n_img):
        for r in range(R):
            n = b * R + r
            st["tokens"][b, r, 1:P + 1] = prefix[b]
            st["logprobs"][b, r, 1:P + 1] = prefix_logp[b]
            st["anc"][n, :P] = b * R
            st["n_elem"][n], st["has_eos"][n], st["row_valid"][n] = P + 1, 0, 1
            st["next_tok"][n] = prefix[b, P - 1]
            if r % group_beams == 0:
                cs = F(0.0)
                for j in range(P + 1):
                    cs = F(cs + st["logprobs"][b, r, j])
                st["cumul"][n] = cs
            else:
                st["cumul"][n] = -np.inf
    st["pos"][0], st["done"][0] = P, 0
    return st


def reset_embedding(embed, pos_table, scale, prefix, R: int) -> np.ndarray:
    """y [n_img·R, d] = embed[last prefix word]·scale + pos_table[P]: the input of position P."""
    prefix = np.asarray(prefix, np.int64)
    P = prefix.shape[1]
    rows = [F(embed[int(prefix[b, P - 1])] * F(scale)) + pos_table[P] for b in range(prefix.shape[0]) for _ in range(R)]
    return np.stack(rows).astype(F)


def fill_caches(lin, qexp, P: int, d: int, eps: float = 1e-9) -> dict:
    """lin [P, >=5d] (one sequence), qexp [E, d] → dict(cond, key, va, vb [P, d]; qk [P, E]; wfa, wfb [P, P, E], entries
    with i > t left at zero), in float64 (the comparison decides the tolerance)."""
    lin, qexp = np.asarray(lin, np.float64)[:P], np.asarray(qexp, np.float64)
    E = qexp.shape[0]
    cond, key, va, vb = (lin[:, k * d:(k + 1) * d] for k in range(4))
    qk = key @ qexp.T                                   # [P, E]
    ck = cond @ key.T                                   # [t, i]
    s = 1.0 / np.sqrt(float(d))
    wfa, wfb = np.zeros((P, P, E)), np.zeros((P, P, E))
    for t in range(P):
        z = (qk[:t + 1, :] + ck[t, :t + 1, None]) * s   # [i, e]
        pa, pb = np.maximum(z, 0.0), np.maximum(-z, 0.0)
        wfa[t, :t + 1] = pa / (pa.sum(0, keepdims=True) + eps)
        wfb[t, :t + 1] = pb / (pb.sum(0, keepdims=True) + eps)
    return dict(cond=cond, key=key, va=va, vb=vb, qk=qk, wfa=wfa, wfb=wfb)
