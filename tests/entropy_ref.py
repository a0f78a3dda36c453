"""float64 numpy restatement of the entropy term of DESIGN.md §27 (kernels.softmax_entropy): the reference of the kernel tests.

    p_i = softmax(z_i),  H_i = -sum_k p_ik log p_ik,  L = sum_i H_i / (P ln C)  (0 for C == 1)
    dL/dz_ij = -p_ij (log p_ij + H_i) / (P ln C)

log p is the log-softmax (z - max - log sum exp); a term with p == 0 contributes 0."""
import numpy as np


def entropy_ref(z, coef=1.0):
    """z: [..., C] (any float dtype; computed in float64) -> (L: float, coef * dL/dz: float64 array of z's shape)"""
    z = np.asarray(z, dtype=np.float64)
    C = z.shape[-1]
    z2 = z.reshape(-1, C)
    P = z2.shape[0]
    zs = z2 - z2.max(axis=1, keepdims=True)
    logp = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    plogp = np.where(p > 0, p * logp, 0.0)
    H = -plogp.sum(axis=1, keepdims=True)
    if C == 1:
        return 0.0, np.zeros_like(z)
    k = 1.0 / (P * np.log(float(C)))
    grad = -k * (plogp + p * H)
    return float(H.sum() * k), (coef * grad).reshape(z.shape)


def special_rows(z, rng):
    """mix the rows the issue names into random logits z [P, C] (in place, P >= 8 and C >= 2 for all of them) -> {kind: row indices}"""
    P, C = z.shape
    idx = {"equal": [], "ahead": [], "huge": []}
    if P < 8 or C < 2:
        return idx
    rows = rng.choice(P, size=6, replace=False)
    z[rows[0]] = 0.37                          # all-equal logits: normalised entropy 1, zero gradient
    z[rows[1]] = -12.5
    idx["equal"] = [int(rows[0]), int(rows[1])]
    z[rows[2], int(rng.integers(C))] += 200.0  # one class ahead by 200: entropy and gradient ~ 0
    z[rows[3], 0] += 200.0
    idx["ahead"] = [int(rows[2]), int(rows[3])]
    z[rows[4]] = np.where(rng.random(C) < 0.5, 1e4, -1e4)      # +-1e4: no NaN, no inf
    z[rows[4], 0], z[rows[4], 1] = 1e4, -1e4
    z[rows[5]] = -1e4
    z[rows[5], C - 1] = 1e4
    idx["huge"] = [int(rows[4]), int(rows[5])]
    return idx
