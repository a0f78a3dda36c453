"""float64 numpy restatement of the class-balanced pseudo-label term and its threshold update (kernels.pseudo_label_loss /
kernels.pseudo_label_update): the reference of the kernel tests.

    k_i = argmax_j z_ij (lowest index on ties),  s_i = sum_j exp(z_ij - max),  c_i = 1 / s_i
    selected_i = [k_i in classes] and c_i >= tau[k_i]
    L = sum_selected log s_i / P,   dL/dz_ij = selected_i (p_ij - [j == k_i]) / P
    q_k = the ceil(portion n_k)-th largest c_i among the n_k pixels with k_i = k,   tau_k <- q_k + beta (tau_k - q_k)
"""
import math

import numpy as np


def class_flags(C, classes=None):
    """bool [C]: the classes the term is restricted to; None = every class, the background included"""
    f = np.zeros(C, dtype=bool)
    f[list(range(C)) if classes is None else [int(c) for c in classes]] = True
    return f


def pseudo_label_ref(z, tau, classes=None, coef=1.0):
    """z [..., C], tau [C] -> dict(value, share, counts int64 [2, C], labels uint8 [...], conf float64 [...], grad = coef * dL/dz, sel)"""
    z = np.asarray(z, dtype=np.float64)
    C = z.shape[-1]
    z2 = z.reshape(-1, C)
    P = z2.shape[0]
    tau = np.asarray(tau, dtype=np.float64)
    k = z2.argmax(axis=1)                       # numpy: the first maximum = the lowest index
    e = np.exp(z2 - z2.max(axis=1, keepdims=True))
    s = e.sum(axis=1)
    conf = 1.0 / s
    sel = class_flags(C, classes)[k] & (conf >= tau[k])
    onehot = np.zeros_like(z2)
    onehot[np.arange(P), k] = 1.0
    grad = (coef / P) * (e / s[:, None] - onehot) * sel[:, None]
    counts = np.stack([np.bincount(k, minlength=C), np.bincount(k[sel], minlength=C)]).astype(np.int64)
    return {"value": float(np.log(s)[sel].sum() / P), "share": float(sel.sum() / P), "counts": counts,
            "labels": (k | (sel.astype(np.int64) << 7)).astype(np.uint8).reshape(z.shape[:-1]), "conf": conf.reshape(z.shape[:-1]),
            "grad": grad.reshape(z.shape), "sel": sel.reshape(z.shape[:-1])}


def rank_of(portion, n):
    """r = ceil(portion * n) in double, within 1 ... n"""
    return min(max(int(math.ceil(float(portion) * float(n))), 1), int(n))


def order_statistic(conf, labels, C, portion):
    """q [C] (the dtype of conf): the rank_of(portion, n_k)-th largest conf among the entries whose class byte (labels & 0x7f) is k, found
    by a walk down from the largest (no sort: numpy's partition); NaN for a class without entries"""
    conf = np.asarray(conf).reshape(-1)
    cls = np.asarray(labels).reshape(-1) & 0x7f
    q = np.full(C, np.nan, dtype=conf.dtype)
    for k in range(C):
        v = conf[cls == k]
        if v.size:
            r = rank_of(portion, v.size)
            q[k] = np.partition(v, v.size - r)[v.size - r]
    return q


def update_ref(tau, q, beta):
    """float64: tau_k <- q_k + beta (tau_k - q_k); a class with q_k = NaN (absent) keeps tau_k"""
    tau, q = np.asarray(tau, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return np.where(np.isnan(q), tau, q + beta * (tau - q))


CONF_MARGIN = 1e-5      # no pixel's float64 confidence lies this close to its class's threshold ...
GAP_MARGIN = 1e-3       # ... and no pixel's two largest logits lie this close to each other


def _near(z, tau):
    z64 = z.astype(np.float64)
    top = np.sort(z64, axis=1)
    gap = top[:, -1] - top[:, -2] if z.shape[1] > 1 else np.full(z.shape[0], np.inf)
    k = z64.argmax(axis=1)
    conf = 1.0 / np.exp(z64 - z64.max(axis=1, keepdims=True)).sum(axis=1)
    return (np.abs(conf - np.asarray(tau, dtype=np.float64)[k]) <= CONF_MARGIN) | (gap < GAP_MARGIN)


def build_logits(P, C, seed, tau):
    """float32 logits [P, C] drawn like tests/test_gpu_entropy.py::_logits (3 * standard normal); every pixel whose float64 confidence
    lies within CONF_MARGIN of its class's threshold, or whose top-2 logit gap is below GAP_MARGIN, is REDRAWN until none remains: a
    comparison of the selected map against float64 then leaves out nothing.  (C == 1: the confidence is exactly 1; tau[0] must keep away
    from 1 by the margin.)"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((P, C)) * 3.0).astype(np.float32)
    for _ in range(64):
        bad = _near(z, tau)
        if not bad.any():
            break
        z[bad] = (rng.standard_normal((int(bad.sum()), C)) * 3.0).astype(np.float32)
    assert not _near(z, tau).any(), "pixels near a threshold or a tie remain after 64 redraws"
    return z
