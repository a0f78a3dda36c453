"""float64 numpy restatement of pnp_paste_ensemble (csrc/paste.hip) — the reference of tests/test_gpu_ensemble.py and
tests/test_gpu_volume_ensemble.py, pinned to scipy.ndimage.map_coordinates(order=1, mode="nearest") + scipy.special.softmax in
tests/test_ensemble_host.py.  Built on paste_ref.coords / paste_ref.interpolate (the interpolation of §14), which it does not change.

  member_logits(logits, invs, X, Y, nb)   [M, nb, X, Y, ncls] float64: every member's logits interpolated through its own inverse map
  softmax(r)                              over the last axis, with the maximum subtracted
  ensemble(logits, invs, X, Y, nb)        -> Result(label [nb, X, Y] uint8 (first maximum of the mean), prob [nb, X, Y, ncls], entropy
                                          [nb, X, Y] normalised by log(ncls); 0 for ncls = 1, a term with P = 0 contributes 0, r)
  paste(...)                              the launch's whole effect on the three flat allocations
  delta_p / admissible / entropy_bound    the bounds, derived in DESIGN.md §15 and restated at the functions
"""
import collections

import numpy as np

import paste_ref as R

Result = collections.namedtuple("Result", ("label", "prob", "entropy", "r"))

U = 2.0 ** -24          # unit roundoff of float32
K_ROUND = 20            # roundings of the probability path in units of 2^-24: see delta_p


def member_logits(logits, invs, X, Y, nb=None):
    out = []
    for lg, inv in zip(logits, invs):
        lg = np.asarray(lg)
        n = lg.shape[0] if nb is None else nb
        pi, pj = R.coords(inv, X, Y)
        out.append(np.stack([R.interpolate(lg[b], pi, pj) for b in range(n)]))
    return np.stack(out)


def softmax(r):
    e = np.exp(r - r.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def entropy(P):
    ncls = P.shape[-1]
    if ncls == 1:
        return np.zeros(P.shape[:-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(P > 0, P * np.log(P), 0.0)
    return -t.sum(axis=-1) / np.log(ncls)


def ensemble(logits, invs, X, Y, nb=None):
    r = member_logits(logits, invs, X, Y, nb)
    P = softmax(r).mean(axis=0)
    return Result(np.argmax(P, axis=-1).astype(np.uint8), P, entropy(P), r)


def paste(vol_flat, prob_flat, ent_flat, res, z0, origin, strides):
    """writes res into the flat uint8 / float32 [ncls * elems] / float32 [elems] arrays like the kernel (an array that is None is skipped)"""
    nb, X, Y = res.label.shape
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    assert idx.min() >= 0 and idx.max() < vol_flat.size and np.unique(idx).size == idx.size
    vol_flat[idx.ravel()] = res.label.ravel()
    if prob_flat is not None:
        prob_flat.reshape(res.prob.shape[-1], vol_flat.size)[:, idx.ravel()] = res.prob.reshape(-1, res.prob.shape[-1]).T
    if ent_flat is not None:
        ent_flat[idx.ravel()] = res.entropy.ravel()
    return idx


def delta_r(logits, invs, X, Y, nb=None):
    """paste_ref.delta (the bound of one member's interpolated logits) maximised over the members"""
    return max(R.delta(np.asarray(lg)[:nb], inv, X, Y) for lg, inv in zip(logits, invs))


def delta_p(logits, invs, X, Y, nb=None):
    """|P_c - P_c^ref| <= delta_r / 2 + K_ROUND 2^-24.
    First term: a softmax row's Jacobian has infinity-norm 2 p (1 - p) <= 1/2, per member, and the mean of M such errors is no larger.
    K_ROUND, with u = 2^-24 and d_c = r_c - max r <= 0: the subtraction perturbs e_c by |d_c| u relatively and expf by 1 ulp = 2 u; the
    class sum s inherits sum_j p_j (|d_j| + 2) u <= (ln ncls + 2) u (sum_j p_j |d_j| <= H(p)) plus ncls - 1 roundings; the division one
    more: |dp_c| <= p_c |d_c| u + p_c (2 + (ln 8 + 2 + 7) + 1) u <= (1/e + 14.08) u = 14.45 u per member.  The member sum rounds at
    partial sums 2, 3, 4 per run of four and once more when the two runs meet: <= 26 u on acc for M = 8, i.e. 3.25 u on acc / M (less for
    every other M); 1.0f / M and the product with it: 2 u.  14.45 + 3.25 + 2 = 19.7 <= 20."""
    return 0.5 * delta_r(logits, invs, X, Y, nb) + K_ROUND * U


def admissible(P, dp):
    """[..., ncls] bool: the classes whose mean probability is within 2 dp of the maximum"""
    return P >= P.max(axis=-1, keepdims=True) - 2.0 * dp


def entropy_bound(dp, ncls):
    """|H - H^ref| <= ncls (-dp ln dp) / ln(ncls) + (4 ncls + 4) 2^-24: x ln x has modulus of continuity -t ln t on [0, 1] (t <= 1/2), per
    class; rounding: logf 1 ulp and the product on a term of magnitude <= 1/e (3 u / e per class), ncls fmaf roundings on |h| <= ln ncls,
    the reciprocal of logf(ncls) and the final product (4 u on H <= 1): (3 ncls / e + ncls ln ncls) u / ln ncls + 4 u <= (4 ncls + 4) u."""
    if ncls == 1:
        return 0.0
    assert 0.0 < dp < 0.5
    return ncls * (-dp * np.log(dp)) / np.log(ncls) + (4 * ncls + 4) * U


# ---- the cases of tests/test_gpu_ensemble.py (shared with the CPU check that the label bound is not vacuous on them) ---------------------
# member m of a launch uses MAPS[m]: the four maps of the check in the issue first
MAPS = ({}, {"rotate": 13.0, "translate": (1.5, -2.25)}, {"flip": True}, {"scale": 1.1, "rotate": -7.0},
        {"rotate": 7.5}, {"rotate": -7.5}, {"scale": 0.95}, {"scale": 1.05})
#          case (paste_ref.CASES), M, ncls
SWEEP = ([(case, 3, 5) for case in sorted(R.CASES)]
         + [("upsample", M, ncls) for M in (1, 3, 8) for ncls in (1, 2, 5, 8) if (M, ncls) != (3, 5)])


def smooth_logits(case, ncls, member, seed=0):
    """[B, H, W, ncls] float32: a standard-normal grid at a quarter of the plane's resolution, upsampled bilinearly, rescaled to max|logit| = 10
    (white noise has top-2 gaps below the bound too often; a network's logits are smooth)"""
    (H, W), _, B = R.CASES[case][:3]
    h, w = max(2, H // 4), max(2, W // 4)
    rng = np.random.default_rng([seed, sorted(R.CASES).index(case), ncls, member])
    coarse = rng.standard_normal((B, h, w, ncls))
    pi, pj = np.meshgrid(np.linspace(0, h - 1, H), np.linspace(0, w - 1, W), indexing="ij")
    up = np.stack([R.interpolate(coarse[b], pi, pj) for b in range(B)])
    return (up * (10.0 / np.abs(up).max())).astype(np.float32)
