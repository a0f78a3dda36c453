"""float64 numpy restatement of pnp_paste_tiles (csrc/paste.hip) — the reference of tests/test_gpu_tiles.py and
tests/test_gpu_volume_tiles.py, pinned to scipy.ndimage.map_coordinates(order=1, mode="nearest") + an explicit weighted mean in
tests/test_tiles_host.py.  Built on paste_ref (coordinates, interpolation, coordinate bound) and ensemble_ref (member logits, softmax,
entropy, the label and entropy bounds), which it does not change.

  member_covers(invs, X, Y, H, W)         [M, X, Y] bool: the columns inside each member's field of view (pnp_paste_*_fov's rule, float64)
  edge_columns(invs, X, Y, H, W)          [X, Y] bool: the columns whose coverage by some member the float32 coordinates may decide otherwise
  window(p, n, ramp)                      g(p; n) = min(1, max(d, 0.5) / ramp), d = min(p + 0.5, (n - 0.5) - p)
  weights(invs, X, Y, H, W, ramp)         [M, X, Y]: w_m = g(pi; H) g(pj; W) where member m covers the column, 0 elsewhere
  tiles(logits, invs, X, Y, ramp, nb)     -> Result(label, prob, entropy, covered, weights): the weighted mean of the covering members' softmax
  paste(...)                              the launch's whole effect on the three flat allocations: covered columns only
  k_tiles / delta_p_tiles                 the probability bound, derived in DESIGN.md §20 and restated at the functions
"""
import collections

import numpy as np

import ensemble_ref as E
import paste_ref as R

Result = collections.namedtuple("Result", ("label", "prob", "entropy", "covered", "weights"))

U = 2.0 ** -24


def _inside(pi, pj, H, W, grow):
    return (pi >= -0.5 - grow) & (pi <= H - 0.5 + grow) & (pj >= -0.5 - grow) & (pj <= W - 0.5 + grow)


def member_covers(invs, X, Y, H, W):
    out = []
    for inv in invs:
        pi, pj = R.coords(inv, X, Y)
        out.append(_inside(pi, pj, H, W, 0.0))
    return np.stack(out)


def edge_columns(invs, X, Y, H, W):
    """a column is left out of the comparison when, for some member, moving its float64 coordinates by paste_ref.coord_eps (the bound of the
    two fmaf roundings, with its margin) changes the side of a +-0.5 border they lie on: there the device may decide the coverage otherwise"""
    edge = np.zeros((X, Y), dtype=bool)
    for inv in invs:
        pi, pj = R.coords(inv, X, Y)
        eps = R.coord_eps(inv, X, Y)
        edge |= _inside(pi, pj, H, W, eps) & ~_inside(pi, pj, H, W, -eps)
    return edge


def window(p, n, ramp):
    d = np.minimum(p + 0.5, (n - 0.5) - p)
    return np.minimum(1.0, np.maximum(d, 0.5) / float(ramp))


def weights(invs, X, Y, H, W, ramp):
    out = []
    for inv in invs:
        pi, pj = R.coords(inv, X, Y)
        out.append(np.where(_inside(pi, pj, H, W, 0.0), window(pi, H, ramp) * window(pj, W, ramp), 0.0))
    return np.stack(out)


def tiles(logits, invs, X, Y, ramp, nb=None):
    """label [nb, X, Y] uint8 (first maximum of the weighted sum), prob [nb, X, Y, ncls], entropy [nb, X, Y] — all three meaningful on
    `covered` [X, Y] only (elsewhere prob is NaN-free filler: 0) — and the weights [M, X, Y]"""
    H, W = np.asarray(logits[0]).shape[1:3]
    w = weights(invs, X, Y, H, W, ramp)                       # [M, X, Y]
    covered = w.sum(axis=0) > 0
    q = E.softmax(E.member_logits(logits, invs, X, Y, nb))    # [M, nb, X, Y, ncls]
    acc = (w[:, None, :, :, None] * q).sum(axis=0)
    wsum = np.where(covered, w.sum(axis=0), 1.0)
    P = acc / wsum[None, :, :, None]
    return Result(np.argmax(acc, axis=-1).astype(np.uint8), P, E.entropy(P), covered, w)


def paste(vol_flat, prob_flat, ent_flat, res, z0, origin, strides):
    """writes res into the flat uint8 / float32 [ncls * elems] / float32 [elems] arrays like the kernel: the covered columns only (an array
    that is None is skipped).  Returns (idx [nb, X, Y], written [nb, X, Y] bool)."""
    nb, X, Y = res.label.shape
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    assert idx.min() >= 0 and idx.max() < vol_flat.size and np.unique(idx).size == idx.size
    wr = np.broadcast_to(res.covered[None], idx.shape)
    vol_flat[idx[wr]] = res.label[wr]
    if prob_flat is not None:
        prob_flat.reshape(res.prob.shape[-1], vol_flat.size)[:, idx[wr]] = res.prob[wr].T
    if ent_flat is not None:
        ent_flat[idx[wr]] = res.entropy[wr]
    return idx, wr


def k_tiles(M):
    """K(M) = 2 M + 18 roundings of 2^-24 on P_c = acc_c / wsum, with u = 2^-24 and every probability <= 1:
      14.45  the softmax of one member as the device computes it (ensemble_ref.delta_p's per-member term); a weighted mean of such errors
             is no larger;
       3.5   the window: p + 0.5 and (n - 0.5) - p round once each (relative u on d; (float)n - 0.5 and max(d, 0.5) are exact), 1.0f / ramp
             and the product with it one each: 3 u on g, 3 + 3 + 1 = 7 u on w = g_i g_j.  Relative errors rho_m on the weights move the
             weighted mean by sum_m omega_m rho_m (q_m - P), at most rho / 2 (the mean absolute deviation of values in [0, 1]);
       1     the product w_m q_mc (relative u, summed with weights that total P_c <= 1);
       2 (M - 1)   two ascending sums of at most M positive terms: every partial sum is at most the total, so each of the <= M - 1
             additions adds at most u relative to the total, on acc_c and on wsum alike, and P_c <= 1;
       1     the division.
    14.45 + 3.5 + 1 + 2 (M - 1) + 1 = 2 M + 17.95 <= 2 M + 18 (M = 1: 20, ensemble_ref.K_ROUND)."""
    return 2 * int(M) + 18


def coords_exact(inv, X, Y):
    """True when both fmaf chains are exact in float32 for every column: the inner sum m1 y + m2 and the whole coordinate are float32
    numbers (then the device's coordinates ARE the float64 ones, and its window sees no coordinate error)"""
    m = np.asarray(inv, dtype=np.float32).astype(np.float64)
    y = np.arange(Y, dtype=np.float64)
    pi, pj = R.coords(inv, X, Y)
    return all(np.array_equal(v, v.astype(np.float32).astype(np.float64)) for v in (m[1] * y + m[2], m[4] * y + m[5], pi, pj))


def coord_shift(invs, X, Y):
    """2 eps over the members whose coordinates are not exact, eps = paste_ref.coord_eps: the coordinate roundings move d = min(p + 0.5,
    (n - 0.5) - p) by at most eps, a weight by at most eps / max(d, 0.5) <= 2 eps relative per axis (4 eps on w = g_i g_j), and relative
    errors rho on the weights move the weighted mean by at most rho / 2: 2 eps on P.  0 when every member's coordinates are exact."""
    return 2.0 * max([R.coord_eps(inv, X, Y) for inv in invs if not coords_exact(inv, X, Y)], default=0.0)


def delta_p_tiles(logits, invs, X, Y, nb=None):
    """|P_c - P_c^ref| <= delta_r / 2 + K(M) 2^-24 + coord_shift: ensemble_ref.delta_p's first term (the softmax row's Jacobian against the
    bound of the interpolated logits, paste_ref.delta maximised over the members), k_tiles' roundings, and — on members whose coordinates
    are not exactly representable only — the effect of the coordinate roundings on the window, which is no multiple of 2^-24 and so no
    part of K(M).  With exact coordinates (axis-aligned planes on the test's grids) the bound is delta_r / 2 + K(M) 2^-24 alone."""
    return 0.5 * E.delta_r(logits, invs, X, Y, nb) + k_tiles(len(logits)) * U + coord_shift(invs, X, Y)


# ---- the cases of tests/test_gpu_tiles.py (shared with the CPU checks that the bounds are not vacuous on them) ----------------------------
def layout(kind, X, Y, Z):
    """-> (elements of the allocation, origin, (sx, sy, sz)): the three store layouts, the z-fastest ones at an odd offset inside a larger
    allocation"""
    if kind == "zup":                        # [X, Y, Z] C order from element 3: sz = +1
        return X * Y * Z + 7, 3, (Y * Z, Z, 1)
    if kind == "zdown":                      # the same with the frames descending: sz = -1
        return X * Y * Z + 7, 3 + Z - 1, (Y * Z, Z, -1)
    if kind == "zfirst":                     # paste_ref's [Z, X, Y] with both in-plane axes flipped: the slicing axis first
        return R.layout("zfirst_flipped", X, Y, Z)
    raise KeyError(kind)


SPACING = (0.5, 0.5)         # mm per voxel
PIXEL = (1.0, 1.0)           # mm per plane pixel


def _grid(ni, nj, step_i, step_j, **kw):
    """ni x nj members on an even grid of plane centres (mm, about the box centre), tile-major"""
    return [dict(kw, translate=((a - (ni - 1) / 2.0) * step_i, (b - (nj - 1) / 2.0) * step_j)) for a in range(ni) for b in range(nj)]


def _vary(members, rotate=(), flip=(), scale=()):
    """member k gets rotate[k % len], flip[k % len], scale[k % len] (an empty tuple changes nothing)"""
    out = []
    for k, m in enumerate(members):
        m = dict(m)
        if rotate:
            m["rotate"] = rotate[k % len(rotate)]
        if flip:
            m["flip"] = flip[k % len(flip)]
        if scale:
            m["scale"] = scale[k % len(scale)]
        out.append(m)
    return out


#        name       (H, W)    (X, Y)   B  nb z0 Z  layout    ncls ramp  members: compose_matrix's keywords, translate in mm
CASES = {
    "one":        ((16, 16), (38, 34), 3, 3, 1, 5, "zup",    5, 1.0, _grid(1, 1, 0, 0)),                     # covered by 0 or 1
    "one_mono":   ((12, 12), (22, 20), 2, 2, 0, 3, "zdown",  1, 2.0, _grid(1, 1, 0, 0, rotate=9.0)),
    "pair":       ((12, 16), (40, 24), 4, 3, 1, 5, "zdown",  2, 4.0, _grid(2, 1, 8.0, 0)),                   # flush along i: 1 or 2
    "pair_deep":  ((12, 16), (40, 24), 2, 2, 2, 5, "zfirst", 8, 6.0, _vary(_grid(2, 1, 6.0, 0), scale=(1.0, 1.1))),
    "quad":       ((12, 12), (40, 36), 5, 4, 1, 7, "zfirst", 5, 5.0, _grid(2, 2, 7.0, 6.0)),                 # 0 (the i rim), 1, 2 and 4
    "quad_views": ((14, 12), (38, 30), 3, 3, 1, 5, "zup",    2, 3.0,                                         # two tiles x (plain, flipped)
                   _vary(_grid(2, 1, 5.0, 0) + _grid(2, 1, 5.0, 0), flip=(False, False, True, True))),
    "nine":       ((16, 12), (40, 34), 4, 3, 2, 6, "zdown",  8, 2.5, _vary(_grid(3, 3, 2.5, 2.625), rotate=(0.0, 7.5, -7.5, 13.0))),
    "nine_flip":  ((12, 14), (38, 36), 3, 3, 1, 5, "zup",    5, 3.0,
                   _vary(_grid(3, 3, 3.5, 2.0), rotate=(0.0, -5.0), flip=(False, True, False), scale=(1.0, 1.0, 0.95, 1.05))),
    "many":       ((12, 12), (40, 36), 3, 2, 1, 4, "zup",    5, 2.0, _vary(_grid(8, 8, 1.125, 0.875), rotate=(0.0, 0.0, 6.0, -4.0, 0.0))),
    "many_first": ((12, 12), (36, 40), 2, 2, 0, 3, "zfirst", 2, 1.0, _vary(_grid(8, 8, 0.875, 1.125), flip=(False, True, False))),
}


def case_logits(name, member, seed=0):
    """[B, H, W, ncls] float32, smooth like ensemble_ref.smooth_logits (a coarse normal grid upsampled bilinearly, max|logit| = 10)"""
    (H, W), _, B = CASES[name][:3]
    ncls = CASES[name][7]
    h, w = max(2, H // 4), max(2, W // 4)
    coarse = np.random.default_rng([seed, sorted(CASES).index(name), member]).standard_normal((B, h, w, ncls))
    pi, pj = np.meshgrid(np.linspace(0, h - 1, H), np.linspace(0, w - 1, W), indexing="ij")
    up = np.stack([R.interpolate(coarse[b], pi, pj) for b in range(B)])
    return (up * (10.0 / np.abs(up).max())).astype(np.float32)
