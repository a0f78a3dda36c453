"""the case tables and the host restatements of the domain pass over the per-pixel loss terms (csrc/pixel_loss.h, csrc/block_sum.h,
csrc/entropy.hip, csrc/boundary.hip, csrc/pseudo_label.hip): a plain module, no fixtures.  tests/
test_pixel_loss_domain_host.py pins the restatements to the library and checks that the tables reach the branches they are there for;
tests/test_gpu_pixel_loss_domain.py runs them.

The per-element bound.  With u = 2^-24, m_i = max_j z_ij and p~ = max(p, 2^-126), a gradient entry is held to

    |g - g64| <= FACTOR * u * (1 + |z_ij - m_i|) * S_ij

    entropy                    S_ij = g_k p~_ij (|log p_ij| + H_i)
    boundary                   S_ij = g_k p~_ij (|q_ij| + sum_k p_ik |q_ik|)
    pseudo-label, selected     S_ij = g_k (p~_ij + [j = k_i])
    pseudo-label, unselected   exactly 0

(1 + |z - m|) is the rounding of z - m amplified by the exponential.  Two things about the float32 FORMAT, not about any kernel:

* p~ also stands inside the two row sums: H_i = sum_k p~_ik |log p_ik| and sum_k p~_ik |q_ik| here.  On a row whose leader is a hundred
  logits or more ahead, the leader's own entry is -g_k (log p + H) (boundary: g_k (q - s), when its q is 0), a sum of the OTHER classes'
  p |log p| (p |q|).  Those p lie below 2^-126, float32 holds them to 2^-150 absolute at best, and with the plain p in the row sums both
  the entry's float64 value and its S are that small: the ratio is 2^24 for arithmetic that is exact to the last bit (measured: 1.6e7
  on the row 104 logits behind, whose exponential rounds to 0).  With p~ the row sums follow the probabilities down to 2^-126 and no
  further, like the entry's own factor.  The difference to S is at most 8 * 2^-126 * |log p| (|q|): 1e-34.
* g_k is the factor the entry point hands the kernel ((float)(coef * scale)); the tests choose coef so that g_k = GK.  With the g_k of a
  mean over 10^5 pixels (1e-7) a product g_k p underflows where p itself does not, and is rounded to a multiple of 2^-149 whatever the
  kernel does: an error of several per cent of an S that follows p down to 2^-126 only.  (coef and scale at their working magnitudes
  are what the feature tests cover.)
"""
import functools
import math

import numpy as np

from entropy_ref import special_rows
from pseudo_label_ref import _near, build_logits, class_flags

# ---- the launch plan of csrc/pixel_loss.h and the workspace layouts ---------------------------------------------------------------------
NT = 256
PIX_PER_THREAD = 8
MAX_BLOCKS = 2048
MAXC = 8
UPD_MAX_BLOCKS = 256


def blocks(P):
    """workgroups of the streaming pass: ceil(P / 2048), at least 1, at most 2048"""
    return int(min(max(-(-int(P) // (NT * PIX_PER_THREAD)), 1), MAX_BLOCKS))


def entropy_workspace_bytes(P, C):
    return 4 * blocks(P)


def boundary_workspace_bytes(P, C):
    return 4 * blocks(P)


def pseudo_label_loss_layout(P, C):
    """-> (offset of the float partials, offset of the int partials [2 C][nblk], total bytes)"""
    n = blocks(P)
    return 0, 4 * n, 4 * n + 4 * 2 * max(int(C), 0) * n


def pseudo_label_loss_workspace_bytes(P, C):
    return pseudo_label_loss_layout(P, C)[2]


def pseudo_label_update_workspace_bytes(P, C):
    """four rounds of [8][256] unsigned bins, then 8 x {prefix, rank, n}"""
    return 4 * MAXC * 256 * 4 + MAXC * 12


def update_blocks(P):
    return int(min(-(-int(P) // NT), UPD_MAX_BLOCKS))


def stream_plan(P, C, vector):
    """what one launch of the streaming pass walks -> dict(nblk, threads, groups, trips: the most grid-stride trips a thread makes over the
    four-pixel groups (vector) or the pixels (generic), ragged: the last trip does not fill the grid, tail: pixels of the scalar loop behind
    the groups)"""
    nblk = blocks(P)
    threads = nblk * NT
    vector = bool(vector) and C == 5 and P >= 4
    work = P >> 2 if vector else P
    return {"nblk": nblk, "threads": threads, "vector": vector, "groups": work if vector else 0, "trips": -(-work // threads),
            "ragged": work % threads != 0, "tail": P & 3 if vector else 0}


# ---- the column pass of the signed distance (csrc/boundary.hip) -------------------------------------------------------------------------
LDS_TILES = 16 * 1024
MIN_STRIP = 2
KR = 8
MAX_PARTS = 8


def strip_width(H, nsel):
    tw = 64
    while tw > MIN_STRIP and nsel * H * tw * 2 > LDS_TILES:
        tw >>= 1
    return tw


def col_plan(H, W, C, nsel):
    """-> dict(tw, nstrips, nch, items, parts, ipb: items per block, n: pixels of a strip, ppb: pixels per block of the unselected classes'
    zeros, overhang: columns of the last strip outside W)"""
    tw = strip_width(H, nsel)
    nstrips = -(-W // tw)
    nch = -(-H // KR)
    items = nsel * nch * tw
    parts = int(min(MAX_PARTS, max(1, items // NT)))
    n = H * tw
    return {"tw": tw, "nstrips": nstrips, "nch": nch, "items": items, "parts": parts, "ipb": -(-items // parts), "n": n,
            "ppb": -(-n // parts), "overhang": nstrips * tw - W, "unselected": C - nsel}


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------
# 1. launch geometry: (P, C, path).  "vector": C = 5 and aligned bases; "generic": another class count; "offset": C = 5 with the logits
# one pixel into their allocation.  2 048 pixels a workgroup, 524 288 threads at the cap
GEOMETRY = [(2047, 5, "vector"), (2048, 5, "vector"), (2049, 5, "vector"), (2050, 5, "vector"),      # (2050: the one P mod 4 = 2)
            (524288, 5, "vector"),            # 256 workgroups: the longest list that one trip of block_sum_of_list covers
            (524293, 5, "vector"),            # 257: the second trip; tail 1
            (524293, 5, "offset"),
            (4194304, 5, "vector"),           # 2 048 workgroups, two groups per thread exactly
            (4196355, 5, "vector"),           # the cap: a ragged third trip, tail 3
            (524293, 2, "generic"), (4196355, 2, "generic")]

# 2. the per-element bound on the shapes of the feature tests (asserted equal to their SHAPES / LOSS_SHAPES in the GPU file)
ENTROPY_SHAPES = [(P, 5) for P in (1, 3, 4, 7, 1021, 2 * 64 * 64)] + [(257, C) for C in (1, 2, 3, 8)] + [(2 * 256 * 256, 5)]
BOUNDARY_SHAPES = [(P, 5) for P in (1, 3, 4, 7, 1021, 2 * 256 * 256)] + [(257, C) for C in (1, 2, 3, 8)]
PSEUDO_LABEL_SHAPES = [(P, 5) for P in (1, 3, 4, 7, 1021, 2 * 64 * 64, 2 * 256 * 256)] + [(257, C) for C in (1, 2, 3, 8)]
ELEMENT_SHAPES = sorted(set(ENTROPY_SHAPES) | set(BOUNDARY_SHAPES) | set(PSEUDO_LABEL_SHAPES), key=lambda s: (s[1] != 5, s[1], s[0]))
BEHIND = (20.0, 60.0, 87.0, 88.0, 100.0, 103.0, 104.0)      # expf of the trailing classes: normal (20, 60, 87), subnormal (88, 100, 103), zero (104)
BEHIND_FROM = 16                                             # the rows of a case with P >= 64 that carry them: BEHIND_FROM ... + 6

# 3. one operand misaligned at a time: operand -> byte offsets into its allocation (an element is four bytes)
MISALIGNED_P = (7, 1021)
MISALIGNED = {"entropy": [("logits", 4), ("dlogits", 4)],
              "boundary": [("logits", 4), ("dlogits", 4), ("phi", 4)],
              "pseudo_label": [("logits", 4), ("dlogits", 4), ("conf", 4), ("labels", 1), ("labels", 2), ("labels", 3)]}

# 4. the selection rule on logits that are not filtered: (P, C, path, seed)
SELECTION = [(2 * 256 * 256, 3, "generic", 41), (2 * 256 * 256, 5, "vector", 42), (2 * 256 * 256, 5, "offset", 42), (2 * 256 * 256, 8, "generic", 43)]
NEAR_CAP = 2e-3

# 5. the threshold update on maps made directly
UPDATE_P = (255, 256, 257, 65536, 65537)
UPDATE_C = 7                                                 # (at most 7: a mutation that takes class byte ncls stays inside the LDS table)
# 0.28 * 25 is 7.000000000000001 in double: rank 8, where the exact product would give 7.  (0.3 * 10 is exactly 3.0 in double: rank 3.)
UPDATE_PORTIONS = (1e-9, 0.3, 0.28, 1.0)
UPDATE_BETAS = (0.0, 0.9, 1.0)

# 6. the workspace extent
EXTENT_P = 524293

# 7. the signed distance: (B, H, W, C, selected classes)
# parts = min(8, items / 256) and the tiles fit 16 KB (nsel * H * TW <= 8192) until the strip is at its floor of two columns: 6 and 7 blocks a
# strip exist ONLY at that floor with all eight classes selected and H >= 761 / 889 (5: also at H = 17 ... 18 with seven classes and at
# 25 with five).  Three columns keep the O(H^2 W) reference cheap at those heights.
SDIST_PARTS = [((1, 17, 70, 8), [1, 2, 3, 4, 5, 6, 7]),      # parts 5: 64 columns a strip, the last 58 outside W; class 0 not selected
               ((1, 770, 3, 8), list(range(8))),             # parts 6
               ((1, 900, 3, 8), list(range(8)))]             # parts 7
SDIST_BATCH = (5, 20, 70, 5)                                 # a different class absent from, or filling, each of the five slices


def tau_of(C):
    """tests/test_gpu_pseudo_label.py::_tau: mixed thresholds per class, exact in float32"""
    return np.array([0.9, 0.35, 0.6, 0.5, 0.75, 0.4, 0.8, 0.55][:C], dtype=np.float32).astype(np.float64)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def maps_like(z, seed):
    """distance-map-like extra input for the boundary term: a few hundred pixels either way, more often outside a class than inside it,
    class 0 not selected (exactly 0), and a few pixels without any distance"""
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal(z.shape) * 100.0 + 25.0).astype(np.float32)
    q[:, 0] = 0.0
    q[rng.random(z.shape[0]) < 0.01] = 0.0
    return q


@functools.lru_cache(maxsize=1)
def geometry_inputs(P, C):
    """-> (logits, maps) shared by the three terms: logits kept clear of the thresholds tau_of(C) and of ties (build_logits), so that the
    class / selected bytes and the counts are exact.  One case is kept at a time: 84 MB a tensor at the cap."""
    z = build_logits(P, C, 1000 * C + P % 997, tau_of(C))
    return z, maps_like(z, P % 991)


def behind_rows(C, rng):
    """[7, C]: a leader, a runner-up one logit behind it (C >= 3), every other class BEHIND[r] logits behind the leader exactly"""
    rows = np.empty((len(BEHIND), C), dtype=np.float32)
    for r, gap in enumerate(BEHIND):
        lead = r % C
        rows[r] = np.float32(1.5) - np.float32(gap)
        rows[r, lead] = 1.5
        if C >= 3:
            rows[r, (lead + 1 + int(rng.integers(C - 1))) % C] = 0.5
    return rows


@functools.lru_cache(maxsize=None)
def element_inputs(P, C):
    """-> (logits, maps): 3 N(0, 1) logits with boundary's +300 / +700 / -400 rows (P >= 7), the rows of entropy_ref.special_rows (P >= 8,
    C >= 2) and, from P = 64 on, the rows of behind_rows at BEHIND_FROM"""
    rng = np.random.default_rng(100 * C + P % 97)
    z = (rng.standard_normal((P, C)) * 3.0).astype(np.float32)
    if P >= 7:
        z[1, int(rng.integers(C))] += 300.0
        z[5, 0] += 700.0
        z[6, C - 1] -= 400.0
    special_rows(z, rng)
    if P >= 64 and C >= 2:
        z[BEHIND_FROM:BEHIND_FROM + len(BEHIND)] = behind_rows(C, rng)
    return z, maps_like(z, 7 * P + C)


@functools.lru_cache(maxsize=None)
def selection_logits(P, C, seed):
    """3 N(0, 1), nothing redrawn"""
    return (np.random.default_rng(seed).standard_normal((P, C)) * 3.0).astype(np.float32)


def update_maps(P, seed):
    """(conf float32 [P], labels uint8 [P]) for UPDATE_C = 7 classes, made directly:
    class 0  keys equal in their top three bytes            class 1  10 pixels in two clusters that differ in the top byte only
    class 2  1.0, 2^-126, a subnormal and +0.0              class 3  one pixel            class 4  empty
    class 5  random confidences                             class 6  exactly 25 pixels
    and a tenth of the bytes in [UPDATE_C, 127]; bit 7 is set on half of all bytes"""
    rng = np.random.default_rng(seed)
    C = UPDATE_C
    n_ignored = P // 10
    n2, n1, n0, n6 = 8, 10, 40, 25
    n5 = P - (n_ignored + n2 + n1 + n0 + 1 + n6)
    cls = np.concatenate([np.full(n0, 0), np.full(n1, 1), np.full(n2, 2), np.full(1, 3), np.full(n5, 5), np.full(n6, 6),
                          rng.integers(C, 128, n_ignored)]).astype(np.uint8)
    bits = np.concatenate([0x3F000000 | rng.integers(0, 256, n0),
                           np.resize(np.array([0x3E123456, 0x3F123456, 0x3F123456]), n1),
                           np.resize(np.array([0x3F800000, 0x00800000, 0x00000123, 0x00000000]), n2),
                           [0x3F1A2B3C], rng.integers(0x3E000000, 0x3F800001, n5), rng.integers(0x3E000000, 0x3F800001, n6),
                           rng.integers(0x3E000000, 0x3F800001, n_ignored)]).astype(np.uint32)
    order = rng.permutation(P)
    cls, bits = cls[order], bits[order]
    lab = cls | (rng.integers(0, 2, P).astype(np.uint8) << 7)
    return bits.view(np.float32), lab


def sdist_labels(B, H, W, C, seed):
    """tests/test_gpu_boundary.py::_labels: coarse random blocks with a little salt -> one-hot float32 [B, H, W, C]"""
    rng = np.random.default_rng(seed)
    bh, bw = max(H // 5, 1), max(W // 5, 1)
    n = max(C, 2)
    coarse = rng.integers(0, n, (B, -(-H // bh), -(-W // bw)))
    lab = np.repeat(np.repeat(coarse, bh, axis=1), bw, axis=2)[:, :H, :W]
    lab = np.where(rng.random((B, H, W)) < 0.02, rng.integers(0, n, (B, H, W)), lab)
    return np.stack([(lab == c) for c in range(C)], axis=-1).astype(np.float32)


# ---- float64 references with the per-element scale --------------------------------------------------------------------------------------------
U = 2.0 ** -24
TINY = 2.0 ** -126
GK = 0.75       # the factor the tests hand the kernels (module docstring)


def scale_of(term, P, C, nsel=None):
    """the scale of the term's entry point: value = scale * sum of the per-pixel contributions"""
    if term == "entropy":
        return 1.0 / (P * math.log(float(C))) if C > 1 else 0.0
    if term == "boundary":
        return 1.0 / (P * float(nsel)) if nsel > 0 else 0.0
    return 1.0 / P


def coef_of(term, P, C, nsel=None):
    """-> (coef as the float32 the entry point receives, g_k = coef * scale in double): g_k = GK but for the rounding of coef"""
    s = scale_of(term, P, C, nsel)
    coef = float(np.float32(GK / s)) if s > 0 else 1.0
    return coef, coef * s


def _softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    d = z - z.max(axis=1, keepdims=True)
    ls = np.log(np.exp(d).sum(axis=1, keepdims=True))
    lp = d - ls
    return d, lp, np.exp(lp)


def entropy_elem(z, gk):
    """-> (value, gradient float64, scale (1 + |z - m|) S float64)"""
    P, C = z.shape
    d, lp, p = _softmax64(z)
    plogp = np.where(p > 0, p * lp, 0.0)
    H = -plogp.sum(axis=1, keepdims=True)
    if C == 1:
        return 0.0, np.zeros_like(d), np.zeros_like(d)
    grad = -gk * (plogp + p * H)
    pt = np.maximum(p, TINY)
    S = gk * pt * (np.abs(lp) + (pt * np.abs(lp)).sum(axis=1, keepdims=True))
    return float(H.sum() * scale_of("entropy", P, C)), grad, (1.0 + np.abs(d)) * S


def boundary_elem(z, q, nsel, gk):
    P, C = z.shape
    d, lp, p = _softmax64(z)
    q = np.asarray(q, dtype=np.float64)
    s = (p * q).sum(axis=1, keepdims=True)
    grad = gk * p * (q - s)
    pt = np.maximum(p, TINY)
    S = gk * pt * (np.abs(q) + (pt * np.abs(q)).sum(axis=1, keepdims=True))
    return float(s.sum() * scale_of("boundary", P, C, nsel)), grad, (1.0 + np.abs(d)) * S


def pseudo_label_elem(z, k, sel, gk):
    """against a given class / selected map (the reference's, or the device's own) -> (value, gradient, scale)"""
    P, C = z.shape
    d, lp, p = _softmax64(z)
    onehot = np.zeros_like(d)
    onehot[np.arange(P), k] = 1.0
    on = np.asarray(sel, dtype=bool)[:, None]
    grad = np.where(on, gk * (p - onehot), 0.0)
    S = np.where(on, gk * (np.maximum(p, TINY) + onehot), 0.0)
    value = float(-(lp[np.arange(P), k])[np.asarray(sel, dtype=bool)].sum() / P)
    return value, grad, (1.0 + np.abs(d)) * S


# ---- float32 restatements of the per-pixel gradients -----------------------------------------------------------------------------------------
# The formulas of the kernels' `pixel` functions in numpy float32, one rounding per operation: the softmax prefix of pixel_loss.h (max,
# expf(z - max), the sum in ascending class order), then the term.  Not the kernels' placement of fused multiply-adds; exp and log are the
# correctly rounded ones (taken in double, rounded once), so that the figures below do not depend on the host's vector library.
F32 = np.float32


def _exp32(x):
    return np.exp(x.astype(np.float64)).astype(F32)


def _log32(x):
    return np.log(x.astype(np.float64)).astype(F32)


def _prefix32(z):
    z = np.ascontiguousarray(z, dtype=F32)
    d = z - z.max(axis=1, keepdims=True)
    e = _exp32(d)
    s = e[:, 0].copy()
    for j in range(1, z.shape[1]):
        s = s + e[:, j]
    return d, e, s


def entropy_grad32(z, gk):
    gk = F32(gk)
    d, e, s = _prefix32(z)
    if z.shape[1] == 1:
        return np.zeros_like(d)
    ls, inv = _log32(s), F32(1.0) / s
    lp = d - ls[:, None]
    p = e * inv[:, None]
    H = np.zeros_like(s)
    for j in range(z.shape[1]):
        H = H + (-p[:, j]) * lp[:, j]
    return (-gk * p) * (lp + H[:, None])


def boundary_grad32(z, q, gk):
    gk = F32(gk)
    d, e, s = _prefix32(z)
    q = np.ascontiguousarray(q, dtype=F32)
    p = e * (F32(1.0) / s)[:, None]
    t = np.zeros_like(s)
    for j in range(z.shape[1]):
        t = t + p[:, j] * q[:, j]
    return (gk * p) * (q - t[:, None])


def pseudo_label_map32(z, tau, classes=None):
    """the kernel's rule in float32 -> (k, selected, conf float32)"""
    d, e, s = _prefix32(z)
    k = np.ascontiguousarray(z, dtype=F32).argmax(axis=1)
    conf = F32(1.0) / s
    sel = class_flags(z.shape[1], classes)[k] & (conf >= np.asarray(tau, dtype=F32)[k])
    return k, sel, conf


def pseudo_label_grad32(z, k, sel, gk):
    gk = F32(gk)
    d, e, s = _prefix32(z)
    conf = F32(1.0) / s
    onehot = np.zeros_like(e)
    onehot[np.arange(z.shape[0]), k] = 1.0
    return np.where(np.asarray(sel, dtype=bool)[:, None], gk * (e * conf[:, None] - onehot), F32(0.0))


def ratio_of(got, ref, scale):
    """max over entries of |got - ref| / (u * scale); an entry whose scale is 0 must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / (U * scale), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# Measured by tests/test_pixel_loss_domain_host.py::test_float32_restatement_stays_under_a_quarter_of_the_factor: the largest ratio of the
# float32 restatement against float64 over every case of GEOMETRY, ELEMENT_SHAPES and SELECTION, per term.  All three maxima come from
# plain 3 N(0, 1) logits, entropy and boundary at (4 196 355, 2): with two classes the leader's entry is the OTHER class's p (log p, q)
# and inherits the rounding of that class's z - m, which the leader's own factor 1 + |z - m| = 1 does not see; the ratio grows with the
# largest gap of the case (17 logits there).  The cases that carry the rows far ahead / behind measure 11.5 at most.
MEASURED_RATIOS = {"entropy": 17.12, "boundary": 19.39, "pseudo_label": 4.81}
# 4 x the largest of them, rounded up: the 4 covers another summation order, fused multiply-adds and an expf / logf / reciprocal that
# differs from the correctly rounded one by an ulp or two
FACTOR = 78.0


def near(z, tau):
    return _near(z, tau)
