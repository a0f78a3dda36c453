"""float64 numpy restatement of the warped gather (pnp_aug_slices_warp) — the reference of tests/test_gpu_warp.py, pinned
on the host in tests/test_warp_host.py.  Built on augment_ref, which it does not change.

  basis(t)                          [4, ...]: the uniform cubic B-spline weights B0 .. B3 at t
  cells(n, G)                       (cell index, t) of the n output rows (columns): g = (k + 0.5) G / n, cell = min(floor(g), G - 1), t = g - cell
  displacement(ctrl, H, W)          [H, W, 2]: d = sum_ab B_a(t) B_b(s) ctrl[ci + a, cj + b] of one sample's control table [G + 3, G + 3, 2]
  coords(m, ctrl, H, W)             augment_ref.coords plus the displacement (ctrl None: no warp)
  fmix32 / uniforms / normal        the counter hash, (u1, u2) of counter e under a seed, Box-Muller's n = sqrt(-2 ln u1) cos(2 pi u2)
  noise_field(H, W, seed)           [H, W, 3]: n of e = 3 (i W + j) + channel
  intensity(v, gain, bias, noise, n)   gain v + bias + noise n
  warp_c(G), warp_eps(ctrl, s)      the constant and the coordinate error of the displacement (derived at warp_c)
  NOISE_C                           the constant of the noise bound c' 2^-24 sigma (derived there)
"""
import numpy as np

import augment_ref as R

U = 2.0 ** -24


def basis(t):
    t = np.asarray(t, dtype=np.float64)
    return np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])


def cells(n, G):
    g = (np.arange(n, dtype=np.float64) + 0.5) * G / n
    c = np.minimum(np.floor(g), G - 1).astype(np.int64)
    return c, g - c


def displacement(ctrl, H, W):
    """ctrl [G + 3, G + 3, 2] -> [H, W, 2] float64 (NaN / inf entries propagate to the pixels whose 4 x 4 support holds them)"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    G = ctrl.shape[0] - 3
    assert ctrl.shape == (G + 3, G + 3, 2) and G >= 1
    ci, t = cells(H, G)
    cj, s = cells(W, G)
    bi, bj = basis(t), basis(s)                        # [4, H], [4, W]
    d = np.zeros((H, W, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(4):
            for b in range(4):
                d += (bi[a][:, None] * bj[b][None, :])[..., None] * ctrl[(ci + a)[:, None], (cj + b)[None, :]]
    return d


def support_holds(ctrl, H, W, bad):
    """[H, W] bool: the pixels whose 4 x 4 support holds an entry where `bad` [G + 3, G + 3] is set"""
    G = ctrl.shape[0] - 3
    ci, _ = cells(H, G)
    cj, _ = cells(W, G)
    out = np.zeros((H, W), dtype=bool)
    for a in range(4):
        for b in range(4):
            out |= bad[(ci + a)[:, None], (cj + b)[None, :]]
    return out


def coords(m, ctrl, H, W):
    sx, sy = R.coords(m, H, W)
    if ctrl is None:
        return sx, sy
    d = displacement(ctrl, H, W)
    with np.errstate(invalid="ignore"):
        return sx + d[..., 0], sy + d[..., 1]


# ---- the noise ---------------------------------------------------------------------------------------------------------------------------
def fmix32(h):
    """the murmur3 finaliser on uint32 arrays (pnp_fmix32, csrc/pnp_common.h)"""
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.uint32)


def uniforms(e, seed):
    """(u1 in (0, 1], u2 in [0, 1)) float64 of the counters e (uint32 array) under `seed`"""
    e = np.asarray(e, dtype=np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFF)
    h1 = fmix32((((2 * e) & 0xFFFFFFFF) * 0xCC9E2D51 & 0xFFFFFFFF) ^ seed)
    h2 = fmix32((((2 * e + 1) & 0xFFFFFFFF) * 0xCC9E2D51 & 0xFFFFFFFF) ^ seed)
    return ((h1 >> 8).astype(np.float64) + 1.0) * U, (h2 >> 8).astype(np.float64) * U


def normal(e, seed):
    u1, u2 = uniforms(e, seed)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise_field(H, W, seed):
    """[H, W, 3] float64: the normal of e = 3 (i W + j) + channel"""
    return normal(np.arange(3 * H * W, dtype=np.uint64), seed).reshape(H, W, 3)


def intensity(v, gain, bias, noise, n):
    g, b, s = (np.float64(np.float32(a)) for a in (gain, bias, noise))
    return g * v + b + (s * n if s != 0 else 0.0)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------------
def warp_c(G):
    """the constant c of eps_warp = c u max|P| (u = 2^-24: one float32 rounding is at most u relative), from the operations the header pins.
    With M = max|P| and d = sum_ab Bi_a Bj_b P_ab, Bi_a, Bj_b >= 0, sum_a Bi_a = sum_b Bj_b = 1:
      rounding of t      rh = fl(G / H) and g = fl((i + 0.5) rh) round once each ((i + 0.5) is exact): |dg| <= 2.01 u G; t = g - cell is exact;
                         d is a C2 spline in g (a neighbouring cell with t beyond [0, 1] describes the same function), |dd/dg| =
                         |sum_a B'_a(t) P_a| <= M sum_a |B'_a(t)| <= 1.5 M (test_warp_host.py holds the 1.5): 3.02 G u M per axis, both axes:   6.1 G
      polynomial weights B0 = ((u u) u) k: 1 - t, three products, the constant k = fl(1/6): 7 u B0 <= 7/6 u;  B3: 4 u B3 <= 4/6 u;
                         B1 = fmaf(t t, fmaf(3, t, -6), 4) k: t t rounds (<= 3 u after the product with |3 t - 6| t t <= 3), the inner fmaf
                         (<= 6 u), the outer (<= 4 u), then k and its product on a value <= 4 (<= 8 u), all over 6: 3.5 u;
                         B2 = fmaf(t, fmaf(t, fmaf(-3, t, 3), 3), 1) k: 3 u, then 3 u + 3.75 u, then 6.75 u + 4 u, then 8 u, over 6: 3.2 u;
                         sum_a |dB_a| <= 8.6 u <= 9 u per axis; |dd| <= M (sum|dBi| sum Bj + sum Bi sum|dBj|):                               18
      16 products        two chains of four fmaf-accumulated products with weights summing to 1: 4 u M for the row contraction, carried
                         through the column chain's weights (sum 1), plus that chain's own 4 u M:                                            8
    so c = 26 + 6.1 G.  The addition s + d rounds once more, at the coordinate: warp_eps adds one ulp there."""
    return 26.0 + 6.1 * G


def warp_eps(ctrl, s_max):
    """eps_warp of one sample: warp_c(G) u max|P| over the finite control values plus one float32 ulp at the largest coordinate s_max"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    fin = np.abs(ctrl[np.isfinite(ctrl)])
    top = float(fin.max()) if fin.size else 0.0
    return warp_c(ctrl.shape[0] - 3) * U * top + float(np.spacing(np.float32(s_max)))


# c' of |out - out(noise = 0) - sigma n| <= c' u sigma when out(noise = 0) == 0 (otherwise the final fmaf also rounds at |out|: half an ulp
# there).  u1, u2 are exact in float32.  n = fl(r c), r = sqrtf(-2 logf(u1)), c = cosf(fl(6.2831855f u2)):
#   |n| <= R = sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77
#   r   logf within 3 ulp = 6 u relative, halved by the square root, plus sqrtf within 3 ulp:  9 u relative
#   c   the float32 constant 6.2831855 is within u of 2 pi and the product rounds once: the argument, < 2 pi, is off by <= 2 u 2 pi = 12.6 u
#       absolute, and so is its cosine (|sin| <= 1); cosf within 4 ulp of a value <= 1: 8 u; together 20.6 u absolute
#   n   R (20.6 + 9 + 1) u = 176.5 u; the fmaf with sigma (exact in the record) rounds sigma n once more: 5.8 u sigma
# c' = 184.  The 3 / 3 / 4 ulp of logf / sqrtf / cosf are OpenCL's full-profile limits, which the ROCm device library is built to; no
# document on the build machine states the library's own figures, so DESIGN.md §18 records the measured error next to this bound.
NOISE_C = 184.0
