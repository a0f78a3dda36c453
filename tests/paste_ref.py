"""float64 numpy restatement of csrc/paste.hip — the reference of tests/test_gpu_paste.py and
tests/test_gpu_volume_predict.py, pinned to scipy.ndimage.map_coordinates(order=1, mode="nearest") + np.argmax in tests/test_paste_host.py.

  coords(inv, X, Y)            output-plane coordinates of every source voxel (x, y) from the SAME six float32 entries the kernel gets
  interpolate(logits, pi, pj)  [X, Y, ncls] float64: clamp into [0, H - 1] x [0, W - 1], bilinear between the four corners, per class
  labels(logits, inv, X, Y)    [nb, X, Y] uint8: np.argmax (first maximum) of the interpolated logits, per slice
  paste(...)                   the kernel's whole effect on a flat uint8 allocation: origin + x sx + y sy + (z0 + b) sz
  delta / admissible           the bound: a device label must lie in {c : r[c] >= max r - 2 delta}
"""
import numpy as np


def coords(inv, X, Y):
    m = np.asarray(inv, dtype=np.float32).astype(np.float64)
    x = np.arange(X, dtype=np.float64)[:, None]
    y = np.arange(Y, dtype=np.float64)[None, :]
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


def interpolate(plane, pi, pj):
    """plane [H, W, ncls] -> [X, Y, ncls] float64"""
    p = np.asarray(plane, dtype=np.float64)
    H, W = p.shape[:2]
    pi = np.where(np.isnan(pi), 0.0, np.clip(pi, 0.0, H - 1.0))
    pj = np.where(np.isnan(pj), 0.0, np.clip(pj, 0.0, W - 1.0))
    i0, j0 = np.floor(pi).astype(np.int64), np.floor(pj).astype(np.int64)
    i1, j1 = np.minimum(i0 + 1, H - 1), np.minimum(j0 + 1, W - 1)
    ti, tj = (pi - i0)[..., None], (pj - j0)[..., None]
    a = p[i0, j0] * (1 - tj) + p[i0, j1] * tj
    b = p[i1, j0] * (1 - tj) + p[i1, j1] * tj
    return a * (1 - ti) + b * ti


def labels(logits, inv, X, Y, nb=None):
    """logits [B, H, W, ncls] -> ([nb, X, Y] uint8 labels, [nb, X, Y, ncls] float64 interpolated logits)"""
    logits = np.asarray(logits)
    nb = logits.shape[0] if nb is None else nb
    pi, pj = coords(inv, X, Y)
    r = np.stack([interpolate(logits[b], pi, pj) for b in range(nb)])
    return np.argmax(r, axis=-1).astype(np.uint8), r


def paste(vol_flat, lab, z0, origin, strides):
    """writes lab [nb, X, Y] into the flat uint8 array like the kernel; returns it"""
    nb, X, Y = lab.shape
    sx, sy, sz = (int(s) for s in strides)
    idx = (int(origin) + np.arange(X)[None, :, None] * sx + np.arange(Y)[None, None, :] * sy + (z0 + np.arange(nb))[:, None, None] * sz)
    assert idx.min() >= 0 and idx.max() < vol_flat.size and np.unique(idx).size == idx.size
    vol_flat[idx.ravel()] = lab.ravel()
    return vol_flat


def coord_eps(inv, X, Y):
    """4 float32 ulps at the largest coordinate term (the two fmaf roundings are half an ulp each; the rest is margin)"""
    m = np.abs(np.asarray(inv, dtype=np.float32).astype(np.float64))
    t = max(float(max(m[0], m[3]) * (X - 1)), float(max(m[1], m[4]) * (Y - 1)), float(max(m[2], m[5])))
    return 4.0 * float(np.spacing(np.float32(t)))


def adjacent_gap(logits):
    """(Gi, Gj): the largest gap between adjacent logits of one class along each plane axis"""
    p = np.asarray(logits, dtype=np.float64)
    gi = float(np.abs(np.diff(p, axis=1)).max()) if p.shape[1] > 1 else 0.0
    gj = float(np.abs(np.diff(p, axis=2)).max()) if p.shape[2] > 1 else 0.0
    return gi, gj


def delta(logits, inv, X, Y):
    """eps (Gi + Gj) + 4 * 2^-24 max|logit|: bilinear-with-clamp is Lipschitz in the coordinates with the adjacent gaps as constants; the
    second term covers the three roundings of the interpolation itself"""
    gi, gj = adjacent_gap(logits)
    return coord_eps(inv, X, Y) * (gi + gj) + 4.0 * 2.0 ** -24 * float(np.abs(np.asarray(logits, dtype=np.float64)).max())


def admissible(r, d):
    """[..., ncls] bool: the classes whose interpolated logit is within 2 d of the maximum"""
    return r >= r.max(axis=-1, keepdims=True) - 2.0 * d


# ---- the cases of tests/test_gpu_paste.py (shared with the CPU check that the bound is not vacuous on them) --------------------------------
#        name                (H, W)    (X, Y)    B, nb, z0  Z  layout
CASES = {"identity":        ((16, 24), (16, 24), 3, 3, 1, 5, "c"),
         "upsample":        ((16, 24), (37, 23), 4, 3, 1, 6, "c"),
         "downsample":      ((32, 32), (8, 12), 2, 2, 0, 2, "c"),
         "sixteen_at_odd":  ((16, 16), (19, 21), 16, 16, 3, 21, "c"),
         "partial_batch":   ((16, 16), (19, 21), 16, 7, 5, 13, "c"),
         "axis_first_flip": ((16, 24), (37, 23), 4, 4, 2, 7, "zfirst_flipped"),
         "sub_box":         ((16, 24), (10, 9), 3, 3, 1, 5, "sub_box")}
MAPS = {"resize": {}, "rotated": {"rotate": 13.0, "translate": (1.5, -2.25)}}


def layout(kind, X, Y, Z):
    """-> (elements of the allocation, origin, (sx, sy, sz))"""
    if kind == "c":                          # [X, Y, Z] C order: z fastest
        return X * Y * Z, 0, (Y * Z, Z, 1)
    if kind == "zfirst_flipped":             # [Z, X, Y] with both in-plane axes flipped: sz largest, sx and sy negative
        return Z * X * Y, (X - 1) * Y + (Y - 1), (-Y, -1, X * Y)
    if kind == "sub_box":                    # the box at (2, 3, 1) of a 14 x 13 x 8 C-order array
        assert X + 2 <= 14 and Y + 3 <= 13 and Z + 1 <= 8
        return 14 * 13 * 8, 2 * 13 * 8 + 3 * 8 + 1, (13 * 8, 8, 1)
    raise KeyError(kind)


def case_logits(name, ncls, seed=0):
    (H, W), _, B = CASES[name][:3]
    return np.random.default_rng([seed, sorted(CASES).index(name), ncls]).standard_normal((B, H, W, ncls)).astype(np.float32)


def written_index(X, Y, nb, z0, origin, strides):
    """[nb, X, Y] flat element index of every voxel the launch writes"""
    sx, sy, sz = (int(s) for s in strides)
    return int(origin) + np.arange(X)[None, :, None] * sx + np.arange(Y)[None, None, :] * sy + (z0 + np.arange(nb))[:, None, None] * sz
