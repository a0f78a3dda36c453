"""Numpy restatement of the label-free body crop (csrc/body.hip, body.py): the yardstick of tests/test_gpu_body.py and
tests/test_body_host.py.  Integers and single float32 operations only — every comparison against it is an equality.

  bins(v, lo, hi, nbins)          the bin of every voxel: min(nbins - 1, int((v - lo) * (float32(nbins) / (hi - lo)))), each operation one
                                  float32 round-to-nearest operation, in this order
  histogram(v, nbins)             ((lo, hi), counts) with lo = min v, hi = max v; a constant v counts in bin 0
  mask(v, lo, hi, k, nbins)       uint8: bin > k; all zeros for a constant v
  otsu_bin(hist)                  brute force over fractions.Fraction, written independently of body.otsu_bin
  box_of_normalised(vn, ...)      the chain from a NORMALISED volume on: histogram, otsu_bin, mask, components_ref.keep_largest, numpy
                                  bounding box, margin.  The GPU tests hand it the device's own normalised copy, brought to the host; the
                                  arithmetic of pnp_volume_preprocess is not restated here.
  normalise_host(v, percentile)   a plain float64 clip-and-z-score for the host tests of the chain (NOT bit-exact with the device)
  phantom(shape, kind, seed)      (volume float32, true box): a torso-like CT or MR phantom"""
from fractions import Fraction

import numpy as np

import components_ref


def bins(v, lo, hi, nbins):
    v = np.asarray(v, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(nbins) / (hi - lo)                   # float32 / float32: one rounding
    assert scale.dtype == np.float32
    t = (v - lo) * scale                                    # two float32 operations, each rounded once; numpy never contracts them
    assert t.dtype == np.float32
    return np.minimum(nbins - 1, t.astype(np.int64))


def histogram(v, nbins=256):
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    lo, hi = v.min(), v.max()
    if hi == lo:
        h = np.zeros(nbins, dtype=np.int64)
        h[0] = v.size
        return (lo, hi), h
    return (lo, hi), np.bincount(bins(v, lo, hi, nbins), minlength=nbins).astype(np.int64)


def mask(v, lo, hi, k, nbins=256):
    v = np.asarray(v, dtype=np.float32)
    if np.float32(hi) == np.float32(lo):
        return np.zeros(v.shape, dtype=np.uint8)
    return (bins(v, lo, hi, nbins) > k).astype(np.uint8)


def otsu_bin(hist):
    """every k in [0, nbins - 2] with 0 < w0 < W, the criterion as an exact Fraction, the first maximum"""
    h = [int(c) for c in hist]
    W = sum(h)
    S = sum(i * c for i, c in enumerate(h))
    best_k, best = 0, None
    for k in range(len(h) - 1):
        w0 = sum(h[:k + 1])
        if not 0 < w0 < W:
            continue
        s0 = sum(i * c for i, c in enumerate(h[:k + 1]))
        crit = Fraction((w0 * S - W * s0) ** 2, w0 * (W - w0))
        if best is None or crit > best:
            best_k, best = k, crit
    return best_k


def grow(box, margin, shape):
    return tuple((max(a - margin, 0), min(b + margin, n)) for (a, b), n in zip(box, shape))


def box_of_normalised(vn, margin=0, nbins=256, connectivity=1, info=None):
    vn = np.asarray(vn, dtype=np.float32)
    whole = tuple((0, int(n)) for n in vn.shape)
    (lo, hi), h = histogram(vn, nbins)
    if hi == lo:
        return whole
    k = otsu_bin(h)
    m = mask(vn, lo, hi, k, nbins)
    kept, stats, _ = components_ref.keep_largest(m, 2, keep=1, connectivity=connectivity)
    if info is not None:
        info.update(k=k, hist=h, stats=stats, range=(lo, hi))
    nz = np.nonzero(kept)
    if len(nz[0]) == 0:
        return whole
    return grow(tuple((int(a.min()), int(a.max()) + 1) for a in nz), margin, vn.shape)


def normalise_host(v, percentile=98):
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    clip = np.sort(v.reshape(-1))[(percentile * (n - 1) + 99) // 100]
    c = np.minimum(v, clip)
    s = c.std()
    return ((c - c.mean()) / (s if s > 0 else 1.0)).astype(np.float32)


def phantom(shape=(48, 40, 12), kind="ct", seed=0):
    """an elliptic-cylinder body of 14 x 11 voxel semi-axes at (22, 18) on the frames 2 .. Z - 2, an air-filled lung inside it;
    ct: air -1000 +- 10, tissue 40 +- 20, a detached table plate (x 40..41, y 4..35, every frame, 200 +- 10), one voxel of 3000 in the body;
    mr: background |N(0, 8)|, tissue 300 +- 60.  -> (float32 volume, the body's box)"""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    body = ((x - 22) / 14.0) ** 2 + ((y - 18) / 11.0) ** 2 <= 1.0
    lung = ((x - 17) / 4.0) ** 2 + ((y - 18) / 5.0) ** 2 <= 1.0
    tissue = np.zeros(shape, dtype=bool)
    tissue[:, :, 2:Z - 1] = (body & ~lung)[:, :, None]
    if kind == "ct":
        v = rng.normal(-1000.0, 10.0, shape)
        v[tissue] = rng.normal(40.0, 20.0, int(tissue.sum()))
        v[40:42, 4:36, :] = rng.normal(200.0, 10.0, (2, 32, Z))
        v[24, 20, Z // 2] = 3000.0
    elif kind == "mr":
        v = np.abs(rng.normal(0.0, 8.0, shape))
        v[tissue] = rng.normal(300.0, 60.0, int(tissue.sum()))
    else:
        raise ValueError(kind)
    bx, by = np.nonzero(body.any(axis=1))[0], np.nonzero(body.any(axis=0))[0]
    return v.astype(np.float32), ((int(bx[0]), int(bx[-1]) + 1), (int(by[0]), int(by[-1]) + 1), (2, Z - 1))
