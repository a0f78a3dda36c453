"""Plain-numpy restatement of foreground-aware slice sampling: the per-frame class table of a label volume and the
sampler's draw rule.  Integer and float64 arithmetic only; every comparison against it is integer-exact or bit-exact.

  frame_stats(label, ncls)   int32 [Z, ncls, 5] by np.nonzero per frame and class
  draw(...)                  the draw rule, line by line, with compose_matrix passed in (it does not change and has tests of its own)
"""
import math

import numpy as np

SAMPLE_DTYPE = np.dtype([("volume", "<i4"), ("frame", "<i4"), ("m", "<f4", (6,))])
SAMPLE_Z_DTYPE = np.dtype([("volume", "<i4"), ("frame", "<i4"), ("dz", "<f4"), ("m", "<f4", (6,))])


def frame_stats(label, ncls):
    """label: integer array [X, Y, Z] -> (count, xmin, xmax, ymin, ymax) per frame z and class c in [0, ncls); an absent class is
    (0, X, -1, Y, -1); a label >= ncls counts nowhere"""
    label = np.asarray(label)
    X, Y, Z = label.shape
    out = np.zeros((Z, ncls, 5), dtype=np.int32)
    for z in range(Z):
        for c in range(ncls):
            xs, ys = np.nonzero(label[:, :, z] == c)
            out[z, c] = (len(xs), xs.min(), xs.max(), ys.min(), ys.max()) if len(xs) else (0, X, -1, Y, -1)
    return out


def draw(compose_matrix, seed, dims, B, out_hw, augment, tables, foreground, classes, centre, sample_mm=None, spacings=None):
    """B samples without the elastic / intensity keys: rng = default_rng(seed) is read as the classic sampler reads it, rng3 =
    default_rng([seed, 2]) gives the foreground draws -> (records, fg_class [B], fallback [B], centre [B, 2])"""
    rng, rng3 = np.random.default_rng(seed), np.random.default_rng([seed, 2])
    rec = np.zeros(B, dtype=SAMPLE_DTYPE if sample_mm is None else SAMPLE_Z_DTYPE)
    fg_class, fallback, cen = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool), np.zeros((B, 2))
    for b in range(B):
        v = int(rng.integers(0, len(dims)))
        X, Y, Z = dims[v]
        z = int(rng.integers(1, Z - 1))
        rotate, scale, tx, ty, flip = 0.0, 1.0, 0.0, 0.0, False
        if augment is not None:
            rotate = rng.uniform(-augment["rotate"], augment["rotate"])
            ls = math.log1p(augment["scale"])
            scale = math.exp(rng.uniform(-ls, ls))
            tx = rng.uniform(-augment["translate"], augment["translate"])
            ty = rng.uniform(-augment["translate"], augment["translate"])
            flip = bool(rng.random() < augment["flip"])
        u = rng3.random()
        if u < foreground:
            count = tables[v][:, :, 0].astype(np.int64)
            present = [c for c in sorted(classes) if count[1:Z - 1, c].sum() > 0]
            if not present:
                fallback[b] = True
            else:
                c = present[int(rng3.integers(len(present)))]
                k = int(rng3.integers(int(count[1:Z - 1, c].sum())))
                z = 1 + int(np.searchsorted(np.cumsum(count[1:Z - 1, c]), k, side="right"))
                fg_class[b] = c
                if centre:
                    _, xmin, xmax, ymin, ymax = (float(t) for t in tables[v][z, c])
                    cen[b] = ((xmin + xmax) / 2 - (X - 1) / 2, (ymin + ymax) / 2 - (Y - 1) / 2)
                    if sample_mm is None:
                        tx, ty = tx + cen[b, 0], ty + cen[b, 1]
                    else:
                        tx, ty = tx + cen[b, 0] * spacings[v][0], ty + cen[b, 1] * spacings[v][1]
        rec["volume"][b], rec["frame"][b] = v, z
        geom = {}
        if sample_mm is not None:
            geom = {"spacing_xy": spacings[v][:2], "pixel_mm": tuple(sample_mm[:2])}
            rec["dz"][b] = np.float32(sample_mm[2] / spacings[v][2])
        rec["m"][b] = compose_matrix((X, Y), out_hw, rotate, scale, (tx, ty), flip, **geom)
    return rec, fg_class, fallback, cen
