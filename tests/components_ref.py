"""Pure-numpy restatement of csrc/components.hip, integers only: the yardstick of tests/test_gpu_components.py.

  roots(vol, ncls, connectivity)                       int32, vol's shape: -1 for background (label 0 or >= ncls), else the smallest flat
                                                       (C order) index among the voxels of the voxel's component
  keep_largest(vol, ncls, keep, min_size, connectivity, classes)   -> (filtered uint8, stats int64 [ncls, 4], roots)

A component is a maximal set of voxels of one non-zero label < ncls joined by steps of the neighbourhood with at most `connectivity`
non-zero offsets in {-1, 0, 1}^3 (scipy.ndimage.generate_binary_structure(3, connectivity); tests/test_components_host.py pins the two
against each other).  Method: every voxel starts as its own root; rounds of (for every pair of same-label
neighbours in different trees the larger root takes the minimum of the smaller roots offered to it, then pointer jumping L = L[L] until it
stands still) until no pair is left.  Links only point downwards, so a tree's root is its smallest index."""
import itertools

import numpy as np


def offsets(connectivity):
    """every non-zero offset with at most `connectivity` non-zero entries: 6, 18 or 26 of them"""
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity %r outside {1, 2, 3}" % (connectivity,))
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(v) for v in o) <= connectivity]


def clean(vol, ncls):
    vol = np.asarray(vol)
    assert vol.dtype == np.uint8 and vol.ndim == 3
    return np.where(vol < ncls, vol, 0).astype(np.uint8)


def roots(vol, ncls, connectivity=1):
    v = clean(vol, ncls)
    n = v.size
    assert n < 2 ** 31
    fg = v > 0
    idx = np.arange(n, dtype=np.int64).reshape(v.shape)
    P, Q = [], []
    for o in offsets(connectivity):
        if o > (0, 0, 0):
            continue                                                            # every pair once: from the later voxel to the earlier
        dst = tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip(o, v.shape))           # voxels p with p + o inside the volume
        src = tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip(o, v.shape))           # their neighbours p + o
        same = fg[dst] & (v[dst] == v[src])
        P.append(idx[dst][same])
        Q.append(idx[src][same])
    p, q = np.concatenate(P), np.concatenate(Q)
    L = np.arange(n, dtype=np.int64)                     # after every round L[x] is the root of x's tree: L[L] == L
    while True:
        lp, lq = L[p], L[q]
        open_ = lp != lq
        if not open_.any():
            break
        p, q, lp, lq = p[open_], q[open_], lp[open_], lq[open_]
        np.minimum.at(L, np.maximum(lp, lq), np.minimum(lp, lq))                # the larger root points to the smaller (minimum over all offers)
        while True:                                                              # pointer jumping
            nxt = L[L]
            if np.array_equal(nxt, L):
                break
            L = nxt
    return np.where(fg, L.reshape(v.shape), -1).astype(np.int32)


def keep_largest(vol, ncls, keep=1, min_size=0, connectivity=1, classes=None):
    """a component of a filtered class survives when size >= min_size and (keep == 0 or it is among the `keep` largest of its class, ties
    to the lower root); classes outside `classes` pass through (kept = before); labels >= ncls become 0"""
    v = clean(vol, ncls)
    r = roots(vol, ncls, connectivity)
    rf, vf = r.reshape(-1), v.reshape(-1)
    sizes = np.bincount(rf[rf >= 0], minlength=v.size).astype(np.int64)
    is_root = rf == np.arange(v.size)
    out = vf.copy()
    stats = np.zeros((ncls, 4), dtype=np.int64)
    filtered = set(range(1, ncls)) if classes is None else set(int(c) for c in classes)
    for c in range(1, ncls):
        rc = np.flatnonzero(is_root & (vf == c))
        sc = sizes[rc]
        stats[c, 0], stats[c, 1], stats[c, 3] = len(rc), sc.sum(), sc.max() if len(rc) else 0
        if c not in filtered:
            stats[c, 2] = stats[c, 1]
            continue
        order = np.lexsort((rc, -sc))                   # size descending, then root ascending
        ok = np.zeros(len(rc), dtype=bool)
        ok[order[:keep] if keep > 0 else order] = True
        ok &= sc >= min_size
        stats[c, 2] = sc[ok].sum()
        gone = np.zeros(v.size, dtype=bool)
        gone[rc[~ok]] = True
        out[(vf == c) & gone[np.maximum(rf, 0)]] = 0
    return out.reshape(v.shape), stats, r


# ---- the cases of tests/test_gpu_components.py and tests/test_components_host.py ----------------------------------------------------------
def case_random(shape=(37, 29, 45), seed=7):
    rng = np.random.default_rng(seed)
    return rng.choice(5, size=shape, p=(.4, .15, .15, .15, .15)).astype(np.uint8)


def case_snake(shape=(33, 33, 64)):
    """a one-voxel-wide boustrophedon path: rows along z on every second y, joined alternately at the two z ends; planes on every second x,
    joined alternately at the two y ends"""
    D0, D1, D2 = shape
    v = np.zeros(shape, np.uint8)
    ys = list(range(0, D1, 2))
    for i, x in enumerate(range(0, D0, 2)):
        for j, y in enumerate(ys):
            v[x, y, :] = 1
            if j + 1 < len(ys):
                v[x, y + 1, (D2 - 1) if j % 2 == 0 else 0] = 1
        if x + 2 < D0:
            y_end = ys[-1] if i % 2 == 0 else ys[0]      # where plane x's path ends = where plane x + 2's path starts
            z_end = _snake_end(len(ys), D2) if i % 2 == 0 else 0
            v[x + 1, y_end, z_end] = 1
    return v


def _snake_end(rows, D2):
    """the z at which a plane's path arrives at its last row's far end, starting at z = 0 of row 0"""
    return (D2 - 1) if rows % 2 == 1 else 0


def _box_blur(a, r):
    """separable box filter of radius r with edge replication, float32 (a stand-in for a Gaussian: three passes)"""
    for ax in range(3):
        p = np.pad(a, [(r, r) if i == ax else (0, 0) for i in range(3)], mode="edge")
        c = np.cumsum(p, axis=ax, dtype=np.float64)
        c = np.insert(c, 0, 0.0, axis=ax)
        n = a.shape[ax]
        hi = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=ax)
        lo = np.take(c, np.arange(0, n), axis=ax)
        a = ((hi - lo) / (2 * r + 1)).astype(np.float32)
    return a


def case_blobs(shape=(96, 80, 72), seed=11, radius=4, passes=2):
    """the argmax of five smoothed noise fields: a few large structures and a tail of small islands, the shape of a real prediction"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((5,) + tuple(shape)).astype(np.float32)
    for c in range(5):
        for _ in range(passes):
            f[c] = _box_blur(f[c], radius)
    f[0] += 0.02                                          # a little more background
    return np.argmax(f, axis=0).astype(np.uint8)


def case_ties():
    """class 1: two components of 4 voxels (roots 1 and 40) and one of 2; class 2: one component of 3 and two single voxels"""
    v = np.zeros((4, 5, 6), np.uint8)
    v[0, 0, 1:5] = 1
    v[1, 1, 4], v[1, 2, 4], v[1, 2, 5], v[2, 2, 5] = 1, 1, 1, 1          # flat 40, 46, 47, 77
    v[3, 0, 0:2] = 1
    v[0, 3, 0:3] = 2
    v[2, 0, 0] = 2
    v[3, 4, 5] = 2
    return v
