"""Pure-numpy restatement of pnp_fill_holes, integers only: the yardstick of tests/test_gpu_holes.py.

  fill_holes(vol, ncls, max_size, classes) -> (filled uint8, stats int64 [ncls, 4], info)

A voxel is background when its label is 0 or >= ncls.  A cavity is a maximal set of background voxels joined by face steps without a voxel
at index 0 or D - 1 of any axis; its contacts with class c are the pairs (v in the cavity, u a face neighbour of v) with label(u) == c, its
winner the class with the most contacts (ties: the lower class).  It is filled with its winner when the winner is in `classes` (None: all)
and max_size == 0 or its size <= max_size.  out = the winner on filled cavities, 0 on all other background, vol elsewhere.  stats: row c
>= 1 = cavities filled with c, voxels filled with c, largest cavity filled with c, cavities won by c and left; row 0 = cavities found,
their voxels, cavities left, voxels left.  info: {"cavities", "ties", "multi", "root", "size", "winner", "filled", "contacts" (int64 [cavities, ncls])} for the
tests' own assertions.  tests/test_holes_host.py pins the set of filled voxels to scipy.ndimage.binary_fill_holes.

The background is labelled by components_ref.roots (the background as the one class of a 2-class volume, connectivity 1)."""
import numpy as np

import components_ref as C

STEPS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def fill_holes(vol, ncls, max_size=0, classes=None):
    v = C.clean(vol, ncls)
    n = v.size
    bg = v == 0
    r = C.roots(bg.astype(np.uint8), 2, 1)                                # -1 on the classes
    rf = r.reshape(-1).astype(np.int64)
    size = np.bincount(rf[rf >= 0], minlength=n).astype(np.int64)
    face = np.zeros(v.shape, dtype=bool)
    for ax in range(3):
        for i in (0, -1):
            face[tuple(i if a == ax else slice(None) for a in range(3))] = True
    is_open = np.zeros(n, dtype=bool)
    is_open[rf[face.reshape(-1) & (rf >= 0)]] = True
    contacts = np.zeros((n, ncls), dtype=np.int64)
    for o in STEPS:
        dst = tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip(o, v.shape))       # voxels p with p + o inside the volume
        src = tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip(o, v.shape))       # their neighbours p + o
        sel = bg[dst] & (v[src] > 0)
        np.add.at(contacts, (r[dst][sel].astype(np.int64), v[src][sel].astype(np.int64)), 1)
    root = np.flatnonzero((rf == np.arange(n)) & ~is_open)                # the cavities, by their smallest flat index
    cc = contacts[root]
    assert (cc[:, 0] == 0).all() and (cc[:, 1:].sum(axis=1) > 0).all(), "every cavity has a contact"
    winner = 1 + np.argmax(cc[:, 1:], axis=1) if len(root) else np.zeros(0, np.int64)   # argmax: the first maximum = the lower class
    allowed = np.zeros(ncls, dtype=bool)
    allowed[list(range(1, ncls)) if classes is None else [int(c) for c in classes]] = True
    filled = allowed[winner] & ((max_size == 0) | (size[root] <= max_size))
    value = np.zeros(n, dtype=np.uint8)
    value[root[filled]] = winner[filled]
    out = v.reshape(-1).copy()
    out[rf >= 0] = value[rf[rf >= 0]]
    stats = np.zeros((ncls, 4), dtype=np.int64)
    for c in range(1, ncls):
        s = size[root[filled & (winner == c)]]
        stats[c] = len(s), s.sum(), s.max() if len(s) else 0, int((~filled & (winner == c)).sum())
    stats[0] = len(root), size[root].sum(), int((~filled).sum()), size[root[~filled]].sum()
    best = cc[:, 1:].max(axis=1) if len(root) else np.zeros(0, np.int64)
    info = {"cavities": len(root), "ties": int(((cc[:, 1:] == best[:, None]).sum(axis=1) > 1).sum()),
            "multi": int(((cc[:, 1:] > 0).sum(axis=1) > 1).sum()), "root": root, "size": size[root], "winner": winner, "filled": filled,
            "contacts": cc}
    return out.reshape(v.shape), stats, info


# ---- the cases of tests/test_gpu_holes.py and tests/test_holes_host.py: name -> uint8 volume ------------------------------------------------
SHAPE = (37, 29, 45)                                    # 5 x 4 x 2 tiles of 8 x 8 x 32, ragged in every axis


def _block(shape=SHAPE, lo=(9, 9, 19), hi=(18, 18, 28), cls=1):
    v = np.zeros(shape, np.uint8)
    v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = cls
    return v


def case_shell():
    """a 3 x 3 x 3 cavity inside one tile, in a block of class 1"""
    v = _block()
    v[12:15, 12:15, 22:25] = 0
    return v


def case_corner():
    """the same cavity across the tile corner (8, 8, 32)"""
    v = _block(lo=(4, 4, 28), hi=(13, 13, 37), cls=2)
    v[7:10, 7:10, 31:34] = 0
    return v


def case_channel(plugged=False):
    """a cavity in a solid volume with a one-voxel channel to the face x = 0; plugged: the channel's face voxel is class 2"""
    v = np.full(SHAPE, 1, np.uint8)
    v[12:15, 12:15, 22:25] = 0
    v[0:12, 13, 23] = 0
    if plugged:
        v[0, 13, 23] = 2
    return v


def case_diagonal():
    """the cavity's only leak is an edge-diagonal step to a channel that reaches the face x = 0: not a face step, so it is a cavity"""
    v = np.full(SHAPE, 1, np.uint8)
    v[12:15, 12:15, 22:25] = 0
    v[0:12, 11, 22] = 0                                 # (11, 11, 22) and (12, 12, 22) share an edge only
    return v


def case_vote():
    """a one-voxel cavity with five neighbours of class 3 and one of class 2"""
    v = np.full(SHAPE, 3, np.uint8)
    v[8, 8, 32] = 0
    v[7, 8, 32] = 2
    return v


def case_tie():
    """a one-voxel cavity with three neighbours of class 3 (the first three the kernel reads) and three of class 2: class 2 wins"""
    v = np.full(SHAPE, 3, np.uint8)
    v[16, 8, 31] = 0
    v[16, 9, 31] = v[16, 8, 30] = v[16, 8, 32] = 2
    return v


def case_sizes():
    """cavities of 1, 8, 27 and 64 voxels in a solid volume of class 1, the largest across tile borders in every axis"""
    v = np.full(SHAPE, 1, np.uint8)
    v[2, 2, 2] = 0
    v[4:6, 4:6, 4:6] = 0
    v[10:13, 10:13, 10:13] = 0
    v[14:18, 14:18, 30:34] = 0
    return v


def case_high():
    """label 7: one voxel inside a block of class 1 and a few in the open background"""
    v = _block()
    v[13, 13, 23] = 7
    v[0, 0, 0] = v[30, 20, 40] = v[20, 2, 2] = 7
    return v


def case_all_labels(seed=3):
    """labels 0 .. 7 at random, half of the voxels label 1: for ncls = 2 (half the volume is background), 4 and 8"""
    rng = np.random.default_rng(seed)
    return rng.choice(8, size=SHAPE, p=(.2, .5) + (.05,) * 6).astype(np.uint8)


def case_thin(shape):
    rng = np.random.default_rng(5)
    return rng.choice(5, size=shape, p=(.3, .175, .175, .175, .175)).astype(np.uint8)


def case_snake(leak=False):
    """a closed one-voxel-wide background path through solid foreground of two classes, 33 x 33 x 64; leak: one end reaches the face x = 0"""
    inner = C.case_snake((31, 31, 62))
    x, y, z = np.indices((33, 33, 64))
    v = (1 + (x + y + z) % 2).astype(np.uint8)
    v[1:-1, 1:-1, 1:-1][inner == 1] = 0
    if leak:
        v[0, 1, 1] = 0
    return v


def case_random(seed=16):
    rng = np.random.default_rng(seed)
    return rng.choice(5, size=SHAPE, p=(.22, .195, .195, .195, .195)).astype(np.uint8)


def case_blobs(shape=(96, 80, 72), seed=16):
    """the argmax of five lightly smoothed noise fields: large structures, an open background and many small enclosed pockets"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((5,) + tuple(shape)).astype(np.float32)
    for c in range(5):
        f[c] = C._box_blur(f[c], 1)
    coarse = rng.standard_normal((5,) + tuple(-(-s // 8) for s in shape)).astype(np.float32)
    for ax in range(3):
        coarse = np.repeat(coarse, 8, axis=ax + 1)
    f += 0.35 * coarse[:, :shape[0], :shape[1], :shape[2]]
    return np.argmax(f, axis=0).astype(np.uint8)


def case_pocket():
    """a pocket of class 3 inside a block of class 1 and a larger structure of class 3 elsewhere: keep_largest(keep=1) empties the pocket,
    fill_holes closes it with class 1"""
    v = _block()
    v[12:14, 12:14, 22:24] = 3
    v[25:30, 5:10, 5:10] = 3
    return v


CASES = {"one_zero": lambda: np.zeros((1, 1, 1), np.uint8), "one_three": lambda: np.full((1, 1, 1), 3, np.uint8),
         "thin_a": lambda: case_thin((2, 9, 33)), "thin_b": lambda: case_thin((9, 2, 33)),
         "background": lambda: np.zeros(SHAPE, np.uint8), "solid": lambda: np.full(SHAPE, 2, np.uint8),
         "shell": case_shell, "corner": case_corner, "channel": case_channel, "plugged": lambda: case_channel(True),
         "diagonal": case_diagonal, "vote": case_vote, "tie": case_tie, "sizes": case_sizes, "high": case_high,
         "all_labels": case_all_labels, "snake": case_snake, "snake_leak": lambda: case_snake(True), "random": case_random,
         "blobs": case_blobs, "pocket": case_pocket}
