"""The case lists of tests/test_gpu_components_domain.py (which runs them on the GPU) and tests/test_components_domain_host.py (which
proves without a GPU, from a restatement of csrc/components.hip's geometry, that every branch is reached by one of them).  numpy only.

A labelling case is (name, ncls); volume(name) builds it once (read-only).  Every labelling case runs under all three connectivities."""
import itertools

import numpy as np

import components_ref as R

T0, T1, T2 = 8, 8, 32                      # csrc/components.hip: the tile
COUNT_BLOCK, RUN = 4096, 16                # cc_count_kernel: voxels per workgroup, per lane
SLOTS = 1024                               # its LDS table
MAX_EXTENT = 4096

OFFSETS26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if any(o)]
# the backward half in kOff's order: sorted by the number of non-zero entries; connectivity 1 takes the first 3, 2 the first 9, 3 all 13
BACKWARD = [(-1, 0, 0), (0, -1, 0), (0, 0, -1),
            (-1, -1, 0), (-1, 1, 0), (-1, 0, -1), (-1, 0, 1), (0, -1, -1), (0, -1, 1),
            (-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1)]
NOFF = {1: 3, 2: 9, 3: 13}

PAIR_SHAPE = (34, 34, 98)                  # 5 x 5 x 4 tiles, ragged in every axis
PAIR_KINDS = ("corner", "straddle", "interior")
DIAG_N = 40
DIAGONALS = {                              # name -> (voxel i of the chain, the connectivity from which it is one component)
    "diag_xyz": (lambda i: (i, i, i), 3), "diag_xy": (lambda i: (i, i, 0), 2), "diag_xz": (lambda i: (i, 0, i), 2),
    "diag_yz": (lambda i: (0, i, i), 2),
    "anti_xy": (lambda i: (i, DIAG_N - 1 - i, 5), 2), "anti_xz": (lambda i: (i, 5, DIAG_N - 1 - i), 2),
    "anti_yz": (lambda i: (5, i, DIAG_N - 1 - i), 2),
    "anti_xyZ": (lambda i: (i, i, DIAG_N - 1 - i), 3), "anti_xYz": (lambda i: (i, DIAG_N - 1 - i, i), 3),
    "anti_xYZ": (lambda i: (i, DIAG_N - 1 - i, DIAG_N - 1 - i), 3),
}
SWEEP_SHAPES = [(a, b, c) for a in (1, 7, 8, 9) for b in (1, 7, 8, 9) for c in (1, 31, 32, 33, 65)]
LINE_SHAPES = [(1, 1, 4096), (1, 4096, 1), (4096, 1, 1)]
CHECKER_SHAPE = (24, 24, 40)


def pair_anchor(kind, o, slot):
    """where the anchor of offset o's pair sits.  corner: the last voxel of a tile in every axis, (8i + 7, 8j + 7, 32k + 31) — the pair
    leaves the tile along every axis in which o is +1.  straddle: the tile's first voxel instead in the axes in which o is -1 — the pair
    crosses a tile border in EVERY axis it moves along.  interior: the middle of a tile."""
    i, j, k = slot % 4, slot // 4 % 4, slot // 16                      # 4 x 4 x 3 anchors, at least 8 voxels apart
    if kind == "interior":
        return (8 * i + 3, 8 * j + 3, 32 * k + 15)
    a = [8 * i + 7, 8 * j + 7, 32 * k + 31]
    if kind == "straddle":
        a = [v + 1 if d < 0 else v for v, d in zip(a, o)]
    return tuple(a)


def case_pairs(kind, two_labels):
    """one two-voxel pair per offset of the 26-neighbourhood; two_labels: the second voxel carries label 2 (never joined)"""
    v = np.zeros(PAIR_SHAPE, np.uint8)
    for slot, o in enumerate(OFFSETS26):
        a = pair_anchor(kind, o, slot)
        b = tuple(p + d for p, d in zip(a, o))
        v[a] = 1
        v[b] = 2 if two_labels else 1
    return v


def pairs_components(conn, two_labels):
    """closed form: a pair is one component when its offset has at most `conn` non-zero entries, else two"""
    if two_labels:
        return 52
    return sum(1 if sum(map(abs, o)) <= conn else 2 for o in OFFSETS26)


def case_sweep(shape):
    return np.random.default_rng(1000 * shape[0] + 100 * shape[1] + shape[2]).integers(0, 3, size=shape).astype(np.uint8)


def case_line_runs(shape):
    """runs of lengths 1, 2, 3, ... with labels 1, 2, 1, 2, ...: every run is one component"""
    n = int(np.prod(shape))
    lab = np.repeat(np.arange(91), np.arange(1, 92))[:n] % 2 + 1       # 1 + 2 + ... + 91 = 4186 >= 4096
    return lab.astype(np.uint8).reshape(shape)


def case_checker():
    x, y, z = np.indices(CHECKER_SHAPE)
    return ((x + y + z) % 2).astype(np.uint8)


def case_diagonal(name):
    v = np.zeros((DIAG_N,) * 3, np.uint8)
    for i in range(DIAG_N):
        v[DIAGONALS[name][0](i)] = 1
    return v


# the filter volume: bars along z, one per (x, y) row on even x and y (no two touch under any connectivity), sizes per class in raster order
FILTER_SHAPE = (16, 16, 48)
FILTER_SIZES = {1: [5, 5, 3, 3, 3, 1, 9, 2, 7, 4], 2: [5, 3, 4, 4], 3: [9], 4: [1, 1, 1], 5: [48, 33, 33], 6: [3], 7: [2, 2, 2, 2, 2, 2, 2, 2, 2]}
FILTER_KEEP = list(range(0, 9))
FILTER_MIN_SIZE = [0, 1, 3, 4, 1 << 40]                                 # 3 exists in classes 1, 2 and 6; 4 = that size + 1
FILTER_MASKS = [None, (), (1,), (2, 5), (7,), (1, 3, 4, 6)]            # None = every class; those naming a class >= ncls are left out
FILTER_NCLS = [2, 8]


def case_filter():
    v = np.zeros(FILTER_SHAPE, np.uint8)
    rows = [(x, y) for x in range(0, 16, 2) for y in range(0, 16, 2)]
    at = 0
    for c in sorted(FILTER_SIZES):
        for s in FILTER_SIZES[c]:
            x, y = rows[at]
            v[x, y, :s] = c
            at += 1
    return v


def filter_configs(ncls):
    for mask in FILTER_MASKS:
        if mask is not None and any(c >= ncls for c in mask):
            continue
        for keep in FILTER_KEEP:
            for min_size in FILTER_MIN_SIZE:
                yield keep, min_size, mask


def snake_along(axis):
    s = R.case_snake((33, 33, 64))
    return np.ascontiguousarray(s.transpose((2, 1, 0) if axis == "x" else (0, 2, 1)))


_BUILDERS = {"checker": case_checker, "snake_x": lambda: snake_along("x"), "snake_y": lambda: snake_along("y"), "filter": case_filter,
             "blobs": lambda: R.case_blobs((112, 80, 72))}           # its largest components hold 71 748, 73 167 and 87 397 voxels
for _k in PAIR_KINDS:
    _BUILDERS["pairs_%s" % _k] = lambda _k=_k: case_pairs(_k, False)
    _BUILDERS["pairs2_%s" % _k] = lambda _k=_k: case_pairs(_k, True)
for _s in SWEEP_SHAPES:
    _BUILDERS["sweep_%dx%dx%d" % _s] = lambda _s=_s: case_sweep(_s)
for _s in LINE_SHAPES:
    _BUILDERS["solid_%dx%dx%d" % _s] = lambda _s=_s: np.ones(_s, np.uint8)
    _BUILDERS["runs_%dx%dx%d" % _s] = lambda _s=_s: case_line_runs(_s)
for _d in DIAGONALS:
    _BUILDERS[_d] = lambda _d=_d: case_diagonal(_d)

PAIR_CASES = [("pairs_%s" % k, 3) for k in PAIR_KINDS] + [("pairs2_%s" % k, 3) for k in PAIR_KINDS]
SWEEP_CASES = [("sweep_%dx%dx%d" % s, 3) for s in SWEEP_SHAPES]
LINE_CASES = [("%s_%dx%dx%d" % ((k,) + s), 3) for s in LINE_SHAPES for k in ("solid", "runs")]
CHECKER_CASES = [("checker", 2)]
SNAKE_CASES = [("snake_x", 2), ("snake_y", 2)]
DIAGONAL_CASES = [(d, 2) for d in DIAGONALS]
LABEL_CASES = PAIR_CASES + SWEEP_CASES + LINE_CASES + CHECKER_CASES + SNAKE_CASES + DIAGONAL_CASES
CONNS = (1, 2, 3)

_cache = {}


def volume(name):
    if name not in _cache:
        v = _BUILDERS[name]()
        assert v.dtype == np.uint8 and v.flags.c_contiguous
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name]


def ref_roots(name, ncls, conn):
    key = (name, ncls, conn)
    if key not in _cache:
        _cache[key] = R.roots(volume(name), ncls, conn)
    return _cache[key]


def ref_filter(name, ncls, conn, keep=1, min_size=0, classes=None):
    """components_ref.keep_largest, once per configuration"""
    key = (name, ncls, conn, keep, min_size, None if classes is None else tuple(classes))
    if key not in _cache:
        _cache[key] = R.keep_largest(volume(name), ncls, keep, min_size, conn, classes)
    return _cache[key]
