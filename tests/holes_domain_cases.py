"""The case list of tests/test_gpu_holes_domain.py (which runs it on the GPU) and tests/test_holes_domain_host.py (which proves without a
GPU, from a restatement of the geometry of pnp_fill_holes' launches, that every branch is reached by one of the cases).  numpy only; the
yardstick is holes_ref.fill_holes (pinned to scipy by the host file).

A RUN is (name, ncls, classes, max_size): volume(name) builds the uint8 volume once (read-only), `classes` is None (every class) or a tuple,
max_size as pnp_fill_holes takes it.  RUNS is everything the GPU file executes; every volume stays under 60 000 voxels."""
import numpy as np

import holes_ref as R

T0, T1, T2 = 8, 8, 32                      # csrc/components.hip: the tile
COUNT_BLOCK, RUN = 4096, 16                # cc_count_kernel: voxels per workgroup, per lane
SLOTS = 1024                               # its LDS table
THREADS = 256                              # lanes per workgroup of the flat and the face grids
MAX_EXTENT = 4096
SHAPE = R.SHAPE                            # 37 x 29 x 45: three different extents, ragged in every axis

# ---- sweep: every combination of the extents 1, 2, 3 (the smallest interior) and one beyond a tile -----------------------------------
SWEEP_SHAPES = [(a, b, c) for a in (1, 2, 3, 9) for b in (1, 2, 3, 9) for c in (1, 2, 3, 33)]
PIN_SHAPES = [s for s in SWEEP_SHAPES if min(s) >= 3]


def case_sweep(shape):
    """labels 0 .. 4 at random, about 30 % background"""
    rng = np.random.default_rng(1000 * shape[0] + 100 * shape[1] + shape[2])
    return rng.choice(5, size=shape, p=(.3, .175, .175, .175, .175)).astype(np.uint8)


def case_pin(shape):
    """solid class 1 with the voxel (1, 1, 1) cleared: the smallest interior holds the smallest cavity"""
    v = np.ones(shape, np.uint8)
    v[1, 1, 1] = 0
    return v


# ---- faces: a 3 x 3 x 3 cavity in solid class 1 and a one-voxel-wide straight channel to ONE face -----------------------------------------
CAVITY = (18, 14, 22)                      # its centre: three different coordinates, so no channel's face voxel has two equal in-plane ones
FACES = [(ax, side) for ax in range(3) for side in (0, 1)]
FACE_NAMES = {(0, 0): "x0", (0, 1): "x1", (1, 0): "y0", (1, 1): "y1", (2, 0): "z0", (2, 1): "z1"}


def face_voxel(ax, side):
    """where the channel to face (ax, side) meets that face"""
    p = list(CAVITY)
    p[ax] = 0 if side == 0 else SHAPE[ax] - 1
    return tuple(p)


def case_face(ax, side, plugged):
    v = np.ones(SHAPE, np.uint8)
    v[tuple(slice(c - 1, c + 2) for c in CAVITY)] = 0
    sl = list(CAVITY)
    sl[ax] = slice(0, CAVITY[ax] - 1) if side == 0 else slice(CAVITY[ax] + 2, SHAPE[ax])
    v[tuple(sl)] = 0
    if plugged:
        v[face_voxel(ax, side)] = 2
    return v


def plugged_size(ax, side):
    """closed form: the cavity and its channel without the channel's face voxel"""
    return 27 + (CAVITY[ax] - 1 if side == 0 else SHAPE[ax] - CAVITY[ax] - 2) - 1


# ---- lines: the extent limit in each axis, the centre line of a 3 x 3 cross-section cleared ----------------------------------------------
LINE_SHAPES = [(4096, 3, 3), (3, 4096, 3), (3, 3, 4096)]
LINE_KINDS = ("closed", "lo", "hi", "alt")


def case_line(ax, kind):
    """closed: the centre line cleared from 1 to 4094, ONE cavity of 4094 voxels through every tile of the long axis; lo / hi: that line
    extended to index 0 / 4095 (open: in `hi` the only face voxel and the component's root lie at opposite ends of the volume); alt:
    the centre line alternates background (odd indices) and the classes 2, 3, 4: 2047 one-voxel cavities, each won by class 1 with 4 : 2"""
    v = np.ones(LINE_SHAPES[ax], np.uint8)
    line = np.ones(MAX_EXTENT, np.uint8)
    if kind == "alt":
        i = np.arange(MAX_EXTENT)
        line[:] = 2 + (i // 2) % 3
        line[1:MAX_EXTENT - 1:2] = 0
    else:
        line[{"closed": 1, "lo": 0, "hi": 1}[kind]:{"closed": 4095, "lo": 4095, "hi": 4096}[kind]] = 0
    v[tuple(slice(None) if a == ax else 1 for a in range(3))] = line
    return v


# ---- checker: more than SLOTS one-voxel cavities in one count workgroup, all seven nibbles in use ------------------------------------------
CHECKER_SHAPE = (24, 24, 40)


def case_checker():
    """the interior's even-parity voxels are background (each a cavity of its own), everything else carries the classes 1 .. 7.  The plain
    pattern 1 + (3x + 5y + z // 2) % 7 makes every cavity a tie; the term (x y) // 3 breaks the symmetry for about two thirds of them."""
    x, y, z = np.indices(CHECKER_SHAPE)
    v = (1 + (3 * x + 5 * y + z // 2 + (x * y) // 3) % 7).astype(np.uint8)
    inner = np.zeros(CHECKER_SHAPE, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    v[inner & ((x + y + z) % 2 == 0)] = 0
    return v


# ---- nibbles: the packed per-voxel contact counts at their limits, ncls = 8 ----------------------------------------------------------
NIBBLE_SHAPE = (12, 12, 40)
NIBBLE_SIX = (8, 8, 32)                    # six neighbours of class 7, one in each of six other tiles' directions: bits 28 .. 31 hold 6
NIBBLE_MIXED = (4, 5, 6)                   # one neighbour each of the classes 7, 6, 5, 4, 3, 2 in the kernel's reading order: 2 wins
NIBBLE_PAIR = ((3, 9, 20), (3, 9, 21))     # two voxels, ten neighbours: every class once and class 4 three times more


def case_nibbles():
    v = np.full(NIBBLE_SHAPE, 7, np.uint8)
    v[NIBBLE_SIX] = 0
    x, y, z = NIBBLE_MIXED
    v[x, y, z] = 0
    for c, (dx, dy, dz) in zip((7, 6, 5, 4, 3, 2), R.STEPS):
        v[x + dx, y + dy, z + dz] = c
    (x, y, z), (_, _, z1) = NIBBLE_PAIR
    v[x, y, z] = v[x, y, z1] = 0
    ring = [(x - 1, y, z), (x + 1, y, z), (x, y - 1, z), (x, y + 1, z), (x, y, z - 1),
            (x - 1, y, z1), (x + 1, y, z1), (x, y - 1, z1), (x, y + 1, z1), (x, y, z1 + 1)]
    for c, p in zip((1, 2, 3, 4, 5, 6, 7, 4, 4, 4), ring):
        v[p] = c
    return v


# ---- balanced: one cavity, more than 256 contacts with each of two classes, decided by ONE contact ----------------------------------------
SLAB_X, SLAB_Y, SLAB_Z = 18, (4, 25), (7, 38)          # the slab x = 18, 21 x 31 = 651 voxels: 651 contacts with each half
BALANCED = {"balanced_low": (52, 51), "balanced_high": (51, 52), "balanced_tie": (52, 52)}       # rim voxels of class 2, of class 3


def slab_rim():
    """the 104 voxels of the plane x = 18 that share a face with the slab, in raster order: each is one contact"""
    (y0, y1), (z0, z1) = SLAB_Y, SLAB_Z
    rim = [(SLAB_X, y, z) for y in (y0 - 1, y1) for z in range(z0, z1)] + [(SLAB_X, y, z) for y in range(y0, y1) for z in (z0 - 1, z1)]
    return sorted(rim)


def case_balanced(name):
    """class 2 below the slab, class 3 above it, class 1 around it in its own plane; the rim's voxels alternate between class 2 and class
    3 until each has its number, the rest is class 4: sums of 651 + 52 against 651 + 51 (either way round) or 703 against 703"""
    k2, k3 = BALANCED[name]
    v = np.ones(SHAPE, np.uint8)
    v[:SLAB_X] = 2
    v[SLAB_X + 1:] = 3
    v[SLAB_X, SLAB_Y[0]:SLAB_Y[1], SLAB_Z[0]:SLAB_Z[1]] = 0
    for i, p in enumerate(slab_rim()):
        c = 2 + i % 2
        if (i // 2 >= k2 and c == 2) or (i // 2 >= k3 and c == 3):
            c = 4
        v[p] = c
    return v


# ---- open: one open background component that fills whole count workgroups, and a cavity inside a block ----------------------------------
def case_open():
    v = R._block(cls=3)
    v[12:15, 12:15, 22:25] = 0
    return v


# ---- options: ncls, the mask and max_size on one volume of the labels 0 .. 7 --------------------------------------------------------
OPTION_NCLS = list(range(2, 9))
OPTION_MASKS = [()] + [(c,) for c in range(1, 8)] + [tuple(k for k in range(1, 8) if k != c) for c in range(1, 8)]


def case_options():
    return R.case_all_labels(seed=26)


def option_size():
    """s: the largest cavity size of the options volume at ncls = 8 (the host test asserts s >= 3: above the fixed 0, 1, 2)"""
    return int(ref("options", 8)[2]["size"].max())


def option_max_sizes():
    s = option_size()
    return [0, 1, 2, s, s + 1, (1 << 31) - 1, 1 << 31, 1 << 32, (1 << 32) + 1, 1 << 40]


_BUILDERS = {"checker": case_checker, "nibbles": case_nibbles, "open": case_open, "options": case_options}
for _s in SWEEP_SHAPES:
    _BUILDERS["sweep_%dx%dx%d" % _s] = lambda _s=_s: case_sweep(_s)
for _s in PIN_SHAPES:
    _BUILDERS["pin_%dx%dx%d" % _s] = lambda _s=_s: case_pin(_s)
for _f in FACES:
    _BUILDERS["leak_" + FACE_NAMES[_f]] = lambda _f=_f: case_face(_f[0], _f[1], False)
    _BUILDERS["plug_" + FACE_NAMES[_f]] = lambda _f=_f: case_face(_f[0], _f[1], True)
for _a in range(3):
    for _k in LINE_KINDS:
        _BUILDERS["line_%s_%s" % ("xyz"[_a], _k)] = lambda _a=_a, _k=_k: case_line(_a, _k)
for _n in BALANCED:
    _BUILDERS[_n] = lambda _n=_n: case_balanced(_n)

_cache = {}


def volume(name):
    if name not in _cache:
        v = _BUILDERS[name]()
        assert v.dtype == np.uint8 and v.flags.c_contiguous and v.size < 60000
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name]


def ref(name, ncls, classes=None, max_size=0):
    """holes_ref.fill_holes, once per run -> (out, stats, info)"""
    key = (name, ncls, classes, max_size)
    if key not in _cache:
        _cache[key] = R.fill_holes(volume(name), ncls, max_size, classes)
    return _cache[key]


def _runs(names, ncls):
    return [(n, ncls, None, 0) for n in names]


SWEEP_RUNS = _runs(["sweep_%dx%dx%d" % s for s in SWEEP_SHAPES] + ["pin_%dx%dx%d" % s for s in PIN_SHAPES], 5)
FACE_RUNS = _runs(["%s_%s" % (k, FACE_NAMES[f]) for f in FACES for k in ("leak", "plug")], 5)
LINE_RUNS = _runs(["line_%s_%s" % (a, k) for a in "xyz" for k in LINE_KINDS], 5)
CHECKER_RUNS = _runs(["checker"], 8)
NIBBLE_RUNS = _runs(["nibbles"], 8)
BALANCED_RUNS = _runs(list(BALANCED), 5)
OPEN_RUNS = _runs(["open"], 5)


def option_runs():
    """needs the reference (for s), so it is a function: 7 values of ncls, 15 masks and 10 size limits"""
    return ([("options", k, None, 0) for k in OPTION_NCLS] + [("options", 8, m, 0) for m in OPTION_MASKS]
            + [("options", 8, None, m) for m in option_max_sizes()])


def all_runs():
    return SWEEP_RUNS + FACE_RUNS + LINE_RUNS + CHECKER_RUNS + NIBBLE_RUNS + BALANCED_RUNS + OPEN_RUNS + option_runs()
