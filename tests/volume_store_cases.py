"""The case lists of tests/test_gpu_paste_domain.py, tests/test_gpu_smooth_domain.py and tests/test_gpu_gather_domain.py (which run them on
the GPU) and tests/test_volume_store_host.py (which proves without a GPU, from restatements of the store paths of csrc/paste.hip and of
the launch geometry of csrc/smooth.hip, that every branch is reached by one of them).  numpy only.

  paste    SWEEP (the z-fastest store paths), AXIS_FIRST, INSTANCES (every template instantiation), FOV_* (the closed field of view),
           WILD_MAPS (maps that leave the plane), EXTENT_* (extents 1 .. 4096)
  smooth   ONEHOT_SHAPES / LONG_SHAPES, TAPS, ROUTE_SHAPES, ROW_CASES; smooth_plan / launch_axis / launch_z restate the host side of
           csrc/smooth.hip, smooth_calls() lists every call of the GPU file as (shape, radii, in place, src aligned, dst aligned)
  gather   ONEHOT_SIZES, PRE_SIZES, PRE_PERCENTILES
"""
import collections
import itertools

import numpy as np

import paste_ref as R

# =========================================================================================================================================
# paste: the z-fastest store paths (csrc/paste.hip: paste_labels_kernel's three loops, pack_label of the soft kernels)
# =========================================================================================================================================
SWEEP_XY = (5, 7)                          # (X, Y) = (H, W): the identity map
SWEEP_NCLS = 8
SWEEP_SZ = (1, -1)
SWEEP_OFF = (0, 1, 2, 3)                   # elements between the (16-byte aligned) allocation and the box
SWEEP_SY = (12, 13)                        # column pitch: every column on one phase of the 4-byte grid / the columns rotate through them
# 6 and 10 are not in the issue's list {1, 2, 3, 4, 5, 7, 8, 9, 12}: with it no frame count puts head + tail = 2 around a dword (6, 10 or
# 14 frames) nor three head and three tail bytes next to each other (6) or around a dword (10) — combinations that exist
SWEEP_NB = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12)
SWEEP_Z0 = (0, 1)
Setting = collections.namedtuple("Setting", ("sz", "off", "sy", "nb", "z0", "B"))
SWEEP = [Setting(sz, off, sy, nb, z0, nb) for sz in SWEEP_SZ for off in SWEEP_OFF for sy in SWEEP_SY for nb in SWEEP_NB for z0 in SWEEP_Z0]
SWEEP += [Setting(1, 1, 13, 7, 1, 8), Setting(-1, 2, 13, 5, 1, 6)]          # a batch that is not written whole: B = nb + 1
SWEEP_B_MAX = 13                           # the reference launch of the soft kernels: every frame the sweep can ask for


def sweep_label(b, x, y):
    """L(b, x, y) = (b + 3 x + 5 y) mod 8: adjacent frames differ, and so do the frames t and nb - 1 - t of every nb <= 12 (they are
    nb - 1 - 2 t apart: odd, or even and below 8) but frames 0 and 8 of nb = 9, whose neighbours 1 and 7 do differ"""
    return (b + 3 * x + 5 * y) % SWEEP_NCLS


def sweep_logits(B):
    """[B, 5, 7, 8] float32: 4.0 at class L(b, x, y), 0 elsewhere"""
    X, Y = SWEEP_XY
    b, x, y = np.meshgrid(np.arange(B), np.arange(X), np.arange(Y), indexing="ij")
    lg = np.zeros((B, X, Y, SWEEP_NCLS), np.float32)
    np.put_along_axis(lg, sweep_label(b, x, y)[..., None], 4.0, axis=-1)
    return lg


def sweep_layout(s):
    """-> (elements, origin, (sx, sy, sz)): columns `sy` apart, rows Y sy apart, the box `off` elements into the allocation; both signs
    of sz put a column's frames on the same addresses base + z0 .. base + z0 + nb - 1, base = off + x sx + y sy"""
    X, Y = SWEEP_XY
    sx = Y * s.sy
    elems = s.off + X * sx + 4
    if s.sz == 1:
        return elems, s.off, (sx, s.sy, 1)
    return elems, s.off + 2 * s.z0 + s.nb - 1, (sx, s.sy, -1)


def column_bases(s):
    """[X, Y]: the lowest element index of every column's run (== its address mod 4: the allocation is 16-byte aligned)"""
    elems, origin, strides = sweep_layout(s)
    return R.written_index(SWEEP_XY[0], SWEEP_XY[1], s.nb, s.z0, origin, strides).min(axis=0)


def label_store_paths(phase, nb):
    """paste_labels_kernel: bytes up to the first 4-byte boundary, packed dwords, the remaining bytes -> (head, dwords, tail)"""
    head = min((-phase) % 4, nb)
    return head, (nb - head) // 4, (nb - head) % 4


def pack_store_paths(phase, nb):
    """pack_label, call by call: a flush at byte lane 3 or at the last label; four collected labels go out as a dword, fewer as bytes.
    -> (head, dwords, tail, kinds): head = bytes flushed at lane 3 (fewer than four collected), tail = bytes flushed by the last label
    elsewhere, kinds = the flushes that happened, of ("lane3", count) / ("last", count)"""
    head = dwords = tail = 0
    kinds = set()
    first = 0
    for t in range(nb):
        lane = (phase + t) % 4
        if lane == 3 or t == nb - 1:
            n = t - first + 1
            kinds.add(("lane3" if lane == 3 else "last", n))
            if n == 4:
                dwords += 1
            elif lane == 3:
                head += n
            else:
                tail += n
            first = t + 1
    return head, dwords, tail, kinds


def store_combination(phase, nb):
    """(head bytes, tail bytes, any dword) of one column"""
    head, dwords, tail = label_store_paths(phase, nb)
    return head, tail, dwords > 0


def combinations_that_exist(max_nb=16):
    return {store_combination(p, nb) for p in range(4) for nb in range(1, max_nb + 1)}


def sweep_reach(settings):
    """{(sz, head, tail, any dword)} and {(sz, pack_label flush kind)} over every column of the settings"""
    combos, kinds = set(), set()
    for s in settings:
        for phase in np.unique(column_bases(s) % 4):
            combos.add((s.sz,) + store_combination(int(phase), s.nb))
            kinds |= {(s.sz,) + k for k in pack_store_paths(int(phase), s.nb)[3]}
    return combos, kinds


# the slicing axis first, [Z, X, Y] from element 2 of an allocation: sy = +1 and sy = -1 (y flipped)
def axis_first_layout(sy, X, Y, Z):
    return Z * X * Y + 5, 2 + (Y - 1 if sy < 0 else 0), (Y, sy, X * Y)


AXIS_FIRST = [(sy, nb, z0) for sy in (1, -1) for nb, z0 in ((3, 1), (5, 0))]

# ---- every instantiation: what the sweeps of test_gpu_ensemble.py (M in {1, 3, 8} x ncls in {1, 2, 5, 8}), test_gpu_spacing.py (fov: ncls 5),
# test_gpu_tiles.py and test_gpu_fuse.py ({1, 2, 5, 8}) leave out --------------------------------------------------------------------------
ENSEMBLE_CASE, TILES_CASE = "upsample", "pair"
ENSEMBLE_INSTANCES = [(2, 3), (4, 4), (5, 6), (6, 7), (7, 5), (5, 3), (6, 4), (7, 6), (2, 7)]     # (M, ncls): ncls 3, 4, 6, 7 and M 2, 4 .. 7
ENSEMBLE_FOV_INSTANCES = [(2, ncls) for ncls in (1, 2, 3, 4, 6, 7, 8)] + [(5, 5), (6, 3), (7, 4)]
TILES_NCLS = (1, 3, 4, 5, 6, 7, 8)         # the case itself runs at 2
FUSE_INSTANCES = [(M, ncls, n) for ncls in (3, 4, 6, 7) for M, n in ((3, 693), (2, 696))]
# seeds for which the admissible sets follow the cap (tests/test_volume_store_host.py checks it on the reference alone)
ENSEMBLE_SEED, TILES_SEED, FUSE_SEED = 3, 1, 0


def pair_logits(ncls, member, seed=TILES_SEED):
    """tiles_ref.case_logits of the `pair` case with another class count: [B, H, W, ncls] float32, smooth, max|logit| = 10"""
    import tiles_ref as T
    (H, W), _, B = T.CASES[TILES_CASE][:3]
    h, w = max(2, H // 4), max(2, W // 4)
    coarse = np.random.default_rng([seed, 77, ncls, member]).standard_normal((B, h, w, ncls))
    pi, pj = np.meshgrid(np.linspace(0, h - 1, H), np.linspace(0, w - 1, W), indexing="ij")
    up = np.stack([R.interpolate(coarse[b], pi, pj) for b in range(B)])
    return (up * (10.0 / np.abs(up).max())).astype(np.float32)


# ---- the closed field of view: plane (4, 4), 12 x 12 columns, dyadic maps — every coordinate is a float32 number ----------------------------
FOV_HW, FOV_XY = (4, 4), (12, 12)
FOV_MAP_A = np.array([0.5, 0, -1, 0, 0.5, -1], np.float32)          # x = 1 -> -0.5, x = 9 -> 3.5 = H - 0.5: both inside; x = 0, 10, 11 outside
FOV_MAP_B = np.array([0.5, 0, -0.5, 0, 0.5, -0.5], np.float32)      # x = 0 -> -0.5, x = 8 -> 3.5; x = 9 .. 11 outside
FOV_NB, FOV_Z0, FOV_Z, FOV_NCLS, FOV_B, FOV_RAMP, FOV_SEED = 3, 1, 5, 5, 3, 2.0, 0


def fov_logits(member):
    """[B, 4, 4, ncls] float32, smooth (spacing_ref.smooth_plane_logits)"""
    import spacing_ref as S
    return S.smooth_plane_logits(FOV_B, FOV_HW[0], FOV_HW[1], FOV_NCLS, [FOV_SEED, 40, member])


def closed_cover(inv, X, Y, H, W):
    """[X, Y] bool: pi in [-0.5, H - 0.5] and pj in [-0.5, W - 0.5], both ends included"""
    pi, pj = R.coords(inv, X, Y)
    return (pi >= -0.5) & (pi <= H - 0.5) & (pj >= -0.5) & (pj <= W - 0.5)


# ---- maps that leave the plane: every coordinate is NaN, or beyond +-1e29 ---------------------------------------------------------------------
WILD_HW, WILD_XY, WILD_NB, WILD_Z0, WILD_Z, WILD_NCLS = (4, 6), (5, 7), 3, 1, 5, 5


def wild_logits():
    """[3, 4, 6, 5] float32: 4.0 at class (b + 3 i + j + j // 2) mod 5, 0 elsewhere — the four corner pixels of a frame carry four classes"""
    (H, W), B = WILD_HW, WILD_NB
    b, i, j = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    lg = np.zeros((B, H, W, WILD_NCLS), np.float32)
    np.put_along_axis(lg, ((b + 3 * i + j + j // 2) % WILD_NCLS)[..., None], 4.0, axis=-1)
    return lg
WILD_MAPS = collections.OrderedDict([
    ("nan", [np.nan] * 6),                                     # every coordinate NaN: pixel (0, 0)
    ("plus_huge", [0, 0, 1e30, 0, 0, 1e30]),                   # beyond the far corner: pixel (H - 1, W - 1)
    ("minus_huge", [0, 0, -1e30, 0, 0, -1e30]),                # pixel (0, 0)
    ("mixed_huge", [1e30, 0, 1e30, 0, -1e30, -1e30]),          # pi = 1e30 (x + 1), pj = -1e30 (y + 1): pixel (H - 1, 0)
    ("inf_times_zero", [np.inf, 0, 0, 0, np.inf, 0]),          # inf * 0 = NaN in column 0 / row 0, +inf elsewhere
])


def wild_coords(inv, X, Y):
    """(pi, pj) [X, Y] float32: the kernel's two chains in float32 arithmetic (these maps overflow float32 or are NaN: the float64
    coordinates of paste_ref.coords would not do).  Unfused, which is the fused result here: of the two terms of every sum one is 0, or
    one is NaN or infinite, or both have one sign."""
    m = np.asarray(inv, np.float32)
    x = np.arange(X, dtype=np.float32)[:, None] * np.ones((1, Y), np.float32)
    y = np.arange(Y, dtype=np.float32)[None, :] * np.ones((X, 1), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple((a * x + (b * y + c)).astype(np.float32) for a, b, c in ((m[0], m[1], m[2]), (m[3], m[4], m[5])))


def wild_pixel(inv, X, Y, H, W):
    """(i, j) [X, Y]: the pixel the clamp takes: fmaxf(NaN, 0) = 0, then fminf with the far border.  Every coordinate is NaN, <= -1 or
    >= the far border + 1: outside the closed field of view, and on a pixel that no rounding moves."""
    out = []
    for p, n in zip(wild_coords(inv, X, Y), (H, W)):
        assert np.all(np.isnan(p) | (p <= -1) | (p >= n)), "a coordinate inside the plane"
        with np.errstate(invalid="ignore"):
            out.append(np.where(np.isnan(p) | (p <= -1), 0, n - 1).astype(np.int64))
    return out[0], out[1]


# ---- extents --------------------------------------------------------------------------------------------------------------------------------
EXTENT_XY = [(1, 1), (1, 65), (65, 1), (3, 85), (16, 16), (257, 1), (1, 257), (19, 27), (4096, 2), (2, 4096)]
EXTENT_HW = [(1, 1), (1, 6), (6, 1), (4, 6)]
EXTENT_NB, EXTENT_B, EXTENT_Z0, EXTENT_Z, EXTENT_NCLS = 2, 2, 1, 4, 5
EXTENT_LAYOUTS = ("c", "zfirst_flipped")                        # paste_ref.layout: one z-fastest, one with the slicing axis first
EXTENT_CASES = [(xy, hw) for xy in EXTENT_XY for hw in EXTENT_HW]
EXTENT_SEED = 0


def extent_maps(XY, HW):
    """two float32 maps: the centre-aligned resize, and the same sheared so that coordinates leave the plane on both sides (the clamp)"""
    (X, Y), (H, W) = XY, HW
    a, b = H / float(X), W / float(Y)
    resize = np.array([a, 0, 0.5 * a - 0.5, 0, b, 0.5 * b - 0.5], np.float32)
    shear = np.array([1.1 * a, 0.07 * b, 0.5 * a - 0.75, -0.05 * a, 1.05 * b, 0.5 * b - 0.4], np.float32)
    return [resize, shear]


def extent_logits(XY, HW, member):
    """[B, H, W, ncls] float32, smooth (spacing_ref.smooth_plane_logits)"""
    import spacing_ref as S
    return S.smooth_plane_logits(EXTENT_B, HW[0], HW[1], EXTENT_NCLS, [EXTENT_SEED, XY[0], XY[1], HW[0], HW[1], member])


# =========================================================================================================================================
# smooth: the host side of csrc/smooth.hip restated
# =========================================================================================================================================
K_TA, K_ZSEG, K_MAX_RADIUS, K_ZMAX_ROUNDS, K_THREADS = 8, 2048, 32, 8, 256
K_ZCAP = 4 * (K_ZSEG + 2 * K_MAX_RADIUS)
Plan = collections.namedtuple("Plan", ("axis", "out", "copy_back", "slots", "steered"))


def smooth_plan(Z, rx, ry, rz, in_place):
    """smooth_plan: the passes (0 = X, 1 = Y, 2 = Z), the buffer each writes (0 = dst, 1 = slot 0, 2 = slot 1), copy_back, the slots in
    use, and `steered`: an intermediate pass that passed over a free dst because the last pass cannot run in place"""
    axis = [a for a, r in enumerate((rx, ry, rz)) if r > 0]
    last_capable = bool(axis) and axis[-1] == 2 and Z <= K_ZSEG
    cur = 0 if in_place else -1
    out, copy_back, steered = [], False, False
    for i in range(len(axis)):
        if i == len(axis) - 1:
            o = 0
            if cur == 0 and not last_capable:
                o, copy_back = 1, True
        else:
            next_last = i + 1 == len(axis) - 1
            for o in range(3):
                barred = o == 0 and next_last and not last_capable
                if o != cur and barred:
                    steered = True
                if o != cur and not barred:
                    break
        out.append(o)
        cur = o
    return Plan(tuple(axis), tuple(out), copy_back, max(out, default=0), steered)


def slot_bytes(n):
    return (4 * n + 255) // 256 * 256


def workspace_bytes(X, Y, Z, rx, ry, rz):
    """pnp_volume_smooth_workspace_bytes: one answer for the in-place and the out-of-place call"""
    return max(smooth_plan(Z, rx, ry, rz, True).slots, smooth_plan(Z, rx, ry, rz, False).slots) * slot_bytes(X * Y * Z)


AxisLaunch = collections.namedtuple("AxisLaunch", ("wide", "inner_v", "chunks", "blocks"))
ZLaunch = collections.namedtuple("ZLaunch", ("nseg", "seg", "m", "blocks", "last_len"))


def launch_axis(outer, n, inner, aligned):
    wide = inner % 4 == 0 and aligned
    inner_v = inner // 4 if wide else inner
    chunks = -(-n // K_TA)
    return AxisLaunch(wide, inner_v, chunks, -(-(outer * chunks * inner_v) // K_THREADS))


def launch_z(rows, Z, r):
    nseg = -(-Z // K_ZSEG)
    seg = Z if nseg == 1 else K_ZSEG
    m = min(K_ZCAP // (4 * (seg + 2 * r)), K_ZMAX_ROUNDS)
    assert m >= 1 and 4 * m * (seg + 2 * r) <= K_ZCAP
    return ZLaunch(nseg, seg, m, -(-rows // (4 * m)) * nseg, Z - (nseg - 1) * seg)


def call_reach(shape, radii, in_place, src_aligned=True, dst_aligned=True):
    """the branches one pnp_volume_smooth call takes"""
    X, Y, Z = shape
    P = smooth_plan(Z, radii[0], radii[1], radii[2], in_place)
    b = set()
    if not P.axis:
        return b
    b.add(("route", P.axis, bool(in_place), Z > K_ZSEG))
    if P.copy_back:
        b.add("copy_back")
    if P.steered:
        b.add("steered")
    ok = {-1: src_aligned, 0: dst_aligned if not in_place else src_aligned, 1: True, 2: True}
    cur = 0 if in_place else -1
    for a, o in zip(P.axis, P.out):
        if a == 2:
            L = launch_z(X * Y, Z, radii[2])
            b |= {("nseg", L.nseg), ("m", "cap" if L.m == K_ZMAX_ROUNDS else L.m)}
            if L.nseg > 1 and L.last_len == 1:
                b.add("last_segment_of_1")
            b.add(("rows", "below" if X * Y < 4 * L.m else "equal" if X * Y == 4 * L.m else "above"))
            if o == cur:
                b.add("z_in_place")
        else:
            outer, n, inner = (1, X, Y * Z) if a == 0 else (X, Y, Z)
            L = launch_axis(outer, n, inner, ok[cur] and ok[o])
            b.add(("vec", "XY"[a], 4 if L.wide else 1))
            if inner % 4 == 0 and not L.wide:
                b.add(("scalar_fallback", "XY"[a]))
            b.add(("extent", "XY"[a], n if n in (1, 7, 8, 9, 15, 16, 17) else "other"))
        cur = o
    return b


ONEHOT_R = (1, 2, 8, 32)
AXIS_EXTENTS = (1, 7, 8, 9, 15, 16, 17)
WIDE_SHAPES = [(13, 6, 8), (9, 5, 4), (5, 2, 2)]
LONG_Z = (2047, 2048, 2049, 4096, 4097)
LONG_XY = [(1, 1), (5, 1), (2, 3)]                                # X * Y in {1, 5, 6}
ONEHOT_SHAPES = ([(n, 3, 5) for n in AXIS_EXTENTS] + [(3, n, 5) for n in AXIS_EXTENTS] + WIDE_SHAPES
                 + [(x, y, z) for z in LONG_Z for x, y in LONG_XY])
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 1)]                       # floats between the allocation and (src, out): one float forces the scalar path


def onehot_taps(r, k):
    w = np.zeros(2 * r + 1, np.float32)
    w[k] = 1.0
    return w


def onehot_filters():
    """(axis, r, k): the only non-zero tap is w[k] = 1, so out[a] = in[clamp(a - r + k)] bit for bit"""
    return [(axis, r, k) for axis in range(3) for r in ONEHOT_R for k in (0, r, 2 * r)]


def gaussian_taps(sigma):
    import prefilter_ref as PF
    return PF.weights(sigma)


ASYM = np.array([0.5, 0.25, 0.125, 0.0625, 0.0625], np.float32)
TAPS = collections.OrderedDict([("asym", ASYM), ("asym_reversed", ASYM[::-1].copy()), ("gauss_0.93", None), ("gauss_8", None)])


def taps(name):
    return TAPS[name] if TAPS[name] is not None else gaussian_taps(float(name.split("_")[1]))


ROUTE_SHAPES = [(6, 5, 40), (3, 2, 2049)]
ROUTE_TAPS = (ASYM, np.array([0.125, 0.5, 0.375], np.float32), np.array([0.0625, 0.125, 0.25, 0.3125, 0.125, 0.0625, 0.0625], np.float32))
ROUTE_RADII = tuple(len(w) // 2 for w in ROUTE_TAPS)              # (2, 1, 3): the radius of an axis when it is filtered; no filter is symmetric
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(range(3), n)]
ROW_COUNTS = (1, 3, 4, 5, 31, 32, 33)
ROW_CASES = [((1, n, 9), 2) for n in ROW_COUNTS] + [((n, 1, 2049), 2) for n in ROW_COUNTS] + [((1, n, 500), 2) for n in (15, 16, 17)]


def smooth_volume(shape, seed=0):
    """float32, finite, no zeros: N(0, 3^2) moved away from 0 by its sign"""
    v = np.random.default_rng([seed] + list(shape)).standard_normal(shape) * 3.0
    return (v + np.where(v >= 0, 0.25, -0.25)).astype(np.float32)


def smooth_calls():
    """every call of tests/test_gpu_smooth_domain.py as (section, shape, (rx, ry, rz), in place, src aligned, dst aligned)"""
    out = []
    for shape in ONEHOT_SHAPES:
        for axis, r, k in onehot_filters():
            radii = tuple(r if a == axis else 0 for a in range(3))
            for so, do in OFFSETS:
                out.append(("onehot", shape, radii, False, so == 0, do == 0))
            for so in (0, 1):
                out.append(("onehot", shape, radii, True, so == 0, so == 0))
        for name in TAPS:
            r = len(taps(name)) // 2
            for in_place, aligned in ((False, True), (True, True), (False, False), (True, False)):
                out.append(("taps", shape, (r, r, r), in_place, aligned, aligned))
    for shape in ROUTE_SHAPES:
        for sub in SUBSETS:
            for a in sub:
                out.append(("route", shape, tuple(ROUTE_RADII[a] if a == b else 0 for b in range(3)), False, True, True))
            radii = tuple(ROUTE_RADII[a] if a in sub else 0 for a in range(3))
            for in_place in (False, True):
                out.append(("route", shape, radii, in_place, True, True))
    for shape, rz in ROW_CASES:
        for in_place in (False, True):
            out.append(("rows", shape, (0, 0, rz), in_place, True, True))
    return out


def smooth_reach(calls):
    b = set()
    for _, shape, radii, in_place, sa, da in calls:
        b |= call_reach(shape, radii, in_place, sa, da)
    return b


def smooth_wanted():
    w = {("vec", a, v) for a in "XY" for v in (1, 4)} | {("nseg", n) for n in (1, 2, 3)}
    w |= {"last_segment_of_1", ("m", "cap"), ("m", 1), ("rows", "below"), ("rows", "equal"), ("rows", "above"), "copy_back", "steered", "z_in_place"}
    w |= {("route", sub, ip, long_) for sub in SUBSETS for ip in (False, True) for long_ in (False, True)}
    w |= {("scalar_fallback", a) for a in "XY"} | {("extent", a, n) for a in "XY" for n in AXIS_EXTENTS}
    return w


# =========================================================================================================================================
# gather and preprocess (csrc/augment.hip)
# =========================================================================================================================================
ONEHOT_NCLS = tuple(range(1, 33))
ONEHOT_SIZES = [(3, 5, 7), (2, 5, 7), (1, 5, 7), (3, 4, 7)]       # B, H, W: B H W mod 4 = 1, 2, 3, 0 — groups cross row and sample borders
ONEHOT_VOLUME = (5, 7, 3)                                         # (X, Y, Z) = (H, W, 3) at most: the identity map reads voxel (i, j)
ONEHOT_ENTRIES_NCLS = (2, 4, 7, 31)                               # also through pnp_aug_slices_z and pnp_aug_slices_warp (G = 0 and G = 2)
GUARD = 64                                                        # floats behind each output


def onehot_label_volume(ncls):
    """uint8 [5, 7, 3]: every label 0 .. ncls + 1 (two beyond the class count) occurs in every frame (35 voxels, ncls + 2 <= 34)"""
    X, Y, Z = ONEHOT_VOLUME
    x, y, z = np.indices(ONEHOT_VOLUME)
    return ((x * Y + y + 11 * z) % (ncls + 2)).astype(np.uint8)


PRE_SIZES = (255, 256, 257, 262143, 262144, 262145, 524289)      # the grid: 1 -> 2 blocks at 256, capped at 1024 blocks = 262144 voxels
PRE_PERCENTILES = (0, 1, 50, 99, 100)
PRE_SMALL = (2, 3, 100, 101)                                      # every percentile 0 .. 100


def pre_values(n, kind="normal"):
    rng = np.random.default_rng([n, len(kind)])
    if kind == "normal":
        return (rng.standard_normal(n) * 300 + 1000).astype(np.float32)
    if kind == "low_byte":                                        # keys that differ in their lowest byte only: 256 neighbouring floats
        return (np.uint32(0x44000000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == "high_byte":                                       # keys that differ in their highest byte only: positive, 2^-125 .. 2^125
        top = rng.choice(np.arange(1, 0x7f, 3, dtype=np.uint32), n)
        return ((top << np.uint32(24)) | np.uint32(0x00400000)).view(np.float32)
    raise KeyError(kind)
