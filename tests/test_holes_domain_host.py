"""not gpu: the host side of tests/test_gpu_holes_domain.py.  (a) tests/holes_ref.py, the yardstick, fills exactly what
scipy.ndimage.binary_fill_holes fills on every volume of tests/holes_domain_cases.py, and the closed forms the GPU file asserts hold for
it.  (b) the geometry of pnp_fill_holes' launches (csrc/components.hip) — fh_open_kernel's six face regions, the face and
the flat grids of 256 lanes, cc_count_kernel's 4096-voxel workgroups with a 1024-slot table and 16-voxel runs, the 4-bit contact nibbles,
the 64-bit size limit — restated in a few lines each: a case list that stops reaching a branch fails here, without a GPU.  (c) the two
preconditions pnp_fill_holes refuses on the host, on host buffers that are never read."""
import ctypes

import numpy as np
import pytest

import components_ref as C
import holes_domain_cases as HD
import holes_ref as R


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------------
def test_restatement_equals_binary_fill_holes_on_every_volume():
    ndimage = pytest.importorskip("scipy.ndimage")
    seen = set()
    for name, ncls, classes, max_size in HD.all_runs():
        v = C.clean(HD.volume(name), ncls)
        bg = v == 0
        want = ndimage.binary_fill_holes(v != 0)
        out, stats, info = HD.ref(name, ncls, classes, max_size)
        assert np.array_equal(out[~bg], v[~bg]), name
        if classes is None and max_size == 0:
            assert np.array_equal(out != 0, want), (name, ncls)
            assert stats[0].tolist() == [info["cavities"], int((want & bg).sum()), 0, 0]
            seen.add((name, ncls))
        else:                                             # masked or size-limited: a subset, and row 0 accounts for what is left
            full = HD.ref(name, ncls)[1]
            assert not ((out != 0) & ~want).any() and stats[0, :2].tolist() == full[0, :2].tolist()
            assert int(((out != 0) & bg).sum()) == stats[0, 1] - stats[0, 3] == stats[1:, 1].sum()
            assert stats[0, 2] == stats[1:, 3].sum() == int((~info["filled"]).sum())
    assert len(seen) == len(HD.SWEEP_RUNS) + 12 + 12 + 1 + 1 + 3 + 1 + len(HD.OPTION_NCLS)


def test_closed_forms_of_sweep_faces_lines_nibbles_and_balanced():
    for shape in HD.SWEEP_SHAPES:
        name = "sweep_%dx%dx%d" % shape
        assert HD.volume(name).shape == shape
        if min(shape) < 3:                               # no interior: nothing is fillable
            out, stats, _ = HD.ref(name, 5)
            assert not stats.any() and np.array_equal(out, HD.volume(name))
    assert len(HD.SWEEP_SHAPES) == 64 and len(HD.PIN_SHAPES) == 8
    for shape in HD.PIN_SHAPES:
        out, stats, _ = HD.ref("pin_%dx%dx%d" % shape, 5)
        assert (out == 1).all() and stats.tolist() == [[1, 1, 0, 0], [1, 1, 1, 0]] + [[0] * 4] * 3
    assert len(set(HD.CAVITY)) == 3
    for ax, side in HD.FACES:
        f = HD.face_voxel(ax, side)
        inplane = [f[a] for a in range(3) if a != ax]
        assert inplane[0] != inplane[1] and all(0 < f[a] < HD.SHAPE[a] - 1 for a in range(3) if a != ax)
        leak, plug = HD.volume("leak_" + HD.FACE_NAMES[ax, side]), HD.volume("plug_" + HD.FACE_NAMES[ax, side])
        assert leak.shape == HD.SHAPE and leak[f] == 0 and plug[f] == 2 and int((leak != plug).sum()) == 1
        out, stats, _ = HD.ref("leak_" + HD.FACE_NAMES[ax, side], 5)
        assert not stats.any() and np.array_equal(out, leak)
        out, stats, _ = HD.ref("plug_" + HD.FACE_NAMES[ax, side], 5)
        s = HD.plugged_size(ax, side)
        assert stats.tolist() == [[1, s, 0, 0], [1, s, s, 0]] + [[0] * 4] * 3 and out[f] == 2 and int((out == 1).sum()) == out.size - 1
    assert [HD.plugged_size(*f) for f in HD.FACES] == [43, 43, 39, 39, 47, 47]
    for ax, a in enumerate("xyz"):
        assert HD.volume("line_%s_closed" % a).shape == HD.LINE_SHAPES[ax]
        out, stats, _ = HD.ref("line_%s_closed" % a, 5)
        assert stats.tolist() == [[1, 4094, 0, 0], [1, 4094, 4094, 0]] + [[0] * 4] * 3 and (out == 1).all()
        for kind in ("lo", "hi"):
            out, stats, info = HD.ref("line_%s_%s" % (a, kind), 5)
            assert info["cavities"] == 0 and not stats.any() and int((out == 0).sum()) == 4095
        out, stats, info = HD.ref("line_%s_alt" % a, 5)
        assert stats.tolist() == [[2047, 2047, 0, 0], [2047, 2047, 1, 0]] + [[0] * 4] * 3 and info["ties"] == 0
        assert (info["contacts"][:, 1] == 4).all() and (info["contacts"][:, 2:].sum(axis=1) == 2).all()
    out, stats, info = HD.ref("nibbles", 8)
    assert out[HD.NIBBLE_SIX] == 7 and out[HD.NIBBLE_MIXED] == 2 and out[HD.NIBBLE_PAIR[0]] == 4 and out[HD.NIBBLE_PAIR[1]] == 4
    assert stats.tolist() == [[3, 4, 0, 0], [0] * 4, [1, 1, 1, 0], [0] * 4, [1, 2, 2, 0], [0] * 4, [0] * 4, [1, 1, 1, 0]]
    assert info["contacts"].tolist() == [[0, 1, 1, 1, 4, 1, 1, 1], [0, 0, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 6]]       # by root: pair, mixed, six
    assert len(HD.slab_rim()) == 104 and len(set(HD.slab_rim())) == 104
    for name, (k2, k3) in HD.BALANCED.items():
        out, stats, info = HD.ref(name, 5)
        win = 2 if k2 >= k3 else 3
        assert info["cavities"] == 1 and info["contacts"].tolist() == [[0, 0, 651 + k2, 651 + k3, 104 - k2 - k3]]
        assert stats[0].tolist() == [1, 651, 0, 0] and stats[win].tolist() == [1, 651, 651, 0] and stats[1:, 0].sum() == 1
        assert (out[HD.SLAB_X, HD.SLAB_Y[0]:HD.SLAB_Y[1], HD.SLAB_Z[0]:HD.SLAB_Z[1]] == win).all()
    out, stats, info = HD.ref("open", 5)
    assert stats.tolist() == [[1, 27, 0, 0], [0] * 4, [0] * 4, [1, 27, 27, 0], [0] * 4]


def test_the_checkerboard_has_ties_and_clear_winners_and_crowds_the_table():
    out, stats, info = HD.ref("checker", 8)
    cc = np.sort(info["contacts"][:, 1:], axis=1)
    clear = int((cc[:, -1] > cc[:, -2]).sum())
    assert (info["cavities"], info["ties"], clear) == (9196, 3477, 5719) and (info["size"] == 1).all()
    assert info["ties"] >= 100 and clear >= 100 and (stats[1:, 0] > 0).all(), "every class wins somewhere"
    assert _max_roots_per_count_group("checker", 8) == 1794 > HD.SLOTS


def test_the_options_volume():
    s = HD.option_size()
    _, stats, info = HD.ref("options", 8)
    assert s >= 3 and s in info["size"] and s + 1 not in info["size"] and info["cavities"] > 50
    assert HD.option_max_sizes() == [0, 1, 2, s, s + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 32 + 1, 2 ** 40]
    assert len(HD.OPTION_MASKS) == 15 and () in HD.OPTION_MASKS and HD.OPTION_NCLS == [2, 3, 4, 5, 6, 7, 8]
    for m in (2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 32 + 1, 2 ** 40):           # no limit in effect: a truncated 2^32 + 1 would be 1
        assert np.array_equal(HD.ref("options", 8, None, m)[1], stats)
    assert not np.array_equal(HD.ref("options", 8, None, 1)[1], stats)
    assert HD.ref("options", 8, None, s)[1][0, 2] == 0 and HD.ref("options", 8, None, s - 1)[1][0, 2] >= 1


# ---- (b) the launches' geometry ------------------------------------------------------------------------------------------------------
def open_regions(shape):
    """fh_open_kernel's lane -> face voxel map: [((axis, side), voxels int64 [m, 3])] in lane order"""
    D0, D1, D2 = shape
    out = []
    for ax, (rows, cols) in enumerate(((D1, D2), (D0, D2), (D0, D1))):
        j = np.arange(rows * cols)
        q, r = j // cols, j % cols                       # j / D2, j % D2 twice, then j / D1, j % D1
        for side in (0, 1):
            at = np.full(len(j), 0 if side == 0 else shape[ax] - 1)
            out.append(((ax, side), np.stack([at, q, r] if ax == 0 else [q, at, r] if ax == 1 else [q, r, at], axis=1)))
    return out


def _face_mask(shape):
    face = np.ones(shape, dtype=bool)
    face[tuple(slice(1, -1) for _ in range(3))] = False
    return face


def test_the_restated_face_decode_covers_the_faces():
    for shape in ((1, 1, 1), (2, 3, 9), (3, 3, 3), (9, 2, 33), HD.SHAPE, (4096, 3, 3)):
        regs = open_regions(shape)
        assert sum(len(p) for _, p in regs) == 2 * (shape[1] * shape[2] + shape[0] * shape[2] + shape[0] * shape[1])
        hit = np.zeros(shape, dtype=bool)
        for _, p in regs:
            hit[tuple(p.T)] = True
        assert np.array_equal(hit, _face_mask(shape))


def _bg_roots(name, ncls):
    key = ("roots", name, ncls)
    if key not in HD._cache:
        HD._cache[key] = C.roots((C.clean(HD.volume(name), ncls) == 0).astype(np.uint8), 2, 1)
    return HD._cache[key]


def _count_groups(name, ncls):
    """per 4096-voxel workgroup of cc_count_kernel: (distinct background roots, all voxels of one root)"""
    r = _bg_roots(name, ncls).reshape(-1)
    for at in range(0, r.size, HD.COUNT_BLOCK):
        blk = r[at:at + HD.COUNT_BLOCK]
        distinct = len(np.unique(blk[blk >= 0]))
        yield distinct, len(blk) == HD.COUNT_BLOCK and distinct == 1 and bool((blk >= 0).all())


def _max_roots_per_count_group(name, ncls):
    return max(d for d, _ in _count_groups(name, ncls))


def _neighbour_counts(v, ncls):
    """[ncls, D0, D1, D2]: how many of a voxel's face neighbours inside the volume carry class c"""
    cnt = np.zeros((ncls,) + v.shape, dtype=np.int64)
    for o in R.STEPS:
        dst = tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip(o, v.shape))
        src = tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip(o, v.shape))
        for c in range(1, ncls):
            cnt[(c,) + dst] += v[src] == c
    return cnt


_reach = {}


def _reached_by_volume(name, ncls):
    """the branches a volume reaches under the default options (every class, no size limit)"""
    if (name, ncls) in _reach:
        return _reach[(name, ncls)]
    v = C.clean(HD.volume(name), ncls)
    out, stats, info = HD.ref(name, ncls)
    n, shape = v.size, v.shape
    b = set()
    for ax, d in enumerate(shape):
        if d in (1, 2, 3, HD.MAX_EXTENT):
            b.add(("extent", ax, d))
    if n < HD.RUN:
        b.add("n<16")
    if n % HD.RUN:
        b.add("n%16")
    if n % HD.THREADS:
        b.add("n%256")
    flat = -(-n // HD.THREADS)
    faces = -(-2 * (shape[1] * shape[2] + shape[0] * shape[2] + shape[0] * shape[1]) // HD.THREADS)
    if faces > flat:
        b.add("face_grid>flat_grid")
    if flat > faces:
        b.add("flat_grid>face_grid")
    for distinct, single in _count_groups(name, ncls):
        if distinct > HD.SLOTS:
            b.add("count_crowded")                       # more roots than slots: some run must find all its kProbes slots taken
        if single:
            b.add("count_single_root")
    # one background voxel on the faces, on ONE face, with two different in-plane coordinates (a transposed decode marks another voxel),
    # and the reference fills a cavity once it is plugged: that lane of fh_open_kernel alone keeps the cavity open
    leaks = np.argwhere((v == 0) & _face_mask(shape))
    if len(leaks) == 1:
        f = tuple(int(c) for c in leaks[0])
        regs = [reg for reg, p in open_regions(shape) if (p == leaks[0]).all(axis=1).any()]
        plugged = v.copy()
        plugged[f] = 1
        if len(regs) == 1 and R.fill_holes(plugged, ncls)[2]["cavities"] == info["cavities"] + 1:
            ax = regs[0][0]
            inplane = [f[a] for a in range(3) if a != ax]
            if inplane[0] != inplane[1]:
                b.add(("open_sole",) + regs[0])
            root = np.unravel_index(int(_bg_roots(name, ncls)[f]), shape)
            for a in range(3):
                if abs(int(root[a]) - f[a]) >= HD.MAX_EXTENT - 2:
                    b.add(("open_mark_travels", a))      # the face voxel and the root it marks lie at opposite ends of the volume
    cavity = (v == 0) & (out != 0)                        # the default options fill every cavity
    if cavity.any():
        cnt = _neighbour_counts(v, ncls)
        if ncls == 8 and (cnt[7][cavity] == 6).any():
            b.add("nibble6_class7")                       # bits 28 .. 31 of the packed word hold 6
        if ((cnt[1:] > 0).sum(axis=0)[cavity] == 6).any():
            b.add("six_nibbles")
    cc = np.sort(info["contacts"][:, 1:], axis=1) if ncls > 2 else np.zeros((0, 2), np.int64)
    for k in range(len(cc)):
        hi, lo = int(cc[k, -1]), int(cc[k, -2])
        if hi == lo:
            b.add("tie")
            if lo > 256:
                b.add("tie_over256")
        if hi - lo == 1 and lo > 256:
            row = info["contacts"][k].tolist()
            b.add(("margin1_over256", "lower_wins" if row.index(hi) < row.index(lo) else "higher_wins"))
    _reach[(name, ncls)] = b
    return b


def reached_by(run):
    name, ncls, classes, max_size = run
    b = set(_reached_by_volume(name, ncls))
    _, stats, info = HD.ref(name, ncls, classes, max_size)
    sizes = set(info["size"].tolist())
    if max_size and max_size in sizes:
        b.add(("max_size", "a_size"))
    if max_size and max_size - 1 in sizes and max_size not in sizes:
        b.add(("max_size", "a_size+1"))
    if sizes and 2 ** 31 <= max_size < 2 ** 32:
        b.add(("max_size", "negative_as_int32"))
    if sizes and max_size > 2 ** 32 and 0 < max_size % 2 ** 32 < max(sizes):
        b.add(("max_size", "low_32_bits_below_a_cavity"))
    if classes == () and info["cavities"] > 0 and stats[0, 2] == info["cavities"] and stats[0, 3] == stats[0, 1] > 0:
        b.add("empty_mask_all_left")
    return b


def reached(runs):
    out = set()
    for run in runs:
        out |= reached_by(run)
    return out


def wanted():
    w = {"n<16", "n%16", "n%256", "face_grid>flat_grid", "flat_grid>face_grid", "count_crowded", "count_single_root", "nibble6_class7",
         "six_nibbles", "tie", "tie_over256", ("margin1_over256", "lower_wins"), ("margin1_over256", "higher_wins"), ("max_size", "a_size"),
         ("max_size", "a_size+1"), ("max_size", "negative_as_int32"), ("max_size", "low_32_bits_below_a_cavity"), "empty_mask_all_left"}
    for ax in range(3):
        w |= {("extent", ax, d) for d in (1, 2, 3, HD.MAX_EXTENT)}
        w |= {("open_sole", ax, 0), ("open_sole", ax, 1), ("open_mark_travels", ax)}
    return w


def test_every_branch_of_the_fill_is_reached():
    got = reached(HD.all_runs())
    assert got == wanted(), (sorted(map(str, wanted() - got)), sorted(map(str, got - wanted())))


def test_a_missing_case_is_noticed():
    """the assertion above is real: without the only case that reaches a branch it fails"""
    runs = HD.all_runs()
    without = lambda *names: [r for r in runs if r[0] not in names]
    for ax, side in HD.FACES:
        assert wanted() - reached(without("leak_" + HD.FACE_NAMES[ax, side])) == {("open_sole", ax, side)}
    assert wanted() - reached(without("checker", "line_z_alt")) == {"count_crowded"}       # the z line: 2047 roots in one row of 4096 voxels
    assert _max_roots_per_count_group("line_z_alt", 5) == 2047 and _max_roots_per_count_group("line_x_alt", 5) <= 456
    assert wanted() - reached(without("open")) == {"count_single_root"}
    assert wanted() - reached(without("nibbles")) == {"nibble6_class7"}       # six different classes also occur in the checkerboard
    assert wanted() - reached(without("balanced_high")) == {("margin1_over256", "higher_wins")}
    assert wanted() - reached(without("balanced_low")) == {("margin1_over256", "lower_wins")}
    assert wanted() - reached(without("balanced_tie")) == {"tie_over256"}
    assert wanted() - reached(without("line_y_hi")) == {("open_mark_travels", 1)}
    assert wanted() - reached(without(*["line_x_" + k for k in HD.LINE_KINDS])) == {("extent", 0, 4096), ("open_mark_travels", 0)}
    assert "n<16" in wanted() - reached([r for r in runs if not r[0].startswith("sweep")])
    s = HD.option_size()
    for m, branch in (((1, 2, s), "a_size"), ((s + 1,), "a_size+1"), ((2 ** 31,), "negative_as_int32"), ((2 ** 32 + 1,), "low_32_bits_below_a_cavity")):
        assert wanted() - reached([r for r in runs if r[3] not in m]) == {("max_size", branch)}       # 1 and 2 are cavity sizes too
    assert wanted() - reached([r for r in runs if r[2] != ()]) == {"empty_mask_all_left"}


# ---- (c) the two preconditions --------------------------------------------------------------------------------------------------------
def test_a_misaligned_workspace_and_a_partial_overlap_are_refused_on_the_host(built):
    """decided before any HIP call, like tests/test_holes_host.py's refusals: host buffers that are never read.  A call that passes both
    checks is still refused here, by the workspace size that is checked after them: no call ever reaches the device."""
    lib = built._lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) // 256 * 256 + 4096
    D, n = (4, 5, 6), 120
    need = int(lib.pnp_fill_holes_workspace_bytes(D[0], D[1], D[2], 5))
    assert 4096 + 2 * n + 4096 + need + 16 < 1 << 16
    vol, ws = base, base + 8192

    def fill(vol=vol, out=vol, ws=ws, wsb=need):
        p = ctypes.c_void_p
        return lib.pnp_fill_holes(p(vol), D[0], D[1], D[2], 5, 0b11110, 0, p(out), p(ws), p(ws), wsb, None)

    def refused(rc, text):
        msg = lib.pnp_last_error()
        assert rc == -1 and text in msg, (rc, msg)

    for off in (1, 2, 4, 8, 15, 17, 24):
        refused(fill(ws=ws + off), b"pnp_fill_holes: ws must be 16-byte aligned")
    for off in (1, -1, 7, n - 1, 1 - n, n // 2):
        refused(fill(out=vol + off), b"pnp_fill_holes: out overlaps vol")
    refused(fill(out=vol + 1, ws=ws + 4), b"pnp_fill_holes: ws must be 16-byte aligned")
    # what is legal passes both: an aligned workspace at 16 and 32 bytes, out == vol, out next to vol on either side, out far away
    for kw in ({"ws": ws + 16}, {"ws": ws + 32}, {"out": vol}, {"out": vol + n}, {"out": vol - n}, {"out": vol + 1000}):
        refused(fill(wsb=need - 1, **kw), b"pnp_fill_holes: workspace too small")
