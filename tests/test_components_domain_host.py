"""not gpu: the host side of tests/test_gpu_components_domain.py.  (a) tests/components_ref.py, the yardstick, equals scipy.ndimage.label
on every case of tests/components_domain_cases.py, and the closed forms the GPU file asserts hold for it.  (b) the geometry of
csrc/components.hip — 8 x 8 x 32 tiles, the 13 backward offsets, the border kernel's skip rule, the count kernel's 4096-voxel blocks with
a 1024-slot table and 16-voxel runs, max(keep, 1) rank launches — restated in a few lines each: a case list that stops reaching a branch
fails here, without a GPU."""
import numpy as np
import pytest

import components_domain_cases as CD
import components_ref as R

TILE = (CD.T0, CD.T1, CD.T2)


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------------
def _equals_scipy(v, ncls, conn, r):
    """the body of test_components_host.py::test_restatement_equals_scipy_label: roots == the minimum flat index per scipy label"""
    ndimage = pytest.importorskip("scipy.ndimage")
    st = ndimage.generate_binary_structure(3, conn)
    v = R.clean(v, ncls)
    idx = np.arange(v.size).reshape(v.shape)
    for c in range(1, ncls):
        lab, nl = ndimage.label(v == c, st)
        if nl == 0:
            continue
        mins = np.asarray(ndimage.minimum(idx, lab, np.arange(1, nl + 1))).astype(np.int64)
        assert np.all(np.diff(mins) > 0)
        assert np.array_equal(r[v == c], mins[lab[v == c] - 1])
    assert np.array_equal(r < 0, v == 0)


@pytest.mark.parametrize("conn", CD.CONNS)
def test_restatement_equals_scipy_label_on_every_case(conn):
    for name, ncls in CD.LABEL_CASES + [("filter", 8), ("filter", 2), ("blobs", 5)]:
        _equals_scipy(CD.volume(name), ncls, conn, CD.ref_roots(name, ncls, conn))


def test_filter_reference_against_scipy_sizes():
    """keep_largest's stats on the filter volume are the sizes the volume was built from"""
    for ncls in CD.FILTER_NCLS:
        _, stats, r = CD.ref_filter("filter", ncls, 1, keep=0)
        for c in range(1, ncls):
            sizes = CD.FILTER_SIZES[c]
            assert stats[c].tolist() == [len(sizes), sum(sizes), sum(sizes), max(sizes)]
            got = np.bincount(r[CD.volume("filter") == c])
            assert sorted(got[got > 0].tolist()) == sorted(sizes)
    out, stats, _ = CD.ref_filter("filter", 8, 1, keep=2, min_size=3)
    assert stats[:, 2].tolist() == [0, 9 + 7, 5 + 4, 9, 0, 48 + 33, 3, 0]
    v = CD.volume("filter")
    assert out[0, 0, 0] == 0 and v[0, 0, 0] == 1 and out[0, 12, 8] == 1            # class 1: 9 and 7 stay, both 5s go
    _, stats, _ = CD.ref_filter("filter", 8, 1, keep=1, min_size=0, classes=(7,))
    assert stats[7].tolist() == [9, 18, 2, 2] and stats[1, 2] == stats[1, 1]       # nine equal sizes: the lowest root stays
    # ties within a class, equal sizes in different classes, fewer components than keep, a component larger than 2^16
    assert CD.FILTER_SIZES[1].count(5) == 2 and 5 in CD.FILTER_SIZES[2] and len(CD.FILTER_SIZES[3]) == 1 < max(CD.FILTER_KEEP)
    assert max(len(s) for s in CD.FILTER_SIZES.values()) > max(CD.FILTER_KEEP)
    assert CD.ref_filter("blobs", 5, 1)[1][:, 3].max() > 1 << 16
    masks = [m for m in CD.FILTER_MASKS]
    assert None in masks and () in masks and any(m is not None and len(m) == 1 for m in masks)
    assert set(CD.FILTER_MIN_SIZE) == {0, 1, 3, 4, 1 << 40} and 3 in CD.FILTER_SIZES[1] and CD.FILTER_NCLS == [2, 8]


def test_closed_forms_of_pairs_lines_checkerboard_and_diagonals():
    assert [CD.pairs_components(c, False) for c in CD.CONNS] == [46, 34, 26] and CD.pairs_components(2, True) == 52
    for name, ncls in CD.PAIR_CASES:
        assert CD.volume(name).shape == (34, 34, 98) and int((CD.volume(name) > 0).sum()) == 52
        for conn in CD.CONNS:
            r = CD.ref_roots(name, ncls, conn)
            assert len(np.unique(r)) - 1 == CD.pairs_components(conn, name.startswith("pairs2")), (name, conn)
    for o, slot in zip(CD.OFFSETS26, range(26)):
        a = CD.pair_anchor("corner", o, slot)
        assert a[0] % 8 == 7 and a[1] % 8 == 7 and a[2] % 32 == 31
    for name, (_, first) in CD.DIAGONALS.items():
        for conn in CD.CONNS:
            r = CD.ref_roots(name, 2, conn)
            assert len(np.unique(r)) - 1 == (1 if conn >= first else 40), (name, conn)
    n = 24 * 24 * 40 // 2
    assert [len(np.unique(CD.ref_roots("checker", 2, c))) - 1 for c in CD.CONNS] == [n, 1, 1] and n == 11520
    for name, ncls in CD.LINE_CASES:
        for conn in CD.CONNS:
            r = CD.ref_roots(name, ncls, conn).reshape(-1)
            if name.startswith("solid"):
                assert (r == 0).all()
            else:
                starts = np.cumsum(np.r_[0, np.arange(1, 91)])                    # run k starts at 0 + 1 + ... + k
                assert np.array_equal(np.unique(r), starts) and np.array_equal(r, np.repeat(starts, np.arange(1, 92))[:4096])
    for name, _ in CD.SNAKE_CASES:
        assert set(np.unique(CD.ref_roots(name, 2, 1))) == {-1, 0} and CD.volume(name).shape in ((64, 33, 33), (33, 64, 33))


# ---- (b) the kernels' geometry -------------------------------------------------------------------------------------------------------
def _pairs(v, o):
    """(p, q = p + o) index arrays [3, m] of the same-label foreground pairs of backward offset o"""
    dst = tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip(o, v.shape))
    src = tuple(slice(max(0, d), s - max(0, -d)) for d, s in zip(o, v.shape))
    same = (v[dst] > 0) & (v[dst] == v[src])
    p = np.argwhere(same) + np.array([max(0, -d) for d in o])
    return p.T, (p + np.array(o)).T


def _exempt(p):
    """cc_border_kernel's skip rule: k > 0 && 0 < ly < 7 && 0 < lz < 31 — the voxel has no backward neighbour outside its tile"""
    k, ly, lz = p[0] % CD.T0, p[1] % CD.T1, p[2] % CD.T2
    return (k > 0) & (ly > 0) & (ly < CD.T1 - 1) & (lz > 0) & (lz < CD.T2 - 1)


_reach = {}


def reached_by(name, ncls):
    """the set of branches one labelling case reaches (under the connectivities it runs with: all three)"""
    if (name, ncls) in _reach:
        return _reach[(name, ncls)]
    v = R.clean(CD.volume(name), ncls)
    b = set()
    n = v.size
    for ax, (d, t) in enumerate(zip(v.shape, TILE)):
        if -(-d // t) > 1:
            b.add(("tiles", ax))
        if d % t:
            b.add(("ragged", ax))
        if d in (1, CD.MAX_EXTENT):
            b.add(("extent", ax, d))
    b.add(("n%16", n % CD.RUN != 0))
    if n < CD.RUN:
        b.add("n<16")
    for j, o in enumerate(CD.BACKWARD):
        p, q = _pairs(v, o)
        if p.shape[1] == 0:
            continue
        tp, tq = [p[a] // TILE[a] for a in range(3)], [q[a] // TILE[a] for a in range(3)]
        cross = [tp[a] != tq[a] for a in range(3)]
        anyc = cross[0] | cross[1] | cross[2]
        allc = np.all([cross[a] for a in range(3) if o[a]], axis=0)
        for conn in CD.CONNS:
            if j < CD.NOFF[conn]:
                if anyc.any():
                    b.add(("cross", j, conn))
                if allc.any():
                    b.add(("cross_every_axis", j, conn))
                if (~anyc).any():
                    b.add(("inside", j, conn))
        # the skip rule: the border kernel passes over p but visits its neighbour, or the other way round — both lie in one component
        if (_exempt(p) != _exempt(q)).any():
            b.add("skip_next_to_visit")
    for conn in CD.CONNS:
        r = CD.ref_roots(name, ncls, conn).reshape(-1)
        for at in range(0, n, CD.COUNT_BLOCK):
            blk = r[at:at + CD.COUNT_BLOCK]
            distinct = len(np.unique(blk[blk >= 0]))
            if distinct > CD.SLOTS:
                b.add("count_crowded")                   # more roots than slots: some run must find all its kProbes slots taken
            if len(blk) == CD.COUNT_BLOCK and distinct == 1 and (blk >= 0).all():
                b.add("count_single_root")
    _reach[(name, ncls)] = b
    return b


def reached(cases):
    out = set()
    for name, ncls in cases:
        out |= reached_by(name, ncls)
    return out


def wanted():
    w = {"n<16", ("n%16", True), ("n%16", False), "skip_next_to_visit", "count_crowded", "count_single_root"}
    for ax in range(3):
        w |= {("tiles", ax), ("ragged", ax), ("extent", ax, 1), ("extent", ax, CD.MAX_EXTENT)}
    for conn in CD.CONNS:
        for j in range(CD.NOFF[conn]):
            w |= {("cross", j, conn), ("cross_every_axis", j, conn), ("inside", j, conn)}
    return w


def test_the_restated_offsets_are_the_backward_half():
    assert len(CD.BACKWARD) == 13 and all(o < (0, 0, 0) for o in CD.BACKWARD)
    for conn in CD.CONNS:
        mine = set(CD.BACKWARD[:CD.NOFF[conn]])
        assert mine | {tuple(-d for d in o) for o in mine} == set(R.offsets(conn))
    assert [o for o in CD.BACKWARD if max(o) > 0] == [(-1, 1, 0), (-1, 0, 1), (0, -1, 1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1)]


def test_every_branch_of_the_labelling_and_the_count_kernel_is_reached():
    missing = wanted() - reached(CD.LABEL_CASES)
    assert not missing, sorted(map(str, missing))


def test_the_pair_volumes_alone_reach_every_offset_isolated():
    """in the pair volumes every pair stands alone, so a missing offset loses exactly that pair (the closed-form counts notice)"""
    offs = {k for k in wanted() if isinstance(k, tuple) and k[0] in ("cross", "cross_every_axis")}
    assert not offs - reached([("pairs_corner", 3), ("pairs_straddle", 3)])
    assert not {k for k in offs if k[0] == "cross"} - reached([("pairs_corner", 3)])
    assert not {k for k in wanted() if isinstance(k, tuple) and k[0] == "inside"} - reached([("pairs_interior", 3)])
    assert not {k for k in reached([("pairs_interior", 3)]) if isinstance(k, tuple) and k[0] == "cross"}
    # the chains that do not run along z lean on the x and y unions; the diagonals on the offsets with a positive component
    for name, j in (("anti_xy", 4), ("anti_xz", 6), ("anti_yz", 8), ("anti_xyZ", 10), ("anti_xYz", 11), ("anti_xYZ", 12)):
        assert {("cross", j, 3), ("inside", j, 3)} <= reached_by(name, 2), name


def test_a_missing_case_is_noticed():
    """the assertions above are real: without the only case that reaches a branch they fail"""
    without = lambda *names: [c for c in CD.LABEL_CASES if c[0] not in names]
    assert "count_crowded" in wanted() - reached(without("checker"))
    assert ("extent", 0, 4096) in wanted() - reached(without("solid_4096x1x1", "runs_4096x1x1"))
    assert "count_single_root" in wanted() - reached(without(*["solid_%dx%dx%d" % s for s in CD.LINE_SHAPES]))
    assert "n<16" in wanted() - reached([c for c in CD.LABEL_CASES if not c[0].startswith("sweep")])


def test_rank_launches_and_filter_sweep():
    assert sorted({max(k, 1) for k in CD.FILTER_KEEP}) == list(range(1, 9)) and 0 in CD.FILTER_KEEP
    for ncls in CD.FILTER_NCLS:
        cfg = list(CD.filter_configs(ncls))
        assert all(m is None or all(0 < c < ncls for c in m) for _, _, m in cfg)
        assert {m for _, _, m in cfg} >= {None, (), (1,)} and len(cfg) == 45 * len({m for _, _, m in cfg})
    assert len(list(CD.filter_configs(8))) == 45 * len(CD.FILTER_MASKS)
