"""not gpu: the host side of tests/test_gpu_paste_domain.py, tests/test_gpu_smooth_domain.py and tests/test_gpu_gather_domain.py.
(a) the store paths of csrc/paste.hip's z-fastest columns restated (paste_labels_kernel's three loops, pack_label's flushes): the sweep
reaches every combination of head bytes, tail bytes and dwords that exists, for both signs of sz, and stops doing so when a frame count
is taken away.  (b) smooth_plan, launch_axis and launch_z of csrc/smooth.hip restated and pinned to pnp_volume_smooth_workspace_bytes
through the library: the calls of the smoothing file reach every vector width, segment count, round count, row count and buffer route.
(c) prefilter_ref.smooth_taps against scipy.ndimage.correlate1d.  (d) every case that is checked through an admissible set follows the
house cap on the reference alone.  A case list that stops reaching a branch fails here, without a GPU."""
import numpy as np
import pytest

import ensemble_ref as E
import fuse_ref as F
import paste_ref as R
import prefilter_ref as PF
import tiles_ref as T
import volume_store_cases as C
from test_ensemble_host import _invs as ensemble_maps
from test_tiles_host import case_maps as tiles_maps


# ---- (a) the store paths ---------------------------------------------------------------------------------------------------------------
def test_pack_label_stores_what_the_three_loops_store():
    """the two codes cut a column into the same bytes and dwords: pack_label's flush at lane 3 with fewer than four labels is the head
    loop, its flush by the last label the tail loop (or a head that ends before the boundary)"""
    for phase in range(4):
        for nb in range(1, 17):
            h, d, t = C.label_store_paths(phase, nb)
            ph, pd, pt, kinds = C.pack_store_paths(phase, nb)
            assert h + 4 * d + t == nb == ph + 4 * pd + pt and d == pd
            if nb >= (-phase) % 4:
                assert (h, t) == (ph, pt), (phase, nb)
            else:                                           # the column ends before its first boundary: head bytes there, a tail flush here
                assert (h, t, ph, pt) == (nb, 0, 0, nb)
            assert all(1 <= n <= 4 and (n < 4 or k == "lane3") for k, n in kinds)


def test_the_sweep_reaches_every_store_combination():
    exist = C.combinations_that_exist()
    assert exist == {(h, t, d) for h in range(4) for t in range(4) for d in (False, True)} - {(0, 0, False)}
    combos, kinds = C.sweep_reach(C.SWEEP)
    want = {(sz,) + c for sz in (1, -1) for c in exist}
    assert not want - combos, sorted(want - combos)
    want_kinds = {(sz, "lane3", n) for sz in (1, -1) for n in (1, 2, 3, 4)} | {(sz, "last", n) for sz in (1, -1) for n in (1, 2, 3)}
    assert kinds == want_kinds


def test_a_missing_frame_count_is_noticed():
    """the assertion above is real: without the only frame counts that reach a combination it fails"""
    want = {(sz,) + c for sz in (1, -1) for c in C.combinations_that_exist()}
    without = lambda *nbs: [s for s in C.SWEEP if s.nb not in nbs]
    assert (1, 0, 1, False) in want - C.sweep_reach(without(1))[0]                   # one tail byte alone: nb = 1 on an aligned column
    assert (-1, 3, 3, False) in want - C.sweep_reach(without(6))[0]                  # three head and three tail bytes and no dword
    assert (1, 3, 3, True) in want - C.sweep_reach(without(10))[0]
    lost = want - C.sweep_reach(without(6, 10))[0]                                   # the frame counts of the issue alone
    assert {(1, 2, 0, True), (1, 1, 1, True), (1, 0, 2, True), (1, 3, 3, True), (1, 3, 3, False)} <= lost
    assert not want - C.sweep_reach(without(12))[0]                                  # three dwords add frames, not a combination
    assert {c for c in want if c[0] == -1} <= want - C.sweep_reach([s for s in C.SWEEP if s.sz == 1])[0]
    # the columns of pitch 12 share one phase, those of pitch 13 rotate through all four
    for s in C.SWEEP:
        phases = set((C.column_bases(s) % 4).ravel().tolist())
        assert len(phases) == (1 if s.sy == 12 else 4), s


def test_sweep_layouts_and_labels():
    X, Y = C.SWEEP_XY
    assert set(C.SWEEP_NB) >= {1, 2, 3, 4, 5, 7, 8, 9, 12} and len(C.SWEEP) == 2 * 4 * 2 * len(C.SWEEP_NB) * 2 + 2
    assert sum(s.B == s.nb + 1 for s in C.SWEEP) >= 1 and all(s.nb <= s.B <= C.SWEEP_B_MAX for s in C.SWEEP)
    for s in C.SWEEP:
        elems, origin, strides = C.sweep_layout(s)
        idx = R.written_index(X, Y, s.nb, s.z0, origin, strides)
        assert idx.min() >= s.off and idx.max() < elems and np.unique(idx).size == idx.size
        up = C.sweep_layout(s._replace(sz=1))
        assert np.array_equal(np.sort(idx.ravel()), np.sort(R.written_index(X, Y, s.nb, s.z0, up[1], up[2]).ravel()))
        assert np.array_equal(C.column_bases(s), s.off + np.arange(X)[:, None] * Y * s.sy + np.arange(Y)[None, :] * s.sy + s.z0)
    lg = C.sweep_logits(C.SWEEP_B_MAX)
    lab = np.argmax(lg, -1)
    assert lg.shape == (13, 5, 7, 8) and np.array_equal(np.sort(lg, -1)[..., -2:], np.broadcast_to(np.float32([0, 4]), lab.shape + (2,)))
    assert np.all(lab[1:] != lab[:-1]) and len(np.unique(lab)) == 8
    for nb in C.SWEEP_NB:                                    # frames descending is not frames ascending
        same = [t for t in range(nb) if t != nb - 1 - t and np.array_equal(lab[t], lab[nb - 1 - t])]
        assert same == ([0, 8] if nb == 9 else []), (nb, same)
        assert nb == 1 or not np.array_equal(lab[:nb], lab[:nb][::-1])
    for sy, nb, z0 in C.AXIS_FIRST:
        elems, origin, strides = C.axis_first_layout(sy, X, Y, z0 + nb)
        idx = R.written_index(X, Y, nb, z0, origin, strides)
        assert idx.min() >= 2 and idx.max() < elems - 3 and np.unique(idx).size == idx.size and strides[1] == sy
    assert {sy for sy, _, _ in C.AXIS_FIRST} == {1, -1}


# ---- the other paste lists ---------------------------------------------------------------------------------------------------------------
def test_every_instantiation_is_launched_by_some_sweep():
    assert {n for _, _, n in E.SWEEP} | {n for _, n in C.ENSEMBLE_INSTANCES} == set(range(1, 9))
    assert {m for _, m, _ in E.SWEEP} | {m for m, _ in C.ENSEMBLE_INSTANCES} == set(range(1, 9))
    assert {5} | {n for _, n in C.ENSEMBLE_FOV_INSTANCES} == set(range(1, 9)) and {m for m, _ in C.ENSEMBLE_FOV_INSTANCES} >= {5, 6, 7}
    assert {T.CASES[C.TILES_CASE][7]} | set(C.TILES_NCLS) == set(range(1, 9))
    assert {n for _, n in F.SWEEP} | {n for _, n, _ in C.FUSE_INSTANCES} == set(range(1, 9))
    assert {n for _, _, n in C.FUSE_INSTANCES} == {693, 696}                          # the scalar and the wide path
    assert not set(C.ENSEMBLE_INSTANCES) & {(m, n) for _, m, n in E.SWEEP}             # nothing runs twice


def test_field_of_view_maps_are_exact_and_sit_on_the_borders():
    (H, W), (X, Y) = C.FOV_HW, C.FOV_XY
    for inv in (C.FOV_MAP_A, C.FOV_MAP_B):
        assert T.coords_exact(inv, X, Y)
    assert T.coord_shift([C.FOV_MAP_A, C.FOV_MAP_B], X, Y) == 0.0
    pi, pj = R.coords(C.FOV_MAP_A, X, Y)
    assert pi[1, 0] == -0.5 and pi[9, 0] == H - 0.5 and pj[0, 1] == -0.5 and pj[0, 9] == W - 0.5
    a, b = C.closed_cover(C.FOV_MAP_A, X, Y, H, W), C.closed_cover(C.FOV_MAP_B, X, Y, H, W)
    inside = lambda lo, hi: (np.arange(12) >= lo) & (np.arange(12) <= hi)
    assert np.array_equal(a, np.outer(inside(1, 9), inside(1, 9))) and np.array_equal(b, np.outer(inside(0, 8), inside(0, 8)))
    assert np.array_equal(a, T.member_covers([C.FOV_MAP_A], X, Y, H, W)[0])            # the house restatement agrees
    # an open interval on either side would lose columns: the test distinguishes > from >=
    assert (a & b).sum() == 64 and (a | b).sum() == 98 and a.sum() == 81
    assert T.edge_columns([C.FOV_MAP_A, C.FOV_MAP_B], X, Y, H, W).any()                # test_gpu_tiles.py's check would exempt these columns


def test_wild_maps_leave_the_plane_everywhere():
    (H, W), (X, Y) = C.WILD_HW, C.WILD_XY
    seen = set()
    for name, inv in C.WILD_MAPS.items():
        pi, pj = C.wild_coords(inv, X, Y)
        with np.errstate(invalid="ignore"):
            assert not ((pi >= -0.5) & (pi <= H - 0.5) & (pj >= -0.5) & (pj <= W - 0.5)).any(), name
        i, j = C.wild_pixel(inv, X, Y, H, W)
        seen |= set(zip(i.ravel().tolist(), j.ravel().tolist()))
    assert seen == {(0, 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1)}
    assert np.isnan(C.wild_coords(C.WILD_MAPS["nan"], X, Y)[0]).all()
    lab = np.argmax(C.wild_logits(), -1)
    assert all(len({lab[b, 0, 0], lab[b, 0, W - 1], lab[b, H - 1, 0], lab[b, H - 1, W - 1]}) == 4 for b in range(C.WILD_NB))
    pi, pj = C.wild_coords(C.WILD_MAPS["inf_times_zero"], X, Y)
    assert np.isnan(pi[0]).all() and np.isinf(pi[1:]).all() and np.isnan(pj[:, 0]).all() and np.isinf(pj[:, 1:]).all()


def test_extents():
    assert {1, 4096} <= {x for x, _ in C.EXTENT_XY} and {1, 4096} <= {y for _, y in C.EXTENT_XY} and (1, 1) in C.EXTENT_XY
    assert {(1, 1), (1, 6), (6, 1)} <= set(C.EXTENT_HW) and len(C.EXTENT_CASES) == 40
    assert any(x * y > 256 for x, y in C.EXTENT_XY) and any(x * y == 256 for x, y in C.EXTENT_XY)       # one workgroup exactly, and more
    for xy, hw in C.EXTENT_CASES:
        for kind in C.EXTENT_LAYOUTS:
            elems, origin, strides = R.layout(kind, xy[0], xy[1], C.EXTENT_Z)
            idx = R.written_index(xy[0], xy[1], C.EXTENT_NB, C.EXTENT_Z0, origin, strides)
            assert idx.min() >= 0 and idx.max() < elems
    pi, pj = R.coords(C.extent_maps((19, 27), (4, 6))[1], 19, 27)
    assert pi.min() < 0 and pi.max() > 3 and pj.min() < 0 and pj.max() > 5                              # the sheared map reaches the clamp


# ---- (d) no vacuous bounds ---------------------------------------------------------------------------------------------------------------
CAP = 1e-3


def test_ensemble_instances_follow_the_cap():
    (H, W), (X, Y), B, nb = R.CASES[C.ENSEMBLE_CASE][:4]
    for M, ncls in sorted(set(C.ENSEMBLE_INSTANCES + C.ENSEMBLE_FOV_INSTANCES)):
        if ncls == 1:
            continue
        logits, invs = [E.smooth_logits(C.ENSEMBLE_CASE, ncls, m, C.ENSEMBLE_SEED) for m in range(M)], ensemble_maps(C.ENSEMBLE_CASE, M)
        res, dp = E.ensemble(logits, invs, X, Y, nb), E.delta_p(logits, invs, X, Y, nb)
        multi = int((E.admissible(res.prob, dp).sum(-1) > 1).sum())
        assert E.K_ROUND * E.U < dp < 1e-4 and multi <= CAP * nb * X * Y, (M, ncls, multi, dp)
        assert len(np.unique(res.label)) == ncls


def test_tiles_instances_follow_the_cap():
    (H, W), (X, Y), B, nb = T.CASES[C.TILES_CASE][:4]
    ramp, invs = T.CASES[C.TILES_CASE][8], tiles_maps(C.TILES_CASE)
    edge = T.edge_columns(invs, X, Y, H, W)
    assert not edge.any()
    for ncls in C.TILES_NCLS:
        logits = [C.pair_logits(ncls, m) for m in range(len(invs))]
        assert logits[0].shape == (B, H, W, ncls) and abs(float(np.abs(logits[0]).max()) - 10.0) < 1e-5
        res, dp = T.tiles(logits, invs, X, Y, ramp, nb), T.delta_p_tiles(logits, invs, X, Y, nb)
        multi = int((E.admissible(res.prob, dp).sum(-1) > 1)[:, res.covered].sum()) if ncls > 1 else 0
        assert T.k_tiles(len(invs)) * T.U < dp < 2e-4 and multi <= CAP * nb * int(res.covered.sum()), (ncls, multi, dp)


def test_fuse_instances_follow_the_cap():
    for M, ncls, n in C.FUSE_INSTANCES:
        probs, w = F.make_case(M, ncls, n, C.FUSE_SEED)
        for weights in (w, None):
            ref = F.fuse(probs, weights)
            assert F.ambiguous(ref, M) <= 2 and int(ref.covered.sum()) >= 0.5 * n and len(np.unique(ref.label[ref.covered])) == ncls


def test_field_of_view_cases_follow_the_cap():
    """432 voxels: no voxel may admit a second class"""
    (H, W), (X, Y), nb = C.FOV_HW, C.FOV_XY, C.FOV_NB
    logits, invs = [C.fov_logits(m) for m in range(2)], [C.FOV_MAP_A, C.FOV_MAP_B]
    _, r = R.labels(logits[0], invs[0], X, Y, nb)
    assert not (R.admissible(r, R.delta(logits[0][:nb], invs[0], X, Y)).sum(-1) > 1).any()
    res = E.ensemble(logits, invs, X, Y, nb)
    assert not (E.admissible(res.prob, E.delta_p(logits, invs, X, Y, nb)).sum(-1) > 1).any() and len(np.unique(res.label)) >= 3
    til = T.tiles(logits, invs, X, Y, C.FOV_RAMP, nb)
    assert not (E.admissible(til.prob, T.delta_p_tiles(logits, invs, X, Y, nb)).sum(-1) > 1)[:, til.covered].any()
    assert np.array_equal(til.covered, C.closed_cover(invs[0], X, Y, H, W) | C.closed_cover(invs[1], X, Y, H, W))


def test_extent_cases_follow_the_cap():
    worst = 0.0
    for xy, hw in C.EXTENT_CASES:
        logits, invs = [C.extent_logits(xy, hw, m) for m in range(2)], C.extent_maps(xy, hw)
        n = C.EXTENT_NB * xy[0] * xy[1]
        for lg, inv in zip(logits, invs):
            _, r = R.labels(lg, inv, xy[0], xy[1], C.EXTENT_NB)
            d = R.delta(lg[:C.EXTENT_NB], inv, xy[0], xy[1])
            multi = int((R.admissible(r, d).sum(-1) > 1).sum())
            assert d < 1e-4 and multi <= CAP * n, (xy, hw, multi, d)
        res, dp = E.ensemble(logits, invs, xy[0], xy[1], C.EXTENT_NB), E.delta_p(logits, invs, xy[0], xy[1], C.EXTENT_NB)
        multi = int((E.admissible(res.prob, dp).sum(-1) > 1).sum())
        worst = max(worst, multi / n)
        assert dp < 1e-4 and multi <= CAP * n, (xy, hw, multi, dp)
    print("extents: the largest share of voxels that admit more than one class: %.2e" % worst)


# ---- (b) the smoothing geometry ----------------------------------------------------------------------------------------------------------
CALLS = C.smooth_calls()


def test_the_restated_plan_is_the_library_s(built):
    lib = built._lib.load()
    seen = set()
    for _, shape, radii, _, _, _ in CALLS:
        if (shape, radii) not in seen:
            seen.add((shape, radii))
            assert lib.pnp_volume_smooth_workspace_bytes(*shape, *radii) == C.workspace_bytes(*shape, *radii), (shape, radii)
    assert len(seen) > 500
    # beyond the calls: every subset of axes on both sides of kZSeg, and the figures of tests/test_prefilter_host.py
    for Z in (1, 4, 2047, 2048, 2049, 4096, 4097):
        for radii in [(a, b, c) for a in (0, 1) for b in (0, 32) for c in (0, 3)]:
            assert lib.pnp_volume_smooth_workspace_bytes(3, 2, Z, *radii) == C.workspace_bytes(3, 2, Z, *radii), (Z, radii)
    assert C.workspace_bytes(4, 4, 4, 1, 1, 0) == 256 and C.workspace_bytes(4, 4, 4, 0, 0, 1) == 0 and C.workspace_bytes(2, 2, 4096, 1, 1, 1) == 2 * 65536


def test_the_restated_plan_by_hand():
    """the comment above smooth_plan in csrc/smooth.hip, case by case"""
    P = C.smooth_plan
    assert P(40, 2, 1, 3, False)[:4] == ((0, 1, 2), (0, 1, 0), False, 1)              # X -> dst, Y -> slot 0, Z -> dst
    assert P(40, 2, 1, 3, True)[:4] == ((0, 1, 2), (1, 0, 0), False, 1)               # in place: X -> slot 0, Y -> dst, Z in place
    assert P(2049, 2, 1, 3, False)[:4] == ((0, 1, 2), (0, 1, 0), False, 1)            # Y must leave dst to the last pass: it does anyway
    assert P(2049, 2, 1, 3, True)[:4] == ((0, 1, 2), (1, 2, 0), False, 2)             # in place and long rows: both slots
    assert P(40, 2, 1, 0, False)[:4] == ((0, 1), (1, 0), False, 1) and P(40, 2, 1, 0, False).steered      # X passes over the free dst
    assert P(2049, 0, 1, 3, False).steered and not P(40, 0, 1, 3, False).steered and P(40, 0, 1, 3, False).out == (0, 0)
    assert P(40, 0, 0, 3, True)[:4] == ((2,), (0,), False, 0)                         # the z pass of a short row in place
    assert P(2049, 0, 0, 3, True)[:4] == ((2,), (1,), True, 1) and P(40, 2, 0, 0, True)[:4] == ((0,), (1,), True, 1)
    assert P(40, 0, 0, 0, True)[:4] == ((), (), False, 0)
    assert C.K_ZCAP == 8448 and C.launch_z(5, 9, 2) == (1, 9, 8, 1, 9) and C.launch_z(33, 9, 2).blocks == 2
    assert C.launch_z(5, 2049, 2) == (2, 2048, 1, 4, 1) and C.launch_z(6, 4097, 32) == (3, 2048, 1, 6, 1) and C.launch_z(16, 500, 2).m == 4
    assert C.launch_axis(1, 13, 48, True) == (True, 12, 2, 1) and C.launch_axis(1, 13, 48, False) == (False, 48, 2, 1)
    assert C.launch_axis(13, 6, 8, True) == (True, 2, 1, 1) and C.launch_axis(3, 17, 5, True) == (False, 5, 3, 1)


def test_the_smoothing_calls_reach_every_branch():
    missing = C.smooth_wanted() - C.smooth_reach(CALLS)
    assert not missing, sorted(map(str, missing))


def test_a_missing_smoothing_case_is_noticed():
    without = lambda keep: [c for c in CALLS if keep(c)]
    W = C.smooth_wanted()
    assert ("nseg", 3) in W - C.smooth_reach(without(lambda c: c[1][2] != 4097))
    assert "last_segment_of_1" in W - C.smooth_reach(without(lambda c: c[1][2] not in (2049, 4097)))
    assert "steered" in W - C.smooth_reach(without(lambda c: c[0] not in ("route", "taps")))          # it takes two passes or more
    assert ("route", (0, 1), True, True) in W - C.smooth_reach(without(lambda c: c[1] != (3, 2, 2049)))
    assert ("rows", "equal") in W - C.smooth_reach(without(lambda c: c[0] != "rows"))
    assert {("scalar_fallback", "X"), ("scalar_fallback", "Y")} <= W - C.smooth_reach(without(lambda c: c[4] and c[5]))
    assert ("extent", "X", 17) in W - C.smooth_reach(without(lambda c: c[1] != (17, 3, 5)))
    assert ("vec", "Y", 4) in W - C.smooth_reach(without(lambda c: c[1][2] % 4 != 0))
    assert ("vec", "X", 1) in W - C.smooth_reach(without(lambda c: c[1][1] * c[1][2] % 4 == 0 and c[4] and c[5]))


def test_smoothing_shapes():
    assert {s[0] for s in C.ONEHOT_SHAPES[:7]} == set(C.AXIS_EXTENTS) == {s[1] for s in C.ONEHOT_SHAPES[7:14]}
    assert {s[2] for s in C.ONEHOT_SHAPES if s[2] > 100} == set(C.LONG_Z) and {x * y for x, y in C.LONG_XY} == {1, 5, 6}
    assert all(s in C.ONEHOT_SHAPES for s in ((13, 6, 8), (9, 5, 4), (5, 2, 2)))
    assert sorted({s[0] * s[1] for s, _ in C.ROW_CASES if s[2] == 9}) == sorted({s[0] * s[1] for s, _ in C.ROW_CASES if s[2] == 2049}) == [1, 3, 4, 5, 31, 32, 33]
    assert len(C.onehot_filters()) == 36 and all(C.onehot_taps(r, k).sum() == 1 and C.onehot_taps(r, k)[k] == 1 for _, r, k in C.onehot_filters())
    v = C.smooth_volume((5, 2, 2))
    assert v.dtype == np.float32 and np.all(np.isfinite(v)) and np.abs(v).min() >= 0.25
    assert np.array_equal(C.taps("asym"), C.taps("asym_reversed")[::-1]) and not np.array_equal(C.taps("asym"), C.taps("asym_reversed"))
    assert [len(C.taps(n)) for n in C.TAPS] == [5, 5, 9, 65]
    for n in C.TAPS:
        PF.bound_taps((C.taps(n), None, None), 1.0)                 # non-negative, sums to 1


# ---- (c) the Gaussian-free references ----------------------------------------------------------------------------------------------------
def test_smooth_taps_is_scipy_correlate1d():
    nd = pytest.importorskip("scipy.ndimage")
    v = C.smooth_volume((9, 7, 11), seed=5)
    taps = (C.taps("asym"), C.taps("asym_reversed"), np.array([0.1, 0.2, 0.7], np.float32))
    ref = v.astype(np.float64)
    for axis, w in enumerate(taps):
        ref = nd.correlate1d(ref, w.astype(np.float64), axis=axis, mode="nearest")
    got = PF.smooth_taps(v, taps)
    assert np.abs(got - ref).max() <= 4 * PF.U * float(np.abs(v).max())
    flipped = PF.smooth_taps(v, tuple(w[::-1] for w in taps))
    assert np.abs(flipped - ref).max() > 1e-2                                          # the order of the taps matters
    assert np.array_equal(PF.smooth_taps(v, (None, None, None)), v.astype(np.float64))
    # Gaussian taps: smooth() and bound() themselves
    sig = (0.93, 0, 8)
    assert np.array_equal(PF.smooth_taps(v, [PF.weights(s) for s in sig]), PF.smooth(v, sig))
    assert PF.bound_taps([PF.weights(s) for s in sig], 3.0) == PF.bound(sig, 3.0)
    for bad in (np.array([0.5, 0.6, -0.1], np.float32), np.array([0.5, 0.25, 0.125], np.float32)):
        with pytest.raises(AssertionError):
            PF.bound_taps((bad, None, None), 1.0)


def test_one_hot_taps_shift_the_index():
    v = C.smooth_volume((9, 4, 3), seed=6)
    for axis, r, k in C.onehot_filters():
        n = v.shape[axis]
        w = [C.onehot_taps(r, k) if a == axis else None for a in range(3)]
        want = np.take(v, np.clip(np.arange(n) - r + k, 0, n - 1), axis=axis)
        assert np.array_equal(PF.smooth_taps(v, w), want.astype(np.float64))


# ---- the gather and the preprocessing ----------------------------------------------------------------------------------------------------
def test_gather_and_preprocess_lists():
    assert [b * h * w % 4 for b, h, w in C.ONEHOT_SIZES] == [1, 2, 3, 0] and C.ONEHOT_NCLS == tuple(range(1, 33))
    assert all(h <= C.ONEHOT_VOLUME[0] and w <= C.ONEHOT_VOLUME[1] for _, h, w in C.ONEHOT_SIZES)
    for ncls in C.ONEHOT_NCLS:
        centre = C.onehot_label_volume(ncls)[:, :, 1]
        assert set(np.unique(centre).tolist()) == set(range(ncls + 2))                 # two labels beyond the class count
    assert set(C.PRE_SIZES) >= {255, 256, 257, 1024 * 256 - 1, 1024 * 256, 1024 * 256 + 1} and max(C.PRE_SIZES) > 2 * 1024 * 256

    def key(v):                                                # csrc/augment.hip: key_of
        u = v.view(np.uint32)
        return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    lo, hi = key(C.pre_values(4096, "low_byte")), key(C.pre_values(4096, "high_byte"))
    assert len(np.unique(lo >> 8)) == 1 and len(np.unique(lo & 255)) == 256
    assert len(np.unique(hi & 0xffffff)) == 1 and len(np.unique(hi >> 24)) > 30
    assert np.all(np.isfinite(C.pre_values(4096, "high_byte"))) and np.all(np.isfinite(C.pre_values(4096, "low_byte")))
