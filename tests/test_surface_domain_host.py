"""not gpu: the host side of tests/test_gpu_surface_domain.py.  The launch geometry of csrc/surface.hip's edt3d, restated in
tests/surface_domain_cases.py, takes every branch over the EDT shape list; the metric cases reach, by the float64 reference, every branch
of the percentile's lerp, an empty side, class 31 and labels outside [0, ncls); the closed forms and the percentile restatement that the
GPU file's expectations use equal the reference and numpy.percentile."""
import math

import numpy as np
import pytest

import surface_domain_cases as SD
import surface_ref as R


# ---- the EDT's launch geometry ---------------------------------------------------------------------------------------------------------
def edt_branches(shapes):
    b = set()
    for s in shapes:
        g = SD.edt_geometry(s)
        b.add(("Tz", "8" if g["Tz"] == 8 else "256" if g["Tz"] == 256 else "between"))
        if g["z_ragged"] and g["z_groups"] > 1:
            b.add("z_ragged_last_group")
        if g["z_groups"] > 1:
            b.add("z_groups>1")
        b.add(("z_tail", g["z_tail"]))
        for axis, p in zip("yx", g["passes"]):
            b.add(("T", p["T"]))
            b.add(("tail", p["tail"]))
            if p["last_nz"] < p["T"]:
                b.add("nz<T")
                if p["groups"] > 1:
                    b.add(("nz<T after a full tile", axis))
            if p["groups"] > 1:
                b.add("z tiles>1")
            if p["n"] * p["T"] == SD.TILE_FLOATS:
                b.add(("tile full", axis))                  # the y pass strides by Z, the x pass by Y Z
    return b


EDT_WANTED = ({("Tz", "8"), ("Tz", "256"), ("Tz", "between"), "z_ragged_last_group", "z_groups>1", ("z_tail", True), ("z_tail", False), "nz<T",
               ("nz<T after a full tile", "y"), ("nz<T after a full tile", "x"), "z tiles>1", ("tile full", "y"), ("tile full", "x"), ("tail", True),
               ("tail", False)} | {("T", t) for t in (1, 2, 4, 8, 16, 32, 64)})


def test_the_restated_geometry_on_known_shapes():
    g = SD.edt_geometry((2, 1024, 9))
    assert g["Tz"] == 256 and g["z_groups"] == 8 and not g["z_ragged"]
    assert g["passes"][0] == {"n": 1024, "T": 8, "logT": 3, "groups": 2, "last_nz": 1, "tail": False}
    assert g["passes"][1] == {"n": 2, "T": 16, "logT": 4, "groups": 1, "last_nz": 9, "tail": True}
    g = SD.edt_geometry((3, 200, 70))
    assert g["Tz"] == 117 and g["z_groups"] == 6 and g["z_ragged"] and [p["T"] for p in g["passes"]] == [32, 64]
    assert SD.edt_geometry((2, 3, 1024))["Tz"] == 8 and [p["T"] for p in SD.edt_geometry((1, 1, 1))["passes"]] == [1, 1]
    assert [p["T"] for p in SD.edt_geometry((3, 1024, 2))["passes"]] == [2, 2] and [p["T"] for p in SD.edt_geometry((7, 6, 3))["passes"]] == [4, 4]
    # T / 2 >= Z: a z extent that is a power of two gets exactly that many lanes, not twice as many
    assert [p["T"] for p in SD.edt_geometry((5, 5, 32))["passes"]] == [32, 32] and [p["T"] for p in SD.edt_geometry((5, 5, 33))["passes"]] == [64, 64]


def test_the_edt_shapes_take_every_branch_of_the_launch_geometry():
    missing = EDT_WANTED - edt_branches(SD.EDT_SHAPES)
    assert not missing, sorted(map(str, missing))
    assert set(SD.EDT_SHAPES) >= {(1, 1, 1), (5, 7, 1), (2, 3, 1024), (3, 1024, 2), (2, 1024, 9), (1024, 2, 9), (3, 200, 70), (130, 9, 33), (9, 5, 257)}
    assert max(int(np.prod(s)) for s in SD.EDT_SHAPES) <= 10 ** 5
    assert {None, (0.7, 1.3, 2.5), (0.05, 1.0, 20.0)} == set(SD.EDT_SPACINGS)
    assert set(SD.EDT_FEATURES) >= {"corner%d" % i for i in range(8)} | {"all", "plane0", "plane1", "plane2", "random", "empty"}


def test_a_missing_edt_shape_is_noticed():
    without = lambda *s: [x for x in SD.EDT_SHAPES if x not in s]
    assert EDT_WANTED - edt_branches(without((2, 1024, 9))) == {("tile full", "y")}         # the only 1024-long y line with a full tile
    assert EDT_WANTED - edt_branches(without((1024, 2, 9))) == {("tile full", "x")}
    assert ("T", 4) in EDT_WANTED - edt_branches(without((7, 6, 3)))
    assert ("Tz", "between") in EDT_WANTED - edt_branches(without((3, 200, 70), (130, 9, 33), (9, 5, 257)))
    assert ("Tz", "8") in EDT_WANTED - edt_branches(without((2, 3, 1024)))


@pytest.mark.parametrize("shape", [(5, 7, 1), (7, 6, 3), (1, 1, 1), (4, 3, 9)])
def test_closed_form_expectations_equal_the_reference(shape):
    for feat in SD.CLOSED_FORM:
        m = SD.edt_mask(shape, feat)
        for spacing in SD.EDT_SPACINGS:
            assert np.array_equal(SD.edt_expected(shape, feat, spacing), R.edt_sq(m, spacing)), (shape, feat, spacing)
    corners = {tuple(np.argwhere(SD.edt_mask((4, 3, 9), "corner%d" % i))[0]) for i in range(8)}
    assert corners == {(x, y, z) for x in (0, 3) for y in (0, 2) for z in (0, 8)}
    assert 3 * 1023 ** 2 < 2 ** 24                                    # every unit-spacing value is an integer that fp32 holds


def test_feature_sets_are_what_they_say():
    for shape in SD.EDT_SHAPES:
        assert SD.edt_mask(shape, "all").all() and not SD.edt_mask(shape, "empty").any()
        for a in range(3):
            assert int(SD.edt_mask(shape, "plane%d" % a).sum()) == int(np.prod(shape)) // shape[a]
        r = SD.edt_mask(shape, "random")
        assert 1 <= int(r.sum()) <= 1 + int(0.03 * r.size)                # about 1 %, and never empty
        for i in range(8):
            assert int(SD.edt_mask(shape, "corner%d" % i).sum()) == 1


# ---- the metric cases ------------------------------------------------------------------------------------------------------------------
def metric_branches(names):
    b = set()
    for name in names:
        p, g = SD.metric_volumes(name)
        ncls, ref = SD.ncls_of(name), SD.metric_reference(name)
        V = p.size
        b.add(("ncls", ncls))
        for v in (p, g):
            for bad in (-1, ncls, 255):
                if (v == bad).any():
                    b.add(("label", "-1" if bad < 0 else "ncls" if bad == ncls else "255", "pred" if v is p else "gt"))
        if p.shape[0] == 1:
            b.add("X=1")
        if p.shape[2] == 1:
            b.add("Z=1")
        if V < 64:
            b.add("V<64")
        if V % 256:
            b.add("V%256")
        if not p.any() and not g.any():
            b.add("all zeros")
        for c in range(1, ncls):
            np_, ng = int(ref["n_border_pred"][c]), int(ref["n_border_gt"][c])
            if np_ == 0 and ng == 0:
                b.add("absent from both")
            elif np_ == 0 or ng == 0:
                b.add(("absent from", "pred" if np_ == 0 else "gt"))
            else:
                n = np_ + ng
                d = np.sort(np.hstack((R.sds(p == c, g == c), R.sds(g == c, p == c))))
                klo, khi, _ = SD.lerp_parts(n)
                b.add(("lerp", SD.lerp_branch(n), "distinct" if d[klo] != d[khi] else "equal"))
                if n == 2:
                    b.add("n=2")
                if c == 31:
                    b.add("class 31")
                if all(((p == c) | (g == c))[sl].any() for a in range(3) for sl in (_face(a, 0), _face(a, -1))):
                    b.add("touches all six faces")
    return b


def _face(axis, at):
    sl = [slice(None)] * 3
    sl[axis] = at
    return tuple(sl)


METRIC_WANTED = ({("ncls", 2), ("ncls", 5), ("ncls", 32), "class 31", "X=1", "Z=1", "V<64", "V%256", "all zeros", "absent from both",
                  ("absent from", "pred"), ("absent from", "gt"), "n=2", "touches all six faces",
                  ("lerp", "g==0", "distinct"), ("lerp", "g<0.5", "distinct"), ("lerp", "g>=0.5", "distinct")}
                 | {("label", l, s) for l in ("-1", "ncls", "255") for s in ("pred", "gt")})


def test_the_metric_cases_reach_every_branch():
    missing = METRIC_WANTED - metric_branches(SD.METRIC_CASES)
    assert not missing, sorted(map(str, missing))
    assert set(SD.EXACT_CASES) >= {"ell5_oob", "shifted_box"} and SD.EXACT_SPACING == (0.8, 1.1, 2.5)
    lerp_exact = {k for k in metric_branches(SD.EXACT_CASES) if isinstance(k, tuple) and k[0] == "lerp"}
    assert lerp_exact >= {k for k in METRIC_WANTED if isinstance(k, tuple) and k[0] == "lerp"}


def test_a_missing_metric_case_is_noticed():
    without = lambda *n: [x for x in SD.METRIC_CASES if x not in n]
    gone = METRIC_WANTED - metric_branches(without("boxes32"))
    assert ("ncls", 32) in gone and "class 31" in gone
    assert ("lerp", "g==0", "distinct") in METRIC_WANTED - metric_branches(without("lerp"))
    assert ("label", "255", "gt") in METRIC_WANTED - metric_branches(without("ell5_oob"))
    assert "all zeros" in METRIC_WANTED - metric_branches(without("zeros"))


def test_the_cases_are_what_the_documents_say():
    ref = SD.metric_reference("lerp")
    assert (ref["n_border_pred"][1:] + ref["n_border_gt"][1:]).tolist() == [21, 12, 8, 2]
    assert [SD.lerp_branch(n) for n in (21, 12, 8, 2)] == ["g==0", "g<0.5", "g>=0.5", "g>=0.5"]
    ref = SD.metric_reference("boxes32")
    assert ref["n_border_pred"][31] == 32 and ref["n_border_gt"][31] == 24 and ref["hd95"][31] > 0
    for side, c in SD.ABSENT32.items():
        assert (ref["n_border_pred"][c] == 0) == (side in ("pred", "both")) and (ref["n_border_gt"][c] == 0) == (side in ("gt", "both"))
        assert np.isnan(ref["hd95"][c])
    ref = SD.metric_reference("single")
    assert ref["hd95"][1] == math.sqrt(29) and ref["n_border_pred"][1] + ref["n_border_gt"][1] == 2
    p, g = SD.metric_volumes("shifted_box")
    d = np.hstack((R.sds(p == 1, g == 1, SD.EXACT_SPACING), R.sds(g == 1, p == 1, SD.EXACT_SPACING)))
    assert set(np.round(d, 9)) == {0.0, 0.8} and len(d) == 2 * 2964 and min(SD.EXACT_SPACING) == SD.EXACT_SPACING[0]


# ---- the percentile restatement --------------------------------------------------------------------------------------------------------
def test_percentile_restatement_equals_numpy():
    rng = np.random.default_rng(5)
    sizes = list(range(1, 130)) + [255, 256, 257, 1000, 4097, 65537] + [int(v) for v in rng.integers(130, 20000, 40)]
    seen = set()
    for n in sizes:
        seen.add(SD.lerp_branch(n))
        for trial in range(3):
            sq = (rng.random(n) * 10 ** rng.uniform(-3, 4)).astype(np.float32) if trial < 2 else rng.integers(0, 6, n).astype(np.float32)
            want = np.percentile(np.sqrt(np.sort(sq).astype(np.float64)), 95)
            assert SD.hd95_of_squares(sq) == want, (n, trial)
            assert SD.hd95_of_squares(sq[::-1].astype(np.float64)) == want
    assert seen == {"g==0", "g<0.5", "g>=0.5"}
    assert SD.lerp_parts(1) == (0, 0, 0.0) and SD.lerp_parts(2)[:2] == (0, 1) and SD.lerp_parts(21) == (19, 20, 0.0)
    assert SD.hd95_of_squares(np.array([4.0, 0.0], np.float32)) == 2.0 - 2.0 * (1.0 - 0.95)
