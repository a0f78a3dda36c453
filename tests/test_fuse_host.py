"""not gpu: the host side of multi-planar fusion — tests/fuse_ref.py against an independent formulation, the rounding
bound's ceiling, the non-vacuity of the GPU sweep's label comparison (the reference alone), check_axes / view_box / the axes-axis
conflict of segment_volume, the three command lines' --axes parsing, and pnp_fuse_views' host refusals by their text (decided before any
HIP call: the buffers are small host buffers, never read)."""
import ctypes

import numpy as np
import pytest

import fuse_ref as F
from conftest import pkg


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def _direct_entropy(p):
    """-sum p ln p.  scipy.stats.entropy normalises p first, and float32 probabilities sum to 1 only within rounding: with s = sum p,
    -sum p ln p = s H(p / s) - s ln s exactly"""
    try:
        from scipy.stats import entropy
        s = float(np.sum(p))
        return s * float(entropy(p)) - s * np.log(s)
    except ImportError:
        return float(-sum(v * np.log(v) for v in p if v > 0))


@pytest.mark.parametrize("M,ncls", [(1, 5), (2, 2), (3, 5), (8, 8), (3, 1)])
def test_restatement_against_an_independent_formulation(M, ncls):
    """per voxel: np.average over the covering views with their weights, scipy.stats.entropy (a direct sum without scipy)"""
    probs, w = F.make_case(M, ncls, 97, seed=3)
    for weights in (w, None):
        ref = F.fuse(probs, weights)
        ww = np.ones(M) if weights is None else w.astype(np.float64)
        seen_uncovered = False
        for e in range(97):
            cov = [v for v in range(M) if probs[v][:, e].astype(np.float64).sum() > 0.5]
            assert bool(ref.covered[e]) == bool(cov)
            if not cov:
                seen_uncovered = True
                assert ref.label[e] == 0 and not ref.prob[:, e].any() and ref.entropy[e] == 0
                continue
            P = np.average(np.stack([probs[v][:, e].astype(np.float64) for v in cov]), axis=0, weights=ww[cov])
            assert np.abs(ref.prob[:, e] - P).max() <= 1e-15
            assert ref.label[e] == int(np.argmax(P))
            H = 0.0 if ncls == 1 else _direct_entropy(P) / np.log(ncls)
            assert abs(ref.entropy[e] - H) <= 1e-12
        assert seen_uncovered or M > 3, "25 % zeroed per view: a small M leaves some element without a view"


def test_first_maximum_and_weights():
    a = np.array([[0.4, 0.2], [0.4, 0.3], [0.2, 0.5]], np.float32)         # [ncls = 3, 2 elements]
    b = np.array([[0.2, 0.0], [0.2, 0.0], [0.6, 0.0]], np.float32)         # covers element 0 only
    r = F.fuse([a, b], [1.0, 3.0])
    assert np.allclose(r.prob[:, 0], (a[:, 0].astype(np.float64) + 3 * b[:, 0].astype(np.float64)) / 4) and r.label[0] == 2
    assert np.array_equal(r.prob[:, 1], a[:, 1].astype(np.float64)) and r.label[1] == 2
    assert F.fuse([a], None).label[0] == 0                                   # 0.4 == 0.4: the lower class
    assert F.fuse([b], None).covered.tolist() == [True, False]


def test_the_bound_stays_under_its_ceiling():
    assert [F.delta_p(M) / F.U for M in (1, 2, 3, 8)] == [3, 5, 7, 17]
    assert all(F.delta_p(M) <= 32 * F.U for M in range(1, 9))
    # and it bounds float32 arithmetic in the kernel's order on the sweep's own inputs (numpy float32, product rounded, then the sum)
    for M, ncls in ((2, 5), (8, 8)):
        probs, w = F.make_case(M, ncls, 693, seed=1)
        ref = F.fuse(probs, w)
        acc, ws = np.zeros((ncls, 693), np.float32), np.zeros(693, np.float32)
        for v in range(M):
            s = np.zeros(693, np.float32)
            for c in range(ncls):
                s = s + probs[v][c]
            cov = s > 0.5
            acc = np.where(cov, acc + w[v] * probs[v], acc).astype(np.float32)
            ws = np.where(cov, ws + w[v], ws).astype(np.float32)
        P = np.where(ws > 0, acc / np.where(ws > 0, ws, 1).astype(np.float32), 0).astype(np.float32)
        assert np.abs(P.astype(np.float64) - ref.prob).max() <= F.delta_p(M)


@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("ncls", [2, 5, 8])
def test_the_label_comparison_is_not_vacuous_on_the_sweep(M, ncls):
    """the reference alone: on the GPU sweep's construction at most 2 covered voxels per case admit more than one class (a top-2 gap
    below 2 delta_p), with 5 seeds per (M, ncls); seed 0 is the GPU test's"""
    n = int(np.prod(F.SHAPE))
    for seed in F.VACUITY_SEEDS:
        probs, w = F.make_case(M, ncls, n, seed)
        for weights in (w, None):
            ref = F.fuse(probs, weights)
            left_out, covered = F.ambiguous(ref, M), int(ref.covered.sum())
            assert left_out <= 2 and covered >= 0.7 * n, (seed, left_out, covered)
            assert len(np.unique(ref.label[ref.covered])) == ncls


def test_the_large_case_is_not_vacuous_either():
    M, ncls, n = F.BIG
    probs, w = F.make_case(M, ncls, n, F.BIG_SEED)
    for weights in (w, None):
        ref = F.fuse(probs, weights)
        assert F.ambiguous(ref, M) <= 2 and 0 < int((~ref.covered).sum()) < 0.05 * n


# ---- options ---------------------------------------------------------------------------------------------------------------------------
def test_check_axes():
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    assert vp.check_axes is vs.check_axes
    assert vp.check_axes((0, 1, 2)) == ((0, 1, 2), None) and vp.check_axes([2, 0], [1, 2.5]) == ((2, 0), (1.0, 2.5))
    assert vp.check_axes((np.int64(1),)) == ((1,), None) and vp.check_axes(range(3))[0] == (0, 1, 2)
    for bad, text in (((), "empty"), ((0, 0), r"\(0, 0\)"), ((0, 3), "3"), ((-1,), "-1"), ("012", "'012'"), (1, "got 1"), ((True,), "True"),
                      ((1.0,), "1.0"), (None, "None")):
        with pytest.raises(ValueError, match=text):
            vp.check_axes(bad)
    for bad, text in (((1.0,), "1 weights"), ((1, 0, 1), "0.0"), ((1, -2, 1), "-2.0"), ((1, float("nan"), 1), "nan"), ((1, float("inf"), 1), "inf"),
                      ("abc", "'abc'"), (5, "got 5")):
        with pytest.raises(ValueError, match=text):
            vp.check_axes((0, 1, 2), bad)


def test_segment_volume_keyword_errors():
    """decided before any device work (device="cpu" would be refused later)"""
    vp = pkg("volume_predict")
    img = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(ValueError, match="exclude each other"):
        vp.segment_volume(None, img, axis=0, axes=(0, 1, 2), device="cpu")
    with pytest.raises(ValueError, match="twice"):
        vp.segment_volume(None, img, axes=(1, 1), device="cpu")
    with pytest.raises(ValueError, match="2 weights"):
        vp.segment_volume(None, img, axes=(0, 1, 2), axis_weights=(1, 1), device="cpu")
    with pytest.raises(ValueError, match="goes with axes"):
        vp.segment_volume(None, img, axis_weights=(1, 1, 1), device="cpu")
    with pytest.raises(pkg("_lib").PnpError, match="no CPU fallback"):        # a valid request reaches the single-axis path's device check
        vp.segment_volume(None, img, axes=(0, 1, 2), axis=2, device="cpu")


@pytest.mark.parametrize("flip", [True, False])
def test_view_box_against_moveaxis(flip):
    """an explicit box in the slicing order of axis 2, re-expressed per view, selects the same voxels of the file as the box itself:
    numpy's moveaxis on an index volume, and file_layout's strides on top of it"""
    vp = pkg("volume_predict")
    shape = (6, 5, 7)
    index = np.arange(np.prod(shape)).reshape(shape)
    flipped = np.flip(np.flip(index, 0), 1) if flip else index
    box = ((1, 4), (0, 3), (2, 7))
    want = np.sort(flipped[tuple(slice(a, b) for a, b in box)].ravel())
    for axis in (0, 1, 2):
        vb = vp.view_box(box, axis)
        view = np.moveaxis(flipped, axis, -1)
        assert np.array_equal(np.sort(view[tuple(slice(a, b) for a, b in vb)].ravel()), want), axis
        origin, strides, dims = vp.file_layout(shape, flip, axis, vb)
        g = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
        assert np.array_equal(np.sort((origin + sum(s * k for s, k in zip(strides, g))).ravel()), want), axis
    assert vp.view_box(box, 2) == box
    with pytest.raises(ValueError):
        vp.view_box(box, 3)


def test_flag_parsing(tmp_path):
    pr, ts, tg, vs, nifti = pkg("predict"), pkg("train_segmenter"), pkg("train_gan"), pkg("volume_source"), pkg("nifti")
    assert vs.parse_axes(None) is None and vs.parse_axes("0,1,2") == (0, 1, 2) and vs.parse_axes("1") == (1,) and vs.parse_axes("2, 0") == (2, 0)
    for bad in ("", "0,0", "3", "0,1,2,1", "a", "0;1", "-1", "0.5", "0,,1"):
        with pytest.raises(ValueError, match="--axes"):
            vs.parse_axes(bad)
    assert vs.parse_axis_weights(None, (0, 1)) is None and vs.parse_axis_weights("1,2.5", (0, 1)) == (1.0, 2.5)
    for bad, axes in (("1", (0, 1)), ("1,0", (0, 1)), ("1,x", (0, 1)), ("1,-1", (0, 1)), ("1,nan", (0, 1)), ("1,1", None)):
        with pytest.raises(ValueError, match="--axis-weights"):
            vs.parse_axis_weights(bad, axes)
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16), np.diag([0.5, 0.7, 2.0, 1.0])), a)
    model = tmp_path / "m.npz"
    np.savez(str(model), x=np.zeros(1))
    base = ["--model", str(model), "--net", "segmenter", "--out", str(tmp_path / "o"), "--images", a]
    plain = pr.parse_args(base)[3]
    assert "axes" not in plain and "axis_weights" not in plain and plain["axis"] == 2
    opt = pr.parse_args(base + ["--axes", "0,1,2"])[3]
    assert opt["axes"] == (0, 1, 2) and "axis_weights" not in opt and opt["axis"] == 2
    opt = pr.parse_args(base + ["--axes", "0,2", "--axis-weights", "1,2", "--axis", "2", "--tta", "default", "--prob", "--entropy", "--keep-largest",
                                "--sample-mm", "1.5", "--tiles", "auto", "--prefilter", "auto"])[3]
    assert opt["axes"] == (0, 2) and opt["axis_weights"] == (1.0, 2.0) and opt["prob"] and opt["entropy"] and opt["tiles"] == "auto"
    for bad in (["--axes", "0,1", "--axis", "1"], ["--axes", "0,0"], ["--axes", "4"], ["--axis-weights", "1,1"],
                ["--axes", "0,1", "--axis-weights", "1"], ["--axes", "0,1", "--axis-weights", "1,0"]):
        with pytest.raises(SystemExit):
            pr.parse_args(base + bad)
    lists = ["--mr-nii-train", "a", "--mr-nii-val", "b", "--ct-nii-train", "c", "--ct-nii-val", "d"]
    assert tg.parse_args("pre-train", lists + ["--axes", "0,1,2"]).axes == (0, 1, 2)
    assert tg.parse_args("pre-train", lists).axes is None
    for bad in ("0,0", "3", "x", ""):
        with pytest.raises(SystemExit):
            ts.main(["--nii-train", "t", "--nii-val", "v", "--axes", bad])
        with pytest.raises(SystemExit):
            tg.parse_args("pre-train", lists + ["--axes", bad])
        with pytest.raises(SystemExit):
            vs.main(["--export", "1", str(tmp_path / "e"), "--list", "l", "--axes", bad])
    with pytest.raises(SystemExit):
        ts.main(["--synthetic", "4", "--axes", "0,1,2"])                 # no NIfTI lists
    with pytest.raises(SystemExit):
        tg.parse_args("pre-train", ["--axes", "0,1,2"])


# ---- argument refusals of pnp_fuse_views ---------------------------------------------------------------------------------------------------
def test_fuse_views_refusals_on_the_host(built):
    lib = built._lib.load()
    ncls0, n0 = 5, 24
    bufs = [np.zeros(ncls0 * n0 + 4, np.float32) for _ in range(9)]
    out_p, out_h, out_l = np.zeros(ncls0 * n0 + 4, np.float32), np.zeros(n0 + 4, np.float32), np.zeros(n0 + 4, np.uint8)
    addr = lambda a, off=0: a.ctypes.data + off

    def call(text, M=3, ncls=ncls0, n=n0, views=None, weights=None, label=addr(out_l), prob=addr(out_p), entropy=addr(out_h), probs_null=False):
        views = [addr(b) for b in bufs[:max(M, 0)]] if views is None else views
        arr = None if probs_null else (ctypes.c_void_p * max(len(views), 1))(*views)
        w = None if weights is None else (ctypes.c_float * len(weights))(*weights)
        rc = lib.pnp_fuse_views(M, arr, w, ncls, n, label, prob, entropy, None)
        assert rc == -1 and text in lib.pnp_last_error(), lib.pnp_last_error()
        assert lib.pnp_last_error().startswith(b"pnp_fuse_views:")

    call(b"n_views = 0 outside [1, 8]", M=0)
    call(b"n_views = 9 outside [1, 8]", M=9)
    call(b"ncls 0 outside [1, 8]", ncls=0)
    call(b"ncls 9 outside [1, 8]", ncls=9)
    call(b"vol_elems = 0", n=0)
    call(b"overflow int64", n=2 ** 61)
    call(b"null pointer", label=None)
    call(b"null pointer", probs_null=True)
    call(b"view 1 of 3 is a null pointer", views=[addr(bufs[0]), None, addr(bufs[2])])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        call(b"weight 1 = ", weights=[1.0, bad, 1.0])
    call(b"not aligned to 4 bytes", views=[addr(bufs[0]), addr(bufs[1], 2), addr(bufs[2])])
    call(b"a view overlaps a view", views=[addr(bufs[0]), addr(bufs[0]), addr(bufs[2])])
    call(b"a view overlaps prob", prob=addr(bufs[0], 4))                          # probs[0], one element in: a partial overlap
    call(b"a view overlaps prob", prob=addr(bufs[1]))                             # exact, but not the first view
    call(b"a view overlaps entropy", entropy=addr(bufs[2], 4 * (ncls0 * n0 - 1)))
    call(b"a view overlaps label", label=addr(bufs[0], 4 * ncls0 * n0 - 1))
    call(b"prob overlaps entropy", entropy=addr(out_p, 8))
    call(b"entropy overlaps label", label=addr(out_h, 4 * n0 - 1))
