"""-m gpu: csrc/surface.hip over its whole domain against the float64 reference tests/surface_ref.py, with the bars of
tests/test_gpu_surface.py: the squared EDT bit-exact with unit spacing and rtol 1e-6 (atol 0) otherwise; border counts, HD and HD95 exact
and the sums to 1e-12 with unit spacing.  With a non-unit spacing the selection is checked EXACTLY against an expectation formed on the host
from the kernel's own fp32 squared distances (pnp_edt3d_sq of the reference's border masks: the same min-plus code as the bitmask path).

The case lists live in tests/surface_domain_cases.py; tests/test_surface_domain_host.py proves without a GPU that they reach every branch
of the launch geometry (Tz, T, partial tiles, chunk tails), every branch of the percentile's lerp, bit 31 of the border mask, labels
outside [0, ncls) and empty sides."""
import math

import numpy as np
import pytest
import torch

import surface_domain_cases as SD
import surface_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

DIST = ("asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95")


def _same(m, ref, rtol_sum):
    """tests/test_gpu_surface.py's bar at unit spacing: counts, HD and HD95 exact, the means to rtol_sum"""
    for k in ("n_border_pred", "n_border_gt"):
        np.testing.assert_array_equal(m[k][1:], ref[k][1:], err_msg=k)
    for k in DIST:
        assert np.isnan(m[k][0]), k
        np.testing.assert_array_equal(np.isnan(m[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        if k in ("hd", "hd95"):
            np.testing.assert_array_equal(m[k][ok], ref[k][ok], err_msg=k)
        else:
            np.testing.assert_allclose(m[k][ok], ref[k][ok], rtol=rtol_sum, atol=0, err_msg=k)


def _rows(dev, name, spacing=None, swap=False):
    K = pkg("kernels")
    p, g = (torch.from_numpy(v.copy()).to(dev) for v in SD.metric_volumes(name))
    if swap:
        p, g = g, p
    rows = K.surface_distances(p, g, SD.ncls_of(name), spacing).cpu().numpy()
    assert rows.shape == (SD.ncls_of(name), 7) and rows.dtype == np.float64
    return rows


# ---- the EDT -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SD.EDT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_edt_over_the_launch_geometry(dev, shape):
    K = pkg("kernels")
    for feat in SD.EDT_FEATURES:
        md = torch.from_numpy(SD.edt_mask(shape, feat)).to(dev)
        for spacing in SD.EDT_SPACINGS:
            got = K.edt_sq(md, spacing).cpu().numpy()
            want = SD.edt_expected(shape, feat, spacing)
            assert got.dtype == np.float32 and got.shape == tuple(shape)
            what = "%s %s spacing %s" % (shape, feat, spacing)
            if feat == "empty":
                assert np.all(np.isposinf(got)), what
            elif spacing is None:
                assert np.array_equal(got.astype(np.float64), want), what + ": %d voxels differ" % int((got != want).sum())
            else:
                np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-6, atol=0, err_msg=what)


# ---- the metrics at unit spacing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SD.METRIC_CASES)
def test_metrics_against_reference(dev, name):
    S = pkg("surface")
    rows = _rows(dev, name)
    ref = SD.metric_reference(name)
    np.testing.assert_array_equal(rows[1:, 0], ref["n_border_pred"][1:])
    _same(S.rows_to_metrics(rows), ref, 1e-12)
    ncls = SD.ncls_of(name)
    empty = (ref["n_border_pred"] == 0) | (ref["n_border_gt"] == 0)
    assert np.isnan(rows[0]).all() and np.isnan(rows[1:][empty[1:], 2:]).all() and not np.isnan(rows[1:][~empty[1:]]).any()
    if name == "zeros":
        assert not rows[1:, :2].any() and np.isnan(rows[:, 2:]).all()
    if name == "single":
        assert rows[1].tolist() == [1, 1, math.sqrt(29), math.sqrt(29), math.sqrt(29), math.sqrt(29), math.sqrt(29)]
    if name == "boxes32":
        assert rows[31, 0] == 32 and rows[31, 1] == 24 and rows[31, 6] > 0 and ncls == 32


def test_metrics_through_the_public_function(dev):
    S = pkg("surface")
    p, g = (v.copy() for v in SD.metric_volumes(SD.PUBLIC_CASE))      # the cached volumes are read-only
    _same(S.surface_metrics(p, g, SD.ncls_of(SD.PUBLIC_CASE)), SD.metric_reference(SD.PUBLIC_CASE), 1e-12)


def test_swapped_arguments_swap_the_directions(dev):
    for name in ("ell5_oob", "lerp", "boxes32"):
        a, b = _rows(dev, name), _rows(dev, name, swap=True)
        for i, j in ((0, 1), (2, 3), (4, 5)):
            np.testing.assert_array_equal(a[:, i], b[:, j], err_msg="%s columns %d / %d" % (name, i, j))
            np.testing.assert_array_equal(a[:, j], b[:, i])
        np.testing.assert_array_equal(a[:, 6], b[:, 6])                 # the pooled list is the same multiset


def test_a_repeat_is_bitwise_identical(dev):
    for name, spacing in (("ell5_oob", None), ("ell5_oob", SD.EXACT_SPACING), ("boxes32", None)):
        assert _rows(dev, name, spacing).tobytes() == _rows(dev, name, spacing).tobytes()


def test_identical_volumes_have_zero_distances(dev):
    K = pkg("kernels")
    g = torch.from_numpy(SD.metric_volumes("ell5_oob")[1].copy()).to(dev)
    rows = K.surface_distances(g, g, 5).cpu().numpy()
    ref = SD.metric_reference("ell5_oob")
    np.testing.assert_array_equal(rows[1:, 0], ref["n_border_gt"][1:])
    np.testing.assert_array_equal(rows[1:, 1], ref["n_border_gt"][1:])
    assert not rows[1:, 2:][rows[1:, 0] > 0].any()


# ---- exact selection with a non-unit spacing -----------------------------------------------------------------------------------------
def _expected_rows(dev, name, spacing):
    """per class, from the kernel's own fp32 squared distances: [n_pred, n_gt, sum, sum, max, max, hd95] and the pooled fp32 list"""
    K = pkg("kernels")
    p, g = SD.metric_volumes(name)
    out = {}
    for c in range(1, SD.ncls_of(name)):
        bp, bg = R.border(p == c), R.border(g == c)
        row = [float(bp.sum()), float(bg.sum())] + [float("nan")] * 5
        pooled = np.zeros(0, np.float32)
        if bp.any() and bg.any():
            e_g = K.edt_sq(torch.from_numpy(bg.astype(np.uint8)).to(dev), spacing).cpu().numpy()
            e_p = K.edt_sq(torch.from_numpy(bp.astype(np.uint8)).to(dev), spacing).cpu().numpy()
            d_pg, d_gp = e_g[bp], e_p[bg]                              # the prediction's border reads the ground truth's EDT, and back
            assert d_pg.dtype == np.float32
            pooled = np.concatenate([d_pg, d_gp])
            row[2:] = [math.fsum(np.sqrt(d_pg.astype(np.float64))), math.fsum(np.sqrt(d_gp.astype(np.float64))),
                       math.sqrt(float(d_pg.max())), math.sqrt(float(d_gp.max())), SD.hd95_of_squares(pooled)]
            assert row[6] == np.percentile(np.sqrt(pooled.astype(np.float64)), 95)
        out[c] = (row, pooled)
    return out


@pytest.mark.parametrize("name", SD.EXACT_CASES)
def test_selection_is_exact_with_non_unit_spacing(dev, name):
    rows = _rows(dev, name, SD.EXACT_SPACING)
    want = _expected_rows(dev, name, SD.EXACT_SPACING)
    digits = [set() for _ in range(4)]
    equal_runs = 0
    for c, (row, pooled) in want.items():
        what = "%s class %d: %s, expected %s" % (name, c, rows[c].tolist(), row)
        for i in (0, 1, 4, 5, 6):
            assert rows[c, i] == row[i] or (math.isnan(row[i]) and math.isnan(rows[c, i])), what
        for i in (2, 3):
            assert math.isnan(row[i]) and math.isnan(rows[c, i]) or abs(rows[c, i] - row[i]) <= 1e-12 * abs(row[i]), what
        for b in range(4):
            digits[b] |= set(((pooled.view(np.uint32) >> (8 * b)) & 255).tolist())
        if len(pooled) >= 1024 and len(np.unique(pooled)) <= 2:
            equal_runs += 1
    if name == "ell5_oob":                                               # the inputs make all four radix rounds discriminate
        assert all(len(d) > 1 for d in digits), [len(d) for d in digits]
    if name == "shifted_box":                                            # two values only: whole waves share a digit (the fast path)
        assert equal_runs == 1 and rows[1, 4] == rows[1, 5] == rows[1, 6] == math.sqrt(float(np.float32(0.8) * np.float32(0.8)))
    # against the float64 reference the existing bar still holds
    S = pkg("surface")
    m, ref = S.rows_to_metrics(rows), SD.metric_reference(name, SD.EXACT_SPACING)
    for k in DIST:
        ok = ~np.isnan(ref[k])
        np.testing.assert_array_equal(np.isnan(m[k][1:]), np.isnan(ref[k][1:]), err_msg=k)
        np.testing.assert_allclose(m[k][ok], ref[k][ok], rtol=1e-6, atol=0, err_msg=k)
