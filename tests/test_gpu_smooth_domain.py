"""-m gpu: pnp_volume_smooth (csrc/smooth.hip) over its launch geometry, its borders and its buffer routes.  The cases are
tests/volume_store_cases.py's; tests/test_volume_store_host.py shows without a GPU which branch each exists for.

Every output lies inside a larger allocation pre-filled with -7.0, 64 floats of guard on either side: the guards must stay untouched,
and so must src in an out-of-place call.

  a  one-hot taps, exact: a filter whose only non-zero tap is w[k] = 1 makes every output the input at clamp(a - r + k), bit for bit
     (finite inputs without zeros: fmaf(0, v, acc) changes nothing).  r in {1, 2, 8, 32}, k in {0, r, 2 r} per axis; extents 1 .. 17
     around kTA = 8 along X and Y, the 16-byte path on both passes, rows of 2047 .. 4097 voxels (1, 2 and 3 segments); out of place and in
     place, and with src, out or both one float into their allocation (the scalar path), which must give the same bits.
  b  asymmetric taps, their reverse and Gaussians (r = 4 and 32) on all three axes of the same shapes, against
     prefilter_ref.smooth_taps within prefilter_ref.bound_taps; no voxel is excluded.
  c  every subset of axes, in place and out of place, on short and on long rows: bit-identical to the composition of the single-axis
     out-of-place calls, and from run to run.
  d  row counts around 4 m at m = 8 (capped), m = 4 and m = 1.
"""
import numpy as np
import pytest
import torch

import prefilter_ref as PF
import volume_store_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 64


def _alloc(dev, shape, off, data=None):
    """(the whole allocation, the volume `off` floats past its 64-float guard): 16-byte aligned exactly when off % 4 == 0"""
    n = int(np.prod(shape))
    whole = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    inner = whole[GUARD + off:GUARD + off + n].view(shape)
    assert whole.data_ptr() % 16 == 0 and inner.data_ptr() % 16 == 4 * (off % 4) and inner.is_contiguous()
    if data is not None:
        inner.copy_(data)
    return whole, inner


def _bad(whole, inner, want):
    """device scalar: guard elements that changed plus elements of `inner` whose bits are not `want`'s"""
    n, lo = inner.numel(), (inner.data_ptr() - whole.data_ptr()) // 4
    return ((whole[:lo] != SENTINEL).sum() + (whole[lo + n:] != SENTINEL).sum()
            + (inner.reshape(-1).view(torch.int32) != want.reshape(-1).view(torch.int32)).sum())


def _smooth(dev, orig, weights, in_place, src_off=0, out_off=0):
    """one call on fresh allocations -> (the result, a device scalar that counts changed guards and, out of place, changed src elements)"""
    K = pkg("kernels")
    ws, src = _alloc(dev, orig.shape, src_off, orig)
    if in_place:
        assert K.volume_smooth(src, weights, out=src) is src
        return src, _bad(ws, src, src)
    wo, out = _alloc(dev, orig.shape, out_off)
    assert K.volume_smooth(src, weights, out=out) is out
    return out, _bad(ws, src, orig) + _bad(wo, out, out)


def _differ(a, b):
    return (a.reshape(-1).view(torch.int32) != b.reshape(-1).view(torch.int32)).sum()


def _report(bad, what):
    """bad: device scalars, one per call; one read for all of them"""
    counts = torch.stack(bad).cpu().numpy()
    wrong = [(what[i], int(c)) for i, c in enumerate(counts) if c]
    assert not wrong, "%d of %d calls differ; the first: %s" % (len(wrong), len(counts), wrong[:4])


def _ids(shapes):
    return ["%dx%dx%d" % s for s in shapes]


# ---- a. one-hot taps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.ONEHOT_SHAPES, ids=_ids(C.ONEHOT_SHAPES))
def test_one_hot_taps_are_an_index_shift(dev, shape):
    v = C.smooth_volume(shape)
    orig = torch.from_numpy(v).to(dev)
    bad, what = [], []
    for axis, r, k in C.onehot_filters():
        n = shape[axis]
        at = torch.clamp(torch.arange(n, device=dev) - r + k, 0, n - 1)
        want = torch.index_select(orig, axis, at)
        weights = [C.onehot_taps(r, k) if a == axis else None for a in range(3)]
        for so, do in C.OFFSETS:
            got, b = _smooth(dev, orig, weights, False, so, do)
            bad.append(b + _differ(got, want))
            what.append(("axis %d r %d k %d out of place, offsets %d / %d" % (axis, r, k, so, do)))
        for so in (0, 1):
            got, b = _smooth(dev, orig, weights, True, so)
            bad.append(b + _differ(got, want))
            what.append(("axis %d r %d k %d in place, offset %d" % (axis, r, k, so)))
    _report(bad, what)


# ---- b. asymmetric and Gaussian taps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.ONEHOT_SHAPES, ids=_ids(C.ONEHOT_SHAPES))
def test_asymmetric_and_gaussian_taps_against_the_restatement(dev, shape):
    v = C.smooth_volume(shape)
    orig = torch.from_numpy(v).to(dev)
    top = float(np.abs(v).max())
    bad, what = [], []
    for name in C.TAPS:
        w = C.taps(name)
        weights = (w, w, w)
        got, b = _smooth(dev, orig, weights, False)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - PF.smooth_taps(v, weights)).max())
        bound = PF.bound_taps(weights, top)
        print("pnp_volume_smooth %s %s: error / bound %.4f" % (shape, name, err / bound))
        assert err <= bound, (shape, name, err, bound)
        for in_place, so, do in ((True, 0, 0), (False, 1, 1), (True, 1, 1)):               # the same bits in place and on the scalar path
            other, b2 = _smooth(dev, orig, weights, in_place, so, do)
            bad.append(b + b2 + _differ(other, got))
            what.append("%s in place %s, offsets %d / %d" % (name, in_place, so, do))
    _report(bad, what)


# ---- c. buffer routing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.ROUTE_SHAPES, ids=_ids(C.ROUTE_SHAPES))
def test_every_route_is_the_composition_of_its_passes(dev, shape):
    v = C.smooth_volume(shape, seed=1)
    orig = torch.from_numpy(v).to(dev)
    top = float(np.abs(v).max())
    only = lambda axes: [C.ROUTE_TAPS[a] if a in axes else None for a in range(3)]
    bad, what = [], []
    for sub in C.SUBSETS:
        want = orig
        for a in sub:                                                                        # the passes one by one, out of place: X, Y, Z
            want, b = _smooth(dev, want, only((a,)), False)
            bad.append(b)
            what.append("single pass %d of %s" % (a, sub))
        err = float(np.abs(want.cpu().numpy().astype(np.float64) - PF.smooth_taps(v, only(sub))).max())
        bound = PF.bound_taps(only(sub), top)
        print("pnp_volume_smooth %s axes %s: error / bound %.4f" % (shape, sub, err / bound))
        assert err <= bound, (shape, sub, err, bound)
        for in_place in (False, True):
            for run in (0, 1):
                got, b = _smooth(dev, orig, only(sub), in_place)
                bad.append(b + _differ(got, want))
                what.append("axes %s in place %s, run %d" % (sub, in_place, run))
    _report(bad, what)


# ---- d. rows -----------------------------------------------------------------------------------------------------------------------------
def test_row_counts_around_the_rows_of_a_workgroup(dev):
    for shape, rz in C.ROW_CASES:
        v = C.smooth_volume(shape, seed=2)
        orig = torch.from_numpy(v).to(dev)
        Z = shape[2]
        bad, what = [], []
        for k in (0, 2 * rz):
            want = torch.index_select(orig, 2, torch.clamp(torch.arange(Z, device=dev) - rz + k, 0, Z - 1))
            for in_place in (False, True):
                got, b = _smooth(dev, orig, [None, None, C.onehot_taps(rz, k)], in_place)
                bad.append(b + _differ(got, want))
                what.append("%s one-hot k %d in place %s" % (shape, k, in_place))
        weights = [None, None, C.taps("asym")]
        assert len(weights[2]) == 2 * rz + 1
        got, b = _smooth(dev, orig, weights, False)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - PF.smooth_taps(v, weights)).max())
        bound = PF.bound_taps(weights, float(np.abs(v).max()))
        print("pnp_volume_smooth %s rows, asymmetric taps along z: error / bound %.4f" % (shape, err / bound))
        assert err <= bound, (shape, err, bound)
        other, b2 = _smooth(dev, orig, weights, True)
        bad.append(b + b2 + _differ(other, got))
        what.append("%s asymmetric in place" % (shape,))
        _report(bad, what)
