"""-m gpu: csrc/components.hip against tests/components_ref.py.  Everything is an integer: every comparison is exact
equality over the WHOLE allocation (roots and out are pre-filled with 0xAB), and after every call both device error counters read 0.

The shapes are the smallest that cross the 8 x 8 x 32 tile borders in every axis with ragged extents and spread over many workgroups:
37 x 29 x 45 = 5 x 4 x 2 tiles, 33 x 33 x 64 = 5 x 5 x 2, 96 x 80 x 72 = 12 x 10 x 3."""
import numpy as np
import pytest
import torch

import components_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name):
    if name not in _cache:
        make = {"random": R.case_random, "snake": R.case_snake, "blobs": R.case_blobs, "ties": R.case_ties,
                "one_zero": lambda: np.zeros((1, 1, 1), np.uint8), "one_three": lambda: np.full((1, 1, 1), 3, np.uint8),
                "background": lambda: np.zeros((37, 29, 45), np.uint8), "solid": lambda: np.full((37, 29, 45), 2, np.uint8),
                "high": lambda: (1 + np.arange(37 * 29 * 45).reshape(37, 29, 45) // 7 % 7).astype(np.uint8)}[name]
        v = make()
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name]


def _ref(name, ncls, conn, keep=1, min_size=0, classes=None):
    key = (name, ncls, conn, keep, min_size, None if classes is None else tuple(classes))
    if key not in _cache:
        _cache[key] = R.keep_largest(_case(name), ncls, keep, min_size, conn, classes)
    return _cache[key]


def _run(dev, name, ncls=5, conn=1, keep=1, min_size=0, classes=None, inplace=False):
    """label and filter through the raw wrappers with 0xAB-filled outputs -> (roots, out, stats) as numpy; checks the counters and that the
    input is left alone"""
    K, C = pkg("kernels"), pkg("components")
    host = _case(name)
    vol = torch.from_numpy(host.copy()).to(dev)
    roots = torch.full(host.shape, -1, dtype=torch.int32, device=dev)
    roots.view(torch.uint8).fill_(0xAB)
    out = vol if inplace else torch.full(host.shape, 0xAB, dtype=torch.uint8, device=dev)
    lib, D, ws = K._components_ws(vol)
    vp = lambda t: ctypes_ptr(t)
    K.check(lib.pnp_label_components(vp(vol), D[0], D[1], D[2], ncls, conn, vp(roots), vp(ws), ws.numel(), K._stream()), "pnp_label_components")
    assert K.components_errors(ws)[0] == 0
    stats = torch.full((ncls, 4), -1, dtype=torch.int64, device=dev)
    K.check(lib.pnp_filter_components(vp(vol), vp(roots), D[0], D[1], D[2], ncls, C.class_mask(ncls, classes), keep, min_size, vp(out), vp(stats),
                                      vp(ws), ws.numel(), K._stream()), "pnp_filter_components")
    assert K.components_errors(ws) == (0, 0)
    if not inplace:
        assert np.array_equal(vol.cpu().numpy(), host), "the input volume was written"
    return roots.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy()


def ctypes_ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def _check(dev, name, ncls=5, conn=1, **kw):
    inplace = kw.pop("inplace", False)
    roots, out, stats = _run(dev, name, ncls, conn, inplace=inplace, **kw)
    want_out, want_stats, want_roots = _ref(name, ncls, conn, **kw)
    assert roots.dtype == np.int32 and np.array_equal(roots, want_roots), "%d of %d roots differ" % (int((roots != want_roots).sum()), roots.size)
    assert np.array_equal(stats, want_stats), (stats.tolist(), want_stats.tolist())
    assert out.dtype == np.uint8 and np.array_equal(out, want_out), "%d of %d voxels differ" % (int((out != want_out).sum()), out.size)
    return roots, out, stats


@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("name", ["one_zero", "one_three", "background", "solid"])
def test_degenerate_volumes(dev, name, conn):
    roots, out, stats = _check(dev, name, conn=conn)
    if name == "solid":
        assert (roots == 0).all() and stats[2].tolist() == [1, 48285, 48285, 48285] and (out == 2).all()
    if name == "one_three":
        assert roots.item() == 0 and out.item() == 3 and stats[3].tolist() == [1, 1, 1, 1]
    if name in ("one_zero", "background"):
        assert (roots == -1).all() and not out.any() and not stats.any()


@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("name", ["random", "snake", "blobs"])
def test_labels_and_filter_equal_the_restatement(dev, name, conn):
    roots, out, stats = _check(dev, name, conn=conn)
    if name == "snake":
        assert stats[1].tolist() == [1, 18784, 18784, 18784] and set(np.unique(roots)) == {-1, 0}
    if name == "random":
        assert stats[1:, 0].sum() > 1000, "the three connectivities must differ: %s" % stats[:, 0]


def test_the_connectivities_differ_on_the_random_case(dev):
    counts = [int(_ref("random", 5, c)[1][:, 0].sum()) for c in (1, 2, 3)]
    assert counts[0] > counts[1] > counts[2] > 0, counts


def test_ties_go_to_the_lower_root(dev):
    roots, out, stats = _check(dev, "ties", keep=1)
    assert out[0, 0, 1:5].all() and not out[1].any() and stats[1].tolist() == [3, 10, 4, 4]
    _, out2, stats2 = _check(dev, "ties", keep=2)
    assert out2[0, 0, 1] == 1 and out2[1, 1, 4] == 1 and not out2[3, 0].any() and stats2[1].tolist() == [3, 10, 8, 4]
    assert out2[2, 0, 0] == 2 and out2[3, 4, 5] == 0
    _, out3, stats3 = _check(dev, "ties", keep=0, min_size=3)
    assert stats3[1].tolist() == [3, 10, 8, 4] and stats3[2].tolist() == [3, 5, 3, 3]
    _check(dev, "ties", keep=8)
    _check(dev, "ties", keep=0)


@pytest.mark.parametrize("conn", [1, 3])
def test_more_ranks_and_min_size_on_the_random_case(dev, conn):
    _check(dev, "random", conn=conn, keep=3, min_size=4)
    _check(dev, "random", conn=conn, keep=0, min_size=5)
    _check(dev, "random", conn=conn, keep=8)


def test_class_mask_filters_only_its_classes(dev):
    _, out, stats = _check(dev, "blobs", keep=1, classes=[2, 4])
    v = _case("blobs")
    assert np.array_equal(out == 1, v == 1) and np.array_equal(out == 3, v == 3)
    assert stats[1, 2] == stats[1, 1] and stats[2, 2] == stats[2, 3] < stats[2, 1]


def test_in_place(dev):
    _check(dev, "blobs", conn=2, inplace=True)
    _check(dev, "random", conn=1, keep=2, min_size=3, inplace=True)


def test_labels_at_or_above_ncls_are_background(dev):
    v = _case("high")
    assert set(np.unique(v)) == set(range(1, 8))
    roots, out, stats = _check(dev, "high", ncls=2, conn=1)
    assert np.array_equal(roots >= 0, v == 1) and not out[v != 1].any() and stats.shape == (2, 4)
    _check(dev, "high", ncls=8, conn=2, keep=2)
    _check(dev, "high", ncls=4, conn=3, keep=0, min_size=7)


def test_two_runs_are_bit_identical(dev):
    a = _run(dev, "blobs", conn=1)
    b = _run(dev, "blobs", conn=1)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_public_functions(dev):
    C = pkg("components")
    v = torch.from_numpy(_case("random").copy()).to(dev)
    want_out, want_stats, want_roots = _ref("random", 5, 2)
    roots = C.label_components(v, connectivity=2)
    assert roots.dtype == torch.int32 and tuple(roots.shape) == tuple(v.shape) and np.array_equal(roots.cpu().numpy(), want_roots)
    out, stats = C.keep_largest(v, connectivity=2)
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(stats.cpu().numpy(), want_stats) and C.last_errors == (0, 0)
    assert np.array_equal(v.cpu().numpy(), _case("random"))
    same, _ = C.keep_largest(v, connectivity=2, out=v)
    assert same is v and np.array_equal(v.cpu().numpy(), want_out)
    with pytest.raises(ValueError, match="contiguous"):
        C.keep_largest(out.permute(2, 0, 1))
    with pytest.raises(ValueError, match="uint8"):
        C.keep_largest(out.to(torch.int32))
    with pytest.raises(ValueError, match=r"\[D0, D1, D2\]"):
        C.label_components(out[0])
    with pytest.raises(ValueError, match="does not match"):
        C.keep_largest(out, out=torch.empty((3, 3, 3), dtype=torch.uint8, device=dev))
