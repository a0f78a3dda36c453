"""-m gpu: csrc/components.hip over its whole domain against tests/components_ref.py, with the contract of
tests/test_gpu_components.py: the raw entry points, roots and out pre-filled with 0xAB, exact equality of roots, stats and out over the
whole allocation, both device error counters 0 after every call, the input left alone.  Everything is an integer: no tolerances.

The case lists live in tests/components_domain_cases.py; tests/test_components_domain_host.py proves without a GPU that they reach every
branch of the kernels' geometry (each backward offset across a tile border and inside a tile, the border kernel's skip rule, the count
kernel's crowded table and its tail loader, rank launches 1 ... 8, extents 1 and 4096) and pins the reference to scipy on every case."""
import ctypes

import numpy as np
import pytest
import torch

import components_domain_cases as CD
from conftest import pkg

pytestmark = pytest.mark.gpu


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _label(dev, host, ncls, conn):
    """-> (vol on the device, roots on the device (0xAB-filled before the call)); the labelling's error counter must read 0"""
    K = pkg("kernels")
    vol = torch.from_numpy(host.copy()).to(dev)
    roots = torch.empty(host.shape, dtype=torch.int32, device=dev)
    roots.view(torch.uint8).fill_(0xAB)
    lib, D, ws = K._components_ws(vol)
    K.check(lib.pnp_label_components(_vp(vol), D[0], D[1], D[2], ncls, conn, _vp(roots), _vp(ws), ws.numel(), K._stream()), "pnp_label_components")
    assert K.components_errors(ws)[0] == 0
    return vol, roots


def _filter(dev, host, vol, roots, ncls, keep, min_size, classes):
    """-> (out, stats) as numpy; both counters must read 0 and the input must be unchanged"""
    K, C = pkg("kernels"), pkg("components")
    out = torch.full(host.shape, 0xAB, dtype=torch.uint8, device=dev)
    stats = torch.full((ncls, 4), -1, dtype=torch.int64, device=dev)
    lib, D, ws = K._components_ws(vol)
    K.check(lib.pnp_filter_components(_vp(vol), _vp(roots), D[0], D[1], D[2], ncls, C.class_mask(ncls, classes), keep, min_size, _vp(out), _vp(stats),
                                      _vp(ws), ws.numel(), K._stream()), "pnp_filter_components")
    assert K.components_errors(ws) == (0, 0)
    assert np.array_equal(vol.cpu().numpy(), host), "the input volume was written"
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(dev, name, ncls, conn, keep=1, min_size=0, classes=None, labelled=None):
    """label (unless `labelled` hands over an earlier labelling of the same case) and filter; everything equals the restatement"""
    host = CD.volume(name)
    want_out, want_stats, want_roots = CD.ref_filter(name, ncls, conn, keep, min_size, classes)
    vol, roots = labelled or _label(dev, host, ncls, conn)
    got = roots.cpu().numpy()
    what = "%s ncls=%d conn=%d keep=%d min_size=%d classes=%s: " % (name, ncls, conn, keep, min_size, classes)
    assert got.dtype == np.int32 and np.array_equal(got, want_roots), what + "%d of %d roots differ" % (int((got != want_roots).sum()), got.size)
    out, stats = _filter(dev, host, vol, roots, ncls, keep, min_size, classes)
    assert np.array_equal(stats, want_stats), what + "stats %s, expected %s" % (stats.tolist(), want_stats.tolist())
    assert out.dtype == np.uint8 and np.array_equal(out, want_out), what + "%d of %d voxels differ" % (int((out != want_out).sum()), out.size)
    return got, out, stats


@pytest.mark.parametrize("conn", CD.CONNS)
def test_one_pair_per_offset_across_tile_corners_and_inside_a_tile(dev, conn):
    for name, ncls in CD.PAIR_CASES:
        two = name.startswith("pairs2")
        roots, out, stats = _check(dev, name, ncls, conn, keep=0)
        assert stats[1:, 0].sum() == CD.pairs_components(conn, two), (name, conn, stats.tolist())
        assert len(np.unique(roots)) - 1 == CD.pairs_components(conn, two)
        assert np.array_equal(out, CD.volume(name))


@pytest.mark.parametrize("conn", CD.CONNS)
def test_extent_sweep(dev, conn):
    for name, ncls in CD.SWEEP_CASES:
        _check(dev, name, ncls, conn)


@pytest.mark.parametrize("conn", CD.CONNS)
def test_lines_at_the_extent_limit(dev, conn):
    for name, ncls in CD.LINE_CASES:
        roots, out, stats = _check(dev, name, ncls, conn, keep=0)
        if name.startswith("solid"):
            assert (roots == 0).all() and stats[1].tolist() == [1, 4096, 4096, 4096]
        else:
            assert stats[1:, 0].sum() == 91 and stats[1, 3] == 89 and stats[2, 3] == 90      # 4096 = 1 + ... + 90 + 1: the 91st run is cut


@pytest.mark.parametrize("conn", CD.CONNS)
def test_checkerboard_crowds_the_count_table(dev, conn):
    roots, out, stats = _check(dev, "checker", 2, conn, keep=0)
    n = 24 * 24 * 40 // 2
    assert stats[1].tolist() == ([n, n, n, 1] if conn == 1 else [1, n, n, n])
    _check(dev, "checker", 2, conn, keep=8)
    _check(dev, "checker", 2, conn, keep=0, min_size=2)


@pytest.mark.parametrize("conn", CD.CONNS)
def test_chains_across_x_and_y(dev, conn):
    for name, ncls in CD.SNAKE_CASES:
        roots, out, stats = _check(dev, name, ncls, conn)
        assert stats[1].tolist() == [1, 18784, 18784, 18784] and set(np.unique(roots)) == {-1, 0}


@pytest.mark.parametrize("conn", CD.CONNS)
def test_diagonals_join_from_their_connectivity_on(dev, conn):
    for name, ncls in CD.DIAGONAL_CASES:
        roots, out, stats = _check(dev, name, ncls, conn, keep=0)
        joined = conn >= CD.DIAGONALS[name][1]
        assert stats[1].tolist() == ([1, 40, 40, 40] if joined else [40, 40, 40, 1]), (name, conn, stats.tolist())


@pytest.mark.parametrize("ncls", CD.FILTER_NCLS)
def test_filter_domain(dev, ncls):
    host = CD.volume("filter")
    labelled = _label(dev, host, ncls, 1)
    for keep, min_size, mask in CD.filter_configs(ncls):
        _check(dev, "filter", ncls, 1, keep, min_size, mask, labelled=labelled)
    for conn in (2, 3):                                   # the bars do not touch: the same answer under every connectivity
        _check(dev, "filter", ncls, conn, 2, 3, None)


def test_filter_a_component_larger_than_2_16(dev):
    labelled = _label(dev, CD.volume("blobs"), 5, 1)
    for keep, min_size, mask in ((1, 0, None), (2, 1 << 16, None), (0, (1 << 16) + 1, (1, 3)), (8, 0, (2,))):
        _, _, stats = _check(dev, "blobs", 5, 1, keep, min_size, mask, labelled=labelled)
        assert stats[:, 3].max() > 1 << 16


def test_filtering_a_filtered_volume_changes_nothing(dev):
    for name, ncls, conn, keep, min_size, mask in (("filter", 8, 1, 2, 3, None), ("filter", 8, 1, 0, 4, (1, 3, 4, 6)), ("filter", 2, 1, 8, 0, None),
                                                   ("sweep_9x9x65", 3, 2, 3, 2, None), ("checker", 2, 1, 5, 0, None), ("blobs", 5, 3, 1, 0, None)):
        _, out, stats = _check(dev, name, ncls, conn, keep, min_size, mask)
        vol, roots = _label(dev, out, ncls, conn)
        again, stats2 = _filter(dev, out, vol, roots, ncls, keep, min_size, mask)
        assert np.array_equal(again, out), (name, keep, min_size, mask)
        assert np.array_equal(stats2[:, 2], stats[:, 2]) and np.array_equal(stats2[:, 1], stats[:, 2])
