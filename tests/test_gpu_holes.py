"""-m gpu: pnp_fill_holes (csrc/components.hip) against tests/holes_ref.py.  Everything is an integer: every comparison is
exact equality over the WHOLE allocation (out and stats are pre-filled with 0xAB), the input is checked untouched, and after every call the
three device error counters read 0.

The shapes are §16's smallest tile-crossing ones: 37 x 29 x 45 = 5 x 4 x 2 tiles of 8 x 8 x 32, 33 x 33 x 64 = 5 x 5 x 2, 96 x 80 x 72 =
12 x 10 x 3."""
import ctypes

import numpy as np
import pytest
import torch

import holes_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name):
    if name not in _cache:
        v = R.CASES[name]()
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name]


def _ref(name, ncls=5, max_size=0, classes=None):
    key = (name, ncls, max_size, None if classes is None else tuple(classes))
    if key not in _cache:
        _cache[key] = R.fill_holes(_case(name), ncls, max_size, classes)
    return _cache[key]


def _run(dev, name, ncls=5, max_size=0, classes=None, inplace=False):
    """the raw entry point through kernels.workspace() with 0xAB-filled outputs -> (out, stats) as numpy"""
    K, C = pkg("kernels"), pkg("components")
    host = _case(name)
    vol = torch.from_numpy(host.copy()).to(dev)
    out = vol if inplace else torch.full(host.shape, 0xAB, dtype=torch.uint8, device=dev)
    stats = torch.empty((ncls, 4), dtype=torch.int64, device=dev)
    stats.view(torch.uint8).fill_(0xAB)
    D = host.shape
    lib = pkg("_lib").load()
    ws = K.workspace(lib.pnp_fill_holes_workspace_bytes(D[0], D[1], D[2], ncls), dev, slot="components")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    K.check(lib.pnp_fill_holes(vp(vol), D[0], D[1], D[2], ncls, C.class_mask(ncls, classes), max_size, vp(out), vp(stats), vp(ws), ws.numel(),
                               K._stream()), "pnp_fill_holes")
    assert K.fill_holes_errors(ws) == (0, 0, 0)
    if not inplace:
        assert np.array_equal(vol.cpu().numpy(), host), "the input volume was written"
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(dev, name, ncls=5, **kw):
    inplace = kw.pop("inplace", False)
    out, stats = _run(dev, name, ncls, inplace=inplace, **kw)
    want_out, want_stats, info = _ref(name, ncls, **kw)
    assert stats.dtype == np.int64 and np.array_equal(stats, want_stats), (stats.tolist(), want_stats.tolist())
    assert out.dtype == np.uint8 and np.array_equal(out, want_out), "%d of %d voxels differ" % (int((out != want_out).sum()), out.size)
    return out, stats, info


@pytest.mark.parametrize("name", ["one_zero", "one_three", "thin_a", "thin_b", "background", "solid"])
def test_volumes_without_a_cavity(dev, name):
    out, stats, info = _check(dev, name)
    assert info["cavities"] == 0 and not stats.any()
    assert np.array_equal(out, _case(name)), "nothing is fillable: the labels come back as they are"


@pytest.mark.parametrize("name, cls", [("shell", 1), ("corner", 2)])
def test_a_cavity_in_a_shell_inside_a_tile_and_across_a_tile_corner(dev, name, cls):
    out, stats, _ = _check(dev, name)
    v = _case(name)
    assert int((v == 0).sum() - (out == 0).sum()) == 27 and np.array_equal(out[v != 0], v[v != 0])
    assert stats[0].tolist() == [1, 27, 0, 0] and stats[cls].tolist() == [1, 27, 27, 0]
    assert (out[7:10, 7:10, 31:34] == 2).all() if name == "corner" else (out[12:15, 12:15, 22:25] == 1).all()


def test_a_channel_to_a_face_leaves_the_cavity_and_a_plug_fills_it(dev):
    out, stats, _ = _check(dev, "channel")
    assert not stats.any() and np.array_equal(out, _case("channel"))
    out, stats, _ = _check(dev, "plugged")
    assert stats[0].tolist() == [1, 38, 0, 0] and stats[1].tolist() == [1, 38, 38, 0] and out[0, 13, 23] == 2 and (out[1:] == 1).all()


def test_an_edge_diagonal_leak_is_no_leak(dev):
    out, stats, _ = _check(dev, "diagonal")
    assert (out[12:15, 12:15, 22:25] == 1).all() and not out[0:12, 11, 22].any() and stats[1].tolist() == [1, 27, 27, 0]


def test_the_vote_and_the_tie_rule(dev):
    out, stats, info = _check(dev, "vote")
    assert out[8, 8, 32] == 3 and stats[3].tolist() == [1, 1, 1, 0] and info["ties"] == 0 and info["multi"] == 1
    out, stats, info = _check(dev, "tie")
    assert out[16, 8, 31] == 2 and stats[2].tolist() == [1, 1, 1, 0] and info["ties"] == 1


def test_a_winner_outside_the_mask_leaves_the_cavity(dev):
    out, stats, _ = _check(dev, "vote", classes=[2])
    assert out[8, 8, 32] == 0 and stats[0].tolist() == [1, 1, 1, 1] and stats[3].tolist() == [0, 0, 0, 1] and not stats[2].any()
    out, stats, _ = _check(dev, "vote", classes=[3, 4])
    assert out[8, 8, 32] == 3 and stats[3].tolist() == [1, 1, 1, 0]


def test_max_size(dev):
    out, stats, _ = _check(dev, "sizes", max_size=8)
    assert stats[0].tolist() == [4, 100, 2, 91] and stats[1].tolist() == [2, 9, 8, 2]
    assert out[2, 2, 2] == 1 and (out[4:6, 4:6, 4:6] == 1).all() and not out[10:13, 10:13, 10:13].any() and not out[14:18, 14:18, 30:34].any()
    _, stats, _ = _check(dev, "sizes", max_size=27)
    assert stats[1].tolist() == [3, 36, 27, 1]
    _, stats, _ = _check(dev, "sizes", max_size=1 << 40)
    assert stats[1].tolist() == [4, 100, 64, 0]
    _, stats, _ = _check(dev, "sizes")
    assert stats[1].tolist() == [4, 100, 64, 0]


def test_labels_at_or_above_ncls_are_background(dev):
    out, stats, _ = _check(dev, "high")
    assert out[13, 13, 23] == 1 and out[0, 0, 0] == 0 and out[30, 20, 40] == 0 and out[20, 2, 2] == 0 and out.max() == 1
    assert stats[0].tolist() == [1, 1, 0, 0]


@pytest.mark.parametrize("ncls", [2, 4, 8])
def test_ncls(dev, ncls):
    out, stats, info = _check(dev, "all_labels", ncls=ncls)
    assert stats.shape == (ncls, 4) and out.max() < ncls and info["cavities"] > 50
    _check(dev, "all_labels", ncls=ncls, max_size=1, classes=[ncls - 1])


def test_in_place(dev):
    _check(dev, "random", inplace=True)
    _check(dev, "blobs", max_size=3, classes=[1, 4], inplace=True)


def test_two_runs_are_bit_identical(dev):
    a = _run(dev, "blobs")
    b = _run(dev, "blobs")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_the_snake(dev):
    """a closed one-voxel-wide path of 16 127 background voxels through every tile: the worst case for chain depth; with one end on a face
    nothing is filled"""
    out, stats, info = _check(dev, "snake")
    assert info["cavities"] == 1 and stats[0].tolist() == [1, 16127, 0, 0] and out.min() >= 1
    out, stats, info = _check(dev, "snake_leak")
    assert info["cavities"] == 0 and not stats.any() and int((out == 0).sum()) == 16128


@pytest.mark.parametrize("name", ["random", "blobs"])
def test_random_volumes(dev, name):
    _, _, info = _ref(name)
    assert info["cavities"] >= 100 and info["ties"] >= 10 and info["multi"] >= 100, {k: info[k] for k in ("cavities", "ties", "multi")}
    _check(dev, name)
    _check(dev, name, max_size=2)
    _check(dev, name, classes=[2, 4])
    _check(dev, name, max_size=5, classes=[1])


def test_keep_largest_then_fill_holes_closes_an_emptied_pocket(dev):
    C = pkg("components")
    v = torch.from_numpy(_case("pocket").copy()).to(dev)
    kept, _ = C.keep_largest(v, keep=1)
    assert not kept[12:14, 12:14, 22:24].any() and (kept[25:30, 5:10, 5:10] == 3).all()
    filled, stats = C.fill_holes(kept)
    want = R._block()
    want[25:30, 5:10, 5:10] = 3
    assert np.array_equal(filled.cpu().numpy(), want) and stats.cpu().numpy()[1].tolist() == [1, 8, 8, 0]
    untouched, stats0 = C.fill_holes(v)                  # without the filter the pocket is anatomy: a class inside a class
    assert np.array_equal(untouched.cpu().numpy(), _case("pocket")) and not stats0.any()


def test_public_function(dev):
    C = pkg("components")
    v = torch.from_numpy(_case("random").copy()).to(dev)
    want_out, want_stats, _ = _ref("random", 5, 4, (1, 3))
    out, stats = C.fill_holes(v, max_size=4, classes=[1, 3])
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(stats.cpu().numpy(), want_stats) and C.last_fill_errors == (0, 0, 0)
    assert stats.dtype == torch.int64 and np.array_equal(v.cpu().numpy(), _case("random"))
    same, _ = C.fill_holes(v, max_size=4, classes=[1, 3], out=v)
    assert same is v and np.array_equal(v.cpu().numpy(), want_out)
    with pytest.raises(ValueError, match="contiguous"):
        C.fill_holes(out.permute(2, 0, 1))
    with pytest.raises(ValueError, match="uint8"):
        C.fill_holes(out.to(torch.int32))
    with pytest.raises(ValueError, match=r"\[D0, D1, D2\]"):
        C.fill_holes(out[0])
    with pytest.raises(ValueError, match="does not match"):
        C.fill_holes(out, out=torch.empty((3, 3, 3), dtype=torch.uint8, device=dev))
