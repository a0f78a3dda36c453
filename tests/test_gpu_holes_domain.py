"""-m gpu: pnp_fill_holes (csrc/components.hip) over everything it accepts, against tests/holes_ref.py.  The contract is
tests/test_gpu_holes.py's, tightened: the raw entry point, exact equality of out and stats, the three device error counters 0 after every
call, the input unchanged unless the call is in place, and
  * out and stats are slices of larger allocations with 64 guard bytes of 0xAB on each side (the slices themselves start as 0xAB, which is
    no label: equality with the reference shows that every byte was written); the guards must be intact;
  * vol and out start at byte offsets 0 or 1, 2, 3 into their allocations;
  * the workspace is EXACTLY pnp_fill_holes_workspace_bytes(...) bytes at a 256-byte-aligned offset inside a larger buffer, pre-filled
    with 0xFF like the buffer around it, which must still read 0xFF after the call; a run on a zero-filled workspace gives the same bytes.
Everything is an integer: no tolerances.

The runs live in tests/holes_domain_cases.py; tests/test_holes_domain_host.py proves without a GPU that they reach every branch (each
face region of fh_open_kernel as the only leak, extents 1, 2, 3 and 4096, the count kernel's crowded table on a sizes array that was
zeroed at roots only, a contact nibble of 6 at class 7, sums decided by one contact, the 64-bit size limit) and pins the reference to
scipy on every volume.  A misaligned workspace and a partially overlapping out are host refusals, tested there only."""
import ctypes

import numpy as np
import pytest
import torch

import holes_domain_cases as HD
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD, WS_GUARD, CANARY, WS_CANARY = 64, 256, 0xAB, 0xFF


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _offsets(place, k):
    """the byte offsets of vol and out into their allocations: place 0 = (0, 0), place 1 = two different ones of (1, 2, 3), by the run"""
    return (0, 0) if place == 0 else ((1, 2, 3)[k % 3], (1, 2, 3)[(k + 1) % 3])


def _run(dev, run, place=0, k=0, inplace=False, ws_fill=WS_CANARY):
    """one raw call under guards -> (out, stats) as numpy"""
    K, C = pkg("kernels"), pkg("components")
    name, ncls, classes, max_size = run
    host = HD.volume(name)
    n, D = host.size, host.shape
    vol_off, out_off = _offsets(place, k)
    out_all = torch.full((out_off + GUARD + n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    out = out_all[out_off + GUARD:out_off + GUARD + n]
    if inplace:
        vol = out
    else:
        vol_all = torch.full((vol_off + n,), CANARY, dtype=torch.uint8, device=dev)
        vol = vol_all[vol_off:]
    vol.copy_(torch.from_numpy(host.reshape(-1).copy()))
    assert out.data_ptr() % 4 == out_off % 4 and vol.data_ptr() % 4 == (out_off if inplace else vol_off) % 4
    stats_all = torch.empty((8 + 4 * ncls + 8,), dtype=torch.int64, device=dev)
    stats_all.view(torch.uint8).fill_(CANARY)
    stats = stats_all[8:8 + 4 * ncls]
    lib = pkg("_lib").load()
    need = int(lib.pnp_fill_holes_workspace_bytes(D[0], D[1], D[2], ncls))
    assert need > 0 and need % 256 == 0
    ws_all = torch.full((512 + need + WS_GUARD,), WS_CANARY, dtype=torch.uint8, device=dev)
    at = (-ws_all.data_ptr()) % 256 + 256
    ws = ws_all[at:at + need]
    assert ws.data_ptr() % 256 == 0 and at + need + WS_GUARD <= ws_all.numel()
    ws.fill_(ws_fill)
    K.check(lib.pnp_fill_holes(_vp(vol), D[0], D[1], D[2], ncls, C.class_mask(ncls, classes), max_size, _vp(out), _vp(stats), _vp(ws), need,
                               K._stream()), "pnp_fill_holes")
    what = "%s ncls=%d classes=%s max_size=%d place=%d inplace=%s: " % (name, ncls, classes, max_size, place, inplace)
    assert K.fill_holes_errors(ws) == (0, 0, 0), what + "error counters"
    assert bool((ws_all[:at] == WS_CANARY).all()) and bool((ws_all[at + need:] == WS_CANARY).all()), what + "written outside the workspace"
    o = out_all.cpu().numpy()
    assert (o[:out_off + GUARD] == CANARY).all() and (o[out_off + GUARD + n:] == CANARY).all(), what + "written outside out"
    s = stats_all.cpu().numpy()
    assert (s[:8].view(np.uint8) == CANARY).all() and (s[8 + 4 * ncls:].view(np.uint8) == CANARY).all(), what + "written outside stats"
    if not inplace:
        assert bool((vol_all[:vol_off] == CANARY).all()) and np.array_equal(vol.cpu().numpy(), host.reshape(-1)), what + "the input volume was written"
    return o[out_off + GUARD:out_off + GUARD + n].reshape(D).copy(), s[8:8 + 4 * ncls].reshape(ncls, 4).copy()


def _check(dev, run, **kw):
    out, stats = _run(dev, run, **kw)
    want_out, want_stats, info = HD.ref(*run)
    what = "%s %s: " % (run, kw)
    assert stats.dtype == np.int64 and np.array_equal(stats, want_stats), what + "stats %s, expected %s" % (stats.tolist(), want_stats.tolist())
    assert out.dtype == np.uint8 and np.array_equal(out, want_out), what + "%d of %d voxels differ" % (int((out != want_out).sum()), out.size)
    return out, stats, info


def _check_both_places(dev, run, k=0):
    _check(dev, run, place=0, k=k)
    return _check(dev, run, place=1, k=k)


def _same_on_a_zeroed_workspace(dev, run):
    a = _check(dev, run)
    b = _run(dev, run, ws_fill=0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "%s: the result depends on what the workspace held" % (run,)


@pytest.mark.parametrize("place", [0, 1])
def test_extent_sweep(dev, place):
    for k, run in enumerate(HD.SWEEP_RUNS):
        out, stats, info = _check(dev, run, place=place, k=k)
        if min(out.shape) < 3:
            assert not stats.any() and np.array_equal(out, HD.volume(run[0]))
        if run[0].startswith("pin"):
            assert (out == 1).all() and stats[:2].tolist() == [[1, 1, 0, 0], [1, 1, 1, 0]]
    _same_on_a_zeroed_workspace(dev, ("sweep_9x9x33", 5, None, 0))


@pytest.mark.parametrize("face", HD.FACES, ids=[HD.FACE_NAMES[f] for f in HD.FACES])
def test_one_channel_to_each_face_leaves_the_cavity_and_a_plug_fills_it(dev, face):
    k = HD.FACES.index(face)
    leak, plug = ("leak_" + HD.FACE_NAMES[face], 5, None, 0), ("plug_" + HD.FACE_NAMES[face], 5, None, 0)
    for kw in ({"place": 0}, {"place": 1, "k": k}, {"inplace": True}, {"inplace": True, "place": 1, "k": k}):
        out, stats, _ = _check(dev, leak, **kw)
        assert not stats.any() and np.array_equal(out, HD.volume(leak[0])), "the channel to %s was not seen" % HD.FACE_NAMES[face]
        out, stats, _ = _check(dev, plug, **kw)
        s = HD.plugged_size(*face)
        assert stats[:2].tolist() == [[1, s, 0, 0], [1, s, s, 0]] and out[HD.face_voxel(*face)] == 2 and int((out == 1).sum()) == out.size - 1


@pytest.mark.parametrize("axis", "xyz")
def test_lines_at_the_extent_limit(dev, axis):
    for k, kind in enumerate(HD.LINE_KINDS):
        out, stats, info = _check_both_places(dev, ("line_%s_%s" % (axis, kind), 5, None, 0), k)
        if kind == "closed":
            assert stats[:2].tolist() == [[1, 4094, 0, 0], [1, 4094, 4094, 0]] and (out == 1).all()
        elif kind == "alt":
            assert stats[:2].tolist() == [[2047, 2047, 0, 0], [2047, 2047, 1, 0]] and out.min() >= 1
        else:
            assert not stats.any() and int((out == 0).sum()) == 4095


def test_checkerboard_crowds_the_count_table_and_uses_every_nibble(dev):
    run = HD.CHECKER_RUNS[0]
    out, stats, info = _check_both_places(dev, run, 1)
    assert info["cavities"] == 9196 and stats[0].tolist() == [9196, 9196, 0, 0] and (stats[1:, 0] > 0).all() and out.min() >= 1
    _check(dev, run, inplace=True)
    _check(dev, run, inplace=True, place=1, k=2)
    _same_on_a_zeroed_workspace(dev, run)
    _check(dev, (run[0], 8, (2, 5), 0))
    _check(dev, (run[0], 8, None, 1))


def test_two_runs_of_the_checkerboard_are_bit_identical(dev):
    a = _run(dev, HD.CHECKER_RUNS[0])
    b = _run(dev, HD.CHECKER_RUNS[0])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_contact_nibbles_at_their_limits(dev):
    out, stats, _ = _check_both_places(dev, HD.NIBBLE_RUNS[0], 2)
    assert out[HD.NIBBLE_SIX] == 7 and out[HD.NIBBLE_MIXED] == 2 and out[HD.NIBBLE_PAIR[0]] == 4 and out[HD.NIBBLE_PAIR[1]] == 4
    assert stats.tolist() == [[3, 4, 0, 0], [0] * 4, [1, 1, 1, 0], [0] * 4, [1, 2, 2, 0], [0] * 4, [0] * 4, [1, 1, 1, 0]]


@pytest.mark.parametrize("name", sorted(HD.BALANCED))
def test_a_cavity_decided_by_one_contact_of_more_than_700(dev, name):
    run = (name, 5, None, 0)
    k2, k3 = HD.BALANCED[name]
    out, stats, info = _check_both_places(dev, run, sorted(HD.BALANCED).index(name))
    win = 2 if k2 >= k3 else 3
    assert info["contacts"].tolist() == [[0, 0, 651 + k2, 651 + k3, 104 - k2 - k3]]
    assert stats[0].tolist() == [1, 651, 0, 0] and stats[win].tolist() == [1, 651, 651, 0]
    assert (out[HD.SLAB_X, HD.SLAB_Y[0]:HD.SLAB_Y[1], HD.SLAB_Z[0]:HD.SLAB_Z[1]] == win).all()
    _same_on_a_zeroed_workspace(dev, run)
    out, stats, _ = _check(dev, (name, 5, (5 - win,), 0))             # the loser alone in the mask: left, never handed over
    assert stats[0].tolist() == [1, 651, 1, 651] and stats[win].tolist() == [0, 0, 0, 1] and not out[HD.SLAB_X, HD.SLAB_Y[0], HD.SLAB_Z[0]]


def test_an_open_background_that_fills_whole_count_workgroups(dev):
    out, stats, _ = _check_both_places(dev, HD.OPEN_RUNS[0])
    assert stats[0].tolist() == [1, 27, 0, 0] and stats[3].tolist() == [1, 27, 27, 0] and (out[12:15, 12:15, 22:25] == 3).all()


def _wrapper(dev, run):
    """components.fill_holes: the Python path of the 64-bit max_size"""
    C = pkg("components")
    name, ncls, classes, max_size = run
    v = torch.from_numpy(HD.volume(name).copy()).to(dev)
    out, stats = C.fill_holes(v, num_cls=ncls, max_size=max_size, classes=classes)
    want_out, want_stats, _ = HD.ref(*run)
    assert C.last_fill_errors == (0, 0, 0) and stats.dtype == torch.int64 and np.array_equal(stats.cpu().numpy(), want_stats), run
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(v.cpu().numpy(), HD.volume(name)), run


@pytest.mark.parametrize("part", ["ncls", "masks", "max_size"])
def test_options(dev, part):
    runs = HD.option_runs()
    runs = {"ncls": runs[:7], "masks": runs[7:22], "max_size": runs[22:]}[part]
    assert len(runs) == {"ncls": 7, "masks": 15, "max_size": 10}[part]
    full = HD.ref("options", 8)[1]
    for k, run in enumerate(runs):
        out, stats, info = _check_both_places(dev, run, k)
        _wrapper(dev, run)
        if part == "ncls":
            assert stats.shape == (run[1], 4) and out.max() < run[1] and info["cavities"] > 50
        elif run[2] == ():
            assert stats[0].tolist() == [full[0, 0], full[0, 1], full[0, 0], full[0, 1]] and not stats[1:, :3].any() and stats[1:, 3].sum() == full[0, 0]
        elif part == "max_size" and (run[3] == 0 or run[3] >= HD.option_size()):       # no limit in effect, whatever the low 32 bits say
            assert np.array_equal(stats, full)
