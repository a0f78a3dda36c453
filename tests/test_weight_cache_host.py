"""weight_cache.py on CPU tensors against a stand-in library: the write log, range-limited bf16 shadows, remembered negative answers, one
identity check for both artefacts of a filter, eviction under a pinned step.  No device."""
import ctypes

import pytest
import torch

from conftest import pkg


class G(object):
    R = S = 3


@pytest.fixture
def host(monkeypatch):
    """a fresh WeightCache behind kernels' entry points, a library that records its calls, casts that record theirs"""
    K, WC = pkg("kernels"), pkg("weight_cache")
    calls, casts = [], []

    class FakeLib(object):
        def pnp_conv2d_wino_filter_bytes(self, C, Kf):
            return 36 * C * Kf * 4

        def pnp_conv2d_wino_filter_bind(self, w, kind, U, n):
            calls.append(("bind" if U is not None else "unbind", getattr(w, "value", w), kind))
            return 0

        def pnp_weights_changed(self, lo, hi):
            calls.append(("changed", getattr(lo, "value", lo), getattr(hi, "value", hi)))

        def pnp_conv2d_wino_chosen(self, g, kind):
            return 4

        def pnp_filter_bf16(self, w, w_io, w_oi, *a):
            casts.append(("refresh", w_io.data_ptr(), w_oi.data_ptr()))
            return 0

    def new_pair(w):
        pair = torch.zeros(1), torch.zeros(1)
        casts.append(("new", pair[0].data_ptr(), pair[1].data_ptr()))
        return pair

    cache = WC.WeightCache()
    monkeypatch.setattr(WC, "CACHE", cache)
    monkeypatch.setattr(K._lib, "load", lambda: FakeLib())
    monkeypatch.setattr(ctypes, "byref", lambda g: g)
    monkeypatch.setattr(K, "U_CACHE", True)
    for name in ("_p", "_ph"):
        monkeypatch.setattr(K, name, lambda t: t)
    monkeypatch.setattr(K, "_stream", lambda: None)
    monkeypatch.setattr(K, "filter_bf16", new_pair)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return K, WC, cache, calls, casts


def _range(w):
    return (w.data_ptr(), w.data_ptr() + 4 * w.numel())


def test_write_log_overlap_floor_and_capacity():
    WC = pkg("weight_cache")
    log = WC.WriteLog()
    assert log.epoch == 0 and not log.touched(0, 0, 1 << 40)
    log.report([(100, 200)])
    e1 = log.epoch
    # half-open at both ends: ranges that only touch do not overlap
    assert not log.touched(0, 0, 100) and not log.touched(0, 200, 300)
    assert log.touched(0, 0, 101) and log.touched(0, 199, 300) and log.touched(0, 120, 130) and log.touched(0, 0, 1000)
    assert not log.touched(e1, 0, 1000)                   # filled at (or after) the report
    log.report(None)                                      # unknown extent: everything filled earlier is stale, named or not
    assert log.touched(e1, 5000, 5001) and not log.touched(log.epoch, 100, 200)
    log = WC.WriteLog()
    for i in range(WC.LOG_MAX):
        log.report([(1000 * i, 1000 * i + 10)])
    assert len(log.pending) == WC.LOG_MAX == 64 and log.floor == 0
    assert log.touched(0, 0, 10) and log.touched(0, 63000, 63010) and not log.touched(0, 500, 600)
    assert not log.touched(1, 0, 10) and log.touched(63, 63005, 63006)
    log.report([(7, 8)])                                  # the 65th: the floor moves
    assert log.floor == log.epoch == 65 and not log.pending
    assert log.touched(64, 500, 600) and not log.touched(65, 0, 10)


def test_range_limited_shadows(host):
    K, WC, cache, calls, casts = host
    w, other = torch.zeros(3, 3, 32, 64), torch.zeros(3, 3, 32, 64)
    io, oi = K.filter_shadows(w)
    assert [c[0] for c in casts] == ["new"] and cache.casts == 1
    K.weights_changed([_range(other)])                    # somebody else's weights
    assert K.filter_shadows(w)[0] is io and len(casts) == 1
    K.weights_changed([_range(other), _range(w)])         # this filter among them: one refresh, into the same buffers
    for _ in range(3):
        got = K.filter_shadows(w)
    assert got[0] is io and got[1] is oi and casts[1:] == [("refresh", io.data_ptr(), oi.data_ptr())]
    K.weights_changed()                                   # the whole arena: one refresh
    for _ in range(3):
        got = K.filter_shadows(w)
    assert got[0] is io and got[1] is oi and casts[2:] == [("refresh", io.data_ptr(), oi.data_ptr())] and cache.casts == 3
    assert K.memory_report()["bf16_filter_entries"] == 1 and calls == []          # nothing is lent: the library is never called


def test_a_negative_answer_is_remembered(host, monkeypatch):
    K, WC, cache, calls, casts = host
    w, other = torch.zeros(3, 3, 32, 64), torch.zeros(3, 3, 32, 64)
    K.filter_shadows(w)
    K.weights_changed([_range(other)])
    scans = []
    touched = cache.log.touched
    monkeypatch.setattr(cache.log, "touched", lambda *a: (scans.append(a), touched(*a))[1])
    K.filter_shadows(w)
    assert len(casts) == 1 and len(scans) == 1            # scanned once, not touched, no cast
    K.filter_shadows(w)
    K.filter_shadows(w)
    assert len(casts) == 1 and len(scans) == 1            # the answer was kept
    K.weights_changed([_range(w)])                        # a later write has a later epoch: still seen
    K.filter_shadows(w)
    assert [c[0] for c in casts] == ["new", "refresh"] and len(scans) == 2


def test_one_identity_check_serves_both_artefacts(host):
    K, WC, cache, calls, casts = host
    w = torch.zeros(3, 3, 32, 32)
    w._pnp_var = True
    K.filter_shadows(w)
    K._wino_u(w, G(), 0)
    K._wino_u(w, G(), 1)
    assert len(cache.records) == 1 and cache.bound(w.data_ptr()) == [0, 1] and len(casts) == 1
    assert calls == [("bind", w.data_ptr(), 0), ("bind", w.data_ptr(), 1)]
    for first in ("shadows", "bind"):                     # whichever reader meets the moved version counter first
        w.add_(1.0)
        del calls[:], casts[:]
        for _ in range(2):
            if first == "shadows":
                K.filter_shadows(w)
            K._wino_u(w, G(), 0)
            K._wino_u(w, G(), 1)
            K.filter_shadows(w)
        assert calls == [("changed",) + _range(w)] and [c[0] for c in casts] == ["refresh"], first
    # a tensor that is not the marked one on the same address: the buffers go back, the shadows (same owner, same version) stay
    K.filter_shadows(w.view(3, 3, 32, 32))
    assert sorted(calls[1:]) == [("unbind", w.data_ptr(), 0), ("unbind", w.data_ptr(), 1)] and len(casts) == 1


def test_eviction_waits_for_the_last_pinned_step(host, monkeypatch):
    K, WC, cache, calls, casts = host
    monkeypatch.setattr(WC, "SHADOW_RECORDS_MAX", 3)
    monkeypatch.setattr(WC, "U_BINDINGS_MAX", 3)
    ws = [torch.zeros(3, 3, 4, 4) for _ in range(4)]
    for w in ws:
        K.filter_shadows(w)
    cache.pin()
    K.weights_changed()
    K.weights_changed([(0, 1)])
    assert K.memory_report()["bf16_filter_entries"] == 4 and K.memory_report()["recorded_steps_alive"] == 1
    assert cache.unpin() == 0
    K.weights_changed([(0, 1)])                           # a ranged report never evicts
    assert K.memory_report()["bf16_filter_entries"] == 4
    K.weights_changed()
    assert K.memory_report()["bf16_filter_entries"] == 0 and not cache.records
    for w in ws[:2]:                                      # the same rule for U bindings: 2 filters x 2 passes > 3
        w._pnp_var = True
        K._wino_u(w, G(), 0)
        K._wino_u(w, G(), 1)
    cache.pin()
    K.weights_changed()
    assert K.memory_report()["winograd_filter_entries"] == 4 and calls[-1] == ("changed", None, None)
    cache.unpin()
    K.weights_changed()
    assert K.memory_report()["winograd_filter_entries"] == 0 and calls[-1] == ("unbind", None, 0) and not cache.records
