"""-m gpu: pnp_fda_amplitude_swap (csrc/fda.hip) over everything it accepts, called directly through ctypes on the case
list of tests/fda_domain_cases.py (which tests/test_fda_domain_host.py proves reaches every edge of the kernels' launch geometry).

Per case: out lies inside a larger allocation between guards of 64 floats at -7.0, its interior filled with NaN; the workspace is exactly
pnp_fda_workspace_bytes, also between guards.  Every guard stays intact, every output element is finite and within
bar = 2 x max(fp32 route error, 1e-6) x max|ref| of the float64 reference (fda_ref.fda_ref, fda_ref.route_bar): the band_ratio condition
alone does not bound the error, which follows the phase sensitivity |T| / |S| over the band, so the bar is built per case on the same
method in float32 (fda_ref.fda_route32).  A run on a workspace of 0xFF bytes (NaN) equals a run on a zeroed one bit for bit: nothing
reads workspace the call did not write.  Band -1 samples come back bit for bit, the inputs are never written.  On the maximum-size and
B = 256 cases in place, out of place and a repeat are bit-equal; on one case kernels.fda_amplitude_swap equals the direct call."""
import ctypes

import numpy as np
import pytest
import torch

import fda_domain_cases as FD
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE = 64, -7.0


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def _guarded(n, dev, fill):
    """-> (the allocation, its interior of n floats filled with fill): GUARD floats of GUARD_VALUE on either side"""
    buf = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=torch.float32, device=dev)
    inner = buf[GUARD:GUARD + n]
    inner.fill_(fill)
    return buf, inner


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[GUARD + n:] == GUARD_VALUE).all())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _swap(dev, name, s, t, out=None, ws_byte=0x00):
    """one direct call on a guarded workspace of exactly the queried size (its bytes set to ws_byte); out None: a guarded, NaN-filled
    output.  Both sets of guards must be intact afterwards.  -> the output as float32 numpy"""
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    _, (B, Bt, H, W, C), band, pair, _, _ = FD.BY_NAME[name]
    need = lib.pnp_fda_workspace_bytes(B, Bt, H, W, C, max(band))
    assert need > 0 and need % 4 == 0, need
    wbuf, ws = _guarded(need // 4, dev, 0.0)
    ws.view(torch.uint8).fill_(ws_byte)
    n = B * H * W * C
    obuf = None
    if out is None:
        obuf, out = _guarded(n, dev, float("nan"))
    rc = lib.pnp_fda_amplitude_swap(_vp(s), B, _vp(t), Bt, H, W, C, _i32(band), _i32(pair), _vp(out), _vp(ws), need, K._stream())
    assert rc == 0, lib.pnp_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(wbuf, need // 4), "%s: a kernel wrote past the workspace" % name
    if obuf is not None:
        assert _guards_intact(obuf, n), "%s: a kernel wrote outside out" % name
    return out.view(B, H, W, C).cpu().numpy()


def _inputs_on(dev, name):
    src, tgt = FD.inputs(name)
    return torch.from_numpy(src.copy()).to(dev), torch.from_numpy(tgt.copy()).to(dev)


@pytest.mark.parametrize("name", [c[0] for c in FD.CASES])
def test_case_against_the_reference_with_guards(dev, name):
    _, shape, band, pair, _, _ = FD.BY_NAME[name]
    src, tgt = FD.inputs(name)
    ref, _, route_err, bar = FD.reference(name)
    s, t = _inputs_on(dev, name)
    got = _swap(dev, name, s, t, ws_byte=0xFF)
    zeroed = _swap(dev, name, s, t, ws_byte=0x00)
    scale = float(np.abs(ref).max())
    finite = bool(np.isfinite(got).all())
    err = float(np.abs(got.astype(np.float64) - ref).max()) if finite else float("inf")
    print("%s %s: device error %.3e, route error %.3e, ratio %.2f, bar %.3e (of max|ref| %.4g)"
          % (name, shape, err / scale, route_err, err / scale / route_err if route_err > 0 else float("nan"), bar / scale, scale))
    assert finite, "%s: %d output elements are not finite (never written?)" % (name, int((~np.isfinite(got)).sum()))
    assert np.array_equal(_bits(got), _bits(zeroed)), "%s: the result depends on the workspace's prior contents" % name
    assert err <= bar, name
    for i, b in enumerate(band):
        if b < 0:
            assert np.array_equal(_bits(got[i]), _bits(src[i])), (name, i)
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(src)) and np.array_equal(_bits(t.cpu().numpy()), _bits(tgt)), name


@pytest.mark.parametrize("name", FD.BIT_EQUAL_CASES)
def test_in_place_out_of_place_and_repeat_are_bit_equal(dev, name):
    _, (B, Bt, H, W, C), _, _, _, _ = FD.BY_NAME[name]
    src, tgt = FD.inputs(name)
    s, t = _inputs_on(dev, name)
    a = _swap(dev, name, s, t)
    b = _swap(dev, name, s, t)
    n = B * H * W * C
    ibuf, inner = _guarded(n, dev, 0.0)
    inner.copy_(s.reshape(-1))
    x = inner.view(B, H, W, C)
    c = _swap(dev, name, x, t, out=x)
    assert _guards_intact(ibuf, n), "%s: in place wrote outside src" % name
    assert np.array_equal(_bits(a), _bits(b)), "%s: a repeat differs" % name
    assert np.array_equal(_bits(a), _bits(c)), "%s: in place differs from out of place" % name
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(tgt)), name


def test_wrapper_equals_the_direct_call(dev):
    K = pkg("kernels")
    name = FD.WRAPPER_CASE
    _, _, band, pair, _, _ = FD.BY_NAME[name]
    s, t = _inputs_on(dev, name)
    direct = _swap(dev, name, s, t)
    wrapped = K.fda_amplitude_swap(s, t, band, pair).cpu().numpy()
    assert np.array_equal(_bits(direct), _bits(wrapped))
