"""gpu: pnp_fda_amplitude_swap (csrc/fda.hip) against the float64 reference tests/fda_ref.py at the project's kernel bar
(1e-5 of max|ref|), and its bit-level properties and refusals.  Inputs come from fda_ref.blobs; a target is 1.5 x such an image + 0.4.
Before a comparison the reference's own input condition is asserted: every band coefficient of every stylised, non-zero source channel
has |S(k)| >= 1e-6 max|S| of its image (a phase at rounding level is undefined in fp32).  The condition is necessary, not sufficient:
the error of an fp32 evaluation follows the phase sensitivity |T| / |S| across the band, and an fp32 matmul version of the kernel's
method can miss the fixed 1e-5 on inputs 500x above the condition.  These five shapes pass it; the kernel's whole domain
is held to a per-case bar built on the fp32 route in tests/test_gpu_fda_domain.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from fda_ref import band_ratio, blobs, fda_ref
from kernel_bars import _bar

pytestmark = pytest.mark.gpu

#        (B, Bt, H, W, C), the band sets run one call each (every sample at that band), pair
CASES = [((1, 1, 8, 8, 1), [[0], [1], [3]], [0]),
         ((3, 2, 7, 9, 3), [[-1] * 3, [0] * 3, [2] * 3, [3] * 3, [-1, 2, 3]], [1, 0, 1]),
         ((4, 5, 16, 12, 3), [[5] * 4], [3, 0, 4, 1]),
         ((2, 2, 64, 64, 3), [[5, 5], [31, 31], [5, 31]], [1, 0]),
         ((2, 3, 256, 256, 3), [[2, 2], [23, 23], [127, 127]], [2, 0])]


def _inputs(shape, seed):
    B, Bt, H, W, C = shape
    rng = np.random.default_rng(seed)
    return blobs(rng, B, H, W, C), (1.5 * blobs(rng, Bt, H, W, C) + 0.4).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    """inputs and float64 references, computed once"""
    out = []
    for n, (shape, bands, pair) in enumerate(CASES):
        src, tgt = _inputs(shape, 10 + n)
        for band in bands:
            ratio = band_ratio(src, band)
            print("%s band %s pair %s: smallest band |S| / max|S| %.2e" % (shape, band, pair, ratio))
            assert ratio >= 1e-6, "input condition"
            out.append((shape, band, pair, src, tgt, fda_ref(src, tgt, band, pair)))
    return out


def test_kernel_against_float64_reference(dev, cases):
    K = pkg("kernels")
    for shape, band, pair, src, tgt, ref in cases:
        s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
        got = K.fda_amplitude_swap(s, t, band, pair)
        _bar(got, ref, "fda %s band %s" % (shape, band))
        for i, b in enumerate(band):
            if b < 0:
                assert torch.equal(got[i], s[i]), (shape, band, i)          # band -1: bit for bit
        assert torch.equal(s.cpu(), torch.from_numpy(src))                 # the inputs are never written


@pytest.mark.parametrize("n", [1, 3])
def test_in_place_and_repeat_are_bit_equal(dev, cases, n):
    K = pkg("kernels")
    shape, band, pair, src, tgt, _ = [c for c in cases if c[0] == CASES[n][0]][-1]      # the mixed band set of the case
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    a = K.fda_amplitude_swap(s, t, band, pair)
    b = K.fda_amplitude_swap(s, t, band, pair)
    c = s.clone()
    r = K.fda_amplitude_swap(c, t, band, pair, out=c)
    assert r.data_ptr() == c.data_ptr()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(t.cpu(), torch.from_numpy(tgt))


def test_all_bands_minus_one_copy_bit_for_bit(dev):
    K = pkg("kernels")
    src, tgt = _inputs((3, 2, 7, 9, 3), 20)
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    o = torch.full_like(s, float("nan"))
    assert torch.equal(K.fda_amplitude_swap(s, t, [-1, -1, -1], [0, 1, 0], out=o), s)
    c = s.clone()
    assert torch.equal(K.fda_amplitude_swap(c, t, [-1, -1, -1], [0, 1, 0], out=c), s)


def test_zero_source_and_zero_target_channels(dev):
    """|S| = 0 exactly takes |T| (phase 0); |T| = 0 takes the band out of the source"""
    K = pkg("kernels")
    src, tgt = _inputs((2, 2, 64, 64, 3), 21)
    src[0, :, :, 1] = 0.0
    tgt[1, :, :, 2] = 0.0
    band, pair = [5, 31], [1, 1]
    ratio = band_ratio(src, band)
    print("smallest band |S| / max|S| of the non-zero channels %.2e" % ratio)
    assert ratio >= 1e-6, "input condition"
    ref = fda_ref(src, tgt, band, pair)
    got = K.fda_amplitude_swap(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), band, pair)
    _bar(got, ref, "fda with zero channels")
    _bar(got[0, :, :, 1], ref[0, :, :, 1], "fda zero source channel")
    _bar(got[1, :, :, 2], ref[1, :, :, 2], "fda zero target channel")


def test_refusals_come_before_any_launch(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    B, Bt, H, W, C = 2, 3, 16, 12, 3
    s = torch.zeros((B, H, W, C), device=dev)
    t = torch.zeros((Bt, H, W, C), device=dev)
    o = torch.zeros_like(s)
    big = torch.zeros((8, H, W, C), device=dev)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)

    def call(src=s, b=B, tgt=t, bt=Bt, h=H, w=W, c=C, band=(2, 5), pair=(0, 2), out=o, wsb=None, wsp=True):
        need = lib.pnp_fda_workspace_bytes(B, Bt, H, W, C, 5)
        return lib.pnp_fda_amplitude_swap(None if src is None else vp(src), b, None if tgt is None else vp(tgt), bt, h, w, c,
                                          None if band is None else arr(band), None if pair is None else arr(pair),
                                          None if out is None else vp(out), vp(ws) if wsp else None, need if wsb is None else wsb, None)

    assert call() == 0
    torch.cuda.synchronize()
    bad = {"null src": dict(src=None), "null tgt": dict(tgt=None), "null band": dict(band=None), "null pair": dict(pair=None),
           "null out": dict(out=None), "null workspace": dict(wsp=False),
           "B = 0": dict(b=0), "B = 257": dict(b=257), "Bt = 0": dict(bt=0), "Bt = 257": dict(bt=257),
           "H = 0": dict(h=0), "H = 1025": dict(h=1025), "W = 0": dict(w=0), "W = 1025": dict(w=1025),
           "C = 0": dict(c=0), "C = 5": dict(c=5),
           "band -2": dict(band=(-2, 5)), "band 6": dict(band=(2, 6)), "pair -1": dict(pair=(0, -1)), "pair Bt": dict(pair=(3, 0)),
           "out overlaps tgt": dict(out=t), "out inside tgt": dict(out=big[1:3], tgt=big),
           "out overlaps src in part": dict(out=big[1:3], src=big[0:2]),
           "workspace one byte short": dict(wsb=lib.pnp_fda_workspace_bytes(B, Bt, H, W, C, 5) - 1)}
    for what, kw in bad.items():
        o.fill_(7.0)
        rc = call(**kw)
        msg = lib.pnp_last_error()
        print("%s: %d %s" % (what, rc, msg))
        assert rc == -1 and msg.startswith(b"pnp_fda_amplitude_swap"), what
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                     # nothing ran
    with pytest.raises(L.PnpError):
        K.fda_amplitude_swap(s, t, [2, 6], [0, 2])
    with pytest.raises(L.PnpError):
        K.fda_amplitude_swap(s, t, [2, 5], [0, 3])
    with pytest.raises(L.PnpError):
        K.fda_amplitude_swap(s, t, [2], [0])
    with pytest.raises(L.PnpError):
        K.fda_amplitude_swap(s, t[:, :8], [2, 2], [0, 0])
