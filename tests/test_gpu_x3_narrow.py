"""-m gpu: the 5x5, 40 -> 5 logits layer's forward and data gradient on the split-bf16 kernels of csrc/conv_x3_narrow.hip (route X3N,
kernels.x3_narrow; mode 2 unless stated), on the smallest shapes that can still go wrong: one forward tile with a data gradient ragged on
both axes, several tiles wider than high and higher than wide (a swapped tiles_x / tiles_y fails the latter), zero-padded borders, and
(ROUNDS) launches with more items than the 512 persistent workgroups whose last round is partial.  Every case checks which kernel symbols
ran, so a silent hand-back cannot pass.  Per element, one product per output: tests/test_gpu_split_bf16_exact.py.

Bar (the rule of tests/test_gpu_x3_wgrad.py): err_new <= 2 x max(err of the fp32 route of the same tree on the same tensors, 1e-6) of
max|ref|, ref = the float64 convolution of the same float32 operands — the factor 2 covers a different but equally long fp32 chain.

Measured on MI355X (split-bf16 / fp32 route, of max|ref|): see DESIGN §25."""
import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import tf_ops as T
from test_gpu_x3_domain import _bit_zero, _oracle, _ran, _rel
from test_gpu_x3_wgrad import _bar, _operands

pytestmark = pytest.mark.gpu

FWD = ["conv_x3_direct_kernel_narrow<0>", "x3n_filter_kernel<false>"]
DGRAD = ["conv_x3_direct_kernel_narrow<1>", "x3n_filter_kernel<true>"]

# (N, H, W, padding)
SHAPES = [
    (1, 20, 20, "VALID"),        # two forward tiles in one column; the data gradient's 2 x 2 tiles ragged on both axes
    (2, 36, 52, "VALID"),        # several tiles, wider than high, two images
    (1, 52, 36, "VALID"),        # higher than wide
    (2, 32, 48, "SAME"),         # zero-padded borders
]


def _no_x3(names):
    return bool(names) and not any("x3" in n for n in names)


@pytest.fixture
def route():
    K = pkg("kernels")
    prev = (K.x3_direct(-1), K.x3_narrow(-1))
    K.x3_direct(1); K.x3_narrow(2)
    yield K
    K.x3_direct(prev[0]); K.x3_narrow(prev[1])


def _case(dev, K, shape, kind="normal", seed=0):
    N, H, W, padding = shape
    rng = np.random.default_rng(N + H + W + seed)
    x = _operands(rng, (N, H, W, 40), kind)
    w = (rng.standard_normal((5, 5, 40, 5)) * np.sqrt(2.0 / 1000)).astype(np.float32)
    g = K.conv_geom(x.shape, w.shape, 1, 1, padding)
    dy = _operands(rng, (N, g.OH, g.OW, 5), kind)
    res = rng.standard_normal(x.shape).astype(np.float32)
    return g, (x, w, dy, res)


def _both_routes(dev, K, L, g, host, fwd_cls=None):
    """forward, data gradient and data gradient + residual with the route off (the fp32 kernels of the same tree) and on.  fwd_cls: the
    profiler classes of the forward (from 8192 output pixels on, the fp32 forward is conv_fwd_narrow_kernel, of the class PROF_CONV_DIRECT)"""
    xd, wd, dyd, resd = (torch.from_numpy(a).to(dev) for a in host)
    out = {}
    for mode in (0, 2):
        K.x3_narrow(mode)
        y, nf = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD if fwd_cls is None else fwd_cls)
        dx, nd = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD)
        dxr, ndr = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g, residual=resd), L.PROF_CONV_DGRAD)
        if mode == 0:
            assert _no_x3(nf) and _no_x3(nd) and _no_x3(ndr), nf + nd + ndr
        else:
            assert K.conv_route(g, 0) == L.ROUTE_X3N and K.conv_route(g, 1) == L.ROUTE_X3N
            assert nf == FWD and nd == DGRAD and ndr == DGRAD, nf + nd + ndr          # (the residual is in the epilogue: no extra launch)
        out[mode] = (y, dx, dxr)
    return out[0], out[2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_fwd_dgrad_vs_float64(dev, route, shape):
    K, L = route, pkg("_lib")
    g, host = _case(dev, K, shape)
    x, w, dy, res = host
    yo, dxo, _ = _oracle(x, w, dy, 1, shape[3])
    old, new = _both_routes(dev, K, L, g, host)
    refs = (yo, dxo, dxo + torch.from_numpy(res).double())
    for name, a_old, a_new, ref in zip(("y", "dx", "dx+res"), old, new, refs):
        e_new, e_old = _rel(a_new, ref), _rel(a_old, ref)
        print("x3 narrow %s %s: split-bf16 %.2e, fp32 route %.2e of max|ref|" % (shape, name, e_new, e_old))
        assert e_new <= _bar(e_old), (name, e_new, e_old)


def test_hard_operands_and_exact_zeros(dev, route):
    """x and dy with magnitudes 1e-6 .. 1e3 and 75 % exact zeros under the same bar; an all-zero image comes out bit-zero both ways"""
    K, L = route, pkg("_lib")
    shape = (2, 36, 52, "VALID")
    g, host = _case(dev, K, shape, "wide", seed=1)
    x, w, dy, res = host
    x[1] = 0.0
    dy[0] = 0.0
    yo, dxo, _ = _oracle(x, w, dy, 1, "VALID")
    assert float(yo.abs().max()) > 0 and float(dxo.abs().max()) > 0
    old, new = _both_routes(dev, K, L, g, host)
    for name, a_old, a_new, ref in zip(("y", "dx"), old, new, (yo, dxo)):
        e_new, e_old = _rel(a_new, ref), _rel(a_old, ref)
        print("x3 narrow wide %s %s: split-bf16 %.2e, fp32 route %.2e of max|ref|" % (shape, name, e_new, e_old))
        assert e_new <= _bar(e_old), (name, e_new, e_old)
    assert _bit_zero(new[0][1]), "an all-zero input image must give a bit-zero output image"
    assert _bit_zero(new[1][0]), "a zero output gradient must give a bit-zero input gradient"


def test_dropout_masks_equal_the_vector_alu_kernel(dev, route):
    """keep 0.75: the zero pattern is that of conv_fwd_narrow_kernel for the same seed and stream id (same counter hash on the flat output
    index); kept values within the bar.  (2, 68, 68): the smallest of the suite's logits shapes that the vector-ALU kernel takes."""
    K, L = route, pkg("_lib")
    shape = (2, 68, 68, "VALID")
    g, host = _case(dev, K, shape)
    x, w, dy, _ = host
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    yo = T.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), 1, 1, "VALID") / 0.75
    for seed, sid in ((5, 3), (1 << 40, 0)):
        K.x3_narrow(0)
        y0, n0 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g, keep_prob=0.75, seed=seed, stream_id=sid), L.PROF_CONV_FWD | L.PROF_CONV_DIRECT)
        assert n0 == ["conv_fwd_narrow_kernel<5, true>"], n0
        K.x3_narrow(2)
        y1, n1 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g, keep_prob=0.75, seed=seed, stream_id=sid), L.PROF_CONV_FWD)
        assert n1 == FWD, n1
        assert torch.equal(y0 == 0, y1 == 0), "dropout masks differ"
        frac = float((y1 == 0).double().mean())
        assert 0.2 < frac < 0.3, frac
        kept = (y1 != 0).cpu()
        ref = torch.where(kept, yo, torch.zeros_like(yo))
        e_new, e_old = _rel(y1, ref), _rel(y0, ref)
        print("x3 narrow dropout seed %d sid %d: split-bf16 %.2e, fp32 route %.2e of max|ref|, dropped %.3f" % (seed, sid, e_new, e_old, frac))
        assert e_new <= _bar(e_old), (e_new, e_old)


# Past the first round of the persistent grid: conv_x3_direct_kernel_narrow launches min(items, 512) workgroups, and SHAPES above stop at 64
# forward / 50 data-gradient items.  Here every launch walks the `id += gridDim.x` loop, prefetches the next tile under the MFMAs, stores a
# prefetched patch and ends on a PARTIAL last round (the `id + gridDim.x < nitems` guard).  shape -> (forward items, data-gradient items)
ROUNDS = [
    ((65, 20, 100, "VALID"), (780, 910)),
    ((48, 32, 96, "SAME"), (1152, 576)),
]
GRID = 512


def _items(g):
    """x3n_items() of csrc/conv_x3_narrow.hip: 8 x 16 forward tiles of y, 16 x 16 data-gradient tiles of dx (ragged ones included)"""
    return g.N * (g.OH // 8) * (g.OW // 16), g.N * -(-g.H // 16) * -(-g.W // 16)


@pytest.mark.parametrize("shape,items", ROUNDS, ids=lambda v: "x".join(str(i) for i in v))
def test_more_items_than_workgroups_vs_float64(dev, route, shape, items):
    """the bar of test_fwd_dgrad_vs_float64 on launches of two and three rounds, and two launches bit-identical"""
    K, L = route, pkg("_lib")
    g, host = _case(dev, K, shape)
    assert _items(g) == items and all(n > GRID and n % GRID for n in items), (_items(g), items)
    x, w, dy, res = host
    yo, dxo, _ = _oracle(x, w, dy, 1, shape[3])
    old, new = _both_routes(dev, K, L, g, host, fwd_cls=L.PROF_CONV_FWD | L.PROF_CONV_DIRECT)
    refs = (yo, dxo, dxo + torch.from_numpy(res).double())
    for name, a_old, a_new, ref in zip(("y", "dx", "dx+res"), old, new, refs):
        e_new, e_old = _rel(a_new, ref), _rel(a_old, ref)
        print("x3 narrow rounds %s %s: split-bf16 %.2e, fp32 route %.2e of max|ref|" % (shape, name, e_new, e_old))
        assert e_new <= _bar(e_old), (name, e_new, e_old)
    xd, wd, dyd, resd = (torch.from_numpy(a).to(dev) for a in host)
    again = (K.conv2d_fwd(xd, wd, g), K.conv2d_dgrad(dyd, wd, g), K.conv2d_dgrad(dyd, wd, g, residual=resd))
    assert all(torch.equal(a, b) for a, b in zip(new, again)), "two launches differ"


@pytest.mark.parametrize("shape,items", ROUNDS, ids=lambda v: "x".join(str(i) for i in v))
def test_more_items_than_workgroups_dropout(dev, route, shape, items):
    """keep 0.75 past the first round: the zero pattern of the mode-0 route of the same tree (conv_fwd_narrow_kernel<5, true>, which
    takes both shapes: >= 8192 output pixels) for the same seed and stream id; kept values within the bar"""
    K, L = route, pkg("_lib")
    g, host = _case(dev, K, shape)
    assert _items(g)[0] == items[0]
    x, w, _, _ = host
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    yo = T.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), 1, 1, shape[3]) / 0.75
    for seed, sid in ((5, 3), (1 << 40, 0)):
        K.x3_narrow(0)
        y0, n0 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g, keep_prob=0.75, seed=seed, stream_id=sid), L.PROF_CONV_FWD | L.PROF_CONV_DIRECT)
        assert n0 == ["conv_fwd_narrow_kernel<5, true>"], n0
        K.x3_narrow(2)
        y1, n1 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g, keep_prob=0.75, seed=seed, stream_id=sid), L.PROF_CONV_FWD)
        assert n1 == FWD, n1
        assert torch.equal(y0 == 0, y1 == 0), "dropout masks differ"
        frac = float((y1 == 0).double().mean())
        assert 0.2 < frac < 0.3, frac
        kept = (y1 != 0).cpu()
        ref = torch.where(kept, yo, torch.zeros_like(yo))
        e_new, e_old = _rel(y1, ref), _rel(y0, ref)
        print("x3 narrow rounds dropout %s seed %d sid %d: split-bf16 %.2e, fp32 route %.2e of max|ref|, dropped %.3f" % (
            shape, seed, sid, e_new, e_old, frac))
        assert e_new <= _bar(e_old), (e_new, e_old)


def test_determinism_modes_and_the_epilogues_that_stay(dev, route):
    """two launches bit-identical; mode 0 and mode 1 (64 tiles: below the 256 of the rule) run the old symbols; x3_direct(0) turns the route
    off; the frozen-BN forward keeps its kernel in mode 2"""
    K, L = route, pkg("_lib")
    g, host = _case(dev, K, (2, 36, 52, "VALID"))
    xd, wd, dyd, resd = (torch.from_numpy(a).to(dev) for a in host)
    y, dx = K.conv2d_fwd(xd, wd, g), K.conv2d_dgrad(dyd, wd, g, residual=resd)
    assert torch.equal(y, K.conv2d_fwd(xd, wd, g)) and torch.equal(dx, K.conv2d_dgrad(dyd, wd, g, residual=resd)), "two launches differ"
    for setup in (lambda: K.x3_narrow(0), lambda: K.x3_narrow(1), lambda: (K.x3_narrow(2), K.x3_direct(0))):
        setup()
        _, nf = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD)
        _, nd = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD)
        assert _no_x3(nf) and _no_x3(nd), nf + nd
        K.x3_direct(1)
    K.x3_narrow(2)
    ss = (torch.ones(5, device=dev), torch.zeros(5, device=dev))
    yb, nb = _ran(L, lambda: K.conv2d_fwd_bn(xd, wd, g, ss, alpha=-1.0), L.PROF_CONV_FWD)
    assert _no_x3(nb), nb
    assert _rel(yb, y) < 5e-6


def test_adjoint_identity(dev, route):
    """<conv(x, w), dy> = <x, dgrad(dy, w)> within 2e-6 of |y||dy| with both directions on the route (test_conv_full_size_adjoint_identities)"""
    K, L = route, pkg("_lib")
    g, host = _case(dev, K, (2, 36, 52, "VALID"), seed=2)
    xd, wd, dyd, _ = (torch.from_numpy(a).to(dev) for a in host)
    y, nf = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD)
    dx, nd = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD)
    assert nf == FWD and nd == DGRAD, nf + nd
    a, b = float((y.double() * dyd.double()).sum()), float((xd.double() * dx.double()).sum())
    scale = float(y.double().norm() * dyd.double().norm())
    print("x3 narrow adjoint: <y,dy> %.9e <x,dx> %.9e, difference %.2e of |y||dy|" % (a, b, abs(a - b) / scale))
    assert abs(a - b) < 2e-6 * scale, (a, b, scale)
