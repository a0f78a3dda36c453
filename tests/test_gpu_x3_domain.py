"""-m gpu: the direct split-bf16 kernels (csrc/conv_x3_direct.hip stride-1 and strided, csrc/conv_x3_wgrad.hip) over what their PLANNERS
accept, not only the model's layer shapes: strides 3 and 4, even and non-square filters, 64-tap filters, non-square maps, launches with more
items than workgroups (every kernel is persistent: grid = min(items, 256), loaders run ahead across items, and consecutive items of a
strided data gradient belong to different groups), operands with exact zeros and a 1e-6 .. 1e3 dynamic range, and the epilogues on a
non-square map.  Reference: the float64 convolution (oracle.tf_ops.conv2d + autograd) of the same float32 operands.  Every case asserts
WHICH SYMBOLS RAN from a restatement of the planner's predicate (x3s_expected / x3d_expected below): a case expected on the route that runs
elsewhere fails.  tests/test_x3_strided_host.py holds the same predicate against the workspace queries on a host without a GPU.

Bars: 5e-6 of max|ref| for forward / data gradient (the kernels' bar in test_gpu_x3_direct.py / test_gpu_x3_strided.py: every product exact,
one fp32 chain per output), test_gpu_x3_wgrad._bar for the filter gradient; for wide operands see test_wide_operands_and_exact_zeros."""
import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import tf_ops as T
from test_gpu_x3_wgrad import _bar, _operands

pytestmark = pytest.mark.gpu

BAR = 5e-6
FWD = "conv_x3_direct_kernel_strided<0>"
DGRAD = "conv_x3_direct_kernel_strided<1>"
TILE = 16

# (N, H, W, C, K, R, S, stride, padding) -> (forward on the route, data gradient on the route) in mode 2
STRIDED = [
    ((2, 96, 48, 64, 64, 5, 5, 3, "SAME"), (True, True)),       # stride 3: 9 phases with 2x2 / 2x1 / 1x2 / 1x1 taps, non-square map
    ((2, 96, 48, 64, 128, 7, 7, 3, "SAME"), (True, True)),      # 49 taps, phases with 3 taps per axis, two filter blocks (chain 3136)
    ((2, 96, 48, 64, 64, 3, 3, 3, "SAME"), (True, True)),       # R == s: one tap per phase
    ((2, 128, 64, 64, 64, 5, 5, 4, "SAME"), (True, True)),      # stride 4: 16 phases / 16 data-gradient groups (X3S_MAXPH)
    ((1, 128, 64, 32, 64, 8, 8, 4, "SAME"), (True, False)),     # forward with 64 taps: the last slot of the tap list (32 channels: no dgrad)
    ((1, 128, 64, 64, 32, 8, 8, 4, "SAME"), (False, True)),     # data gradient with 64 taps (32 filters: no forward)
    ((2, 128, 64, 64, 64, 4, 4, 4, "SAME"), (True, True)),      # stride 4, R == s
    ((3, 64, 96, 64, 64, 4, 4, 2, "SAME"), (True, True)),       # even filter (pad 1, 1)
    ((3, 64, 96, 64, 64, 6, 6, 2, "SAME"), (True, True)),       # even filter (pad 2, 2), R == 3 s
    ((3, 64, 96, 32, 64, 3, 5, 2, "SAME"), (True, False)),      # R != S, pad_t != pad_l
    ((3, 64, 96, 64, 64, 5, 3, 2, "SAME"), (True, True)),       # ... and the other way round
    ((3, 32, 96, 64, 64, 3, 3, 2, "SAME"), (True, True)),       # the model's k3s2, wider than high, odd N
    ((3, 96, 32, 128, 128, 5, 5, 2, "SAME"), (True, True)),     # the model's k5s2, higher than wide
    ((2, 64, 64, 64, 64, 3, 3, 2, "VALID"), (False, True)),     # 31 x 31 outputs: forward refused; the gradient's phases are 32 x 32
    ((2, 96, 48, 64, 64, 5, 5, 3, "VALID"), (False, True)),     # 31 x 15 outputs
    ((6, 224, 256, 64, 64, 3, 3, 2, "SAME"), (True, True)),     # 336 forward items; 1344 data-gradient items over 4 groups on 256 workgroups
    ((3, 160, 192, 64, 64, 5, 5, 2, "SAME"), (True, True)),     # 90 / 360 items: uneven shares, workgroups that cross group boundaries
]

# stride-1 3x3 SAME layers (N, H, W, C, K)
STRIDE1 = [
    (5, 128, 144, 64, 128),       # 720 forward items on 256 workgroups (data and filter gradient: other routes)
    (5, 128, 144, 32, 32),        # the 32-filter block, 360 items, forward and data gradient
    (3, 160, 176, 64, 64),        # 330 tiles: forward, data gradient, filter gradient on 256 workgroups, non-square
    (3, 160, 176, 32, 64),        # ... one channel half; two partials per workgroup in the filter gradient
    (1, 16, 144, 32, 64),         # a single tile row
]


def same_pad(n, k, s):
    """TF SAME: (outputs, leading pad)"""
    o = -(-n // s)
    return o, max((o - 1) * s + k - n, 0) // 2


def x3s_expected(case, kind, mode=2):
    """x3s_plan() of csrc/conv_x3_direct.hip restated: -> number of (tile, filter block) items if the strided split-bf16 kernel takes the
    forward (kind 0) / data gradient (kind 1) of an fp32, zero-padded, undilated layer, else 0"""
    N, H, W, C, K, R, S, s, padding = case
    if not (2 <= s <= 4 and s <= R <= 3 * s and s <= S <= 3 * s and R * S <= 64):
        return 0
    (OH, pt), (OW, pl) = (same_pad(H, R, s), same_pad(W, S, s)) if padding == "SAME" else (((H - R) // s + 1, 0), ((W - S) // s + 1, 0))
    cin, kout = (C, K) if kind == 0 else (K, C)           # channels of the convolution the kernel computes
    if cin % 32 or kout % 64:
        return 0
    if (N * OH * OW * K if kind == 0 else N * H * W * C) >= 1 << 30:
        return 0
    if kind == 0:
        grids = [(OH, OW)]
    else:                                                  # one group per output stride phase: the pixels h0, h0 + s, ... of dx
        grids = []
        for a in range(s):
            for b in range(s):
                h0, w0 = (a - pt) % s, (b - pl) % s
                T_, U_ = -(-(R - a) // s), -(-(S - b) // s)
                if T_ - 1 - (h0 + pt - a) // s < 0 or U_ - 1 - (w0 + pl - b) // s < 0:
                    return 0
                grids.append(((H - 1 - h0) // s + 1 if h0 < H else 0, (W - 1 - w0) // s + 1 if w0 < W else 0))
    if any(gh <= 0 or gw <= 0 or gh % TILE or gw % TILE for gh, gw in grids):
        return 0
    items = sum(N * (gh // TILE) * (gw // TILE) * (kout // 64) for gh, gw in grids)
    if mode < 2 and (items < 256 or not (R * S >= 4 * s * s or (kind == 1 and cin <= 64))):
        return 0
    return items


def x3d_expected(case, kind):
    """the stride-1 kernel's predicate (dims_ok, x3w_chosen) for a 3x3 SAME layer in mode 2: -> symbols of the launch, or None"""
    N, H, W, C, K = case
    if H % TILE or W % TILE:
        return None
    if kind == 0:
        return ["x3d_filter_kernel<false>", "conv_x3_direct_kernel<%d, %d, 0>" % (C // 32, 32 if K == 32 else 64)] \
            if C in (32, 64) and K in (32, 64, 128) else None
    if kind == 1:                                          # a convolution of dy: K input channels, C filters
        return ["x3d_filter_kernel<true>", "conv_x3_direct_kernel<%d, %d, 1>" % (K // 32, 32 if C == 32 else 64)] \
            if K in (32, 64) and C in (32, 64, 128) else None
    return ["conv_x3_wgrad_kernel<%d>" % (C // 32), "split_sum::sliced_kernel<4>"] if C in (32, 64) and K == 64 else None


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def route_of(L, names):
    """the kernel family (L.ROUTE_*) the recorded symbols of one launch belong to; None: a family this file does not name"""
    for mark, r in (("conv_x3_direct_kernel_strided<", L.ROUTE_X3S), ("conv_x3_direct_kernel<", L.ROUTE_X3D), ("conv_x3_wgrad_kernel<", L.ROUTE_X3W),
                    ("wino_wgrad_out_kernel<", L.ROUTE_WINO_WGRAD), ("wino_out_kernel<", L.ROUTE_WINO), ("conv_wgrad_ring_kernel<", L.ROUTE_RING),
                    ("conv_wgrad_kernel<", L.ROUTE_RING)):
        if any(n.startswith(mark) for n in names):
            return r
    return None


def _ran(L, fn, cls, g=None):
    """-> (result, symbols that ran); with g: the route the library reports for that pass of g is the family of those symbols"""
    L.prof_summary()
    L.prof_enable(cls)
    out = fn()
    torch.cuda.synchronize()
    L.prof_enable(0)
    names = sorted(r["name"] for r in L.prof_summary())
    if g is not None:
        said = pkg("kernels").conv_route(g, {L.PROF_CONV_FWD: 0, L.PROF_CONV_DGRAD: 1, L.PROF_CONV_WGRAD: 2}[cls])
        fam = route_of(L, names)
        named = (L.ROUTE_X3S, L.ROUTE_X3D, L.ROUTE_X3W, L.ROUTE_WINO_WGRAD, L.ROUTE_WINO, L.ROUTE_RING)
        assert said == fam if fam is not None else said not in named, (said, fam, names)
    return out, names


def _no_x3(names):
    return bool(names) and not any("x3" in n for n in names)


def _bit_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _id(c):
    return "x".join(str(v) for v in (c[0] if isinstance(c[0], tuple) else c))


@pytest.fixture
def route():
    """mode 2 of the family (wherever the shapes allow); the Winograd filter-gradient planner, which is asked before the split-bf16 one,
    off; restores what was in force"""
    K = pkg("kernels")
    prev = (K.x3_direct(-1), K.x3_strided(-1), K.x3_wgrad(-1), K.wino_mode(-1), K.wino_wgrad_mode(0))
    K.x3_direct(2)
    yield K
    K.x3_direct(prev[0]); K.x3_strided(prev[1]); K.x3_wgrad(prev[2]); K.wino_mode(prev[3]); K.wino_wgrad_mode(prev[4])


def _oracle(x, w, dy, stride, padding):
    xg = torch.from_numpy(x).double().requires_grad_(True)
    wg = torch.from_numpy(w).double().requires_grad_(True)
    yo = T.conv2d(xg, wg, stride, 1, padding)
    yo.backward(torch.from_numpy(dy).double())
    return yo.detach(), xg.grad, wg.grad


def _strided_pair(K, L, xd, wd, dyd, g, case, want):
    """forward and data gradient with the strided route off (the fp32-pipe kernels of the same tree) and on; the symbols of both checked"""
    K.x3_strided(0)
    y0, n0 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD, g)
    dx0, n0d = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD, g)
    assert _no_x3(n0) and _no_x3(n0d), n0 + n0d
    K.x3_strided(1)
    y1, n1 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD, g)
    dx1, n1d = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD, g)
    taken = (x3s_expected(case, 0) > 0, x3s_expected(case, 1) > 0)
    assert taken == want, (case, taken, want)
    if taken[0]:
        assert n1 == sorted(["x3s_filter_kernel<false>", FWD]), n1
    else:
        assert _no_x3(n1), n1
    if taken[1]:
        assert n1d == sorted(["x3s_filter_kernel<true>", DGRAD]), n1d
    else:
        assert _no_x3(n1d), n1d
    return (y0, dx0), (y1, dx1), n1 + n1d


@pytest.mark.parametrize("case,want", STRIDED, ids=[_id(c) for c in STRIDED])
def test_strided_domain_fwd_dgrad_vs_float64(dev, route, case, want):
    K, L = route, pkg("_lib")
    N, H, W, C, Kf, R, S, s, padding = case
    rng = np.random.default_rng(sum(case[:8]))
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((R, S, C, Kf)) * np.sqrt(2.0 / (R * S * C))).astype(np.float32)
    g = K.conv_geom(x.shape, w.shape, s, 1, padding)
    dy = rng.standard_normal((N, g.OH, g.OW, Kf)).astype(np.float32)
    res = rng.standard_normal(x.shape).astype(np.float32)
    xd, wd, dyd, resd = (torch.from_numpy(a).to(dev) for a in (x, w, dy, res))
    yo, dxo, _ = _oracle(x, w, dy, s, padding)
    (y0, dx0), (y1, dx1), names = _strided_pair(K, L, xd, wd, dyd, g, case, want)
    dxr = K.conv2d_dgrad(dyd, wd, g, residual=resd)
    errs = {"y": _rel(y1, yo), "dx": _rel(dx1, dxo), "dx+res": _rel(dxr, dxo + torch.from_numpy(res).double()),
            "y fp32 pipe": _rel(y0, yo), "dx fp32 pipe": _rel(dx0, dxo)}
    print("x3 domain strided %s: %s items fwd %d dgrad %d; ran %s" % (case, {k: "%.2e" % v for k, v in errs.items()}, x3s_expected(case, 0),
                                                                     x3s_expected(case, 1), names))
    assert errs["y"] < BAR and errs["dx"] < BAR and errs["dx+res"] < BAR, errs


@pytest.mark.parametrize("case", STRIDE1, ids=_id)
def test_stride1_domain_fwd_dgrad_wgrad_vs_float64(dev, route, case):
    """forward / data gradient at 5e-6; the filter gradient against the fp32-pipe route's own error (test_gpu_x3_wgrad._bar), its
    accumulating entry bit-equal to pre-fill + gradient, two launches bit-equal"""
    K, L = route, pkg("_lib")
    N, H, W, C, Kf = case
    K.wino_mode(2)                   # (as test_gpu_x3_direct.py: the narrow layers are the Winograd route's, which hands them over)
    rng = np.random.default_rng(sum(case))
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rng.standard_normal((3, 3, C, Kf)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    g = K.conv_geom(x.shape, w.shape, 1, 1, "SAME")
    dy = rng.standard_normal((N, H, W, Kf)).astype(np.float32)
    res = rng.standard_normal(x.shape).astype(np.float32)
    pre = (rng.standard_normal(w.shape) * 50.0).astype(np.float32)
    xd, wd, dyd, resd, pred = (torch.from_numpy(a).to(dev) for a in (x, w, dy, res, pre))
    yo, dxo, dwo = _oracle(x, w, dy, 1, "SAME")
    errs, ran = {}, []
    want_f, want_d, want_w = (x3d_expected(case, k) for k in (0, 1, 2))
    assert want_f is not None, "every case of the table is a forward case"
    y1, names = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD, g)
    assert names == sorted(want_f), names
    ran += names
    errs["y"] = _rel(y1, yo)
    dx1, names = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD, g)
    ran += names
    if want_d is not None:
        assert names == sorted(want_d), names
        errs["dx"] = _rel(dx1, dxo)
        errs["dx+res"] = _rel(K.conv2d_dgrad(dyd, wd, g, residual=resd), dxo + torch.from_numpy(res).double())
    else:
        assert names and not any("x3_direct" in n or "x3d" in n for n in names), names
    bar_w = None
    if want_w is not None:
        K.x3_wgrad(0)                                     # the fp32-pipe route of the same tree: the yardstick of the bar
        dw0, names0 = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g), L.PROF_CONV_WGRAD, g)
        assert _no_x3(names0), names0
        K.x3_wgrad(1)
        dw1, names = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g), L.PROF_CONV_WGRAD, g)
        assert names == sorted(want_w), names
        ran += names
        acc, names_a = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g, into=pred.clone()), L.PROF_CONV_WGRAD, g)
        assert names_a == sorted(want_w), names_a
        assert torch.equal(acc, pred + dw1), "accumulate differs from pre-fill + gradient"
        assert torch.equal(dw1, K.conv2d_wgrad(xd, dyd, g)), "two launches differ"
        assert torch.equal(acc, K.conv2d_wgrad(xd, dyd, g, into=pred.clone())), "two accumulating launches differ"
        errs["dw"], errs["dw fp32 route"] = _rel(dw1, dwo), _rel(dw0, dwo)
        bar_w = _bar(errs["dw fp32 route"])
    else:
        _, names = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g), L.PROF_CONV_WGRAD, g)
        assert names and not any("x3w" in n or "x3_wgrad" in n for n in names), names
    print("x3 domain stride-1 %s: %s; ran %s" % (case, {k: "%.2e" % v for k, v in errs.items()}, ran))
    assert all(errs[k] < BAR for k in ("y", "dx", "dx+res") if k in errs), errs
    assert bar_w is None or errs["dw"] <= bar_w, (errs, bar_w)


# (stride-1: (N, H, W, C, K) | strided: a case of the table's form)
WIDE = [
    (2, 32, 48, 64, 64),
    (3, 32, 96, 64, 64, 3, 3, 2, "SAME"),
    (2, 96, 48, 64, 64, 5, 5, 3, "SAME"),
]


@pytest.mark.parametrize("case", WIDE, ids=_id)
def test_wide_operands_and_exact_zeros(dev, route, case):
    """x and dy with magnitudes 1e-6 .. 1e3 and 75 % exact zeros (test_gpu_x3_wgrad._operands "wide"), filters as elsewhere.  The loaders
    split every activation into three bf16 planes (24 significand bits, the third plane rounded), so a product keeps ~2^-24 of its own
    size and the error is that of one fp32 chain — the same class as the fp32 pipe.  No absolute bar has been measured on such data, so
    the yardstick is the fp32-pipe route of the same tree on the same tensors: err_x3 <= 2 x max(err_fp32_route, 1e-6) of max|ref|.
    Exact zeros stay exact: image 1 of x is all zero -> image 1 of y is bit-zero; dy zero on image 0 -> dx of image 0 is bit-zero.

    Measured on MI355X (of max|ref|, split-bf16 / fp32-pipe route):
      stride-1 (2, 32, 48, 64 -> 64):  y 5.13e-07 / 2.77e-07, dx 4.46e-07 / 2.41e-07
      k3s2 (3, 32, 96, 64 -> 64):      y 5.76e-07 / 2.17e-07, dx 4.85e-07 / 2.46e-07
      k5s3 (2, 96, 48, 64 -> 64):      y 5.20e-07 / 2.79e-07, dx 2.50e-07 / 2.91e-07
    (both at the level of one fp32 accumulation chain; the 1e-6 floor of the bar is what decides here)"""
    K, L = route, pkg("_lib")
    strided = len(case) > 5
    if strided:
        N, H, W, C, Kf, R, S, s, padding = case
    else:
        (N, H, W, C, Kf), R, S, s, padding = case, 3, 3, 1, "SAME"
        K.wino_mode(0)               # the yardstick of the stride-1 kernel: the direct fp32-MFMA kernels, not a Winograd transform
    rng = np.random.default_rng(sum(case[:5]) + 1)
    x = _operands(rng, (N, H, W, C), "wide")
    x[1] = 0.0
    w = (rng.standard_normal((R, S, C, Kf)) * np.sqrt(2.0 / (R * S * C))).astype(np.float32)
    g = K.conv_geom(x.shape, w.shape, s, 1, padding)
    dy = _operands(rng, (N, g.OH, g.OW, Kf), "wide")
    dy[0] = 0.0
    xd, wd, dyd = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    yo, dxo, _ = _oracle(x, w, dy, s, padding)
    if strided:
        (y0, dx0), (y1, dx1), names = _strided_pair(K, L, xd, wd, dyd, g, case, (True, True))
    else:
        K.x3_direct(0)
        y0, n0 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD, g)
        dx0, n0d = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD, g)
        assert _no_x3(n0) and _no_x3(n0d), n0 + n0d
        K.x3_direct(2)
        y1, n1 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD, g)
        dx1, n1d = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD, g)
        assert n1 == sorted(x3d_expected(case, 0)) and n1d == sorted(x3d_expected(case, 1)), n1 + n1d
        names = n1 + n1d
    errs = {"y": _rel(y1, yo), "y fp32 route": _rel(y0, yo), "dx": _rel(dx1, dxo), "dx fp32 route": _rel(dx0, dxo)}
    print("x3 domain wide %s: %s; ran %s" % (case, {k: "%.2e" % v for k, v in errs.items()}, names))
    assert float(yo.abs().max()) > 0 and float(dxo.abs().max()) > 0
    assert errs["y"] <= _bar(errs["y fp32 route"]) and errs["dx"] <= _bar(errs["dx fp32 route"]), errs
    assert _bit_zero(y1[1]), "an all-zero input image must give a bit-zero output image"
    assert _bit_zero(dx1[0]), "a zero output gradient must give a bit-zero input gradient"


def test_strided_epilogues_on_a_non_square_map_equal_the_fp32_kernels(dev, route):
    """dropout (identical zero pattern) and BN statistics partials -> mean / variance on maps higher than wide and wider than high: route
    on versus off (the partials are indexed by the tile number: a rows / columns mix-up moves them)"""
    K, L = route, pkg("_lib")
    rng = np.random.default_rng(6)
    for (N, H, W, C, Kf, R) in ((2, 64, 160, 64, 64, 3), (1, 96, 32, 128, 128, 5)):
        x = torch.from_numpy(rng.standard_normal((N, H, W, C)).astype(np.float32)).to(dev)
        w = torch.from_numpy((rng.standard_normal((R, R, C, Kf)) * np.sqrt(2.0 / (R * R * C))).astype(np.float32)).to(dev)
        g = K.conv_geom(tuple(x.shape), tuple(w.shape), 2, 1, "SAME")
        shift = torch.from_numpy((rng.standard_normal(Kf) * 0.1).astype(np.float32)).to(dev)
        out = {}
        for on in (0, 1):
            K.x3_strided(on)
            yd, names = _ran(L, lambda: K.conv2d_fwd(x, w, g, keep_prob=0.75, seed=99, stream_id=3), L.PROF_CONV_FWD)
            assert (FWD in names) == bool(on), names
            nparts = K.conv_stats_parts(g)
            if nparts > 0:
                ys, parts = K.conv2d_fwd_stats(x, w, g, shift, keep_prob=0.75, seed=99, stream_id=3)
                mean, var = K.bn_stats_finish(parts, shift, N * g.OH * g.OW)
            else:                                     # (the fp32 kernels split small layers' reductions: statistics from the output)
                ys = yd
                mean, var = K.bn_stats(yd)
            out[on] = (yd, ys, mean, var, nparts)
        (yd0, ys0, m0, v0, _), (yd1, ys1, m1, v1, np1) = out[0], out[1]
        assert np1 == N * g.OH * g.OW // 64
        assert torch.equal(yd0 == 0, yd1 == 0), "dropout masks differ"
        assert 0.2 < float((yd1 == 0).float().mean()) < 0.3
        assert torch.equal(ys1, yd1)
        yd64 = yd1.double().reshape(-1, Kf)
        errs = {"drop": _rel(yd1, yd0), "mean": _rel(m1, m0), "var": _rel(v1, v0),
                "mean vs f64": float((m1.double() - yd64.mean(0)).abs().max() / yd64.std()), "var vs f64": _rel(v1, yd64.var(0, unbiased=False))}
        print("x3 domain strided epilogues (%d, %d, %d, %d->%d k%d): %s" % (N, H, W, C, Kf, R, {k: "%.2e" % v for k, v in errs.items()}))
        assert max(errs.values()) < 1e-5, errs
