"""-m gpu: the Winograd route (csrc/conv_wino.hip, csrc/conv_wino_x3.hip) over what its planner accepts, not only what the model feeds it.

tests/test_gpu_wino.py holds the route to float64 at nine shapes whose filter counts are all multiples of 32, whose smallest launch has 16
tiles, whose dilated layers all pad SAME and whose operands are all N(0, 1).  eligible_dims admits far more — any stride-1 3x3 layer with
C % 32 == 0, K % 4 == 0, K >= 32, dil 1 / 2, padding 0 / dil / 2 dil — and in mode 2 at any tile count.  This file walks that domain at the
smallest shapes that reach each place (tables in tests/test_wino_domain_host.py), every test once per arithmetic: F(2x2) and F(4x4), on the
fp32 matrix pipe and on split-bf16 operands.  Route mode 2 and filter-gradient mode 2 throughout.

Every launch asserts (a) kernels.wino_chosen against the Python restatement of the planner (test_wino_domain_host.expected_tile, itself held
to the library on the CPU) and (b) which kernel symbols ran: the route's, of the predicted tile and arithmetic — or, where the planner
refuses a pass (the data gradient over K = 36 / 100 / 132 filters: its reduction length is not a multiple of 32), no `wino` symbol at all;
the result is held to float64 either way.

Oracles: the float64 convolution (oracle.tf_ops.conv2d + autograd) of the same float32 operands at the route's bar (2e-5 of max|ref|,
test_gpu_wino.BAR); for wide-range operands the project's own float32 restatement of the same algorithm with the same tile and arithmetic
(oracle.tf_ops.conv3x3_winograd_np / wgrad3x3_winograd_np: equal to the convolution to 1e-10 in float64, tests/test_wino_domain_host.py).

Measured on an MI355X (68 tests, all four arithmetics): the tests themselves take 4 s (the slowest 1.1 s — the first launch of the process —
every other under 0.15 s, float64 references included); the file alone, with the 30 s the session's build fixture spends, 34 s.  Largest
error per arithmetic over the shape table, of max|ref| (bar 2e-5): F2x2 1.5e-6, F4x4 2.9e-6, F2x2-x3 1.1e-6, F4x4-x3 2.9e-6."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import tf_ops as T
from test_gpu_wino import BAR, _ran, _rel, _route_names, _where
from test_gpu_x3_wgrad import _bar, _operands
from test_wino_domain_host import ARITH, ARITH_IDS, SHAPES, SPLITS, WIDE, _pad, case_id, expected_tile, float64_reference, tiles, wgrad_splits, x3_gemm

pytestmark = pytest.mark.gpu


@pytest.fixture(params=ARITH, ids=ARITH_IDS)
def wino(request):
    """the switches of test_gpu_wino.py's `wino` fixture with both route modes at 2: yields the kernels module with .tile / .x3 of this run;
    restores what was in force"""
    K = pkg("kernels")
    tile, x3 = request.param
    prev = (K.wino_mode(2), K.wino_wgrad_mode(2), K.wino_tile(tile), K.wino_x3(2 if x3 else 0))

    class Route(object):
        pass
    r = Route()
    r.K, r.tile, r.x3 = K, tile, x3
    yield r
    K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.wino_tile(prev[2]); K.wino_x3(prev[3])


PROF = {0: "PROF_CONV_FWD", 1: "PROF_CONV_DGRAD", 2: "PROF_CONV_WGRAD"}


def expected_names(case, kind, tile, x3):
    """kernel symbols of one launch of pass `kind` on the route (wino_splitsum_kernel apart); [] where the planner refuses the pass"""
    N, H, W, C, Kf, dil, padding = case
    m = expected_tile(case, kind, tile, x3)
    if m == 0:
        return []
    bf = x3_gemm(case, kind, m, x3)
    if kind == 2:
        if bf:        # split-bf16 GEMMs (sym 4 / 5) on operands the transforms transpose (the reduction runs over the tiles)
            return sorted(["wino_dy_t_kernel<%d>" % m, "wino_in_t_kernel<%d>" % m, "wino_wgrad_out_kernel<%d>" % m,
                           "wino_gemm_x3_kernel<128, %d, %d>" % (64 if Kf <= 64 else 128, 4 if m == 2 else 5)])
        return sorted(n % m for n in ("wino_dy_kernel<%d>", "wino_in_kernel<%d, false>", "wino_wgrad_gemm_kernel<128, 128, 2, 2, %d>", "wino_wgrad_out_kernel<%d>"))
    cols = Kf if kind == 0 else C            # the GEMM's columns: the forward's filters, the data gradient's channels
    return _route_names(m, bf, kind == 1, 64 if cols <= 64 else 128, (0 if m == 2 else 2) + kind)


def launch(wino, g, case, kind, fn):
    """one launch of pass `kind`: the planner's choice as predicted, the symbols of that choice and no others"""
    K, L = wino.K, pkg("_lib")
    m = expected_tile(case, kind, wino.tile, wino.x3)
    assert K.wino_chosen(g, kind) == m, (case, kind, K.wino_chosen(g, kind), m)
    out, names = _ran(L, fn, getattr(L, PROF[kind]) | L.PROF_CONV_DIRECT)
    want = expected_names(case, kind, wino.tile, wino.x3)
    if m == 0:
        assert names and not any("wino" in n for n in names), (case, kind, names)
    else:
        assert sorted(n for n in names if n != "wino_splitsum_kernel") == want, (case, kind, names, want)
    return out, names


def operands(case, seed=0, kinds=("normal", "normal")):
    """x, He-scaled w, dy, a residual and a held filter gradient (float32 numpy), and the geometry"""
    K = pkg("kernels")
    N, H, W, C, Kf, dil, padding = case
    rng = np.random.default_rng(sum(case[:6]) + seed)
    g = K.conv_geom((N, H, W, C), (3, 3, C, Kf), 1, dil, padding)
    x = _operands(rng, (N, H, W, C), kinds[0])
    w = (rng.standard_normal((3, 3, C, Kf)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    dy = _operands(rng, (N, g.OH, g.OW, Kf), kinds[1])
    res = rng.standard_normal(x.shape).astype(np.float32)
    held = rng.standard_normal(w.shape).astype(np.float32)
    return g, x, w, dy, res, held


def tag(wino):
    return "F(%dx%d)%s" % (wino.tile, wino.tile, " x3" if wino.x3 else "")


@pytest.mark.parametrize("case", SHAPES, ids=case_id)
def test_shape_table_vs_float64(dev, wino, case):
    """forward, data gradient (plain and with residual=), filter gradient (plain and into= a buffer that holds a contribution) of every row of
    the shape table: N(0, 1) operands, He-scaled filters, against the float64 convolution and its autograd gradients at the route's bar.
    Largest of the five errors on an MI355X, of max|ref| (the run prints all five per case):
                                         F2x2     F4x4     F2x2-x3  F4x4-x3
      (1, 3, 3, 32, 32, 1, 'VALID')      2.3e-07  9.2e-07  2.3e-07  9.2e-07
      (1, 2, 2, 64, 64, 1, 'SAME')       3.6e-07  1.3e-06  3.1e-07  1.3e-06
      (3, 5, 7, 32, 36, 1, 'SAME')       6.4e-07  1.2e-06  6.4e-07  1.2e-06
      (2, 6, 10, 64, 100, 1, 'SAME')     3.2e-07  2.0e-06  3.2e-07  2.2e-06
      (1, 7, 9, 96, 132, 1, 'VALID')     4.3e-07  2.9e-06  4.3e-07  2.9e-06
      (1, 8, 12, 64, 64, 2, 'VALID')     2.7e-07  1.9e-06  2.3e-07  1.4e-06
      (2, 4, 4, 64, 32, 2, 'SAME')       4.5e-07  1.6e-06  4.5e-07  1.6e-06
      (1, 2, 130, 32, 32, 1, 'SAME')     3.6e-07  1.3e-06  2.9e-07  1.3e-06
      (130, 2, 2, 32, 32, 1, 'SAME')     4.0e-07  1.9e-06  3.1e-07  1.4e-06
      (1, 4, 4, 1056, 32, 1, 'SAME')     1.1e-06  1.6e-06  1.1e-06  1.6e-06
      (1, 4, 4, 1088, 32, 1, 'SAME')     1.5e-06  1.5e-06  2.6e-07  1.9e-06"""
    K = wino.K
    g, x, w, dy, res, held = operands(case)
    xd, wd, dyd, resd, heldd = (torch.from_numpy(a).to(dev) for a in (x, w, dy, res, held))
    yo, dxo, dwo = float64_reference(x, w, dy, case[5], case[6])
    y, _ = launch(wino, g, case, 0, lambda: K.conv2d_fwd(xd, wd, g))
    dx, _ = launch(wino, g, case, 1, lambda: K.conv2d_dgrad(dyd, wd, g))
    dxr, _ = launch(wino, g, case, 1, lambda: K.conv2d_dgrad(dyd, wd, g, residual=resd))
    dw, _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g))
    dwa, _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g, into=heldd.clone()))
    errs = {"y": _rel(y, yo), "dx": _rel(dx, dxo), "dx+res": _rel(dxr, dxo + res.astype(np.float64)), "dw": _rel(dw, dwo),
            "dw+held": _rel(dwa, dwo + held.astype(np.float64))}
    print("wino domain %s %s tiles (y, dx, dw) %s: %s" % (tag(wino), case, [expected_tile(case, k, wino.tile, wino.x3) for k in (0, 1, 2)],
                                                          {k: "%.2e" % v for k, v in errs.items()}))
    if errs["y"] > BAR:
        print("  forward mismatch:", _where(y.cpu().double() - torch.from_numpy(yo), case[4]))
    if errs["dx"] > BAR:
        print("  data-gradient mismatch:", _where(dx.cpu().double() - torch.from_numpy(dxo), case[3]))
    if errs["dw"] > BAR:
        e = (dw.cpu().double() - torch.from_numpy(dwo)).abs()
        print("  filter-gradient mismatch: per tap", [["%.1e" % float(e[r, s].max()) for s in range(3)] for r in range(3)],
              "per 32 channels", ["%.1e" % float(e[:, :, i:i + 32].max()) for i in range(0, min(case[3], 256), 32)],
              "per 32 filters", ["%.1e" % float(e[..., i:i + 32].max()) for i in range(0, min(case[4], 256), 32)])
    assert max(errs.values()) < BAR, errs


@pytest.mark.parametrize("case", SPLITS, ids=case_id)
def test_filter_gradient_reduction_splits(dev, wino, case):
    """the filter gradient of two narrow layers with many tiles: the planners (wgrad_split: up to 16 ways, wgrad_split_x3: up to 32) cut the
    reduction over the tiles, the second shape with a ragged last chunk (T = 3 069 / 816) and K = 36.  The split count is read off the
    workspace query (test_wino_domain_host.wgrad_splits), not assumed; wino_splitsum_kernel runs exactly where the code launches it (more
    than two splits over fewer than 131 072 (channel, filter quad) vectors).
    Split counts (splits x chunks per split), the same on the CPU host and the GPU box: (4, 64, 64, 32, 32) F2x2 16 x 8, F4x4 4 x 8,
    F2x2-x3 16 x 4, F4x4-x3 6 x 3; (3, 62, 66, 32, 36) F2x2 12 x 8 (96 chunks), F4x4 3 x 9 (26), F2x2-x3 16 x 3 (48), F4x4-x3 7 x 2 (13)."""
    K, lib = wino.K, pkg("_lib").load()
    N, H, W, C, Kf, dil, padding = case
    g, x, w, dy, res, held = operands(case)
    xd, dyd, heldd = (torch.from_numpy(a).to(dev) for a in (x, dy, held))
    _, _, dwo = float64_reference(x, w, dy, dil, padding)
    assert x3_gemm(case, 2, wino.tile, wino.x3) == bool(wino.x3)
    ns, cps, chunks = wgrad_splits(int(lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g))), case, wino.tile, wino.x3)
    Tn = tiles(case, 2, wino.tile)
    assert ns > 1, ns
    if case is SPLITS[1]:
        assert Tn % (64 if wino.x3 else 32) != 0 or ns * cps != chunks, (Tn, ns, cps, chunks)
    dw, names = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g))
    assert ("wino_splitsum_kernel" in names) == (ns > 2 and C * (Kf // 4) < 256 * 512), (ns, names)
    dw2, _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g))
    dwa, names_a = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g, into=heldd.clone()))
    assert ("wino_splitsum_kernel" in names_a) == ("wino_splitsum_kernel" in names)
    err, err_acc = _rel(dw, dwo), _rel(dwa, held.astype(np.float64) + dw.cpu().double().numpy())
    print("wino domain %s %s filter gradient: T = %d, %d splits of %d chunks (%d), splitsum %s: dw %.2e of max|ref|, into= vs held + dw %.2e"
          % (tag(wino), case, Tn, ns, cps, chunks, "wino_splitsum_kernel" in names, err, err_acc))
    assert err < BAR, err
    assert torch.equal(dw, dw2), "two launches differ"
    assert err_acc < 2e-6, err_acc                      # (tests/test_gpu_conv.py's figure for the accumulating entry point)


@pytest.mark.parametrize("case", WIDE, ids=case_id)
def test_wide_operands_and_exact_zeros(dev, wino, case):
    """x and dy with magnitudes 1e-6 .. 1e3 and 75 % exact zeros (test_gpu_x3_wgrad._operands "wide"), one all-zero image each where N > 1.
    Yardstick: the float32 restatement of the same algorithm (same m, same arithmetic) on the same tensors, both measured against float64:
    err_kernel <= 2 x max(err_restatement, 1e-6) (test_gpu_x3_wgrad._bar: the accumulation order differs, the class of error does not), and
    below the route's bar in any case.  A zero image gives exactly zero, forward and backward.
    The restatement alone, on a CPU host: F(2x2) 0.6e-7 .. 4.1e-7, F(4x4) 2.2e-7 .. 2.1e-6 over both shapes and the three passes.
    Kernel / restatement on an MI355X, (2, 12, 20, 64, 64) SAME then (1, 8, 12, 64, 64) dil 2 VALID:
      F2x2     y 3.1e-7 / 3.5e-7, dx 3.9e-7 / 3.9e-7, dw 1.3e-7 / 1.3e-7;   y 2.4e-7 / 3.0e-7, dx 3.0e-7 / 3.0e-7, dw 8.2e-8 / 6.0e-8
      F4x4     y 2.3e-6 / 2.3e-6, dx 1.9e-6 / 1.9e-6, dw 3.8e-7 / 6.7e-7;   y 1.5e-6 / 1.3e-6, dx 1.6e-6 / 1.8e-6, dw 5.4e-7 / 2.1e-7
      F2x2-x3  y 3.2e-7 / 2.4e-7, dx 4.1e-7 / 2.2e-7, dw 1.3e-7 / 1.3e-7;   y 2.4e-7 / 1.8e-7, dx 3.7e-7 / 2.5e-7, dw 1.5e-7 / 6.0e-8
      F4x4-x3  y 1.9e-6 / 1.5e-6, dx 1.8e-6 / 1.2e-6, dw 5.8e-7 / 4.3e-7;   y 1.3e-6 / 1.5e-6, dx 1.6e-6 / 1.1e-6, dw 8.5e-7 / 2.5e-7
    (first shape: dw of the operands before the zeroing — with both zero images in place every product of the filter gradient has a zero
    factor and dw is exactly zero, which is asserted too)."""
    K = wino.K
    N, H, W, C, Kf, dil, padding = case
    pad = _pad(case)
    g, x, w, dy, res, held = operands(case, seed=1, kinds=("wide", "wide"))
    x_all, dy_all = x.copy(), dy.copy()
    if N > 1:
        x[1] = 0.0
        dy[0] = 0.0
    xd, wd, dyd = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    yo, dxo, dwo = float64_reference(x, w, dy, dil, padding)
    y, _ = launch(wino, g, case, 0, lambda: K.conv2d_fwd(xd, wd, g))
    dx, _ = launch(wino, g, case, 1, lambda: K.conv2d_dgrad(dyd, wd, g))
    dw, _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g))
    m = [expected_tile(case, kind, wino.tile, wino.x3) for kind in (0, 1, 2)]
    bf = [x3_gemm(case, kind, m[kind], wino.x3) for kind in (0, 1, 2)]
    assert m == [wino.tile] * 3 and bf == [bool(wino.x3)] * 3
    rest = {"y": T.conv3x3_winograd_np(x, w, dil, dtype=np.float32, pad=pad, m=m[0], x3=bf[0]),
            "dx": T.conv3x3_winograd_np(dy, w, dil, flip_transpose=True, dtype=np.float32, pad=2 * dil - pad, m=m[1], x3=bf[1]),
            "dw": T.wgrad3x3_winograd_np(x, dy, dil, dtype=np.float32, pad=pad, m=m[2], x3=bf[2])}
    ref = {"y": yo, "dx": dxo, "dw": dwo}
    got = {"y": y, "dx": dx, "dw": dw}
    if N == 2:
        # (with image 1 of x and image 0 of dy zeroed every product of the filter gradient has a zero factor: it is exactly zero, and says
        # nothing about accuracy — the filter gradient of the operands BEFORE the zeroing is held to the yardstick as well)
        assert bool((dw == 0).all()) and not rest["dw"].any() and not dwo.any()
        xa, dya = torch.from_numpy(x_all).to(dev), torch.from_numpy(dy_all).to(dev)
        got["dw, no zero image"], _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xa, dya, g))
        rest["dw, no zero image"] = T.wgrad3x3_winograd_np(x_all, dy_all, dil, dtype=np.float32, pad=pad, m=m[2], x3=bf[2])
        ref["dw, no zero image"] = float64_reference(x_all, w, dy_all, dil, padding)[2]
    errs = {k: (_rel(got[k], ref[k]), _rel(rest[k], ref[k])) for k in got}
    print("wino domain %s %s wide operands, kernel / restatement of max|ref|: %s" % (tag(wino), case, {k: "%.2e / %.2e" % v for k, v in errs.items()}))
    for k, (ek, er) in errs.items():
        assert ek <= _bar(er) and ek < BAR, (k, ek, er)
    if N > 1:
        assert bool((y[1] == 0).all()) and bool((dx[0] == 0).all()), "a zero image does not give exact zeros"
        assert bool((y[0] != 0).any()) and bool((dx[1] != 0).any())


def test_power_of_two_scaling_is_exact(dev, wino):
    """conv(2^k x, w) == 2^k conv(x, w) bit for bit, k = -40 and +40, and the same for the data gradient (dy scaled) and the filter gradient
    (x scaled): without overflow or underflow every rounding of the transforms, of the three-way bf16 split and of the accumulation is
    scale-invariant — a flushed or clamped plane, or any absolute threshold, breaks the equality.  K = 100: the data gradient runs on the
    direct kernels (held to the same property); the (dil 2, VALID) shape adds a data gradient on the route."""
    K = wino.K
    for case in (SHAPES[3], SHAPES[5]):
        g, x, w, dy, res, held = operands(case, seed=2)
        xd, wd, dyd = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
        y, _ = launch(wino, g, case, 0, lambda: K.conv2d_fwd(xd, wd, g))
        dx, _ = launch(wino, g, case, 1, lambda: K.conv2d_dgrad(dyd, wd, g))
        dw, _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xd, dyd, g))
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
        for k in (-40, 40):
            s = 2.0 ** k
            xs, dys = xd * s, dyd * s
            assert torch.equal(xs / s, xd) and torch.equal(dys / s, dyd)            # (the scaling itself is exact)
            ys, _ = launch(wino, g, case, 0, lambda: K.conv2d_fwd(xs, wd, g))
            dxs, _ = launch(wino, g, case, 1, lambda: K.conv2d_dgrad(dys, wd, g))
            dws, _ = launch(wino, g, case, 2, lambda: K.conv2d_wgrad(xs, dyd, g))
            for name, a, b in (("y", ys, y), ("dx", dxs, dx), ("dw", dws, dw)):
                same = torch.equal(a, b * s)
                if not same:
                    print("wino domain %s %s 2^%d scaling, %s: %d of %d values differ, max relative %.2e" % (
                        tag(wino), case, k, name, int((a != b * s).sum()), a.numel(), _rel(a / s, b)))
                assert same, (case, k, name)


def test_two_launches_are_bit_identical(dev, wino):
    """forward, data gradient and filter gradient of the K = 132 row twice: the same bits"""
    K = wino.K
    case = SHAPES[4]
    g, x, w, dy, res, held = operands(case, seed=3)
    xd, wd, dyd = (torch.from_numpy(a).to(dev) for a in (x, w, dy))
    for kind, fn in ((0, lambda: K.conv2d_fwd(xd, wd, g)), (1, lambda: K.conv2d_dgrad(dyd, wd, g)), (2, lambda: K.conv2d_wgrad(xd, dyd, g))):
        a, _ = launch(wino, g, case, kind, fn)
        b, _ = launch(wino, g, case, kind, fn)
        assert torch.equal(a, b), ("two launches differ", kind)
