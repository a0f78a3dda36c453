"""-m gpu: the critics' strided layers on the direct split-bf16 kernels (csrc/conv_x3_direct.hip, kernels.x3_strided): the forward as a sum of
stride-1 convolutions over the input's stride phases, the data gradient as all output stride phases in one launch.  Forward and data
gradient against the float64 convolution of the same float32 operands, the epilogues (dropout mask stream, BN statistics partials, residual
data gradient) against the fp32-pipe kernels, and the planner.  Each case checks which kernel symbols ran.

Bar: 5e-6 of max|ref| (every product exact; one fp32 chain per output)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

# (N, H, C, K, R, stride, padding)
CASES = [
    (1, 64, 64, 64, 3, 2, "SAME"),        # critic k3s2 (pad 0, 1): phase sub-filters 2x2, 2x1, 1x2, 1x1
    (1, 64, 128, 128, 5, 2, "SAME"),      # critic k5s2 (pad 1, 2): 3x3, 3x2, 2x3, 2x2
    (1, 32, 256, 256, 3, 2, "SAME"),      # eight channel halves, four filter blocks
    (2, 33, 64, 128, 3, 2, "VALID"),      # VALID: forward 16 x 16 outputs; the data gradient's phases (17 / 16 rows) are not taken
]
BAR = 5e-6
FWD = "conv_x3_direct_kernel_strided<0>"
DGRAD = "conv_x3_direct_kernel_strided<1>"


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _ran(L, fn, cls):
    L.prof_summary()
    L.prof_enable(cls)
    out = fn()
    torch.cuda.synchronize()
    L.prof_enable(0)
    return out, sorted(r["name"] for r in L.prof_summary())


@pytest.fixture
def route():
    K = pkg("kernels")
    prev = (K.x3_direct(-1), K.x3_strided(-1))
    yield K
    K.x3_direct(prev[0]); K.x3_strided(prev[1])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_strided_split_bf16_fwd_dgrad_vs_float64(dev, route, case):
    K, L = route, pkg("_lib")
    N, H, C, Kf, R, s, padding = case
    rng = np.random.default_rng(sum(case[:6]))
    x = rng.standard_normal((N, H, H, C)).astype(np.float32)
    w = (rng.standard_normal((R, R, C, Kf)) * np.sqrt(2.0 / (R * R * C))).astype(np.float32)
    g = K.conv_geom(x.shape, w.shape, s, 1, padding)
    dy = rng.standard_normal((N, g.OH, g.OW, Kf)).astype(np.float32)
    res = rng.standard_normal(x.shape).astype(np.float32)
    xd, wd, dyd, resd = (torch.from_numpy(a).to(dev) for a in (x, w, dy, res))
    xg = torch.from_numpy(x).double().requires_grad_(True)
    yo = T.conv2d(xg, torch.from_numpy(w).double(), s, 1, padding)
    yo.backward(torch.from_numpy(dy).double())

    K.x3_direct(2)
    K.x3_strided(0)                                   # the fp32-pipe kernels of the same tree
    y0, names0 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD)
    dx0, names0d = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD)
    assert not any("x3" in n for n in names0 + names0d), names0 + names0d
    K.x3_strided(1)
    y1, names1 = _ran(L, lambda: K.conv2d_fwd(xd, wd, g), L.PROF_CONV_FWD)
    assert names1 == sorted(["x3s_filter_kernel<false>", FWD]), names1
    dx1, names2 = _ran(L, lambda: K.conv2d_dgrad(dyd, wd, g), L.PROF_CONV_DGRAD)
    taken_d = padding == "SAME"
    if taken_d:
        assert names2 == sorted(["x3s_filter_kernel<true>", DGRAD]), names2
    else:
        assert not any("x3" in n for n in names2), names2
    dxr = K.conv2d_dgrad(dyd, wd, g, residual=resd)
    errs = {"y": _rel(y1, yo), "dx": _rel(dx1, xg.grad), "dx+res": _rel(dxr, xg.grad + torch.from_numpy(res).double()),
            "y fp32 pipe": _rel(y0, yo), "dx fp32 pipe": _rel(dx0, xg.grad)}
    print("x3 strided %s: %s" % (case, {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["y"] < BAR and errs["dx"] < BAR and errs["dx+res"] < BAR, errs


def test_strided_split_bf16_epilogues_equal_the_fp32_kernels(dev, route):
    """dropout (identical zero pattern), BN statistics partials -> mean / variance, residual data gradient: route on versus off"""
    K, L = route, pkg("_lib")
    K.x3_direct(2)
    rng = np.random.default_rng(5)
    for (N, H, C, Kf, R) in ((2, 64, 64, 64, 3), (1, 64, 128, 128, 5)):
        x = torch.from_numpy(rng.standard_normal((N, H, H, C)).astype(np.float32)).to(dev)
        w = torch.from_numpy((rng.standard_normal((R, R, C, Kf)) * np.sqrt(2.0 / (R * R * C))).astype(np.float32)).to(dev)
        g = K.conv_geom(tuple(x.shape), tuple(w.shape), 2, 1, "SAME")
        dy = torch.from_numpy(rng.standard_normal((N, g.OH, g.OW, Kf)).astype(np.float32)).to(dev)
        res = torch.from_numpy(rng.standard_normal((N, H, H, C)).astype(np.float32)).to(dev)
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
            dxr = K.conv2d_dgrad(dy, w, g, residual=res)
            out[on] = (yd, ys, mean, var, nparts, dxr)
        (yd0, ys0, m0, v0, _, dr0), (yd1, ys1, m1, v1, np1, dr1) = out[0], out[1]
        assert np1 == N * g.OH * g.OW // 64
        assert torch.equal(yd0 == 0, yd1 == 0), "dropout masks differ"
        assert torch.equal(ys1, yd1)
        errs = {"drop": _rel(yd1, yd0), "mean": _rel(m1, m0), "var": _rel(v1, v0), "dx+res": _rel(dr1, dr0)}
        print("x3 strided epilogues (%d, %d, %d->%d k%d): %s" % (N, H, C, Kf, R, {k: "%.2e" % v for k, v in errs.items()}))
        assert max(errs.values()) < 1e-5, errs


def test_strided_split_bf16_planner(dev, route):
    """mode 0 leaves nothing on the route; mode 1 takes a layer only with >= 256 items and where it measured faster; bf16 and SYMMETRIC
    geometries never"""
    K, L = route, pkg("_lib")
    rng = np.random.default_rng(7)

    def names_of(N, H, C, Kf, R, padding="SAME"):
        x = torch.from_numpy(rng.standard_normal((N, H, H, C)).astype(np.float32)).to(dev)
        w = torch.from_numpy((rng.standard_normal((R, R, C, Kf)) * 0.05).astype(np.float32)).to(dev)
        g = K.conv_geom(tuple(x.shape), tuple(w.shape), 2, 1, padding)
        dy = torch.from_numpy(rng.standard_normal((N, g.OH, g.OW, Kf)).astype(np.float32)).to(dev)
        _, nf = _ran(L, lambda: K.conv2d_fwd(x, w, g), L.PROF_CONV_FWD)
        _, nd = _ran(L, lambda: K.conv2d_dgrad(dy, w, g), L.PROF_CONV_DGRAD)
        return nf + nd

    K.x3_strided(1)
    K.x3_direct(0)
    assert not any("x3" in n for n in names_of(4, 64, 64, 64, 3)), "mode 0 must leave nothing on the bf16 pipe"
    K.x3_direct(1)
    # 4 x 2 x 2 tiles x 1 filter block = 16 forward items, 64 data-gradient items: refused in mode 1, taken in mode 2
    assert not any("x3" in n for n in names_of(4, 64, 64, 64, 3))
    # k3s2 64@256: its data gradient is taken (4096 items); its forward (2.25 taps per phase patch) is left to the fp32 pipe
    n = names_of(16, 256, 64, 64, 3)
    assert DGRAD in n and FWD not in n, n
    # k5s2 128@128: both
    n = names_of(16, 128, 128, 128, 5)
    assert DGRAD in n and FWD in n, n
    K.x3_direct(2)
    assert FWD in names_of(4, 64, 64, 64, 3)
    assert not any("x3" in n for n in names_of(4, 64, 64, 64, 3, padding="SYMMETRIC"))
    # bf16 operands: never on the split-bf16 route (the workspace is the same with the route on and off)
    gb = K.conv_geom((16, 128, 128, 128), (5, 5, 128, 128), 2, 1, "SAME", dtype=L.DTYPE_BF16)
    g32 = K.conv_geom((16, 128, 128, 128), (5, 5, 128, 128), 2, 1, "SAME")
    lib = L.load()
    ws = lambda g: (int(lib.pnp_conv2d_fwd_workspace_bytes(ctypes.byref(g))), int(lib.pnp_conv2d_dgrad_workspace_bytes(ctypes.byref(g))))
    K.x3_direct(1)
    on_b, on_f = ws(gb), ws(g32)
    K.x3_strided(0)
    off_b, off_f = ws(gb), ws(g32)
    assert on_b == off_b
    assert on_f[0] >= 5 * 5 * 128 * 128 * 6 and on_f[1] >= 5 * 5 * 128 * 128 * 6 and on_f != off_f
