"""-m gpu: the filter gradient of the narrow stride-1 3x3 layers (32 / 64 input channels, 64 filters) on the direct split-bf16 kernel
(csrc/conv_x3_wgrad.hip, kernels.x3_wgrad): accuracy against the float64 filter gradient of the same float32 operands, with the fp32-pipe
route of the same tree (ring kernel + partial sum) as the yardstick of the bar; the accumulating entry point; determinism; the planner and
its workspace.  Each case checks which kernel symbols ran.

Bar: err_new <= 2 x max(err_fp32_route, 1e-6) of max|ref| — 2x because the partition of the pixel sum differs (one chain per workgroup
against split chunks), which moves the rounding pattern but not its class; the 1e-6 floor keeps a lucky reference run from making the bar
unattainable (a CPU emulation of both arithmetics puts them at 0.3 .. 1.4e-6)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

# (N, H, C, K, operands)
CASES = [
    (1, 64, 32, 64, "normal"),
    (1, 64, 64, 64, "normal"),
    (2, 128, 64, 64, "normal"),
    (3, 48, 64, 64, "normal"),          # 27 tiles: an odd number of tiles per workgroup share
    (1, 64, 64, 64, "wide"),            # magnitudes 1e-6 .. 1e3, 75 % exact zeros
]
NEW, NEW_SUM = "conv_x3_wgrad_kernel<%d>", "split_sum::sliced_kernel<4>"


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


def _operands(rng, shape, kind):
    a = rng.standard_normal(shape)
    if kind == "wide":
        a = a * 10.0 ** rng.uniform(-6.0, 3.0, shape) * (rng.random(shape) < 0.25)
    return a.astype(np.float32)


def _bar(err_old):
    return 2.0 * max(err_old, 1e-6)


@pytest.fixture
def route():
    K = pkg("kernels")
    prev = (K.x3_direct(-1), K.x3_wgrad(-1), K.wino_wgrad_mode(0))       # (the Winograd filter-gradient planner is asked first: off here)
    yield K
    K.x3_direct(prev[0]); K.x3_wgrad(prev[1]); K.wino_wgrad_mode(prev[2])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_wgrad_split_bf16_vs_float64(dev, route, case):
    K, L = route, pkg("_lib")
    N, H, C, Kf, kind = case
    rng = np.random.default_rng(N + H + C + Kf + len(kind))
    x = _operands(rng, (N, H, H, C), kind)
    dy = _operands(rng, (N, H, H, Kf), kind)
    g = K.conv_geom(x.shape, (3, 3, C, Kf), 1, 1, "SAME")
    xd, dyd = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
    wg = torch.zeros((3, 3, C, Kf), dtype=torch.float64, requires_grad=True)
    T.conv2d(torch.from_numpy(x).double(), wg, 1, 1, "SAME").backward(torch.from_numpy(dy).double())

    K.x3_direct(2)
    K.x3_wgrad(0)                                     # the parent's route: fp32-pipe kernel + partial sum
    dw0, names0 = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g), L.PROF_CONV_WGRAD)
    assert not any("x3" in n for n in names0), names0
    K.x3_wgrad(1)
    dw1, names1 = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g), L.PROF_CONV_WGRAD)
    assert names1 == sorted([NEW % (C // 32), NEW_SUM]), names1
    err_new, err_old = _rel(dw1, wg.grad), _rel(dw0, wg.grad)
    print("x3 wgrad %s: split-bf16 %.2e, fp32 route %.2e (%s) of max|ref|" % (case, err_new, err_old, ", ".join(names0)))
    assert err_new <= _bar(err_old), (err_new, err_old)


def test_wgrad_split_bf16_accumulates_and_is_deterministic(dev, route):
    K, L = route, pkg("_lib")
    K.x3_direct(2)
    rng = np.random.default_rng(11)
    for (N, H, C) in ((2, 64, 32), (2, 64, 64)):
        x = torch.from_numpy(rng.standard_normal((N, H, H, C)).astype(np.float32)).to(dev)
        dy = torch.from_numpy(rng.standard_normal((N, H, H, 64)).astype(np.float32)).to(dev)
        pre = torch.from_numpy(rng.standard_normal((3, 3, C, 64)).astype(np.float32) * 50.0).to(dev)
        g = K.conv_geom(tuple(x.shape), (3, 3, C, 64), 1, 1, "SAME")
        wg = torch.zeros((3, 3, C, 64), dtype=torch.float64, requires_grad=True)
        T.conv2d(x.cpu().double(), wg, 1, 1, "SAME").backward(dy.cpu().double())
        ref = pre.cpu().double() + wg.grad
        K.x3_wgrad(0)
        acc0 = K.conv2d_wgrad(x, dy, g, into=pre.clone())
        K.x3_wgrad(1)
        dw, names = _ran(L, lambda: K.conv2d_wgrad(x, dy, g), L.PROF_CONV_WGRAD)
        assert NEW % (C // 32) in names, names
        acc1, names_a = _ran(L, lambda: K.conv2d_wgrad(x, dy, g, into=pre.clone()), L.PROF_CONV_WGRAD)
        assert NEW % (C // 32) in names_a, names_a
        assert torch.equal(acc1, pre + dw), "accumulate differs from pre-fill + gradient"
        err_new, err_old = _rel(acc1, ref), _rel(acc0, ref)
        print("x3 wgrad accumulate (%d, %d, %d->64): split-bf16 %.2e, fp32 route %.2e of max|ref|" % (N, H, C, err_new, err_old))
        assert err_new <= _bar(err_old), (err_new, err_old)
        assert torch.equal(dw, K.conv2d_wgrad(x, dy, g)), "two launches differ"
        assert torch.equal(acc1, K.conv2d_wgrad(x, dy, g, into=pre.clone())), "two accumulating launches differ"


# (N, OH, OW, C) -> partials: one per 16 x 16 tile, two where C = 32.  The sum (split_sum::sliced_kernel<4>) gives slice s the partials
# s, s + 16, ...: fewer partials than slices (3, 6), one and two past a full round of 16 (17, 34).  CASES above reach 16, 27, 32, 64, 128.
FEW_PARTS = [((1, 16, 48, 64), 3), ((1, 16, 48, 32), 6), ((17, 16, 16, 64), 17), ((17, 16, 16, 32), 34)]


@pytest.mark.parametrize("shape,parts", FEW_PARTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wgrad_split_bf16_part_counts_off_the_slice_count(dev, route, shape, parts):
    K, L = route, pkg("_lib")
    N, H, W, C = shape
    rng = np.random.default_rng(N + W + C)
    x, dy = _operands(rng, (N, H, W, C), "normal"), _operands(rng, (N, H, W, 64), "normal")
    pre = torch.from_numpy(rng.standard_normal((3, 3, C, 64)).astype(np.float32) * 50.0).to(dev)
    g = K.conv_geom(x.shape, (3, 3, C, 64), 1, 1, "SAME")
    xd, dyd = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
    wg = torch.zeros((3, 3, C, 64), dtype=torch.float64, requires_grad=True)
    T.conv2d(torch.from_numpy(x).double(), wg, 1, 1, "SAME").backward(torch.from_numpy(dy).double())
    K.x3_direct(2)
    K.x3_wgrad(0)
    dw0, acc0 = K.conv2d_wgrad(xd, dyd, g), K.conv2d_wgrad(xd, dyd, g, into=pre.clone())
    K.x3_wgrad(1)
    assert int(L.load().pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g))) == parts * 9 * C * 64 * 4
    dw1, names = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g), L.PROF_CONV_WGRAD)
    assert names == sorted([NEW % (C // 32), NEW_SUM]), names
    acc1, names_a = _ran(L, lambda: K.conv2d_wgrad(xd, dyd, g, into=pre.clone()), L.PROF_CONV_WGRAD)
    assert names_a == names, names_a
    ref_acc = pre.cpu().double() + wg.grad
    errs = (_rel(dw1, wg.grad), _rel(dw0, wg.grad), _rel(acc1, ref_acc), _rel(acc0, ref_acc))
    print("x3 wgrad %s, %d partials: split-bf16 %.2e (fp32 route %.2e), accumulating %.2e (%.2e) of max|ref|" % ((shape, parts) + errs))
    assert errs[0] <= _bar(errs[1]) and errs[2] <= _bar(errs[3]), errs
    assert torch.equal(acc1, pre + dw1), "accumulate differs from pre-fill + gradient"


def test_wgrad_split_bf16_planner(dev, route):
    """shapes the predicate refuses run the old symbols; x3_direct(0) and x3_wgrad(0) each leave the new symbol out; mode 1 needs >= 256
    tiles; the workspace query covers the launch (kernels.conv2d_wgrad allocates exactly that many bytes: conftest's canary)"""
    K, L = route, pkg("_lib")
    lib = L.load()
    rng = np.random.default_rng(13)

    def names_of(N, H, C, Kf=64, stride=1, dil=1, padding="SAME", dtype=None):
        x = torch.from_numpy(rng.standard_normal((N, H, H, C)).astype(np.float32)).to(dev)
        g = K.conv_geom(tuple(x.shape), (3, 3, C, Kf), stride, dil, padding) if dtype is None else \
            K.conv_geom(tuple(x.shape), (3, 3, C, Kf), stride, dil, padding, dtype=dtype)
        dy = torch.from_numpy(rng.standard_normal((N, g.OH, g.OW, Kf)).astype(np.float32)).to(dev)
        _, n = _ran(L, lambda: K.conv2d_wgrad(x, dy, g), L.PROF_CONV_WGRAD | L.PROF_CONV_DIRECT)
        return n

    K.x3_direct(2); K.x3_wgrad(1)
    assert NEW % 2 in names_of(1, 64, 64)
    for kw in (dict(H=40), dict(C=48), dict(stride=2), dict(dil=2), dict(padding="SYMMETRIC"), dict(dtype=L.DTYPE_BF16), dict(Kf=128), dict(Kf=32)):
        args = dict(N=1, H=64, C=64)
        args.update(kw)
        n = names_of(**args)
        assert n and not any("x3w" in s or "x3_wgrad" in s for s in n), (kw, n)
    K.x3_direct(0)
    assert not any("x3" in s for s in names_of(1, 64, 64))
    K.x3_direct(2); K.x3_wgrad(0)
    assert not any("x3" in s for s in names_of(1, 64, 64))
    K.x3_wgrad(1); K.x3_direct(1)
    assert not any("x3" in s for s in names_of(1, 64, 64)), "mode 1 takes a layer only with >= 256 tiles"
    assert NEW % 1 in names_of(16, 256, 32) and NEW % 2 in names_of(16, 256, 64)
    # a layer the Winograd filter-gradient planner chooses stays there
    K.x3_direct(2); K.wino_wgrad_mode(2)
    assert K.wino_chosen(K.conv_geom((1, 64, 64, 64), (3, 3, 64, 64), 1, 1, "SAME"), 2)
    assert not any("x3w" in s or "x3_wgrad" in s for s in names_of(1, 64, 64))
    K.wino_wgrad_mode(0); K.x3_direct(1)
    # the workspace: the partial sums of the route, one predicate for the query and the launch
    g = K.conv_geom((16, 256, 256, 64), (3, 3, 64, 64), 1, 1, "SAME")
    g32 = K.conv_geom((16, 256, 256, 32), (3, 3, 32, 64), 1, 1, "SAME")
    gb = K.conv_geom((16, 256, 256, 64), (3, 3, 64, 64), 1, 1, "SAME", dtype=L.DTYPE_BF16)
    ws = lambda q: int(lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(q)))
    on = (ws(g), ws(g32), ws(gb))
    K.x3_wgrad(0)
    off = (ws(g), ws(g32), ws(gb))
    assert on[0] == 256 * 9 * 64 * 64 * 4 and on[1] == 512 * 9 * 32 * 64 * 4 and on[2] == off[2] and on[:2] != off[:2], (on, off)
