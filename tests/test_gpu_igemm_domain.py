"""-m gpu: the fp32 convolution kernels of csrc/conv_igemm.hip and csrc/conv_small.hip (routes IGEMM, N16, NARROW, PHASES, RING, N16_WGRAD,
WGD) over what their planner routes, with the Winograd and split-bf16 switches at 0.  The tables and the restatement of the planner
(`plan`, `fp32_expected`) live in tests/test_igemm_domain_host.py, where they are held to pnp_conv2d_route and the workspace queries without
a GPU; here every pass of every row asserts WHICH SYMBOLS RAN against that restatement (a case expected on one variant that runs on another
fails), and the file ends with a test that the asserted variants cover test_igemm_domain_host.REQUIRED.

What is OBSERVED and what is only RESTATED: the profiler records the convolution kernels' symbols, and those are compared.  It does not
record the summing kernels (split_sum::serial_kernel<Plain / Drop / Scatter>: they open no profiler scope), the number of reduction splits a launch
took, or which instance of the wgrad_direct family ran ("wgrad_direct_kernel<KK> (all variants)").  The tags for those — the reducers,
"ring split", "phases one at a time", the WGD variants, tpw > 1 — enter ASSERTED from the restatement alone, and check A is by design
independent of the split count.  The split count itself is observed where the partials lie at the start of the workspace (the forward
and the RING filter gradient: _splits_written poisons the workspace and counts the slabs the launch filled); for the data gradients
and the per-workgroup partials of N16_WGRAD / WGD it rests on the host file, which holds every row's count to the workspace queries.

Per case and pass (forward, data gradient, data gradient + residual, filter gradient, filter gradient into a pre-filled slot):

A. exact operands — x, w, dy, residual and the slot are integers in [-2, 2] stored as float32: every product and every partial sum is an
   integer below 2^24 (asserted on the float64 reference: 4 x the longest reduction, and the largest reference value), so every summation
   order gives the same float32 and the results must EQUAL the float64 reference bit for bit, split or not.  With keep_prob = 0.5 the
   dropout epilogue is exact too (mask x 2).  A dropped or doubled tap / channel group / split / phase, a transposed fragment or a wrong
   scatter stride cannot pass this.
B. random operands against float64, relative to max|ref|.  The yardstick of each pass is the error of the SAME convolution evaluated in
   float32 on the CPU (oracle.tf_ops.conv2d + autograd on float32 tensors: an independent float32 evaluation of the same sums); a pass
   passes at max(FACTOR x yardstick, 2^-22) — an MFMA accumulator is a longer sequential chain than the CPU's blocked sums and rounding error
   grows like the square root of the chain length; 2^-22 is 4 ulp of the largest output.  One variant has a factor of its own, the un-split
   filter gradients of the RING route (UNSPLIT_WGRAD_FACTOR below, with the reason).  No bar exceeds test_gpu_conv.TOL = 1e-4.
   The measured table of the MI355X run is profiles/igemm_domain_tolerance.txt: the largest ratio at factor 4 is 3.78, at factor 8 it is
   6.39 (the 8192-pixel chain of the no-workspace fall-back).
C. the statistics and fused-BN epilogues on one layer per forward tile class.
D. the fall-back candidates of ConvPlan::pick (no workspace / a short one), through ctypes."""
import ctypes

import numpy as np
import pytest
import torch

import test_igemm_domain_host as H
from conftest import pkg
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# Un-split filter gradients of the RING route (conv_wgrad_kernel / conv_wgrad_ring_kernel with one reduction split): ONE MFMA accumulator per
# output walks all N OH OW pixels in order — 189 .. 400 terms on the small maps of the tables, 8192 in the no-workspace fall-back — while
# the CPU's float32 GEMM spreads the same reduction over at least 64 partial sums (16 SIMD lanes x 4 or more unrolled accumulators) that it
# adds at the end.  Rounding error grows like the square root of the chain length: sqrt(64) = 8.  (Every split launch, and every forward /
# data gradient, whose chains are R S C long on both sides, stays at FACTOR.)  The 64 partial sums are an argument about how a float32 GEMM
# is written for 512-bit SIMD, not something this file measures.  The class is set by that argument, not by which rows needed it: on the
# MI355X run (profiles/igemm_domain_tolerance.txt) its un-split ring-kernel rows of the tables measured at most 3.2, conv_wgrad_kernel mode 1
# 4.05 / 4.41 / 4.97, and the no-workspace fall-backs, whose chain is 8192 pixels, 5.51 / 6.24 (ring kernel) and 6.39 (conv_wgrad_kernel mode 3).
# MARGINS ARE THIN in places, at both factors: 6.39 of 8 above, and at FACTOR 3.78 (dw of 2x16x16x32x32x3x5) and 3.68 (dx of
# 2x68x68x40x5x5x5) of 4 — a change of summation order on either side (a kernel's, or the CPU library's) can trip these rows without
# anything being wrong; the figures to compare with are in the profile file, and every such row also has check A.
UNSPLIT_WGRAD_FACTOR = 8.0
FLOOR = 2.0 ** -22
CAP = 1e-4                     # test_gpu_conv.TOL: no bar of this file is wider
SEED, SID = 1234567, 5
ASSERTED = set()               # variant tags whose symbols were asserted (test_every_required_variant_was_asserted)
RAN = set()                    # table rows that ran


@pytest.fixture
def fp32(dev):
    """the Winograd and split-bf16 switches at 0; restores what was in force"""
    K = pkg("kernels")
    prev = (K.wino_mode(0), K.wino_wgrad_mode(0), K.x3_direct(0), K.x3_strided(0), K.x3_wgrad(0))
    yield K
    K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.x3_direct(prev[2]); K.x3_strided(prev[3]); K.x3_wgrad(prev[4])


def _ran(fn):
    """-> (result, sorted distinct symbols the launch recorded, over all four profiler classes: NARROW and WGD record under PROF_CONV_DIRECT)"""
    L = pkg("_lib")
    L.prof_summary()
    L.prof_enable(L.PROF_CONV_FWD | L.PROF_CONV_DGRAD | L.PROF_CONV_WGRAD | L.PROF_CONV_DIRECT)
    out = fn()
    torch.cuda.synchronize()
    L.prof_enable(0)
    return out, sorted({r["name"] for r in L.prof_summary()})


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _bar(yard, factor=FACTOR):
    bar = max(factor * yard, FLOOR)
    assert bar <= CAP, bar
    return bar


def _bit_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _reference(x, w, dy, case, dtype):
    """(y, dx, dw) of oracle.tf_ops.conv2d + autograd in `dtype` on the CPU"""
    st, dil, padding = case[7:]
    xg = torch.from_numpy(x).to(dtype).requires_grad_(True)
    wg = torch.from_numpy(w).to(dtype).requires_grad_(True)
    y = T.conv2d(xg, wg, st, dil, padding)
    y.backward(torch.from_numpy(dy).to(dtype))
    return y.detach(), xg.grad, wg.grad


def _ints(rng, shape):
    return rng.integers(-2, 3, size=shape).astype(np.float32)


def _operands(case, exact):
    N, Hh, W, C, Kf, R, S, st, dil, padding = case
    g = H.geom_of(case)
    rng = np.random.default_rng(sum(case[:9]) + (0 if exact else 1))
    if exact:
        x, w, dy = _ints(rng, (N, Hh, W, C)), _ints(rng, (R, S, C, Kf)), _ints(rng, (N, g.OH, g.OW, Kf))
        res, pre = _ints(rng, x.shape), _ints(rng, w.shape)
    else:
        x = rng.standard_normal((N, Hh, W, C)).astype(np.float32)
        w = (rng.standard_normal((R, S, C, Kf)) * np.sqrt(2.0 / (R * S * C))).astype(np.float32)
        dy = rng.standard_normal((N, g.OH, g.OW, Kf)).astype(np.float32)
        res, pre = rng.standard_normal(x.shape).astype(np.float32), rng.standard_normal(w.shape).astype(np.float32)
    return x, w, dy, res, pre


def _assert_exact_range(case, refs):
    """every product is at most 4 and a partial sum has at most `terms` of them (+ the residual / slot value): all integers below 2^24"""
    g = H.geom_of(case)
    terms = max(g.R * g.S * g.C, g.R * g.S * g.K, g.N * g.OH * g.OW)
    assert 4.0 * terms + 2.0 < 2.0 ** 24, (case, terms)
    for r in refs:
        assert float(r.abs().max()) + 2.0 < 2.0 ** 24 and bool((r == r.round()).all()), case


def _unread_rows(case):
    """VALID: input rows / columns past the last tap of the last output, which no output reads"""
    N, Hh, W, C, Kf, R, S, st, dil, padding = case
    g = H.geom_of(case)
    if padding != "VALID":
        return Hh, W
    return (g.OH - 1) * st + (R - 1) * dil + 1, (g.OW - 1) * st + (S - 1) * dil + 1


def _passes(K, case, dev, exact):
    """all five launches of one case on one operand set -> dict of results, dict of symbols, references (y, dx, dw, res, pre)"""
    x, w, dy, res, pre = _operands(case, exact)
    g = H.lib_geom(K, case)
    xd, wd, dyd, resd, pred = (torch.from_numpy(a).to(dev) for a in (x, w, dy, res, pre))
    out, names = {}, {}
    out["y"], names[0] = _ran(lambda: K.conv2d_fwd(xd, wd, g))
    out["dx"], names[1] = _ran(lambda: K.conv2d_dgrad(dyd, wd, g))
    out["dx+res"], names["1r"] = _ran(lambda: K.conv2d_dgrad(dyd, wd, g, residual=resd))
    out["dw"], names[2] = _ran(lambda: K.conv2d_wgrad(xd, dyd, g))
    out["dw into"], names["2a"] = _ran(lambda: K.conv2d_wgrad(xd, dyd, g, into=pred.clone()))
    return out, names, (x, w, dy, res, pre)


def _splits_written(K, dev, nbytes, slab, launch):
    """how many `slab`-float partial results at the start of the workspace a launch wrote: the workspace (the buffer kernels.workspace hands
    out again for the same request) is filled with NaN bit patterns first; the written slabs must be whole and lead the buffer"""
    ws = K.workspace(nbytes, dev).view(torch.float32)
    ws.fill_(float("nan"))
    launch()
    torch.cuda.synchronize()
    n = ws.numel() // slab
    clean = ~torch.isnan(ws[:n * slab].reshape(n, slab))
    whole = clean.all(1)
    count = int(whole.sum())
    assert bool(whole[:count].all()) and not bool(clean[count:].any()), "partials must be whole slabs at the start of the workspace"
    return count


def _check_split_counts(K, dev, case, xd, wd, dyd):
    """the forward (route IGEMM) and the filter gradient (route RING) take the number of reduction splits the restatement gives"""
    g, r = H.lib_geom(K, case), H.geom_of(case)
    p = H.plan(case, 0)
    if p["route"] == H.IGEMM and p["nsplit"] > 1:
        ns = p["launches"][0]["ns"]
        got = _splits_written(K, dev, p["ws_bytes"], r.N * r.OH * r.OW * r.K, lambda: K.conv2d_fwd(xd, wd, g))
        assert got == (ns if ns > 1 else 0), (case, "forward splits", got, ns)
    p = H.plan(case, 2)
    if p["route"] == H.RING and p["ws_bytes"] > 0:
        ns = p["launches"][0]["ns"]
        got = _splits_written(K, dev, p["ws_bytes"], r.R * r.S * r.C * r.K, lambda: K.conv2d_wgrad(xd, dyd, g))
        assert got == (ns if ns > 1 else 0), (case, "filter-gradient splits", got, ns)


def _check_symbols(K, case, names):
    g = H.lib_geom(K, case)
    for kind, keys in ((0, (0,)), (1, (1, "1r")), (2, (2, "2a"))):
        p = H.plan(case, kind)
        assert K.conv_route(g, kind) == p["route"], (case, kind)
        for k in keys:
            assert names[k] == p["symbols"], (case, k, names[k], p["symbols"])
        ASSERTED.update(p["tags"])


def _check_case(K, dev, case):
    # A. exact operands
    out, names, (x, w, dy, res, pre) = _passes(K, case, dev, True)
    _check_symbols(K, case, names)
    y64, dx64, dw64 = _reference(x, w, dy, case, torch.float64)
    _assert_exact_range(case, (y64, dx64, dw64))
    want = {"y": y64, "dx": dx64, "dx+res": dx64 + torch.from_numpy(res).double(), "dw": dw64, "dw into": dw64 + torch.from_numpy(pre).double()}
    for k, ref in want.items():
        got = out[k].cpu()
        assert torch.equal(got, ref.float()), "%s of %s differs from the float64 reference on exact operands: %d of %d values, max |diff| %g; ran %s" % (
            k, case, int((got != ref.float()).sum()), got.numel(), float((got.double() - ref).abs().max()), names)
    uh, uw = _unread_rows(case)
    if uh < case[1] or uw < case[2]:
        assert _bit_zero(out["dx"][:, uh:]) and _bit_zero(out["dx"][:, :, uw:]), "input rows no output reads must get a bit-zero gradient"
    _check_split_counts(K, dev, case, *(torch.from_numpy(a).to(dev) for a in (x, w, dy)))
    # B. random operands
    out, names2, (x, w, dy, res, pre) = _passes(K, case, dev, False)
    assert names2 == names, (case, names, names2)
    y64, dx64, dw64 = _reference(x, w, dy, case, torch.float64)
    y32, dx32, dw32 = _reference(x, w, dy, case, torch.float32)
    rows = []
    pw = H.plan(case, 2)
    fac_w = UNSPLIT_WGRAD_FACTOR if pw["route"] == H.RING and pw["launches"][0]["ns"] == 1 else FACTOR
    for k, got, ref, ref32 in (("y", out["y"], y64, y32), ("dx", out["dx"], dx64, dx32), ("dw", out["dw"], dw64, dw32)):
        err, yard = _rel(got, ref), _rel(ref32, ref)
        bar = _bar(yard, fac_w if k == "dw" else FACTOR)
        rows.append((k, err, yard, bar))
        print("igemm domain %-40s %-2s err %.3e yardstick %.3e ratio %5.2f bar %.3e  %s" % (
            H.case_id(case), k, err, yard, err / max(yard, 1e-300), bar, names[{"y": 0, "dx": 1, "dw": 2}[k]]))
    # the add-into entry points against the plain results + the addend, in float64, at the bar of the pass
    r_dx = _rel(out["dx+res"], dx64 + torch.from_numpy(res).double())
    r_dw = _rel(out["dw into"], dw64 + torch.from_numpy(pre).double())
    for k, err, yard, bar in rows:
        assert err <= bar, (case, k, err, yard, bar)
    assert r_dx <= rows[1][3] and r_dw <= rows[2][3], (case, r_dx, r_dw, rows)
    RAN.add(case)


@pytest.mark.parametrize("case", H.FWD, ids=H.case_id)
def test_forward_and_stride1_data_gradient_domain(fp32, dev, case):
    _check_case(fp32, dev, case)


@pytest.mark.parametrize("case", H.STRIDED, ids=H.case_id)
def test_strided_data_gradient_domain(fp32, dev, case):
    _check_case(fp32, dev, case)


@pytest.mark.parametrize("case", H.WGRAD, ids=H.case_id)
def test_filter_gradient_domain(fp32, dev, case):
    _check_case(fp32, dev, case)


@pytest.mark.parametrize("case", H.DROPOUT, ids=H.case_id)
def test_dropout_epilogue_is_exact_on_exact_operands(fp32, dev, case):
    """keep_prob = 0.5: y = conv x mask x 2, bit for bit — in the kernel's epilogue, and in split_sum::serial_kernel<Drop> where the forward
    splits its reduction"""
    K = fp32
    x, w, dy, _, _ = _operands(case, True)
    g = H.lib_geom(K, case)
    xd, wd = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    yd, names = _ran(lambda: K.conv2d_fwd(xd, wd, g, keep_prob=0.5, seed=SEED, stream_id=SID))
    p = H.plan(case, 0, drop=True)
    assert names == p["symbols"], (case, names, p["symbols"])
    ASSERTED.update(p["tags"])
    y64 = T.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), *case[7:])
    mask = torch.from_numpy(T.dropout_mask(tuple(y64.shape), 0.5, SEED, SID)).double()
    assert 0.45 < float(mask.mean()) < 0.55
    assert torch.equal(yd.cpu(), (y64 * mask * 2.0).float()), (case, names)


# ---- C. epilogues on this family's tiles -----------------------------------------------------------------------------------------------
EPILOGUE = H.EPILOGUE


def _bn_reference(y, scale, shift, sc, alpha):
    """bn_epilogue of csrc/conv_common.h in the dtype of y: y scale + shift, + the channel-padded shortcut, leaky-ReLU"""
    Kf, Cs = y.shape[-1], sc.shape[-1]
    v = y * scale.to(y.dtype) + shift.to(y.dtype)
    lo = (Kf - Cs) // 2
    v[..., lo:lo + Cs] += sc.to(y.dtype)
    return torch.where(v < 0, v * alpha, v)


@pytest.mark.parametrize("case,symbol", EPILOGUE, ids=[H.case_id(c) for c, _ in EPILOGUE])
def test_epilogues_on_each_forward_tile_class(fp32, dev, case, symbol):
    K = fp32
    N, Hh, W, C, Kf, R, S, st, dil, padding = case
    g = H.lib_geom(K, case)
    narrow = H.plan(case, 0)["route"] == H.NARROW
    if not narrow:
        assert H.plan(case, 0)["symbols"] == [symbol] and H.plan(case, 0)["nsplit"] == 1, case
    P = g.N * g.OH * g.OW
    # statistics (bars of test_bn_statistics_from_the_conv_epilogue): y bit for bit the plain forward, moments to float32 round-off
    x, w, dy, _, _ = _operands(case, False)
    xd, wd = torch.from_numpy(x + np.float32(0.3)).to(dev), torch.from_numpy(w + np.float32(0.01)).to(dev)
    rng = np.random.default_rng(sum(case[:9]) + 2)
    if K.conv_stats_parts(g) > 0:
        mm = torch.from_numpy((0.2 * rng.standard_normal(Kf)).astype(np.float32)).to(dev)
        y_ref = K.conv2d_fwd(xd, wd, g, 0.75, 5, 2)
        (y, parts), names = _ran(lambda: K.conv2d_fwd_stats(xd, wd, g, mm, 0.75, 5, 2))
        assert names == [symbol], (case, names)
        mean, var = K.bn_stats_finish(parts, mm, P)
        assert torch.equal(y, y_ref)
        y64 = y_ref.double().reshape(P, Kf)
        m64, v64 = y64.mean(0), y64.var(0, unbiased=False)
        rel = lambda a, b: float((a.double().cpu() - b.cpu()).abs().max() / b.abs().max())
        print("igemm domain epilogue stats %s: mean %.2e var %.2e" % (H.case_id(case), rel(mean, m64), rel(var, v64)))
        assert rel(mean, m64) < 2e-6 and rel(var, v64) < 1e-5, (case, rel(mean, m64), rel(var, v64))
    else:
        assert symbol.startswith("conv_n16_kernel") or narrow, case          # (no statistics epilogue on the N16 / NARROW kernels)
    # fused BN + channel-padded shortcut (Cs < K) + leaky-ReLU 0.25: exact operands bit for bit, random operands against float64
    Cs = Kf - 4 if Kf > 8 else (Kf - 2 if Kf > 2 else Kf)
    for exact in (True, False):
        x, w, _, _, _ = _operands(case, exact)
        if exact:
            scale = (2.0 ** rng.integers(-1, 3, size=Kf)).astype(np.float32)
            shift, sc = _ints(rng, (Kf,)), _ints(rng, (g.N, g.OH, g.OW, Cs))
        else:
            scale, shift = rng.uniform(0.5, 1.5, Kf).astype(np.float32), rng.standard_normal(Kf).astype(np.float32)
            sc = rng.standard_normal((g.N, g.OH, g.OW, Cs)).astype(np.float32)
        ss = torch.from_numpy(np.stack([scale, shift])).to(dev)
        yb, names = _ran(lambda: K.conv2d_fwd_bn(torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), g, ss,
                                                 shortcut=torch.from_numpy(sc).to(dev), alpha=0.25))
        assert names == [symbol], (case, names)                               # a NARROW layer must take IGEMM here
        y64 = T.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), st, dil, padding)
        ref = _bn_reference(y64, torch.from_numpy(scale), torch.from_numpy(shift), torch.from_numpy(sc), 0.25)
        if exact:
            assert float(ref.abs().max()) * 4 < 2.0 ** 24
            assert torch.equal(yb.cpu(), ref.float()), (case, names, int((yb.cpu() != ref.float()).sum()))
        else:
            y32 = T.conv2d(torch.from_numpy(x), torch.from_numpy(w), st, dil, padding)
            yard = _rel(_bn_reference(y32, torch.from_numpy(scale), torch.from_numpy(shift), torch.from_numpy(sc), 0.25), ref)
            err = _rel(yb, ref)
            print("igemm domain epilogue fused bn %s: err %.3e yardstick %.3e ratio %.2f  %s" % (H.case_id(case), err, yard, err / yard, names))
            assert err <= _bar(yard), (case, err, yard)
    ASSERTED.add("epilogues " + symbol)


# ---- D. the fall-back candidates of ConvPlan::pick ---------------------------------------------------------------------------------
def _cp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_ab(case, kind, launch, dev, factor=FACTOR):
    """A and B of one pass through `launch(x, w, dy, pre)` (device tensors; pre: the slot of the accumulating entry point or None)"""
    rows = []
    for exact in (True, False):
        x, w, dy, res, pre = _operands(case, exact)
        xd, wd, dyd, pred = (torch.from_numpy(a).to(dev) for a in (x, w, dy, pre))
        refs = _reference(x, w, dy, case, torch.float64)
        got, names = _ran(lambda: launch(xd, wd, dyd, None))
        ref = refs[kind]
        if kind == 2:
            acc, names_a = _ran(lambda: launch(xd, wd, dyd, pred.clone()))
            assert names_a == names
        if exact:
            _assert_exact_range(case, refs)
            assert torch.equal(got.cpu(), ref.float()), (case, kind, names)
            if kind == 2:
                assert torch.equal(acc.cpu(), (ref + torch.from_numpy(pre).double()).float()), (case, names)
        else:
            yard = _rel(_reference(x, w, dy, case, torch.float32)[kind], ref)
            err = _rel(got, ref)
            print("igemm domain fall-back %-34s %-2s err %.3e yardstick %.3e ratio %5.2f bar %.3e  %s" % (
                H.case_id(case), ("y", "dx", "dw")[kind], err, yard, err / yard, _bar(yard, factor), names))
            assert err <= _bar(yard, factor), (case, kind, err, yard)
            if kind == 2:
                assert _rel(acc, ref + torch.from_numpy(pre).double()) <= _bar(yard, factor)
        rows.append(names)
    assert rows[0] == rows[1]
    return rows[0]


@pytest.mark.parametrize("case", [(1, 8, 8, 160, 64, 3, 3, 1, 1, "SAME"), (2, 64, 64, 112, 7, 3, 3, 1, 1, "SAME")], ids=H.case_id)
def test_forward_without_workspace_runs_unsplit(fp32, dev, case):
    """pnp_conv2d_fwd_ws with a null workspace on a layer whose plan splits the reduction: the un-split candidate"""
    K, lib = fp32, pkg("_lib").load()
    g = H.lib_geom(K, case)
    r = H.geom_of(case)
    assert H.plan(case, 0)["nsplit"] > 1
    want = H.igemm_launch(r.N * r.OH * r.OW, r.K, r.C, r.R, r.S, True, 0, False)
    assert want["ns"] == 1 and want["reducer"] is None

    def launch(xd, wd, dyd, _):
        y = torch.empty((g.N, g.OH, g.OW, g.K), dtype=torch.float32, device=dev)
        K.check(lib.pnp_conv2d_fwd_ws(_cp(xd), _cp(wd), _cp(y), ctypes.byref(g), 1.0, 0, 0, None, 0, _stream()), "pnp_conv2d_fwd_ws")
        return y
    assert _check_ab(case, 0, launch, dev) == [want["sym"]]
    ASSERTED.add("forward fall-back un-split")


# (case, workspace in partial filters [None: null pointer], splits the ring kernel then takes)
SHORT_WS = [
    ((2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"), None, 1),        # an N16_WGRAD geometry without workspace
    ((2, 64, 64, 20, 12, 3, 3, 1, 1, "SAME"), None, 1),        # a WGD geometry without workspace
    ((2, 64, 64, 16, 3, 3, 3, 1, 1, "SAME"), None, 1),         # ... with K % 4 != 0: the RING route's scalar-B kernel (conv_wgrad_kernel mode 3)
    ((2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"), 2.0, 2),         # room for 2 partial filters, 32 blocks planned: the ring kernel with 2 splits
    ((3, 37, 41, 64, 64, 3, 3, 1, 1, "SAME"), 2.0, 2),         # a RING layer that plans 17 splits: as many as fit
    ((3, 37, 41, 64, 64, 3, 3, 1, 1, "SAME"), 1.5, 1),         # one partial is no split
    ((2, 64, 64, 16, 3, 3, 3, 1, 1, "SAME"), 1.5, 1),
]


@pytest.mark.parametrize("case,room,ns", SHORT_WS, ids=["%s-%s" % (H.case_id(c), r) for c, r, _ in SHORT_WS])
def test_filter_gradient_with_a_short_workspace_runs_the_ring_kernel(fp32, dev, case, room, ns):
    """pnp_conv2d_wgrad / _wgrad_acc with no workspace or a short one: the RING route (the ring kernel; its scalar-B sibling for K % 4 != 0),
    with as many reduction splits as fit; the workspace comes from kernels.workspace so that the canary of conftest.py guards it"""
    K, lib = fp32, pkg("_lib").load()
    g = H.lib_geom(K, case)
    r = H.geom_of(case)
    nout = r.R * r.S * r.C * r.K
    nbytes = 0 if room is None else int(room * nout * 4)
    assert nbytes < H.plan(case, 2)["ws_bytes"]
    want = H.ring_launch(r, nbytes)
    assert want["ns"] == ns and want["sym"].startswith("conv_wgrad_ring_kernel<" if r.K % 4 == 0 else "conv_wgrad_kernel<128, 32, 4, 1, 3, false>"), want

    def launch(xd, wd, dyd, slot):
        ws = K.workspace(nbytes, dev, slot="short") if nbytes else None
        dw = slot if slot is not None else torch.empty((g.R, g.S, g.C, g.K), dtype=torch.float32, device=dev)
        fn = lib.pnp_conv2d_wgrad_acc if slot is not None else lib.pnp_conv2d_wgrad
        K.check(fn(_cp(xd), _cp(dyd), _cp(dw), ctypes.byref(g), _cp(ws) if ws is not None else None, ws.numel() if ws is not None else 0, _stream()),
                "pnp_conv2d_wgrad")
        return dw
    assert _check_ab(case, 2, launch, dev, UNSPLIT_WGRAD_FACTOR if ns == 1 else FACTOR) == [want["sym"]]
    ASSERTED.add("ring fall-back %s" % ("no workspace" if room is None else ("%d splits" % ns)))


def test_every_required_variant_was_asserted(fp32):
    """the symbols asserted above, with the variant tags of the restatement, cover every variant of the family (REQUIRED of the host file).
    This test closes the file: it fails when the file did not run as a whole (a deselection, or a row that failed before its tags counted)."""
    rows = set(H.FWD + H.STRIDED + H.WGRAD)
    assert RAN == rows, "table rows that did not run to the end: %s" % sorted(rows - RAN, key=str)
    for case in RAN:
        for kind in (0, 1, 2):
            assert H.plan(case, kind)["tags"] <= ASSERTED, (case, kind)
    extra = ["forward fall-back un-split", "ring fall-back no workspace", "ring fall-back 2 splits", "ring fall-back 1 splits"] + \
            ["epilogues " + s for _, s in EPILOGUE]
    missing = [t for t in H.REQUIRED + extra if t not in ASSERTED]
    assert not missing, missing
