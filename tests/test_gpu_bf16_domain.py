"""-m gpu: the two bf16 convolution families — csrc/conv_bf16r.hip (operands resident as bf16, LDS-DMA pipeline) and csrc/conv_bf16.hip
(operands rounded while staged) — over what their planners route, with the Winograd and split-bf16 switches at 0.  The tables and the
restatement of the host side live in tests/test_bf16_domain_host.py, where they are held to the library's queries without a GPU; here
every pass of every row asserts WHICH SYMBOLS RAN (and, for the stride phases, how often) against that restatement, and the file ends with
a test that the asserted variants cover test_bf16_domain_host.REQUIRED.

Per RESIDENT row and pass the row is served for (forward, data gradient, data gradient + residual, filter gradient, filter gradient into
a pre-filled slot):

A. exact operands — integers in [-2, 2] are exact in bf16, every product and partial sum is an integer below 2^24 (asserted on the float64
   reference: 4 x the longest reduction, and the largest reference value), so the result must EQUAL the reference bit for bit whatever the
   tile, the stage count, the split or the phase.  With keep_prob = 0.5 the dropout epilogue of the forward is exact too.  A dropped or
   doubled tap / channel group / stage / split / phase, a transposed fragment, a wrong swizzle or a mis-clamped prologue cannot pass this.
B. random operands against a float64 convolution of the bf16-ROUNDED operands (oracle.tf_ops.round_bf16), relative to max|ref|.  A
   bf16 x bf16 product is exact in float32, so what is left is float32 summation order; the yardstick is the same rounded-operand
   convolution evaluated in float32 on the CPU and a pass passes at max(FACTOR x yardstick, 2^-22) — rule and reasoning of
   tests/test_gpu_igemm_domain.py.  Un-split filter gradients have UNSPLIT_WGRAD_FACTOR (below, with the reason).  No bar is wider than the
   2e-5 of tests/test_gpu_bf16.py and tests/test_gpu_bf16r.py (asserted).  The measured table of the MI355X run is
   profiles/bf16_domain_tolerance.txt: 271 comparisons, the largest ratio at factor 4 is 2.42 (the BKC 32 data gradient of
   2x50x46x128x96, the same on all three tiles), at factor 8 it is 1.83 (the staged filter gradient without workspace).
   Side outputs: `yh` / `dxh` equal the float32 output of the same launch rounded once, on the A and on the B operands.
C. the epilogues (statistics partials, fused BN + shortcut + leaky-ReLU, dropout stream) on one row per tile class.
D. the filter-gradient fall-backs (no workspace, room for fewer partials than planned, room for exactly one) through ctypes, with the
   partial slabs actually written counted.

The STAGED family runs test_igemm_domain_host.FWD + STRIDED + WGRAD with dtype = PNP_DTYPE_BF16 through the ordinary entry points: where
the restatement names a bf16 symbol, checks A and B and the symbol; where it names the fp32 symbol, the result must be bit-identical to the
PNP_DTYPE_F32 result of the same call ("a layer that stays fp32 is exact, never looser", csrc/conv_bf16.hip).

What is OBSERVED and what is only RESTATED: as in tests/test_gpu_igemm_domain.py the profiler records the convolution kernels' symbols
and launch counts; the summing kernels open no profiler scope, so the reducer tags and "staged ... split" enter ASSERTED from the
restatement (check A does not depend on the split).  The resident filter gradient's split count is observed (_splits_written)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_bf16_domain_host as BH
import test_gpu_igemm_domain as G
import test_igemm_domain_host as H
from conftest import pkg
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# Un-split filter gradients (conv_wgrad_bf16r_kernel / conv_wgrad_bf16_kernel with one reduction split — the no-workspace and one-partial
# fall-backs): ONE accumulator per output walks all N OH OW pixels in order (4096 and more here), while the CPU's float32 GEMM spreads the
# same reduction over at least 64 partial sums (16 SIMD lanes x 4 or more unrolled accumulators).  Rounding error grows like the square root
# of the chain length: sqrt(64) = 8 — the argument, and the figure, of test_gpu_igemm_domain.UNSPLIT_WGRAD_FACTOR.  Every split launch, and
# every forward / data gradient (chains of R S C or R S K on both sides), stays at FACTOR.
UNSPLIT_WGRAD_FACTOR = 8.0
FLOOR = 2.0 ** -22
CAP = 2e-5                     # the bar of tests/test_gpu_bf16.py and tests/test_gpu_bf16r.py: no bar of this file is wider
SEED, SID = 1234567, 5
ASSERTED = set()               # variant tags whose symbols were asserted (test_every_required_variant_was_asserted)
RAN = set()                    # (table, row) that ran to the end
RATIOS = []                    # (line of the table, ratio, bar, factor) of every check-B comparison


@pytest.fixture
def fp32(dev):
    """the Winograd and split-bf16 switches at 0; restores what was in force"""
    K = pkg("kernels")
    prev = (K.wino_mode(0), K.wino_wgrad_mode(0), K.x3_direct(0), K.x3_strided(0), K.x3_wgrad(0))
    yield K
    K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.x3_direct(prev[2]); K.x3_strided(prev[3]); K.x3_wgrad(prev[4])


def _launches(fn):
    """-> (result, {symbol: launches} the profiler recorded over all four convolution classes)"""
    L = pkg("_lib")
    L.prof_summary()
    L.prof_enable(L.PROF_CONV_FWD | L.PROF_CONV_DGRAD | L.PROF_CONV_WGRAD | L.PROF_CONV_DIRECT)
    out = fn()
    torch.cuda.synchronize()
    L.prof_enable(0)
    return out, {r["name"]: r["launches"] for r in L.prof_summary()}


def _bar(yard, factor=FACTOR):
    bar = max(factor * yard, FLOOR)
    assert bar <= CAP, bar
    return bar


def _rb(a):
    return T.round_bf16(torch.from_numpy(a)).numpy()


def _refs(x, w, dy, case, dtype, kinds):
    """(y, dx, dw) of oracle.tf_ops.conv2d + autograd in `dtype` on the CPU; only the gradients `kinds` asks for"""
    st, dil, padding = case[7:]
    xg = torch.from_numpy(x).to(dtype).requires_grad_(1 in kinds)
    wg = torch.from_numpy(w).to(dtype).requires_grad_(2 in kinds)
    y = T.conv2d(xg, wg, st, dil, padding)
    if 1 in kinds or 2 in kinds:
        y.backward(torch.from_numpy(dy).to(dtype))
    return y.detach(), xg.grad, wg.grad


def _record(label, k, got, ref, ref32, factor, symbols):
    err, yard = G._rel(got, ref), G._rel(ref32, ref)
    bar = _bar(yard, factor)
    line = "bf16 domain %-44s %-7s err %.3e yardstick %.3e ratio %5.2f bar %.3e  %s" % (label, k, err, yard, err / max(yard, 1e-300), bar, sorted(symbols))
    RATIOS.append((line, err / max(yard, 1e-300), bar, factor))
    print(line)
    return err, bar


def _rounded_once(h, y):
    return torch.equal(h.float(), y.bfloat16().float())


# ---- the resident family ---------------------------------------------------------------------------------------------------------------
def resident_passes(K, dev, case, x, w, dy, res, pre, kinds):
    """every pass of `kinds` on one operand set -> results, {pass: {symbol: launches}}"""
    g = BH.lib_geom(K, case)
    xd, wd, dyd, resd, pred = (torch.from_numpy(a).to(dev) for a in (x, w, dy, res, pre))
    xh, dyh = K.cast_bf16(xd), K.cast_bf16(dyd)
    w_io, w_oi = K.filter_bf16(wd)
    out, names = {}, {}
    if 0 in kinds:
        (out["y"], out["yh"], _), names["y"] = _launches(lambda: K.conv2d_fwd_bf16r(xh, w_oi, g, want_h=True))
        (out["y drop"], _, _), names["y drop"] = _launches(lambda: K.conv2d_fwd_bf16r(xh, w_oi, g, keep_prob=0.5, seed=SEED, stream_id=SID))
    if 1 in kinds:
        s1 = g.stride == 1           # (a strided data gradient is one launch per stride phase, rows scattered: no bf16 copy, no residual)
        (out["dx"], out["dxh"]), names["dx"] = _launches(lambda: K.conv2d_dgrad_bf16r(dyh, w_io, g, want_h=s1))
        if s1:
            (out["dx+res"], _), names["dx+res"] = _launches(lambda: K.conv2d_dgrad_bf16r(dyh, w_io, g, residual=resd))
    if 2 in kinds:
        out["dw"], names["dw"] = _launches(lambda: K.conv2d_wgrad_bf16r(xh, dyh, g))
        out["dw into"], names["dw into"] = _launches(lambda: K.conv2d_wgrad_bf16r(xh, dyh, g, into=pred.clone()))
    return out, names


def _wants(refs, res, pre, kinds, stride):
    y, dx, dw = refs
    want = {}
    if 0 in kinds:
        want["y"] = y
    if 1 in kinds:
        want["dx"] = dx
        if stride == 1:
            want["dx+res"] = dx + torch.from_numpy(res).to(dx.dtype)
    if 2 in kinds:
        want["dw"], want["dw into"] = dw, dw + torch.from_numpy(pre).to(dw.dtype)
    return want


def check_resident_row(K, dev, case, kinds, force_tile=-1, force_split=0, label=""):
    """symbols, A, B and the side outputs of one resident row -> the variant tags asserted"""
    plans = {k: BH.rplan(case, k, force_tile=force_tile, force_split=force_split) for k in kinds}
    assert all(plans.values()), (case, kinds)
    key_kind = {"y": 0, "y drop": 0, "dx": 1, "dx+res": 1, "dw": 2, "dw into": 2}
    tags = set()
    all_names = None
    for exact in (True, False):
        x, w, dy, res, pre = G._operands(case, exact)
        out, names = resident_passes(K, dev, case, x, w, dy, res, pre, kinds)
        for k, got in names.items():
            assert got == plans[key_kind[k]]["symbols"], (case, k, got, plans[key_kind[k]]["symbols"])
        assert all_names in (None, names)
        all_names = names
        xr, wr, dyr = (x, w, dy) if exact else (_rb(x), _rb(w), _rb(dy))
        refs = _refs(xr, wr, dyr, case, torch.float64, kinds)
        want = _wants(refs, res, pre, kinds, case[7])
        if exact:
            G._assert_exact_range(case, [r for r in refs if r is not None])
            for k, ref in want.items():
                got = out[k].cpu()
                assert torch.equal(got, ref.float()), "%s of %s differs from the float64 reference on exact operands: %d of %d values, max |diff| %g; ran %s" % (
                    k, case, int((got != ref.float()).sum()), got.numel(), float((got.double() - ref).abs().max()), names)
            if 0 in kinds:
                mask = torch.from_numpy(T.dropout_mask(tuple(refs[0].shape), 0.5, SEED, SID)).double()
                assert 0.45 < float(mask.mean()) < 0.55
                assert torch.equal(out["y drop"].cpu(), (refs[0] * mask * 2.0).float()), (case, names["y drop"])
        else:
            refs32 = _refs(xr, wr, dyr, case, torch.float32, kinds)
            want32 = _wants(refs32, res, pre, kinds, case[7])
            unsplit = 2 in kinds and plans[2]["launches"][0]["ns"] == 1
            fails = []
            for k, ref in want.items():
                err, bar = _record(label + BH.case_id(case), k, out[k], ref, want32[k], UNSPLIT_WGRAD_FACTOR if (unsplit and key_kind[k] == 2) else FACTOR,
                                   names[k])
                if err > bar:
                    fails.append((k, err, bar))
            assert not fails, (case, fails)
        if 0 in kinds:
            assert _rounded_once(out["yh"], out["y"]), (case, "yh", exact)
        if 1 in kinds and case[7] == 1:
            assert _rounded_once(out["dxh"], out["dx"]), (case, "dxh", exact)
    for k in kinds:
        tags |= plans[k]["tags"]
    return tags


def _resident_kinds(case):
    return tuple(k for k in (0, 1, 2) if BH.rplan(case, k) is not None)


@pytest.mark.parametrize("case", BH.RESIDENT, ids=BH.case_id)
def test_resident_domain(fp32, dev, case):
    K = fp32
    g = BH.lib_geom(K, case)
    kinds = _resident_kinds(case)
    assert kinds and kinds == tuple(k for k in (0, 1, 2) if K.bf16r_served(g, k)), (case, kinds)
    ASSERTED.update(check_resident_row(K, dev, case, kinds))
    if 2 in kinds:               # the split count the launch really took: partial slabs at the start of the workspace
        L = BH.rplan(case, 2)["launches"][0]
        x, w, dy, _, _ = G._operands(case, True)
        xh, dyh = K.cast_bf16(torch.from_numpy(x).to(dev)), K.cast_bf16(torch.from_numpy(dy).to(dev))
        nout = g.R * g.S * g.C * g.K
        got = G._splits_written(K, dev, max(L["planned"] * nout * 4, 4), nout, lambda: K.conv2d_wgrad_bf16r(xh, dyh, g))
        assert got == (L["ns"] if L["ns"] > 1 else 0), (case, got, L)
    RAN.add(("resident", case))


# ---- C. epilogues of the resident forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BH.EPILOGUE, ids=BH.case_id)
def test_resident_epilogues_on_each_tile_class(fp32, dev, case):
    """statistics partials (the tile's own row geometry: bm 128 x wm 2, bm 256 x wm 4, rows past M masked) -> bn_stats_finish against bn_stats
    of the output and against float64 moments, with dropout on; the dropout stream against pnp_dropout; fused BN + shortcut + leaky-ReLU
    against bn_apply, with the bf16 copy of the RESULT"""
    K = fp32
    g = BH.lib_geom(K, case)
    p = BH.rplan(case, 0)
    rng = np.random.default_rng(sum(case[:9]) + 2)
    x, w, _, _, _ = G._operands(case, False)
    xd, wd = torch.from_numpy(x + np.float32(0.3)).to(dev), torch.from_numpy(w + np.float32(0.01)).to(dev)
    xh, w_oi = K.cast_bf16(xd), K.filter_bf16(wd)[1]
    P, Kf = g.N * g.OH * g.OW, g.K
    (y0, _, _), names = _launches(lambda: K.conv2d_fwd_bf16r(xh, w_oi, g))
    assert names == p["symbols"], (case, names)
    yd = K.conv2d_fwd_bf16r(xh, w_oi, g, keep_prob=0.75, seed=7, stream_id=3)[0]
    assert torch.equal(yd, K.dropout(y0, 0.75, 7, 3))
    shift = torch.from_numpy((0.2 * rng.standard_normal(Kf)).astype(np.float32)).to(dev)
    (y1, _, parts), names = _launches(lambda: K.conv2d_fwd_bf16r(xh, w_oi, g, keep_prob=0.75, seed=7, stream_id=3, stat_shift=shift, want_stats=True))
    assert names == p["symbols"] and torch.equal(y1, yd)
    assert parts[1] == BH.stats_parts(case) > 0, (case, parts[1])
    mean, var = K.bn_stats_finish(parts, shift, P)
    m2, v2 = K.bn_stats(yd)
    y64 = yd.double().reshape(P, Kf)
    m64, v64 = y64.mean(0), y64.var(0, unbiased=False)
    errs = (G._rel(mean, m2), G._rel(var, v2), G._rel(mean, m64), G._rel(var, v64))
    print("bf16 domain epilogue stats %s: vs bn_stats mean %.2e var %.2e; vs float64 mean %.2e var %.2e" % ((BH.case_id(case),) + errs))
    assert all(e < 1e-5 for e in errs), (case, errs)              # the bars of tests/test_gpu_bf16r.py
    gamma, beta = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (1 + 0.1 * rng.standard_normal(Kf), 0.1 * rng.standard_normal(Kf)))
    sc = torch.from_numpy(rng.standard_normal((g.N, g.OH, g.OW, Kf // 2)).astype(np.float32)).to(dev)
    ss = K.bn_fold(gamma, beta, mean, var, 1e-3)
    (out, outh, _), names = _launches(lambda: K.conv2d_fwd_bf16r(xh, w_oi, g, want_h=True, bn=(ss, sc, 0.2)))
    assert names == p["symbols"]
    ref = K.bn_apply(y0, mean, var, gamma, beta, sc, 1e-3, 0.2)
    e = G._rel(out, ref)
    print("bf16 domain epilogue fused bn %s: vs bn_apply %.2e" % (BH.case_id(case), e))
    assert e < 2e-6 and _rounded_once(outh, out), (case, e)
    ASSERTED.update(p["tags"])
    ASSERTED.add("epilogues " + BH.case_id(case))


# ---- D. fall-backs of the resident filter gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,room", BH.FALLBACK, ids=["%s-%s" % (BH.case_id(c), r) for c, r in BH.FALLBACK])
def test_resident_filter_gradient_with_a_short_workspace(fp32, dev, case, room):
    """pnp_conv2d_wgrad_bf16r with a null workspace, or one with room for fewer partials than planned: as many splits as fit, a single
    partial is no split — exact either way, plain and accumulating; the partial slabs the launch wrote are counted"""
    K, lib = fp32, pkg("_lib").load()
    g, r = BH.lib_geom(K, case), H.geom_of(case)
    nout = r.R * r.S * r.C * r.K
    nbytes = 0 if room is None else int(room * nout * 4)
    want = BH.wgrad_launch(r, nbytes)
    assert nbytes < want["planned"] * nout * 4 and want["ns"] == (1 if room is None or room < 2 else int(room)), want
    x, w, dy, _, pre = G._operands(case, True)
    xh, dyh = K.cast_bf16(torch.from_numpy(x).to(dev)), K.cast_bf16(torch.from_numpy(dy).to(dev))
    ref = _refs(x, w, dy, case, torch.float64, (2,))
    G._assert_exact_range(case, (ref[0], ref[2]))
    for acc in (0, 1):
        dw = torch.from_numpy(pre).to(dev) if acc else torch.empty((g.R, g.S, g.C, g.K), dtype=torch.float32, device=dev)
        ws = K.workspace(nbytes, dev, slot="short").view(torch.float32) if nbytes else None
        if ws is not None:
            ws.fill_(float("nan"))
        _, names = _launches(lambda: K.check(lib.pnp_conv2d_wgrad_bf16r(K._ph(xh), K._ph(dyh), K._p(dw), acc, ctypes.byref(g), G._cp(ws) if ws is not None else None,
                                                                        nbytes, G._stream()), "pnp_conv2d_wgrad_bf16r"))
        assert names == {want["sym"]: 1}, (case, room, names)
        assert torch.equal(dw.cpu(), (ref[2] + (torch.from_numpy(pre).double() if acc else 0.0)).float()), (case, room, acc)
        if ws is not None:
            n = ws.numel() // nout
            whole = (~torch.isnan(ws[:n * nout].reshape(n, nout))).all(1)
            count = int(whole.sum())
            assert bool(whole[:count].all()) and not bool((~torch.isnan(ws[count * nout:])).any())
            assert count == (want["ns"] if want["ns"] > 1 else 0), (case, room, count, want)
    ASSERTED.update({want["sym"], "resident wgrad split" if want["ns"] > 1 else "unsplit"})
    ASSERTED.add("resident fall-back %s" % ("no workspace" if room is None else "%d splits" % want["ns"]))


# ---- PNP_BF16R_TILE / PNP_BF16R_WSPLIT: read once per process ------------------------------------------------------------------------
def _worker(env):
    env = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "bf16r_tile_worker.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "BF16R WORKER OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    for line in r.stdout.splitlines():
        if line.startswith("bf16 domain ") and " err " in line:          # (the worker's comparisons are all at FACTOR: forward, data gradient, split)
            RATIOS.append((line, float(line.split(" ratio ")[1].split()[0]), float(line.split(" bar ")[1].split()[0]), FACTOR))
    return set(json.loads([l for l in r.stdout.splitlines() if l.startswith("TAGS ")][-1][5:]))


@pytest.mark.parametrize("tile", [0, 1, 2])
def test_forced_tile_in_a_process_of_its_own(dev, tile):
    """PNP_BF16R_TILE = 0 / 1 / 2 (tests/bf16r_tile_worker.py): FORCED rows, forward and data gradient with checks A and B, the statistics
    partials of the forced tile's row geometry and the side outputs, the forced symbol asserted.  Tile 1 (128x128, NBUF = 2) is reached
    in no other way."""
    tags = _worker({"PNP_BF16R_TILE": str(tile)})
    want = set()
    for case in BH.FORCED:
        for kind in (0, 1):
            p = BH.rplan(case, kind, force_tile=tile)
            if p:
                want |= p["tags"]
    assert tags == want, (sorted(tags ^ want))
    assert all(("forced " + s in tags) or (s in tags) for s in BH.all_conv_instances(tile)), tile
    ASSERTED.update(tags)


def test_forced_split_with_a_short_last_part(dev):
    """PNP_BF16R_WSPLIT=3 on 64 reduction chunks: parts of 22, 22 and 20"""
    tags = _worker({"PNP_BF16R_WSPLIT": str(BH.WSPLIT)})
    assert tags == BH.rplan(BH.WSPLIT_ROW, 2, force_split=BH.WSPLIT)["tags"] and "split with a short last part" in tags, tags
    ASSERTED.add("forced split 3")


# ---- the staged family -------------------------------------------------------------------------------------------------------------------
def _staged_passes(K, g, xd, wd, dyd, resd, pred):
    out, names = {}, {}
    out["y"], names["y"] = G._ran(lambda: K.conv2d_fwd(xd, wd, g))
    out["dx"], names["dx"] = G._ran(lambda: K.conv2d_dgrad(dyd, wd, g))
    out["dx+res"], names["dx+res"] = G._ran(lambda: K.conv2d_dgrad(dyd, wd, g, residual=resd))
    out["dw"], names["dw"] = G._ran(lambda: K.conv2d_wgrad(xd, dyd, g))
    out["dw into"], names["dw into"] = G._ran(lambda: K.conv2d_wgrad(xd, dyd, g, into=pred.clone()))
    return out, names


KEY_KIND = {"y": 0, "dx": 1, "dx+res": 1, "dw": 2, "dw into": 2}


@pytest.mark.parametrize("case", BH.STAGED, ids=H.case_id)
def test_staged_domain(fp32, dev, case):
    K = fp32
    gb, gf = BH.lib_geom(K, case), BH.lib_geom(K, case, bf16=False)
    plans = {k: BH.bf16_plan(case, k) for k in (0, 1, 2)}
    on_bf16 = tuple(k for k in (0, 1, 2) if plans[k]["bf16"])
    for exact in (True, False):
        x, w, dy, res, pre = G._operands(case, exact)
        dv = [torch.from_numpy(a).to(dev) for a in (x, w, dy, res, pre)]
        out, names = _staged_passes(K, gb, *dv)
        for k, got in names.items():
            assert got == plans[KEY_KIND[k]]["symbols"], (case, k, got, plans[KEY_KIND[k]]["symbols"])
        if len(on_bf16) < 3:              # a pass that stays fp32 is the PNP_DTYPE_F32 call, bit for bit
            out32, names32 = _staged_passes(K, gf, *dv)
            for k in out:
                if KEY_KIND[k] not in on_bf16:
                    assert names32[k] == names[k] and torch.equal(out[k], out32[k]), (case, k, names[k], names32[k])
        if not on_bf16:
            continue
        xr, wr, dyr = (x, w, dy) if exact else (_rb(x), _rb(w), _rb(dy))
        refs = _refs(xr, wr, dyr, case, torch.float64, on_bf16)
        want = _wants(refs, res, pre, on_bf16, 1)
        if exact:
            G._assert_exact_range(case, [r for r in refs if r is not None])
            for k, ref in want.items():
                got = out[k].cpu()
                assert torch.equal(got, ref.float()), "%s of %s (bf16 operands) differs from the float64 reference on exact operands: %d of %d values; ran %s" % (
                    k, case, int((got != ref.float()).sum()), got.numel(), names)
        else:
            refs32 = _refs(xr, wr, dyr, case, torch.float32, on_bf16)
            want32 = _wants(refs32, res, pre, on_bf16, 1)
            fails = []
            for k, ref in want.items():
                unsplit = KEY_KIND[k] == 2 and plans[2]["launches"][0]["ns"] == 1
                err, bar = _record("staged " + H.case_id(case), k, out[k], ref, want32[k], UNSPLIT_WGRAD_FACTOR if unsplit else FACTOR, names[k])
                if err > bar:
                    fails.append((k, err, bar))
            assert not fails, (case, fails)
    for k in on_bf16:
        ASSERTED.update(plans[k]["tags"])
    RAN.add(("staged", case))


@pytest.mark.parametrize("case", BH.STAGED_DROPOUT, ids=H.case_id)
def test_staged_dropout_is_exact_on_exact_operands(fp32, dev, case):
    """keep_prob = 0.5 on a bf16 taps forward: in the kernel's epilogue, and in split_sum::serial_kernel<Drop> where the forward splits"""
    K = fp32
    x, w, _, _, _ = G._operands(case, True)
    g = BH.lib_geom(K, case)
    yd, names = G._ran(lambda: K.conv2d_fwd(torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), g, keep_prob=0.5, seed=SEED, stream_id=SID))
    p = BH.bf16_plan(case, 0, drop=True)
    assert p["bf16"] and names == p["symbols"], (case, names, p["symbols"])
    y64 = T.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), *case[7:])
    mask = torch.from_numpy(T.dropout_mask(tuple(y64.shape), 0.5, SEED, SID)).double()
    assert torch.equal(yd.cpu(), (y64 * mask * 2.0).float()), (case, names)
    ASSERTED.update(p["tags"])


@pytest.mark.parametrize("case", BH.STAGED_FALLBACK, ids=H.case_id)
def test_staged_filter_gradient_without_workspace_runs_unsplit(fp32, dev, case):
    """pnp_conv2d_wgrad / _wgrad_acc with a null workspace and dtype = PNP_DTYPE_BF16: conv_wgrad_bf16_kernel with one reduction split"""
    K, lib = fp32, pkg("_lib").load()
    g, r = BH.lib_geom(K, case), H.geom_of(case)
    sym = "conv_wgrad_bf16_kernel<%s>" % H.TILE_ARGS[H.ring_tile(r.K)]
    for exact in (True, False):
        x, w, dy, _, pre = G._operands(case, exact)
        xd, dyd = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
        xr, wr, dyr = (x, w, dy) if exact else (_rb(x), _rb(w), _rb(dy))
        ref = _refs(xr, wr, dyr, case, torch.float64, (2,))[2]
        got = {}
        for acc in (0, 1):
            dw = torch.from_numpy(pre).to(dev) if acc else torch.empty((g.R, g.S, g.C, g.K), dtype=torch.float32, device=dev)
            fn = lib.pnp_conv2d_wgrad_acc if acc else lib.pnp_conv2d_wgrad
            _, names = G._ran(lambda: K.check(fn(G._cp(xd), G._cp(dyd), G._cp(dw), ctypes.byref(g), None, 0, G._stream()), "pnp_conv2d_wgrad"))
            assert names == [sym], (case, names)
            got[acc] = dw
        want = {0: ref, 1: ref + torch.from_numpy(pre).double()}
        if exact:
            G._assert_exact_range(case, (ref,))
            assert all(torch.equal(got[a].cpu(), want[a].float()) for a in (0, 1)), case
        else:
            ref32 = _refs(xr, wr, dyr, case, torch.float32, (2,))[2]
            for a in (0, 1):
                err, bar = _record("staged no workspace " + H.case_id(case), ("dw", "dw into")[a], got[a], want[a],
                                   ref32 + (torch.from_numpy(pre) if a else 0.0), UNSPLIT_WGRAD_FACTOR, [sym])
                assert err <= bar, (case, a, err, bar)
    ASSERTED.update({sym, "staged wgrad unsplit"})


def test_every_required_variant_was_asserted(dev):
    """the symbols asserted above, with the variant tags of the restatement, cover test_bf16_domain_host.REQUIRED.  This test closes the
    file: it fails when the file did not run as a whole (a deselection, or a row that failed before its tags counted).  It prints the
    check-B table (profiles/bf16_domain_tolerance.txt is this output; PNP_BF16_DOMAIN_TABLE names a file to write it to)."""
    rows = {("resident", c) for c in BH.RESIDENT} | {("staged", c) for c in BH.STAGED}
    assert RAN == rows, "table rows that did not run to the end: %s" % sorted(rows - RAN, key=str)
    extra = ["epilogues " + BH.case_id(c) for c in BH.EPILOGUE] + ["resident fall-back no workspace", "resident fall-back 2 splits",
                                                                   "resident fall-back 1 splits", "forced split 3"]
    missing = [t for t in list(BH.REQUIRED) + extra if t not in ASSERTED]
    assert not missing, missing
    # the table: a comparison whose bar is the 2^-22 floor has a yardstick below 2^-24 and its ratio says nothing about the factor
    worst = {}
    for line, ratio, bar, factor in RATIOS:
        if bar > FLOOR and ratio > worst.get(factor, (0.0, ""))[0]:
            worst[factor] = (ratio, " ".join(line.split(" err ")[0].split()[2:]))
    head = "%d check-B comparisons.  " % len(RATIOS) + "  ".join("Largest ratio above the 2^-22 floor at factor %g: %.2f (%s)." % (f, v[0], v[1])
                                                                for f, v in sorted(worst.items()))
    text = "\n".join([head, ""] + [r[0] for r in RATIOS]) + "\n"
    print(text)
    path = os.environ.get("PNP_BF16_DOMAIN_TABLE")
    if path:
        with open(path, "w") as fh:
            fh.write(text)
