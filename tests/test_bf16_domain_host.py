"""not gpu: the domain of the two bf16 convolution families as tests/test_gpu_bf16_domain.py walks it.

RESIDENT family (csrc/conv_bf16r.hip: operands stored as bf16, LDS-DMA pipeline).  This file restates its host side in plain Python —
plan_tile, served, strided_dgrad_served (on test_igemm_domain_host.plan_phases), wgrad_bf16r_tile, the cost-model split planner
wgrad_bf16r_plan of csrc/conv_igemm.hip, and the conv_bf16r_kernel<...> / conv_wgrad_bf16r_kernel<...> symbol strings as the profiler
prints them — and holds every row of RESIDENT, FORCED and BOUNDARY to the library's three queries: pnp_conv2d_bf16r_served(g, 0 / 1 / 2),
pnp_conv2d_fwd_bf16r_stats_parts and pnp_conv2d_wgrad_bf16r_workspace_bytes (which encodes the split count).  BOUNDARY rows are queries
only: nothing is allocated for them.

STAGED family (csrc/conv_bf16.hip: fp32 tensors, operands rounded while a tile is staged).  It takes the fp32 planner's tiles, reduction
splits, reducers and phase launches, so `bf16_plan(case, kind)` is test_igemm_domain_host.plan with two substitutions: the taps symbol
becomes conv_taps_bf16_kernel<BM, BN, WM, WN, KIND, R, S> wherever `taps` holds (there is no taps3 variant on this side), and the filter
gradient's symbol becomes conv_wgrad_bf16_kernel<128, BN, WM, WN> wherever `lin` and `vecb` hold.  Everything else — the stride phases in
one launch, N16, NARROW, WGD, conv_fwd_kernel, strided or short-row filter gradients — keeps its fp32 symbol.

The 128x128 tile of conv_bf16r_kernel (plan_tile 1, NBUF = 2) is unreachable from plan_tile: see
test_resident_128x128_tile_is_unreachable_from_the_planner.  It runs under PNP_BF16R_TILE=1 only (tests/bf16r_tile_worker.py), and its
instances are in REQUIRED as "forced ..." tags."""
import ctypes
import math
import re

import numpy as np
import pytest

import test_igemm_domain_host as H
from conftest import pkg

cdiv = H.cdiv
CHUNK = 64               # kWgradBf16rChunk: pixels per reduction chunk of the resident filter gradient


def row(N, Hh, W, C, K, k, stride, dil, padding):
    """(N, H, W, C, K, k, stride, dil, padding) -> the 10-tuple of test_igemm_domain_host"""
    return (N, Hh, W, C, K, k, k, stride, dil, padding)


# ---- case tables --------------------------------------------------------------------------------------------------------------------
# Smallest shapes the predicates admit: M = 4096 pixels is the floor of `served`.
RESIDENT = [
    row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"),         # the floor: M = 4096, 128x64 tile, BKC 64, nst 9; 64x64 filter-gradient tile
    row(3, 37, 41, 64, 128, 3, 1, 1, "SAME"),        # ragged M = 4551, non-power-of-two map (split_row's divisions), forward and data gradient
    row(3, 37, 41, 96, 64, 3, 1, 1, "SAME"),         # BKC 32 forward (C = 96: three 32-groups), ragged, non-power-of-two
    row(2, 48, 48, 64, 96, 3, 1, 1, "SAME"),         # BKC 32 data gradient (K = 96), non-power-of-two map; the forward is refused (K % 64)
    row(1, 66, 66, 32, 2560, 3, 1, 1, "VALID"),      # 256x128 tile under the planner, BKC 32: 16 x 20 tiles
    row(1, 64, 64, 64, 64, 5, 1, 1, "SAME"),         # 5x5, nst 25: nst % NBUF = 1
    row(1, 64, 64, 128, 64, 5, 1, 1, "SAME"),        # 5x5, nst 50: nst % NBUF = 2; 128x64 filter-gradient tile over 25 taps
    row(1, 64, 64, 32, 64, 5, 1, 1, "SAME"),         # 5x5 BKC 32, nst 25
    row(4, 64, 64, 64, 64, 3, 2, 1, "SAME"),         # stride 2: sub-filters 1x1 .. 2x2 with one channel group: nst 1 (< NBUF - 1), 2, 2, 4
    row(4, 64, 64, 64, 128, 3, 2, 1, "SAME"),        # ... with two channel groups: nst 2, 4, 4, 8
    row(4, 64, 64, 64, 64, 5, 2, 1, "SAME"),         # 5x5 stride 2: sub-filters 3x3, 3x2, 2x3, 2x2
    row(4, 128, 128, 64, 64, 5, 4, 1, "SAME"),       # 5x5 stride 4: 16 phases, sub-filters 2x2, 2x1, 1x2, 1x1
    row(4, 65, 65, 64, 64, 3, 2, 1, "SAME"),         # odd map: the four phases differ in size (32x32 = 4096 pixels .. 33x33), all ragged but one
    row(2, 50, 46, 64, 64, 3, 1, 2, "SAME"),         # dilation 2 on a ragged, non-power-of-two map
    row(2, 32, 64, 128, 128, 3, 1, 1, "SAME"),       # H != W; 128x128 filter-gradient tile (NBUF = 2)
    row(1, 64, 64, 64, 128, 3, 1, 1, "SAME"),        # 64x128 filter-gradient tile
    row(1, 64, 64, 128, 64, 3, 1, 1, "SAME"),        # 128x64 filter-gradient tile
    row(1, 64, 64, 128, 128, 3, 1, 1, "SAME"),       # 128x128 filter-gradient tile
    row(5, 32, 32, 64, 64, 3, 1, 1, "SAME"),         # 80 reduction chunks of the filter gradient (N = 5: the split need not divide them)
    row(8, 64, 32, 64, 64, 3, 2, 1, "SAME"),         # stride 2 on H != W: OW = 16, OH OW = 512, 4096 pixels in the forward and in every phase
]
# rows tests/bf16r_tile_worker.py runs with PNP_BF16R_TILE = 0, 1, 2: small, output channels in whole 128-groups (forward: K, data gradient: C),
# and between them every instance launch_tile can emit
FORCED = [
    row(3, 37, 41, 64, 128, 3, 1, 1, "SAME"),        # forward 3x3 BKC 64 on a ragged, non-power-of-two map
    row(3, 37, 41, 96, 128, 3, 1, 1, "SAME"),        # forward 3x3 BKC 32, ragged
    row(1, 64, 64, 128, 128, 3, 1, 1, "SAME"),       # forward and data gradient 3x3 BKC 64
    row(2, 50, 46, 128, 96, 3, 1, 1, "SAME"),        # data gradient BKC 32 (K = 96), ragged M = 4600, non-power-of-two
    row(1, 64, 64, 64, 128, 5, 1, 1, "SAME"),        # forward 5x5 BKC 64
    row(1, 64, 64, 32, 128, 5, 1, 1, "SAME"),        # forward 5x5 BKC 32
    row(4, 64, 64, 128, 64, 3, 2, 1, "SAME"),        # stride phases 1x1, 1x2, 2x1, 2x2 over 128 output channels
    row(4, 65, 65, 128, 64, 5, 2, 1, "SAME"),        # stride phases 3x3, 3x2, 2x3, 2x2, ragged and unequal
]
WSPLIT_ROW, WSPLIT = row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"), 3       # 64 chunks under PNP_BF16R_WSPLIT=3: parts of 22, 22 and 20
# one row per tile class for the epilogues (check C): 128x64 and 256x128, BKC 32 and 64, one with M % BM != 0
EPILOGUE = [
    row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"),         # 128x64, BKC 64
    row(3, 37, 41, 96, 64, 3, 1, 1, "SAME"),         # 128x64, BKC 32, rows past M in the last tile (M = 4551)
    row(1, 66, 66, 32, 2560, 3, 1, 1, "VALID"),      # 256x128 (bm 256 x wm 4 statistics rows), BKC 32
    row(1, 69, 69, 64, 2560, 3, 1, 1, "VALID"),      # 256x128, BKC 64, rows past M (M = 4489: 18 tiles, the last with 137 rows)
]
# filter-gradient fall-backs (check D): (row, room in partial filters [None: a null workspace])
FALLBACK = [
    (row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"), None),
    (row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"), 2.5),          # fewer partials than planned
    (row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"), 1.5),          # exactly one: no split
    (row(2, 32, 64, 128, 128, 3, 1, 1, "SAME"), None),
    (row(2, 32, 64, 128, 128, 3, 1, 1, "SAME"), 2.0),
]
# staged filter gradients through pnp_conv2d_wgrad with a null workspace: the un-split conv_wgrad_bf16_kernel (no row of the fp32 tables
# with rows of >= 32 pixels plans fewer than two splits)
STAGED_FALLBACK = [(3, 37, 41, 64, 64, 3, 3, 1, 1, "SAME"), (1, 36, 40, 64, 32, 3, 3, 1, 1, "VALID")]
ALL = RESIDENT + [c for c in FORCED + EPILOGUE if c not in RESIDENT]


def case_id(c):
    return "x".join(str(v) for v in c)


# ---- the resident family restated -----------------------------------------------------------------------------------------------------
def plan_tile(M, K, force=-1):
    """0 = 256x128 (8 waves, 3 LDS stages), 1 = 128x128 (4 waves, 2 stages), 2 = 128x64 (4 waves, 3 stages); -1: not served.
    force: PNP_BF16R_TILE (honoured for the two 128-wide tiles only where K comes in whole 128-groups)"""
    if K % 64:
        return -1
    if K % 128 == 0 and cdiv(M, 256) * (K // 128) >= 256:
        tile = 0
    elif K % 128 == 0 and cdiv(M, 128) * (K // 128) >= 512:
        tile = 1
    else:
        tile = 2
    if force >= 0 and not (force <= 1 and K % 128 != 0):
        tile = force
    return tile


CAP = 1 << 30            # elements: both tensors stay under 2 GiB as bf16 and their 32-bit byte offsets under 2^31


def strided_dgrad_served(g):
    if g.K % 64 or g.C % 64:
        return False
    ph = H.plan_phases(g)
    if not ph:
        return False
    for p in ph:
        if p["I"] == 0 or p["J"] == 0:
            continue
        if p["T"] > 3 or p["U"] > 3 or (p["T"], p["U"]) in ((3, 1), (1, 3)):
            return False
        if g.N * p["I"] * p["J"] < 4096:
            return False
    return g.N * g.H * g.W * g.C < CAP and g.N * g.OH * g.OW * g.K < CAP


def served(g, kind):
    if g.sym:
        return False
    if kind == 1 and g.stride != 1:
        return strided_dgrad_served(g)
    red, outc = (g.K, g.C) if kind == 1 else (g.C, g.K)
    r_shape = (g.R, g.S) == (3, 3) or ((g.R, g.S) == (5, 5) and kind == 0)
    if not r_shape or red % 32 or outc % 64:
        return False
    if kind == 1 and (g.dil * (g.R - 1) < g.pad_t or g.dil * (g.S - 1) < g.pad_l):
        return False
    if g.N * g.H * g.W * g.C >= CAP or g.N * g.OH * g.OW * g.K >= CAP:
        return False
    M = g.N * g.H * g.W if kind == 1 else g.N * g.OH * g.OW
    if M < 4096:
        return False
    return plan_tile(M, outc) >= 0


def pow2(v):
    return v & (v - 1) == 0


def wgrad_bf16r_tile(g):
    """0 = 128x128, 1 = 128x64, 2 = 64x128, 3 = 64x64 (channels of one tap x filters); -1: not served"""
    if g.sym or g.C % 64 or g.K % 64:
        return -1
    P = g.N * g.OH * g.OW
    if P < 4096 or not pow2(g.OW) or not pow2(g.OH * g.OW):
        return -1
    if g.N * g.H * g.W * g.C >= CAP or P * g.K >= CAP:
        return -1
    return (0 if g.C % 128 == 0 else 2) + (0 if g.K % 128 == 0 else 1)


WG_TILE = {0: (128, 128, 2), 1: (128, 64, 3), 2: (64, 128, 3), 3: (64, 64, 3)}        # BM, BN, NBUF


def wgrad_bf16r_plan(g, force=0):
    """the split count of the cost model (microseconds: dispatch rounds x (stages x 0.7 x tile / 128^2 + 6) + partials at 4 TB/s);
    0: not served.  force: PNP_BF16R_WSPLIT"""
    tile = wgrad_bf16r_tile(g)
    if tile < 0:
        return 0
    bm, bn, _ = WG_TILE[tile]
    nblk = (g.R * g.S * g.C // bm) * (g.K // bn)
    if force > 0:
        return force
    nchunks = cdiv(g.N * g.OH * g.OW, CHUNK)
    t_stage = 0.7 * (bm * bn) / (128.0 * 128.0)
    nout_mb = float(g.R * g.S * g.C * g.K) * 4.0 / 1e6
    best, best_t = 1, 1e30
    for ns in range(1, max(1, min(nchunks // 4, 64)) + 1):
        rounds = math.ceil(nblk * ns / 512.0)
        t = rounds * (math.ceil(nchunks / ns) * t_stage + 6.0) + (2.0 * ns * nout_mb / 4.0 + 3.0 if ns > 1 else 0.0)
        if t < best_t - 1e-9:
            best_t, best = t, ns
    return best


def wgrad_launch(g, ws_bytes, force=0):
    """pnp_conv2d_wgrad_bf16r with a workspace of ws_bytes -> dict(sym, planned, ns, per, total): as many of the planned partials as fit, a
    single one is no split; ns parts of `per` chunks, the last one shorter when ns * per != total"""
    bm, bn, nbuf = WG_TILE[wgrad_bf16r_tile(g)]
    planned = ns = wgrad_bf16r_plan(g, force)
    nout = g.R * g.S * g.C * g.K
    if ns > 1 and ws_bytes < ns * nout * 4:
        ns = ws_bytes // (nout * 4)
        if ns < 2:
            ns = 1
    total = cdiv(g.N * g.OH * g.OW, CHUNK)
    per = cdiv(total, ns)
    ns = cdiv(total, per)
    return dict(sym="conv_wgrad_bf16r_kernel<%d, %d, 2, 2, %d>" % (bm, bn, nbuf), planned=planned, ns=ns, per=per, total=total)


CONV_TILE = {0: (256, 128, 4, 2, 3), 1: (128, 128, 2, 2, 2), 2: (128, 64, 2, 2, 3)}         # BM, BN, WM, WN, NBUF
INSTANCE_SHAPES = {0: [(3, 3), (5, 5)], 1: [(3, 3), (1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 2)]}      # launch_tile's PNP_R lists


def conv_symbol(tile, bkc, kind, R, S):
    bm, bn, wm, wn, nbuf = CONV_TILE[tile]
    return "conv_bf16r_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d, 1>" % (bm, bn, wm, wn, bkc, kind, R, S, nbuf)


def all_conv_instances(tile):
    """every instance launch_kind / launch_tile can emit on one tile: 3x3 and (forward) 5x5 at both BKC, the stride-phase sub-filters at BKC 64"""
    out = []
    for kind in (0, 1):
        for (R, S) in INSTANCE_SHAPES[kind]:
            for bkc in ((64, 32) if (R, S) in ((3, 3), (5, 5)) else (64,)):
                out.append(conv_symbol(tile, bkc, kind, R, S))
    return out


def conv_launch(M, outc, red, kind, R, S, OW, OHW, force):
    """launch_kind<KIND> + launch_tile of one resident convolution with M output rows -> dict(sym, tile, nst, nbuf, tags)"""
    tile = plan_tile(M, outc, force)
    forced = force >= 0 and tile != plan_tile(M, outc)
    bkc = 64 if red % 64 == 0 else 32
    assert (R, S) in INSTANCE_SHAPES[kind] and (bkc == 64 or (R, S) in ((3, 3), (5, 5))), (kind, R, S, bkc)
    bm, nbuf = CONV_TILE[tile][0], CONV_TILE[tile][4]
    nst = (red // bkc) * R * S
    sym = conv_symbol(tile, bkc, kind, R, S)
    pre = "forced " if forced else ""
    tags = {pre + sym}
    if nst % nbuf:
        tags.add("%snst %% NBUF = %d" % (pre, nst % nbuf))
    if nst < nbuf - 1:
        tags.add(pre + "nst < NBUF - 1")
    if M % bm:
        tags.add("%sragged M kind %d" % (pre, kind))
        if tile == 0:
            tags.add("ragged last 256x128 tile")
    if not (pow2(OW) and pow2(OHW)):
        tags.add("%snon-power-of-two map kind %d" % (pre, kind))
    return dict(sym=sym, tile=tile, bkc=bkc, nst=nst, nbuf=nbuf, tags=tags, M=M)


def rplan(case, kind, force_tile=-1, force_split=0):
    """the resident plan of one pass (0 forward, 1 data gradient, 2 filter gradient) -> None (not served) or
    dict(symbols {symbol: launches}, tags, launches)"""
    g = H.geom_of(case)
    if kind == 2:
        if wgrad_bf16r_tile(g) < 0:
            return None
        ns = wgrad_bf16r_plan(g, force_split)
        L = wgrad_launch(g, ns * g.R * g.S * g.C * g.K * 4 if ns > 1 else 0, force_split)
        tags = {L["sym"], "resident wgrad split" if L["ns"] > 1 else "unsplit"}
        if L["ns"] > 1 and L["ns"] * L["per"] != L["total"]:
            tags.add("split with a short last part")
        return dict(symbols={L["sym"]: 1}, tags=tags, launches=[L], nsplit=ns)
    if not served(g, kind):
        return None
    if kind == 0:
        Ls = [conv_launch(g.N * g.OH * g.OW, g.K, g.C, 0, g.R, g.S, g.OW, g.OH * g.OW, force_tile)]
    elif g.stride == 1:
        Ls = [conv_launch(g.N * g.H * g.W, g.C, g.K, 1, g.R, g.S, g.W, g.H * g.W, force_tile)]
    else:
        ph = [p for p in H.plan_phases(g) if p["I"] * p["J"] > 0]
        Ls = [conv_launch(g.N * p["I"] * p["J"], g.C, g.K, 1, p["T"], p["U"], p["J"], p["I"] * p["J"], force_tile) for p in ph]
    symbols, tags = {}, set()
    for L in Ls:
        symbols[L["sym"]] = symbols.get(L["sym"], 0) + 1
        tags |= L["tags"]
    if len(Ls) > 1 and len({L["M"] for L in Ls}) > 1:
        tags.add("ragged stride phases")
    return dict(symbols=symbols, tags=tags, launches=Ls)


def stats_parts(case, force=-1):
    g = H.geom_of(case)
    if not served(g, 0):
        return 0
    M = g.N * g.OH * g.OW
    tile = plan_tile(M, g.K, force)
    return cdiv(M, 256 if tile == 0 else 128) * (4 if tile == 0 else 2)


# ---- the staged family: test_igemm_domain_host.plan with the two substitutions -----------------------------------------------------------
def _wgrad_lin_vecb(g):
    """`lin && VECB` of launch_wgrad_tile: the linear pixel walk (stride 1, rows of >= 32 pixels) on a vector-B tile"""
    rows_ok = g.OW >= H.BK or (H.BK % g.OW == 0 and g.OH > H.BK // g.OW and (g.OH * g.OW) % H.BK == 0)
    lin = (not g.sym) and g.C % 4 == 0 and rows_ok and g.stride == 1 and g.OW >= H.BK
    return lin and H.ring_tile(g.K) != 3


def bf16_plan(case, kind, drop=False):
    """test_igemm_domain_host.plan for a geometry with dtype = PNP_DTYPE_BF16 -> the same dict with the bf16 symbols in place, `bf16`
    (did any symbol change) and tags prefixed "staged\""""
    p = dict(H.plan(case, kind, drop=drop) if kind == 0 else H.plan(case, kind))
    g = H.geom_of(case)
    names, tags = [], set()
    if kind == 2:
        if p["route"] == H.RING and _wgrad_lin_vecb(g):
            L = p["launches"][0]
            names = ["conv_wgrad_bf16_kernel<%s>" % H.TILE_ARGS[H.ring_tile(g.K)]]
            tags = {names[0], "staged wgrad split" if L["ns"] > 1 else "staged wgrad unsplit"}
    elif p["launches"] and "taps" in p["launches"][0]:
        syms = []
        for L in p["launches"]:
            if L["taps"]:
                s = re.sub(r"^conv_taps3?_kernel<", "conv_taps_bf16_kernel<", L["sym"])
                tags |= {s, "staged taps split" if L["ns"] > 1 else "staged taps unsplit"}
                if L["reducer"]:
                    tags.add("staged " + L["reducer"])
                syms.append(s)
            else:
                syms.append(L["sym"])
        if tags:
            names = sorted(set(syms))
    p["bf16"] = bool(tags)
    if tags:
        p["symbols"] = names
    p["tags"] = tags
    return p


def bf16_expected(case, kind):
    """(route, symbols, nsplit) of the pass for dtype = PNP_DTYPE_BF16 with the Winograd and split-bf16 switches at 0"""
    p = bf16_plan(case, kind)
    return p["route"], p["symbols"], p["nsplit"]


STAGED = H.FWD + H.STRIDED + H.WGRAD
# forward cases the GPU file also runs with dropout: the reduction-split taps launch leaves dropout to split_sum::serial_kernel<Drop>
STAGED_DROPOUT = [c for c in H.DROPOUT if bf16_plan(c, 0, drop=True)["bf16"]]


# ---- REQUIRED -------------------------------------------------------------------------------------------------------------------------
_KINDS = (0, 1)
REQUIRED = (
    # tile 2 (128x64): every instance under the planner
    all_conv_instances(2)
    # tile 0 (256x128): every instance under PNP_BF16R_TILE=0 at minimum size, and the forward the table reaches under the planner (a
    # planner-chosen 256x128 data gradient needs >= 256 tiles: tests/test_gpu_bf16r.py has it at (16, 64, 64, 128 -> 128))
    + [conv_symbol(0, 32, 0, 3, 3), conv_symbol(0, 64, 0, 3, 3)] + ["forced " + s for s in all_conv_instances(0)]
    # tile 1 (128x128, NBUF = 2): forced-only
    + ["forced " + s for s in all_conv_instances(1)]
    + ["conv_wgrad_bf16r_kernel<%d, %d, 2, 2, %d>" % WG_TILE[t] for t in range(4)]
    + ["resident wgrad split", "split with a short last part", "unsplit"]
    + ["nst % NBUF = 1", "nst % NBUF = 2", "nst < NBUF - 1", "forced nst % NBUF = 1"]
    + ["ragged M kind %d" % k for k in _KINDS] + ["non-power-of-two map kind %d" % k for k in _KINDS]
    + ["forced ragged M kind %d" % k for k in _KINDS] + ["forced non-power-of-two map kind %d" % k for k in _KINDS]
    + ["ragged last 256x128 tile", "ragged stride phases"]
    # the staged family: the image of test_igemm_domain_host.REQUIRED's taps and ring entries
    + sorted({re.sub(r"^conv_taps3?_kernel<", "conv_taps_bf16_kernel<", s) for s in H.REQUIRED if s.startswith("conv_taps")})
    + ["conv_wgrad_bf16_kernel<128, 128, 2, 2>", "conv_wgrad_bf16_kernel<128, 64, 2, 2>", "conv_wgrad_bf16_kernel<128, 32, 4, 1>"]
    + ["staged taps split", "staged taps unsplit", "staged wgrad split", "staged wgrad unsplit",
       "staged split_sum::serial_kernel<Plain>", "staged split_sum::serial_kernel<Drop>", "staged split_sum::serial_kernel<Scatter>"]
)


def tags_of_tables():
    tags = set()
    for case in RESIDENT + EPILOGUE:
        for kind in ((0, 1, 2) if case in RESIDENT else (0,)):
            p = rplan(case, kind)
            if p:
                tags |= p["tags"]
    for force in (0, 1, 2):
        for case in FORCED:
            for kind in (0, 1):
                p = rplan(case, kind, force_tile=force)
                if p:
                    tags |= {t for t in p["tags"] if t.startswith("forced ")}
    tags |= rplan(WSPLIT_ROW, 2, force_split=WSPLIT)["tags"]
    for case, room in FALLBACK:
        g = H.geom_of(case)
        L = wgrad_launch(g, 0 if room is None else int(room * g.R * g.S * g.C * g.K * 4))
        tags.add("resident wgrad split" if L["ns"] > 1 else "unsplit")
    for case in STAGED:
        for kind in (0, 1, 2):
            tags |= bf16_plan(case, kind)["tags"]
    for case in STAGED_DROPOUT:
        tags |= bf16_plan(case, 0, drop=True)["tags"]
    for case in STAGED_FALLBACK:
        assert bf16_plan(case, 2)["bf16"] and H.ring_launch(H.geom_of(case), 0)["ns"] == 1, case
        tags.add("staged wgrad unsplit")
    return tags


def test_the_tables_reach_every_required_variant():
    tags = tags_of_tables()
    missing = [t for t in REQUIRED if t not in tags]
    assert not missing, missing
    # the 128x128 instance is reached by forcing only, and every instance of the other two tiles is in REQUIRED
    assert not [t for t in tags if t.startswith("conv_bf16r_kernel<128, 128,")]
    assert len(set(REQUIRED)) == len(REQUIRED)


def test_table_anchors():
    """what the tables' comments claim, spelled out"""
    nst = lambda c, k: sorted(L["nst"] for L in rplan(c, k)["launches"])
    assert nst(RESIDENT[0], 0) == [9] and nst(row(1, 64, 64, 64, 64, 5, 1, 1, "SAME"), 0) == [25]
    assert nst(row(1, 64, 64, 128, 64, 5, 1, 1, "SAME"), 0) == [50]
    assert nst(row(4, 64, 64, 64, 64, 3, 2, 1, "SAME"), 1) == [1, 2, 2, 4] and nst(row(4, 64, 64, 64, 128, 3, 2, 1, "SAME"), 1) == [2, 4, 4, 8]
    assert sorted(rplan(row(4, 64, 64, 64, 64, 5, 2, 1, "SAME"), 1)["symbols"]) == sorted(conv_symbol(2, 64, 1, r, s) for (r, s) in ((2, 2), (2, 3), (3, 2), (3, 3)))
    p = rplan(row(4, 128, 128, 64, 64, 5, 4, 1, "SAME"), 1)
    assert sum(p["symbols"].values()) == 16 and p["symbols"][conv_symbol(2, 64, 1, 1, 1)] == 9 and p["symbols"][conv_symbol(2, 64, 1, 2, 2)] == 1
    assert sorted(L["M"] for L in rplan(row(4, 65, 65, 64, 64, 3, 2, 1, "SAME"), 1)["launches"]) == [4096, 4224, 4224, 4356]
    c = row(1, 66, 66, 32, 2560, 3, 1, 1, "VALID")
    assert rplan(c, 0)["launches"][0]["tile"] == 0 and cdiv(4096, 256) * (2560 // 128) == 320 and stats_parts(c) == 16 * 4
    assert rplan(c, 1) is None and rplan(c, 2) is None
    c = row(1, 69, 69, 64, 2560, 3, 1, 1, "VALID")
    assert rplan(c, 0)["launches"][0]["tile"] == 0 and 67 * 67 == 4489 and stats_parts(c) == 18 * 4
    assert rplan(row(2, 48, 48, 64, 96, 3, 1, 1, "SAME"), 0) is None
    assert list(rplan(row(2, 48, 48, 64, 96, 3, 1, 1, "SAME"), 1)["symbols"]) == [conv_symbol(2, 32, 1, 3, 3)]
    assert [wgrad_bf16r_tile(H.geom_of(row(1, 64, 64, C, K, 3, 1, 1, "SAME"))) for C in (128, 64) for K in (128, 64)] == [0, 1, 2, 3]
    L = rplan(WSPLIT_ROW, 2, force_split=WSPLIT)["launches"][0]
    assert (L["ns"], L["per"], L["total"]) == (3, 22, 64)
    for c, room in FALLBACK:
        g = H.geom_of(c)
        assert wgrad_bf16r_plan(g) >= 3, (c, wgrad_bf16r_plan(g))
    for c in EPILOGUE:
        assert rplan(c, 0) is not None
    assert sorted((L["tile"], L["bkc"]) for L in (rplan(c, 0)["launches"][0] for c in EPILOGUE)) == [(0, 32), (0, 64), (2, 32), (2, 64)]
    assert [H.geom_of(c).N * H.geom_of(c).OH * H.geom_of(c).OW % (256 if rplan(c, 0)["launches"][0]["tile"] == 0 else 128) != 0 for c in EPILOGUE] == [False, True, False, True]
    for c in FORCED:                      # every forced row keeps each reference under a GMAC or so and has 128-groups to force
        g = H.geom_of(c)
        assert g.K % 128 == 0 or g.C % 128 == 0
        assert g.N * g.OH * g.OW * g.R * g.S * g.C * g.K < 2.5e9
    for c in RESIDENT + EPILOGUE:
        g = H.geom_of(c)
        assert g.N * g.OH * g.OW * g.R * g.S * g.C * g.K < 11e9, c


# ---- against the library ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def lib_(built):
    return pkg("kernels"), pkg("_lib").load()


def lib_geom(K, case, bf16=True):
    N, Hh, W, C, Kf, R, S, st, dil, padding = case
    return K.conv_geom((N, Hh, W, C), (R, S, C, Kf), st, dil, padding, dtype=pkg("_lib").DTYPE_BF16 if bf16 else pkg("_lib").DTYPE_F32)


def _queries(lib, g):
    return ([int(lib.pnp_conv2d_bf16r_served(ctypes.byref(g), k)) for k in (0, 1, 2)], int(lib.pnp_conv2d_fwd_bf16r_stats_parts(ctypes.byref(g))),
            int(lib.pnp_conv2d_wgrad_bf16r_workspace_bytes(ctypes.byref(g))))


def _restated(r):
    ns = wgrad_bf16r_plan(r)
    M = r.N * r.OH * r.OW
    tile = plan_tile(M, r.K)
    parts = cdiv(M, 256 if tile == 0 else 128) * (4 if tile == 0 else 2) if served(r, 0) else 0
    return ([int(served(r, 0)), int(served(r, 1)), int(wgrad_bf16r_tile(r) >= 0)], parts, ns * r.R * r.S * r.C * r.K * 4 if ns > 1 else 0)


def test_restatement_against_the_queries_for_every_row(lib_):
    K, lib = lib_
    for case in ALL + [c for c, _ in FALLBACK] + STAGED:
        g, r = lib_geom(K, case), H.geom_of(case)
        assert (g.OH, g.OW, g.pad_t, g.pad_l) == (r.OH, r.OW, r.pad_t, r.pad_l), case
        assert _queries(lib, g) == _restated(r), (case, _queries(lib, g), _restated(r))
        for kind in (0, 1, 2):
            assert (rplan(case, kind) is not None) == bool(_queries(lib, g)[0][kind]), (case, kind)


# (row, what the three served queries must say) — queries only, nothing is allocated
BOUNDARY = [
    (row(1, 63, 65, 64, 64, 3, 1, 1, "SAME"), [0, 0, 0]),            # M = 4095: one pixel under the floor ...
    (row(1, 64, 64, 64, 64, 3, 1, 1, "SAME"), [1, 1, 1]),            # ... and M = 4096
    (row(1, 64, 64, 64, 96, 3, 1, 1, "SAME"), [0, 1, 0]),            # K % 64 just off: the data gradient reduces over K in 32-groups
    (row(1, 64, 64, 64, 48, 3, 1, 1, "SAME"), [0, 0, 0]),            # K % 32 off too
    (row(1, 64, 64, 48, 64, 3, 1, 1, "SAME"), [0, 0, 0]),            # C % 32 just off
    (row(1, 64, 64, 32, 64, 3, 1, 1, "SAME"), [1, 0, 0]),            # C = 32: forward only
    (row(1, 64, 64, 64, 64, 5, 1, 1, "SAME"), [1, 0, 1]),            # a 5x5 stride-1 data gradient is refused
    (row(3, 37, 41, 64, 64, 3, 1, 1, "SAME"), [1, 1, 0]),            # non-power-of-two OW: no resident filter gradient
    (row(2, 48, 64, 64, 64, 3, 1, 1, "SAME"), [1, 1, 0]),            # power-of-two OW, OH OW not
    (row(1, 64, 64, 64, 64, 3, 1, 1, "SYMMETRIC"), [0, 0, 0]),       # mirror padding
    (row(64, 512, 512, 64, 64, 3, 1, 1, "SAME"), [0, 0, 0]),         # 2^30 elements exactly: the cap ...
    (row(63, 512, 512, 64, 64, 3, 1, 1, "SAME"), [1, 1, 1]),         # ... and just under it (N need not be a power of two: only OW and OH OW)
    (row(4, 63, 63, 64, 64, 3, 2, 1, "SAME"), [1, 0, 1]),            # strided data gradient: one phase has 4 x 31 x 31 = 3844 pixels (the forward has 4096)
    (row(4, 65, 65, 64, 64, 3, 2, 1, "SAME"), [1, 1, 0]),            # strided: the smallest phase has exactly 4096
    (row(4, 64, 64, 64, 96, 3, 2, 1, "SAME"), [0, 0, 0]),            # strided data gradient: K in whole 64-groups
    (row(4, 128, 128, 64, 64, 7, 2, 1, "SAME"), [0, 0, 1]),          # 7x7 stride 2: 4x4 sub-filters are no instance
    (row(4, 64, 64, 64, 64, 3, 2, 2, "SAME"), [1, 0, 1]),            # stride 2 with dilation 2: no phases
]


def test_boundary_rows_against_the_queries(lib_):
    K, lib = lib_
    for case, want in BOUNDARY:
        g, r = lib_geom(K, case), H.geom_of(case)
        got = _queries(lib, g)
        assert got == _restated(r), (case, got, _restated(r))
        assert got[0] == want, (case, got[0], want)
    # dil (R - 1) < pad_t: a geometry conv_geom never makes (more padding than the filter reaches) — no data gradient
    g, r = lib_geom(K, RESIDENT[0]), H.geom_of(RESIDENT[0])
    g.pad_t = r.pad_t = 3
    assert _queries(lib, g) == _restated(r) and _queries(lib, g)[0] == [1, 0, 1]
    g.pad_t = r.pad_t = 2
    assert _queries(lib, g) == _restated(r) and _queries(lib, g)[0] == [1, 1, 1]


def test_resident_128x128_tile_is_unreachable_from_the_planner():
    """plan_tile takes tile 1 when K % 128 == 0, cdiv(M, 256) (K / 128) < 256 and cdiv(M, 128) (K / 128) >= 512.  But
    cdiv(M, 128) <= 2 cdiv(M, 256) (256 cdiv(M, 256) >= M gives 128 (2 cdiv(M, 256)) >= M), so cdiv(M, 128) k >= 512 implies
    cdiv(M, 256) k >= 256: tile 0 always wins first and conv_bf16r_kernel<128, 128, 2, 2, ..., 2, 1> (NBUF = 2) is compiled, routed and
    never launched without PNP_BF16R_TILE=1.  Exhaustive over K = 64 .. 8192 in steps of 64 and every M = 1 .. 2^20.
    If this test fails someone moved a threshold and made the tile reachable: add RESIDENT rows that reach it under the planner and move
    its "forced ..." tags of REQUIRED to plain ones."""
    M = np.arange(1, (1 << 20) + 1, dtype=np.int64)
    m256, m128 = -(-M // 256), -(-M // 128)
    for K in range(64, 8192 + 1, 64):
        if K % 128:
            assert plan_tile(4096, K) == 2 and plan_tile(1 << 20, K) == 2
            continue
        k = K // 128
        tile = np.where(m256 * k >= 256, 0, np.where(m128 * k >= 512, 1, 2))
        assert not bool((tile == 1).any()), K
    for (Mi, K) in ((4096, 128), (65536, 128), (65280, 128), (4096, 2560), (3329, 2560), (3328, 2560), (300000, 4096)):          # the vector form is plan_tile
        k = K // 128
        assert plan_tile(Mi, K) == (0 if cdiv(Mi, 256) * k >= 256 else (1 if cdiv(Mi, 128) * k >= 512 else 2))
        assert plan_tile(Mi, K) != 1


def test_staged_routes_and_split_counts_do_not_depend_on_the_dtype(built):
    """conv_bf16.hip: "PNP_DTYPE_BF16 in a geometry PERMITS bf16 operands" — route, workspace and split count are the fp32 planner's"""
    K, lib = pkg("kernels"), pkg("_lib").load()
    prev = (K.wino_mode(0), K.wino_wgrad_mode(0), K.x3_direct(0), K.x3_strided(0), K.x3_wgrad(0))
    try:
        for case in STAGED:
            gb, gf = lib_geom(K, case), lib_geom(K, case, bf16=False)
            for kind in (0, 1, 2):
                assert K.conv_route(gb, kind) == K.conv_route(gf, kind) == bf16_expected(case, kind)[0], (case, kind)
            for q in (lib.pnp_conv2d_fwd_workspace_bytes, lib.pnp_conv2d_dgrad_workspace_bytes, lib.pnp_conv2d_wgrad_workspace_bytes):
                assert int(q(ctypes.byref(gb))) == int(q(ctypes.byref(gf))), case
    finally:
        K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.x3_direct(prev[2]); K.x3_strided(prev[3]); K.x3_wgrad(prev[4])


def test_staged_symbols_change_only_where_the_header_says():
    for case in STAGED:
        for kind in (0, 1, 2):
            p, b = H.plan(case, kind), bf16_plan(case, kind)
            assert (p["route"], p["nsplit"], p["ws_bytes"]) == (b["route"], b["nsplit"], b["ws_bytes"])
            if b["bf16"]:
                assert any("bf16" in s for s in b["symbols"]) and p["route"] in (H.IGEMM, H.PHASES, H.RING), (case, kind)
                assert not any(s.startswith("conv_taps") and "bf16" not in s for s in b["symbols"]), (case, kind)
            else:
                assert p["symbols"] == b["symbols"] and not any(s.startswith("conv_taps") for s in p["symbols"]), (case, kind)
    # anchors
    assert bf16_expected((2, 68, 68, 64, 96, 3, 3, 1, 1, "VALID"), 0)[1] == ["conv_taps_bf16_kernel<128, 64, 2, 2, 0, 3, 3>"]
    assert bf16_expected((2, 16, 16, 64, 64, 3, 3, 2, 1, "SAME"), 1)[1] == ["conv_dgrad_phases_kernel<128, 32, 4, 1>"]
    assert bf16_expected((2, 33, 45, 64, 96, 3, 3, 1, 1, "SAME"), 2)[1] == ["conv_wgrad_bf16_kernel<128, 128, 2, 2>"]
    assert bf16_expected((2, 67, 65, 32, 48, 3, 3, 2, 1, "SAME"), 2)[1] == ["conv_wgrad_ring_kernel<128, 64, 2, 2, 2>"]          # strided: fp32
    assert bf16_expected((1, 32, 16, 64, 32, 3, 3, 1, 1, "SAME"), 2)[1] == ["conv_wgrad_ring_kernel<128, 32, 4, 1, 2>"]          # short rows: fp32
    assert bf16_expected((2, 64, 64, 16, 16, 3, 3, 1, 1, "SAME"), 0)[1] == ["conv_n16_kernel<16, 0>"]
