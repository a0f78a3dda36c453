"""not gpu: the domain of the Winograd route (csrc/conv_wino.hip, csrc/conv_wino_x3.hip) as tests/test_gpu_wino_domain.py walks it.

Two things live here, both without a GPU:

1. `expected_tile(case, kind, tile, x3)`: a Python restatement of the route's planner with both route switches at 2 ("wherever the geometry
   allows") — eligible_dims (stride-1 3x3, dil 1 / 2, padding 0 / dil / 2 dil, extents divisible by dil, C % 32 == 0, K % 4 == 0, K >= 32),
   the F(4x4) cap of the fp32 pipe (reductions over > 1 024 channels fall to F(2x2)) and the C % 64 condition under which the split-bf16
   GEMM takes a forward / data-gradient launch (and with it lifts the cap).  It is held to pnp_conv2d_wino_chosen of the built library (a host
   function) for every row of the GPU file's tables, in all four arithmetics and all three passes; the GPU file imports it (and the tables)
   from here, so a reader of a GPU log can tell without a GPU which launches the route owns.  `wgrad_splits` derives the reduction-split
   count of a filter-gradient launch from pnp_conv2d_wgrad_workspace_bytes — also a host function, so the split properties the GPU file
   relies on (more than one split on both shapes, a ragged last split on the second) are asserted here as well.

2. The yardstick of the GPU file's wide-operand test is the project's own restatement of the algorithm, oracle.tf_ops.conv3x3_winograd_np
   and wgrad3x3_winograd_np.  In float64 they must BE the convolution: forward, data gradient (flip_transpose on dy, padding 2 dil - pad:
   this includes padding 2 dil with dil = 2, which tests/test_host.py does not reach) and filter gradient equal the float64 convolution and
   its autograd gradients to 1e-10 of max|ref| at every table shape, for m in {2, 4}."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import tf_ops as T

# (N, H, W, C, K, dil, padding): table (a) of tests/test_gpu_wino_domain.py — the smallest shapes that reach each place
SHAPES = [
    (1, 3, 3, 32, 32, 1, "VALID"),         # one output pixel, T = 1, minimum C and K; data gradient: padding 2 on a 1x1 map
    (1, 2, 2, 64, 64, 1, "SAME"),          # a map smaller than an F(4x4) tile; split-bf16 operands with T = 1
    (3, 5, 7, 32, 36, 1, "SAME"),          # K = 36: nine channel quads, a ragged 32-column filter tile; the data gradient is refused (K % 32)
    (2, 6, 10, 64, 100, 1, "SAME"),        # K = 100 inside one 128-wide GEMM block; the split-bf16 forward runs (C = 64); no data gradient (K % 32)
    (1, 7, 9, 96, 132, 1, "VALID"),        # the second GEMM column block is 4 wide; C = 96: no split-bf16 forward; no data gradient (K % 32)
    (1, 8, 12, 64, 64, 2, "VALID"),        # dilation 2 with padding 0; its data gradient: padding 4 (ps = 2 on the sub-images)
    (2, 4, 4, 64, 32, 2, "SAME"),          # 2x2 sub-images, each smaller than a tile
    (1, 2, 130, 32, 32, 1, "SAME"),        # one tile row of 65 (F(2x2)) / 33 (F(4x4)) tile columns
    (130, 2, 2, 32, 32, 1, "SAME"),        # T = 130: the 128-row GEMM tile boundary falls between images
    (1, 4, 4, 1056, 32, 1, "SAME"),        # C > 1 024 and C % 64 != 0: the forward falls to F(2x2) in both F(4x4) arithmetics
    (1, 4, 4, 1088, 32, 1, "SAME"),        # C = 17 x 64: F(4x4) on split-bf16 keeps tile 4 (17 accumulation chunks), the fp32 pipe falls to 2
]
# table (b): filter-gradient reduction splits (the second: T = 3 069 / 816 tiles, a ragged last chunk; K = 36)
SPLITS = [(4, 64, 64, 32, 32, 1, "SAME"), (3, 62, 66, 32, 36, 1, "SAME")]
# table (c): wide operands and exact zeros
WIDE = [(2, 12, 20, 64, 64, 1, "SAME"), (1, 8, 12, 64, 64, 2, "VALID")]
# (largest output tile, split-bf16 GEMMs?) — the four arithmetics of the route
ARITH = [(2, 0), (4, 0), (2, 1), (4, 1)]
ARITH_IDS = ["F2x2", "F4x4", "F2x2-x3", "F4x4-x3"]


def case_id(c):
    return "x".join(str(v) for v in c)


def _pad(case):
    return case[5] if case[6] == "SAME" else 0


def as_conv(case, kind):
    """(N, H, W, C, K, dil, pad, OH, OW) of the stride-1 zero-padded convolution a pass is for the planner: the layer itself (forward,
    filter gradient) or the convolution of dy that its data gradient is (channels and filters swapped, padding 2 dil - pad)"""
    N, H, W, C, K, dil, _ = case
    pad = _pad(case)
    OH, OW = H + 2 * pad - 2 * dil, W + 2 * pad - 2 * dil
    if kind == 1:
        return N, OH, OW, K, C, dil, 2 * dil - pad, H, W
    return N, H, W, C, K, dil, pad, OH, OW


def tiles(case, kind, m):
    """tile count of the pass on F(m x m): every dilation phase's OUTPUT sub-image cut into m x m tiles (make_wgeom)"""
    N, H, W, C, K, dil, pad, OH, OW = as_conv(case, kind)
    return N * dil * dil * (-(-(OH // dil) // m)) * (-(-(OW // dil) // m))


def eligible(case, kind, m):
    """eligible_dims of csrc/conv_wino.hip for a float32 stride-1 3x3 zero-padded layer"""
    N, H, W, C, K, dil, pad, OH, OW = as_conv(case, kind)
    if OH <= 0 or OW <= 0 or dil not in (1, 2) or pad % dil != 0 or not 0 <= pad <= 2 * dil:
        return False
    if H % dil or W % dil or OH % dil or OW % dil:
        return False
    if C % 32 or K % 4 or K < 32:
        return False
    Tn = tiles(case, kind, m)
    return Tn * C < (1 << 29) and Tn * K < (1 << 29) and C * K < (1 << 29)


def x3_gemm(case, kind, m, x3):
    """does the GEMM of this pass run on split-bf16 operands (x3 = mode 2: wherever the shapes allow)?  Forward / data gradient: a reduction
    over a multiple of 64 channels, every operand under one 2 GiB buffer descriptor; filter gradient: the reduction runs over the tiles,
    padded to a multiple of 64 — always"""
    if not x3:
        return False
    N, H, W, C, K, dil, pad, OH, OW = as_conv(case, kind)
    Tn = tiles(case, kind, m)
    if kind == 2:
        Tp = (Tn + 63) & ~63
        return 36.0 * max(C, K) * Tp * 6.0 < 2.0 ** 31
    return C % 64 == 0 and 36.0 * Tn * C * 6.0 < 2.0 ** 31 and 36.0 * K * C * 6.0 < 2.0 ** 31


def expected_tile(case, kind, tile, x3):
    """pnp_conv2d_wino_chosen(g, kind) with wino_mode = wino_wgrad_mode = 2, wino_tile = tile, wino_x3 = 2 if x3 else 0: the output tile
    edge (2 / 4) of the launch, 0 = the direct kernels.  kind 0 forward, 1 data gradient, 2 filter gradient."""
    for m in range(tile, 0, -2):
        if not eligible(case, kind, m):
            continue
        C = as_conv(case, kind)[3]
        if m == 4 and kind != 2 and C > 1024 and not x3_gemm(case, kind, m, x3):      # fp32 pipe: F(4x4) stays under 1 024-channel reductions
            continue
        return m
    return 0


def al256(b):
    return (b + 255) & ~255


def wgrad_splits(ws_bytes, case, m, x3):
    """reduction splits of the route's filter-gradient launch, from the bytes pnp_conv2d_wgrad_workspace_bytes asks for:
    [transformed x: np T C] [transformed dy: np T K] [ns partial products: np C K fp32], each rounded up to 256 bytes; operands fp32, or
    (x3) three bf16 planes = 6 bytes over the tiles padded to a multiple of 64.  Returns (ns, chunks per split, chunks): a chunk is one
    GEMM stage of 32 tiles (x3: an accumulation chunk of 64)"""
    N, H, W, C, K, dil, pad, OH, OW = as_conv(case, 2)
    npos, Tn = (m + 2) ** 2, tiles(case, 2, m)
    Tp, eb = ((Tn + 63) & ~63, 6) if x3 else (Tn, 4)
    rest = ws_bytes - al256(npos * Tp * C * eb) - al256(npos * Tp * K * eb)
    per = npos * C * K * 4
    assert rest > 0 and per % 256 == 0 and rest % per == 0, (ws_bytes, rest, per)
    ns = rest // per
    chunks = Tp // 64 if x3 else -(-Tn // 32)
    cps = -(-chunks // ns)
    assert -(-chunks // cps) == ns, (chunks, ns)          # (the planner only keeps split counts that every split really gets work from)
    return ns, cps, chunks


@pytest.fixture
def planner(built):
    """the route switches of tests/test_gpu_wino.py's `wino` fixture: call with (tile, x3) -> both route modes at 2; restored afterwards"""
    K = pkg("kernels")
    prev = (K.wino_mode(-1), K.wino_wgrad_mode(-1), K.wino_tile(-1), K.wino_x3(-1))

    def setter(tile, x3):
        K.wino_mode(2); K.wino_wgrad_mode(2); K.wino_tile(tile); K.wino_x3(2 if x3 else 0)
        return K
    yield setter
    K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.wino_tile(prev[2]); K.wino_x3(prev[3])


def geom(K, case):
    N, H, W, C, Kf, dil, padding = case
    return K.conv_geom((N, H, W, C), (3, 3, C, Kf), 1, dil, padding)


def test_restated_planner_against_the_library_for_every_gpu_row(planner):
    for (tile, x3) in ARITH:
        K = planner(tile, x3)
        for case in SHAPES + SPLITS + WIDE:
            g = geom(K, case)
            for kind in (0, 1, 2):
                assert K.wino_chosen(g, kind) == expected_tile(case, kind, tile, x3), (case, kind, tile, x3)


def test_restated_planner_anchors(planner):
    """what the tables' comments claim, spelled out (so that the restatement and the library cannot drift together unnoticed), and a few
    layers just outside the domain"""
    k36, c1056, c1088 = SHAPES[2], SHAPES[9], SHAPES[10]
    for (tile, x3) in ARITH:
        assert [expected_tile(k36, kind, tile, x3) for kind in (0, 1, 2)] == [tile, 0, tile]          # K % 32 != 0: no data gradient
        assert expected_tile(c1056, 0, tile, x3) == 2 and expected_tile(c1056, 1, tile, x3) == tile and expected_tile(c1056, 2, tile, x3) == tile
        assert expected_tile(c1088, 0, tile, x3) == (4 if (tile == 4 and x3) else 2)
        for case in SHAPES + SPLITS + WIDE:          # everything else is on the route, but for the data gradients over K = 36 / 100 / 132 filters
            assert expected_tile(case, 0, tile, x3) in (2, tile) and expected_tile(case, 2, tile, x3) == tile, case
            assert expected_tile(case, 1, tile, x3) == (tile if case[4] % 32 == 0 else 0), case
    assert [tiles(SHAPES[0], 0, m) for m in (2, 4)] == [1, 1] and [tiles(SHAPES[1], 0, m) for m in (2, 4)] == [1, 1]
    assert [tiles(SHAPES[7], 0, m) for m in (2, 4)] == [65, 33] and tiles(SHAPES[8], 0, 4) == 130
    assert [tiles(SPLITS[1], 2, m) for m in (2, 4)] == [3069, 816]
    assert as_conv(SHAPES[5], 1)[6] == 4 and as_conv(SHAPES[0], 1)[6] == 2                             # data-gradient paddings 2 dil
    assert x3_gemm(SHAPES[3], 0, 4, 1) and not x3_gemm(SHAPES[3], 1, 4, 1) and not x3_gemm(SHAPES[4], 0, 4, 1) and x3_gemm(k36, 2, 2, 1)
    K = planner(4, 1)
    outside = [(1, 8, 8, 48, 64, 1, "SAME"), (1, 8, 8, 64, 34, 1, "SAME"), (1, 8, 8, 64, 28, 1, "SAME"), (1, 8, 8, 64, 64, 3, "SAME"),
               (1, 9, 8, 64, 64, 2, "SAME"), (1, 9, 12, 64, 64, 2, "VALID")]
    for case in outside:
        assert expected_tile(case, 0, 4, 1) == 0 and expected_tile(case, 2, 4, 1) == 0, case
        assert K.wino_chosen(geom(K, case), 0) == 0 and K.wino_chosen(geom(K, case), 2) == 0, case


def test_filter_gradient_split_counts_from_the_workspace_query(planner):
    """the shapes of the GPU file's split test really split, the second one raggedly — read off the workspace query, not assumed"""
    lib = pkg("_lib").load()
    for (tile, x3) in ARITH:
        K = planner(tile, x3)
        for i, case in enumerate(SPLITS):
            g = geom(K, case)
            assert K.wino_chosen(g, 2) == tile
            ns, cps, chunks = wgrad_splits(int(lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g))), case, tile, x3)
            Tn = tiles(case, 2, tile)
            print("filter-gradient splits %s F(%dx%d)%s: T = %d, %d chunks, %d splits of %d" % (case, tile, tile, " x3" if x3 else "", Tn, chunks, ns, cps))
            assert ns > 1, (case, tile, x3, ns)
            if i == 1:          # a last chunk that is not full, or a last split with fewer chunks than the others
                assert Tn % (64 if x3 else 32) != 0 or ns * cps != chunks, (case, tile, x3, Tn, ns, cps)
        # a layer with few tiles does not split: the layout formula gives exactly one partial product
        g = geom(K, SHAPES[3])
        assert wgrad_splits(int(lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g))), SHAPES[3], tile, x3)[0] == 1


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def float64_reference(x, w, dy, dil, padding):
    """(y, dx, dw) of the float64 convolution of these (float32 or float64) numpy operands: oracle.tf_ops.conv2d and autograd"""
    xg = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    wg = torch.from_numpy(np.asarray(w, np.float64)).requires_grad_(True)
    y = T.conv2d(xg, wg, 1, dil, padding)
    y.backward(torch.from_numpy(np.asarray(dy, np.float64)))
    return y.detach().numpy(), xg.grad.numpy(), wg.grad.numpy()


@pytest.mark.parametrize("case", SHAPES + SPLITS + WIDE, ids=case_id)
def test_winograd_restatement_is_the_convolution_in_float64(case):
    N, H, W, C, Kf, dil, padding = case
    pad = _pad(case)
    OH, OW = H + 2 * pad - 2 * dil, W + 2 * pad - 2 * dil
    rng = np.random.default_rng(sum(case[:6]))
    x = rng.standard_normal((N, H, W, C))
    w = rng.standard_normal((3, 3, C, Kf)) * np.sqrt(2.0 / (9 * C))
    dy = rng.standard_normal((N, OH, OW, Kf))
    y, dx, dw = float64_reference(x, w, dy, dil, padding)
    for m in (2, 4):
        errs = {"y": _rel(T.conv3x3_winograd_np(x, w, dil, dtype=np.float64, pad=pad, m=m), y),
                "dx": _rel(T.conv3x3_winograd_np(dy, w, dil, flip_transpose=True, dtype=np.float64, pad=2 * dil - pad, m=m), dx),
                "dw": _rel(T.wgrad3x3_winograd_np(x, dy, dil, dtype=np.float64, pad=pad, m=m), dw),
                "dw, 3 splits": _rel(T.wgrad3x3_winograd_np(x, dy, dil, dtype=np.float64, pad=pad, nsplit=3, m=m), dw)}
        assert max(errs.values()) < 1e-10, (case, m, errs)
