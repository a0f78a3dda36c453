"""not gpu: the planner of the strided split-bf16 kernels (x3s_plan, csrc/conv_x3_direct.hip) is a host function; the workspace queries of
the C-ABI show its choice wherever the split filter image (R S C K 6 bytes) is larger than what the fp32-pipe route asks for.  Relations,
not absolute numbers: route taken -> on == max(off, image) (and on != off in the rows listed as moving); refused -> on == off.  The same
Python restatement of the predicate (test_gpu_x3_domain.x3s_expected) decides which symbols tests/test_gpu_x3_domain.py expects on the GPU,
so this file tells a reader of a GPU log, without a GPU, which of that table's cases the route owns.  Where the fp32 route's own
reduction-split workspace is larger than the image the byte counts cannot show the choice; pnp_conv2d_route says it outright, and every
row is held to it as well: route == X3S exactly where the table says the route takes the layer."""
import ctypes

import pytest

from conftest import pkg
import test_gpu_x3_domain as D

# pnp_conv2d_dgrad_workspace_bytes with wino_mode(1), x3_direct(2): ((N, H, W, C, K, R, S, stride, padding), taken, the query moves)
# (bytes off -> on, read on a CPU host: for the reader, not asserted)
DGRAD_ROWS = [
    ((2, 96, 48, 64, 64, 5, 5, 3, "SAME"), True, True),          # 409600 -> 614400
    ((2, 96, 48, 64, 64, 5, 5, 3, "VALID"), True, True),         # 409600 -> 614400
    ((2, 95, 47, 64, 64, 5, 5, 3, "VALID"), False, False),       # 409600 -> 409600: phase grids not multiples of 16
    ((2, 96, 48, 64, 64, 3, 3, 3, "SAME"), True, True),          # 147456 -> 221184
    ((2, 128, 64, 64, 64, 5, 5, 4, "SAME"), True, True),         # 409600 -> 614400
    ((2, 128, 64, 64, 64, 4, 4, 4, "SAME"), True, True),         # 262144 -> 393216
    ((1, 128, 64, 64, 32, 8, 8, 4, "SAME"), True, True),         # 524288 -> 786432
    ((1, 128, 64, 64, 64, 8, 8, 4, "SAME"), True, True),         # 1048576 -> 1572864
    ((1, 128, 64, 32, 64, 8, 8, 4, "SAME"), False, False),       # 524288 -> 524288: 32 output channels of the data gradient
    ((3, 64, 96, 64, 64, 4, 4, 2, "SAME"), True, True),          # 262144 -> 393216
    ((2, 64, 64, 64, 64, 3, 3, 2, "VALID"), True, True),         # 147456 -> 221184
    ((6, 224, 256, 64, 64, 3, 3, 2, "SAME"), True, True),        # 147456 -> 221184
    ((6, 224, 256, 32, 64, 3, 3, 2, "SAME"), False, False),      # 73728 -> 73728
    ((2, 64, 64, 96, 64, 3, 3, 2, "SAME"), False, False),        # 221184 -> 221184: 96 output channels
]
# pnp_conv2d_fwd_workspace_bytes, every row taken: 0 -> the image
FWD_ROWS = [
    (3, 64, 96, 32, 64, 3, 5, 2, "SAME"),                        # 184320
    (3, 64, 96, 32, 64, 5, 3, 2, "SAME"),                        # 184320
    (6, 224, 256, 32, 64, 3, 3, 2, "SAME"),                      # 110592
    (6, 224, 256, 64, 64, 3, 3, 2, "SAME"),                      # 221184
    (3, 160, 192, 64, 64, 5, 5, 2, "SAME"),                      # 614400
]


def _geom(K, case, **kw):
    N, H, W, C, Kf, R, S, s, padding = case
    return K.conv_geom((N, H, W, C), (R, S, C, Kf), s, 1, padding, **kw)


def _image(case):
    N, H, W, C, Kf, R, S, s, padding = case
    return R * S * C * Kf * 6


@pytest.fixture
def queries(built):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    prev = (K.x3_direct(-1), K.x3_strided(-1), K.wino_mode(1))

    def ws(case, kind, strided, **kw):
        K.x3_strided(strided)
        g = _geom(K, case, **kw)
        fn = lib.pnp_conv2d_dgrad_workspace_bytes if kind else lib.pnp_conv2d_fwd_workspace_bytes
        ws.route = K.conv_route(g, kind)                                # (what the library says it launches, in the same setting)
        return int(fn(ctypes.byref(g)))
    yield K, L, ws
    K.x3_direct(prev[0]); K.x3_strided(prev[1]); K.wino_mode(prev[2])


def _check(ws, case, kind, taken, moves=None):
    off = ws(case, kind, 0)
    assert ws.route != pkg("_lib").ROUTE_X3S, (case, kind)
    on = ws(case, kind, 1)
    assert (ws.route == pkg("_lib").ROUTE_X3S) == taken, (case, kind, ws.route)
    if taken:
        assert on == max(off, _image(case)), (case, kind, off, on)
    else:
        assert on == off, (case, kind, off, on)
    if moves is not None:
        assert (on != off) == moves, (case, kind, off, on)
    return off, on


def test_x3_strided_switch_round_trips(queries):
    K, _, _ = queries
    prev = K.x3_strided(-1)
    assert K.x3_strided(0) == prev and K.x3_strided(-1) == 0
    assert K.x3_strided(1) == 0 and K.x3_strided(-1) == 1


def test_x3_strided_planner_through_the_workspace_queries(queries):
    K, L, ws = queries
    K.x3_direct(2)
    for case, taken, moves in DGRAD_ROWS:
        assert (D.x3s_expected(case, 1) > 0) == taken, case            # the restated predicate agrees with the table
        _check(ws, case, 1, taken, moves)
    for case in FWD_ROWS:
        assert D.x3s_expected(case, 0) > 0, case
        off, on = _check(ws, case, 0, True, True)
        assert off == 0 and on == _image(case), (case, off, on)
    # x3_direct(0): the family's mode switches the route off whatever x3_strided says
    K.x3_direct(0)
    for case, kind in [(c, 1) for c, _, _ in DGRAD_ROWS] + [(c, 0) for c in FWD_ROWS]:
        base = ws(case, kind, 0)
        assert ws(case, kind, 1) == base, (case, kind)
        K.x3_direct(2)
        assert ws(case, kind, 0) == base, (case, kind)                  # ... and is what "off" reports in mode 2
        K.x3_direct(0)
    # a bf16 geometry and a SYMMETRIC one never change
    K.x3_direct(2)
    for case, kind in (((2, 96, 48, 64, 64, 5, 5, 3, "SAME"), 1), ((6, 224, 256, 64, 64, 3, 3, 2, "SAME"), 0), ((3, 160, 192, 64, 64, 5, 5, 2, "SAME"), 1)):
        assert ws(case, kind, 1, dtype=L.DTYPE_BF16) == ws(case, kind, 0, dtype=L.DTYPE_BF16), (case, kind)
        sym = case[:8] + ("SYMMETRIC",)
        assert ws(sym, kind, 1) == ws(sym, kind, 0), (sym, kind)


def test_x3_strided_planner_at_the_default_mode(queries):
    """mode 1: >= 256 items and (taps >= 4 s^2, or a data gradient of <= 64 dy channels) — strides 3 and 4 are reachable by a caller of the
    public API at the library's defaults"""
    K, L, ws = queries
    K.x3_direct(1)
    k7s3 = (16, 192, 192, 32, 64, 7, 7, 3, "SAME")
    assert D.x3s_expected(k7s3, 0, mode=1) > 0
    off, on = _check(ws, k7s3, 0, True, True)                           # 0 -> 602112
    assert off == 0 and on == _image(k7s3)
    for case in ((16, 192, 192, 64, 64, 5, 5, 3, "SAME"), (16, 256, 256, 64, 64, 5, 5, 4, "SAME")):
        assert D.x3s_expected(case, 1, mode=1) > 0 and D.x3s_expected(case, 0, mode=1) == 0
        _check(ws, case, 1, True, True)                                 # 409600 -> 614400
        off, on = _check(ws, case, 0, False, False)                     # 25 taps < 4 s^2
        assert off == 0
    small = (3, 64, 96, 64, 64, 5, 3, 2, "SAME")                        # 72 data-gradient items: under the 256 of mode 1
    assert D.x3s_expected(small, 1, mode=1) == 0 and D.x3s_expected(small, 1, mode=2) == 72
    _check(ws, small, 1, False, False)                                  # 245760 -> 245760
    K.x3_direct(2)
    _check(ws, small, 1, True, True)                                    # 245760 -> 368640


def test_restated_predicate_against_the_queries_for_every_gpu_case(queries):
    """every case of tests/test_gpu_x3_domain.py: what the table says the route owns is what the predicate says, and the workspace queries
    agree wherever they can show it"""
    K, L, ws = queries
    K.x3_direct(2)
    for case, want in D.STRIDED:
        for kind in (0, 1):
            taken = D.x3s_expected(case, kind) > 0
            assert taken == want[kind], (case, kind)
            _check(ws, case, kind, taken)
    assert D.x3s_expected(D.STRIDED[-2][0], 0) == 336 and D.x3s_expected(D.STRIDED[-2][0], 1) == 1344
    assert D.x3s_expected(D.STRIDED[-1][0], 0) == 90 and D.x3s_expected(D.STRIDED[-1][0], 1) == 360
