"""not gpu: the planner of the logits layer's split-bf16 kernels (csrc/conv_x3_narrow.hip, route X3N) is a host function of the C-ABI: the
switch pnp_conv2d_x3_narrow / PNP_X3_NARROW (0 off, 1 where a launch fills the chip, 2 wherever the shapes allow), the routes and the
workspace queries of the forward and the data gradient, the 256-tile rule of mode 1 and what the predicate refuses."""
import ctypes
import importlib

import pytest

FWD_IMAGE = 8 * 5 * 3 * 64 * 16         # forward filter image: [k-slab][tap row][plane][lane][8] bf16
DGRAD_IMAGE = 7 * 3 * 40 * 64           # data gradient: [k-slab][plane][channel][32] bf16


@pytest.fixture
def KL(built):
    K, L = importlib.import_module(built.__name__ + ".kernels"), built._lib
    prev = (K.x3_direct(-1), K.x3_narrow(-1))
    yield K, L
    K.x3_direct(prev[0]); K.x3_narrow(prev[1])


def _logits(K, N, H, W, pad="VALID", dtype=None):
    return K.conv_geom((N, H, W, 40), (5, 5, 40, 5), 1, 1, pad, dtype=dtype)


def _routes(K, g):
    return tuple(K.conv_route(g, k) for k in (0, 1, 2))


def _ws(L, g):
    lib = L.load()
    return int(lib.pnp_conv2d_fwd_workspace_bytes(ctypes.byref(g))), int(lib.pnp_conv2d_dgrad_workspace_bytes(ctypes.byref(g)))


def test_switch_reads_and_clamps(KL):
    K, _ = KL
    prev = K.x3_narrow(-1)
    assert K.x3_narrow(0) == prev and K.x3_narrow(-1) == 0
    assert K.x3_narrow(1) == 0 and K.x3_narrow(-1) == 1
    assert K.x3_narrow(7) == 1 and K.x3_narrow(-1) == 2          # (clamped)
    assert K.x3_narrow(prev) == 2


def test_model_geometry_routes_and_workspace_in_every_mode(KL):
    K, L = KL
    g = _logits(K, 16, 260, 260)
    K.x3_direct(1)
    K.x3_narrow(0)
    off = _routes(K, g)
    ws_off = _ws(L, g)
    assert off == (L.ROUTE_NARROW, L.ROUTE_IGEMM, L.ROUTE_WGD)
    for mode in (1, 2):
        K.x3_narrow(mode)
        assert _routes(K, g) == (L.ROUTE_X3N, L.ROUTE_X3N, L.ROUTE_WGD), mode           # the filter gradient keeps its kernel
        assert _ws(L, g) == (max(ws_off[0], FWD_IMAGE), max(ws_off[1], DGRAD_IMAGE)), mode
        assert K.conv_stats_parts(g) == 0                                               # (as on the vector-ALU kernel: no statistics epilogue)
    # x3_direct(0) turns the family off, this route with it: exactly the routes and bytes of the switch-off library
    for mode in (1, 2):
        K.x3_narrow(mode)
        K.x3_direct(0)
        assert _routes(K, g) == off and _ws(L, g) == ws_off, mode
        K.x3_direct(1)


def test_small_shapes_keep_their_route_in_mode_1(KL):
    K, L = KL
    K.x3_direct(1)
    for N, H, pad in ((2, 68, "VALID"), (2, 24, "VALID"), (2, 24, "SAME")):
        g = _logits(K, N, H, H, pad)
        K.x3_narrow(0)
        off, ws_off = _routes(K, g), _ws(L, g)
        K.x3_narrow(1)
        assert _routes(K, g) == off and _ws(L, g) == ws_off, (N, H, pad)
        assert L.ROUTE_X3N not in off
    g = _logits(K, 2, 68, 68)
    assert K.conv_route(g, 0) == L.ROUTE_NARROW                                         # 64 tiles: the 256-tile rule
    K.x3_narrow(2)
    assert _routes(K, g)[:2] == (L.ROUTE_X3N, L.ROUTE_X3N)
    assert _routes(K, _logits(K, 2, 24, 24, "SAME"))[:2] == (L.ROUTE_IGEMM, L.ROUTE_X3N)     # 24 x 24 outputs: no 8 x 16 forward tiles


def test_the_256_tile_boundary(KL):
    K, L = KL
    K.x3_direct(1); K.x3_narrow(1)
    # forward tiles of 8 x 16 outputs: (132 - 4) / 8 x (260 - 4) / 16 = 16 x 16 = 256; 15 x 17 = 255
    assert K.conv_route(_logits(K, 1, 132, 260), 0) == L.ROUTE_X3N
    assert K.conv_route(_logits(K, 1, 124, 276), 0) == L.ROUTE_NARROW
    # data-gradient tiles of 16 x 16 pixels of dx, ragged ones counted: 16 x 16 = 256; 15 x 17 = 255
    assert K.conv_route(_logits(K, 1, 256, 256), 1) == L.ROUTE_X3N
    assert K.conv_route(_logits(K, 1, 241, 256), 1) == L.ROUTE_X3N                      # ceil(241 / 16) = 16
    assert K.conv_route(_logits(K, 1, 240, 272), 1) == L.ROUTE_IGEMM
    # per direction: 252 x 252 outputs are no multiple of the forward tile, the data gradient does not mind
    assert K.conv_route(_logits(K, 1, 256, 256), 0) == L.ROUTE_NARROW


def test_what_the_predicate_refuses(KL):
    K, L = KL
    K.x3_direct(2); K.x3_narrow(2)
    geo = lambda x, w, stride=1, dil=1, pad="VALID", dt=None: K.conv_geom(x, w, stride, dil, pad, dtype=dt)
    assert _routes(K, geo((2, 36, 52, 40), (5, 5, 40, 5)))[:2] == (L.ROUTE_X3N, L.ROUTE_X3N)
    refused = [
        geo((2, 36, 52, 40), (5, 5, 40, 5), dt=L.DTYPE_BF16),           # bf16 geometry
        geo((2, 36, 52, 40), (5, 5, 40, 5), pad="SYMMETRIC"),           # the mirror pad inside the kernel
        geo((2, 36, 52, 40), (5, 5, 40, 5), dil=2),
        geo((2, 36, 52, 40), (5, 5, 40, 5), stride=2),
        geo((2, 36, 52, 40), (3, 3, 40, 5)),
        geo((2, 36, 52, 40), (5, 5, 40, 8)),
        geo((2, 36, 52, 32), (5, 5, 32, 5)),
        geo((2, 36, 52, 5), (5, 5, 5, 40)),
    ]
    for g in refused:
        assert L.ROUTE_X3N not in _routes(K, g), (g.C, g.K, g.R, g.stride, g.dil, g.pad_mode, g.dtype)
    assert K.conv_route(geo((2, 35, 52, 40), (5, 5, 40, 5)), 0) != L.ROUTE_X3N        # 31 output rows
    assert K.conv_route(geo((2, 35, 52, 40), (5, 5, 40, 5)), 1) == L.ROUTE_X3N
