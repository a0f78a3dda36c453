"""not gpu: the planner of the direct split-bf16 filter gradient (csrc/conv_x3_wgrad.hip) is a host function of the C-ABI: the switch
round-trips, and with it off pnp_conv2d_wgrad_workspace_bytes reports exactly what the fp32-pipe route asked for before the route existed"""
import ctypes

from conftest import pkg

# (N, C) of the cls1 layers at 256^2 -> bytes reported before the route existed (ring kernel: split count x 9 C 64 floats)
BEFORE = {(16, 32): 25141248, (16, 64): 30081024, (2, 32): 33546240}


def test_x3_wgrad_switch_and_workspace(built):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    ws = lambda g: int(lib.pnp_conv2d_wgrad_workspace_bytes(ctypes.byref(g)))
    prev = K.x3_wgrad(-1)
    prev_d = K.x3_direct(-1)
    try:
        assert K.x3_wgrad(0) == prev and K.x3_wgrad(-1) == 0
        assert K.x3_wgrad(1) == 0 and K.x3_wgrad(-1) == 1
        assert K.x3_wgrad(5) == 1 and K.x3_wgrad(-1) == 1          # (clamped to on)
        K.x3_direct(1)
        for (N, C), nbytes in BEFORE.items():
            g = K.conv_geom((N, 256, 256, C), (3, 3, C, 64), 1, 1, "SAME")
            before = L.ROUTE_N16_WGRAD if (N, C) == (2, 32) else L.ROUTE_RING    # (B = 2, 32 -> 64: the 16x16x4-MFMA kernel, one partial per workgroup)
            K.x3_wgrad(0)
            assert ws(g) == nbytes, (N, C, ws(g))
            assert K.conv_route(g, 2) == before, (N, C, K.conv_route(g, 2))
            K.x3_wgrad(1)
            parts = min(256, N * 16 * 16) * (2 if C == 32 else 1)
            assert ws(g) == parts * 9 * C * 64 * 4, (N, C, ws(g))
            assert K.conv_route(g, 2) == L.ROUTE_X3W
            K.x3_direct(0)                                          # the family's mode switches it off too
            assert ws(g) == nbytes, (N, C, ws(g))
            assert K.conv_route(g, 2) == before
            K.x3_direct(1)
        # mode 1 needs a tile per CU; bf16 geometries never
        g = K.conv_geom((1, 64, 64, 32), (3, 3, 32, 64), 1, 1, "SAME")
        on = ws(g)
        assert K.conv_route(g, 2) != L.ROUTE_X3W
        K.x3_wgrad(0)
        assert ws(g) == on
        gb = K.conv_geom((16, 256, 256, 64), (3, 3, 64, 64), 1, 1, "SAME", dtype=L.DTYPE_BF16)
        off_b = ws(gb)
        K.x3_wgrad(1)
        assert ws(gb) == off_b and K.conv_route(gb, 2) != L.ROUTE_X3W
    finally:
        K.x3_direct(prev_d)
        K.x3_wgrad(prev)
