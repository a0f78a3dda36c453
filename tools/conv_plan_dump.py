"""CPU: every answer of the convolution planners' C-ABI queries over a fixed grid, one line per (geometry, switch setting) — the evidence
that a change to the host planning (csrc/conv_igemm.hip: plan_fwd / plan_dgrad / plan_wgrad) did not move the policy:

    PNP_LIB=<old libpnp_hip.so> python tools/conv_plan_dump.py > old.txt;  PNP_LIB=<new> python tools/conv_plan_dump.py > new.txt;  diff old.txt new.txt

The library is opened with plain ctypes and only the queries named below are called, so a library older than the current binding loads.
Grid: the base shapes (N, H, W, C, K, R, S, stride) of every convolution of the segmenter and both critics at B = 2, 4, 16 (from the
symbolic build pass; a SYMMETRIC layer also as the mirror-pre-padded VALID layer that runs) and of every case of tests/test_gpu_x3_domain.py,
test_x3_strided_host.py, test_x3_wgrad_host.py and test_gpu_wino.py, each x {SAME, VALID, SYMMETRIC} x dilation {1, 2} x {fp32, bf16},
crossed with every value of every run-time switch.  Pruned only where one switch masters another: wino_mode 0 switches the whole Winograd
route off (wino_wgrad_mode, wino_tile, wino_x3 are not read) and x3_direct 0 the split-bf16 family (x3_strided, x3_wgrad are not read)."""
import ctypes
import importlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PKG = "medical-cross-modality-domain-adaptation_amd"
K, L = importlib.import_module(PKG + ".kernels"), importlib.import_module(PKG + "._lib")       # (imports torch before the CDLL below)

QUERIES = ("fwd_workspace_bytes", "dgrad_workspace_bytes", "wgrad_workspace_bytes", "fwd_stats_parts", "fwd_stats_ws_parts")
SWITCHES = ("wino_mode", "wino_wgrad_mode", "wino_tile", "wino_x3", "x3_direct", "x3_strided", "x3_wgrad")


def model_shapes():
    """(N, H, W, C, K, R, S, stride) of every conv_geom() call of the adaptation model's build pass (segmenter + both critics)"""
    import bench
    adv = importlib.import_module(PKG + ".adversarial")
    seen, orig = [], K.conv_geom

    def spy(x_shape, w_shape, stride=1, dil=1, padding="SAME", dtype=None):
        g = orig(x_shape, w_shape, stride, dil, padding, dtype)
        seen.append((g.N, g.H, g.W, g.C, g.K, g.R, g.S, g.stride))
        if padding == "SYMMETRIC":
            seen.append((g.N, g.H + 2 * g.pad_t, g.W + 2 * g.pad_l, g.C, g.K, g.R, g.S, g.stride))
        return g
    K.conv_geom = spy
    try:
        for B in (2, 4, 16):
            adv.Full_DRN(channels=3, n_class=5, batch_size=B, device="cpu", seed=0, cost_kwargs=dict(bench.GAN_COST), network_config=dict(bench.GAN_NETCFG))
    finally:
        K.conv_geom = orig
    return seen


def test_shapes():
    import test_gpu_wino as Wn
    import test_gpu_x3_domain as D
    import test_x3_strided_host as Sh
    import test_x3_wgrad_host as Wh
    strided = [c for c, _ in D.STRIDED] + [c for c in D.WIDE if len(c) > 5] + [c for c, _, _ in Sh.DGRAD_ROWS] + list(Sh.FWD_ROWS)
    strided += [(16, 192, 192, 32, 64, 7, 7, 3, "SAME"), (16, 192, 192, 64, 64, 5, 5, 3, "SAME"), (16, 256, 256, 64, 64, 5, 5, 4, "SAME"),
                (3, 64, 96, 64, 64, 5, 3, 2, "SAME")]                               # test_x3_strided_planner_at_the_default_mode
    out = [c[:8] for c in strided]
    out += [(N, H, W, C, Kf, 3, 3, 1) for N, H, W, C, Kf in D.STRIDE1 + [c for c in D.WIDE if len(c) == 5]]
    out += [(N, 256, 256, C, 64, 3, 3, 1) for N, C in Wh.BEFORE] + [(1, 64, 64, 32, 64, 3, 3, 1), (16, 256, 256, 64, 64, 3, 3, 1)]
    out += [(N, H, W, C, Kf, 3, 3, 1) for N, H, W, C, Kf, _, _ in Wn.CASES]
    return out


def settings():
    wino = [(0, 0, 2, 0)] + list(itertools.product((1, 2), (0, 1, 2), (2, 4), (0, 1, 2)))
    x3 = [(0, 0, 0)] + list(itertools.product((1, 2), (0, 1), (0, 1)))
    return [w + x for w in wino for x in x3]


def main():
    lib = ctypes.CDLL(L.LIB_PATH)
    G = ctypes.POINTER(L.ConvGeom)
    q = {}
    for n in QUERIES:
        q[n] = getattr(lib, "pnp_conv2d_" + n)
        q[n].restype, q[n].argtypes = (ctypes.c_size_t if "bytes" in n else ctypes.c_int32), [G]
    lib.pnp_conv2d_wino_chosen.restype, lib.pnp_conv2d_wino_chosen.argtypes = ctypes.c_int32, [G, ctypes.c_int32]
    sw = [getattr(lib, "pnp_conv2d_" + n) for n in SWITCHES]
    geoms = []
    for shape in sorted(set(model_shapes() + test_shapes())):
        N, H, W, C, Kf, R, S, stride = shape
        for padding, dil, dt in itertools.product(("SAME", "VALID", "SYMMETRIC"), (1, 2), (L.DTYPE_F32, L.DTYPE_BF16)):
            g = K.conv_geom((N, H, W, C), (R, S, C, Kf), stride, dil, padding, dtype=dt)
            if g.OH > 0 and g.OW > 0:
                geoms.append(("%s %s d%d t%d" % (" ".join(map(str, shape)), padding, dil, dt), g))
    for s in settings():
        for fn, v in zip(sw, s):
            fn(v)
        tag = ",".join(map(str, s))
        for name, g in geoms:
            r = ctypes.byref(g)
            print(name, "|", tag, "|", *[int(q[n](r)) for n in QUERIES], *[int(lib.pnp_conv2d_wino_chosen(r, k)) for k in (0, 1, 2)])


if __name__ == "__main__":
    main()
