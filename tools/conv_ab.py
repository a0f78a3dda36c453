"""Bit-for-bit A/B of the convolution entry points between two builds of the library (the split planning of csrc/conv_igemm.hip, the
partial sums of csrc/split_sum.h, the vector-ALU route file csrc/conv_valu.hip).

    PNP_LIB=<one libpnp_hip.so>     python tools/conv_ab.py dump a.json
    PNP_LIB=<another libpnp_hip.so> python tools/conv_ab.py dump b.json
    python tools/conv_ab.py compare a.json b.json        # one line per array, exit status 1 if any differs

`dump` runs conv2d_fwd (with and without dropout 0.5), conv2d_dgrad (with and without residual) and conv2d_wgrad (with and without into=)
over the FWD, STRIDED and WGRAD tables of tests/test_igemm_domain_host.py in fp32 and bf16 arithmetic, at the library's default switches and
(filter gradient only) with the Winograd and split-bf16 routes off, which is where the fp32 routes of the tables run; FWD and WGRAD once more
with the Winograd route wherever eligible and its GEMMs in fp32 (wino_x3 0) and again on split-bf16 operands (wino_x3 2); the SHAPES,
SPLITS and WIDE tables of tests/test_wino_domain_host.py in that file's four arithmetics (tile 2 / 4 x wino_x3 0 / 2), at every pass the
route's planner takes, the forward also through conv2d_fwd_stats (output and partial rows) and conv2d_fwd_bn; the X3W part counts of
tests/test_gpu_x3_wgrad.py (FEW_PARTS, x3_direct mode 2); and the bf16-resident filter gradient of one layer.  PNP_BF16R_WSPLIT is read once
per process: `dump <file> bf16r` runs that layer alone, for one dump per forced split.  Inputs are seeded on the device; the file holds one
SHA-256 per output array."""
import hashlib
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PKG = "medical-cross-modality-domain-adaptation_amd"
BF16R_CASE = (4, 32, 32, 64, 64, 3, 3, 1, 1, "SAME")


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _rand(gen, shape, dev, scale=1.0):
    return torch.randn(shape, generator=gen, device=dev, dtype=torch.float32) * scale


def _layer(K, L, out, tag, case, dt, dev, gen, passes=(0, 1, 2)):
    N, H, W, C, Kf, R, S, st, dil, padding = case
    g = K.conv_geom((N, H, W, C), (R, S, C, Kf), st, dil, padding, dtype=dt)
    x, w = _rand(gen, (N, H, W, C), dev), _rand(gen, (R, S, C, Kf), dev, 0.05)
    dy, res, pre = _rand(gen, (N, g.OH, g.OW, Kf), dev), _rand(gen, (N, H, W, C), dev), _rand(gen, (R, S, C, Kf), dev, 50.0)
    if 0 in passes:
        out[tag + " y"] = _sha(K.conv2d_fwd(x, w, g))
        out[tag + " y drop"] = _sha(K.conv2d_fwd(x, w, g, keep_prob=0.5, seed=11, stream_id=3))
    if 1 in passes:
        out[tag + " dx"] = _sha(K.conv2d_dgrad(dy, w, g))
        out[tag + " dx+res"] = _sha(K.conv2d_dgrad(dy, w, g, residual=res))
    if 2 in passes:
        out[tag + " dw"] = _sha(K.conv2d_wgrad(x, dy, g))
        out[tag + " dw into"] = _sha(K.conv2d_wgrad(x, dy, g, into=pre.clone()))


def _wino_row(K, L, out, tag, case, dev, gen):
    """a (N, H, W, C, K, dil, padding) row of tests/test_wino_domain_host.py at every pass the route's planner takes: the six arrays of
    _layer, and for the forward the statistics entry point (output and partial rows) and the fused inference BN"""
    N, H, W, C, Kf, dil, padding = case
    g = K.conv_geom((N, H, W, C), (3, 3, C, Kf), 1, dil, padding)
    _layer(K, L, out, tag, (N, H, W, C, Kf, 3, 3, 1, dil, padding), L.DTYPE_F32, dev, gen, passes=[k for k in (0, 1, 2) if K.wino_chosen(g, k)])
    if K.wino_chosen(g, 0):
        x, w = _rand(gen, (N, H, W, C), dev), _rand(gen, (3, 3, C, Kf), dev, 0.05)
        shift, scale, sc = _rand(gen, (Kf,), dev, 0.1), _rand(gen, (Kf,), dev), _rand(gen, (N, g.OH, g.OW, Kf), dev)
        y, (parts, nparts) = K.conv2d_fwd_stats(x, w, g, shift, keep_prob=0.5, seed=11, stream_id=3)
        out[tag + " stats y"] = _sha(y)
        out[tag + " stats parts %d" % nparts] = _sha(parts.view(torch.uint8).flatten()[:nparts * 2 * Kf * 4])
        out[tag + " bn y"] = _sha(K.conv2d_fwd_bn(x, w, g, (scale, shift), shortcut=sc))


def _bf16r(K, L, out, dev, gen):
    N, H, W, C, Kf, R, S, st, dil, padding = BF16R_CASE
    g = K.conv_geom((N, H, W, C), (R, S, C, Kf), st, dil, padding, dtype=L.DTYPE_BF16)
    assert K.bf16r_served(g, 2)
    xh, dyh = K.cast_bf16(_rand(gen, (N, H, W, C), dev)), K.cast_bf16(_rand(gen, (N, g.OH, g.OW, Kf), dev))
    pre = _rand(gen, (R, S, C, Kf), dev, 50.0)
    tag = "bf16r wsplit=%s" % os.environ.get("PNP_BF16R_WSPLIT", "planned")
    out[tag + " dw"] = _sha(K.conv2d_wgrad_bf16r(xh, dyh, g))
    out[tag + " dw into"] = _sha(K.conv2d_wgrad_bf16r(xh, dyh, g, into=pre.clone()))


def dump(path, only=None):
    K, L = importlib.import_module(PKG + ".kernels"), importlib.import_module(PKG + "._lib")
    import test_igemm_domain_host as H
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    out = {}
    _bf16r(K, L, out, dev, gen)
    if only != "bf16r":
        for table, cases in (("FWD", H.FWD), ("STRIDED", H.STRIDED), ("WGRAD", H.WGRAD)):
            for case in cases:
                for dt, dn in ((L.DTYPE_F32, "f32"), (L.DTYPE_BF16, "bf16")):
                    _layer(K, L, out, "%s %s %s" % (table, H.case_id(case), dn), case, dt, dev, gen)
        prev = (K.wino_mode(0), K.wino_wgrad_mode(0), K.x3_direct(0), K.x3_strided(0), K.x3_wgrad(0))       # the fp32 routes of the tables
        for table, cases in (("FWD", H.FWD), ("STRIDED", H.STRIDED), ("WGRAD", H.WGRAD)):
            for case in cases:
                _layer(K, L, out, "%s %s f32 fp32-routes" % (table, H.case_id(case)), case, L.DTYPE_F32, dev, gen)
        K.x3_direct(2); K.x3_wgrad(1)
        for N, OH, OW, C in ((1, 16, 48, 64), (1, 16, 48, 32), (17, 16, 16, 64), (17, 16, 16, 32)):           # test_gpu_x3_wgrad.FEW_PARTS
            _layer(K, L, out, "X3W %dx%dx%dx%d" % (N, OH, OW, C), (N, OH, OW, C, 64, 3, 3, 1, 1, "SAME"), L.DTYPE_F32, dev, gen, passes=(2,))
        K.wino_mode(prev[0]); K.wino_wgrad_mode(prev[1]); K.x3_direct(prev[2]); K.x3_strided(prev[3]); K.x3_wgrad(prev[4])
        # the Winograd route wherever eligible, its GEMMs on the fp32 matrix pipe (wino_gemm_kernel, wino_wgrad_gemm_kernel)
        prev = (K.wino_x3(0), K.wino_mode(2), K.wino_wgrad_mode(2), K.x3_direct(0), K.x3_wgrad(0))
        for table, cases in (("FWD", H.FWD), ("WGRAD", H.WGRAD)):
            for case in cases:
                _layer(K, L, out, "%s %s f32 wino-fp32" % (table, H.case_id(case)), case, L.DTYPE_F32, dev, gen)
        # ... and on split-bf16 operands wherever the shapes allow (the persistent wino_gemm_x3_kernel grid, wino_splitsum_kernel, the filter
        # gradient's tiles padded to 64)
        K.wino_x3(2)
        for table, cases in (("FWD", H.FWD), ("WGRAD", H.WGRAD)):
            for case in cases:
                _layer(K, L, out, "%s %s f32 wino-x3" % (table, H.case_id(case)), case, L.DTYPE_F32, dev, gen)
        # every instance of the route's own kernels: the tables of tests/test_wino_domain_host.py in its four arithmetics
        import test_wino_domain_host as Wd
        prev_t = K.wino_tile(-1)
        for (tile, x3), an in zip(Wd.ARITH, Wd.ARITH_IDS):
            K.wino_tile(tile); K.wino_x3(2 if x3 else 0)
            for table, cases in (("SHAPES", Wd.SHAPES), ("SPLITS", Wd.SPLITS), ("WIDE", Wd.WIDE)):
                for case in cases:
                    _wino_row(K, L, out, "WINO %s %s %s" % (an, table, Wd.case_id(case)), case, dev, gen)
        K.wino_tile(prev_t)
        K.wino_x3(prev[0]); K.wino_mode(prev[1]); K.wino_wgrad_mode(prev[2]); K.x3_direct(prev[3]); K.x3_wgrad(prev[4])
    json.dump(out, open(path, "w"), indent=0, sort_keys=True)
    print("%s: %d arrays, library %s" % (path, len(out), os.environ.get("PNP_LIB", "(the tree's)")))


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    n = 0
    for name in sorted(set(a) | set(b)):
        same = name in a and name in b and a[name] == b[name]
        n += not same
        print("%-9s %s" % ("equal" if same else ("DIFFERS" if name in a and name in b else "MISSING"), name))
    print("VERDICT: %d arrays, %d differ" % (len(set(a) | set(b)), n))
    return 1 if n else 0


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3] if len(sys.argv) == 4 else None)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
