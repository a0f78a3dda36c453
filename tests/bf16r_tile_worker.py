"""worker of tests/test_gpu_bf16_domain.py::test_forced_tile_in_a_process_of_its_own and ::test_forced_split_with_a_short_last_part.
PNP_BF16R_TILE and PNP_BF16R_WSPLIT are read once per process, so each value runs in a process of its own.

PNP_BF16R_TILE = 0 / 1 / 2: the FORCED rows of tests/test_bf16_domain_host.py — forward and data gradient with the forced symbol asserted,
checks A (exact operands, bit for bit) and B (random operands against the rounded-operand float64 convolution) of the GPU file, the bf16 side
outputs, and the statistics partials of the forced tile's row geometry against float64 moments of the output.
PNP_BF16R_WSPLIT = 3: the filter gradient of WSPLIT_ROW (64 reduction chunks in parts of 22, 22 and 20), checks A and B, the three partial
slabs counted.

Prints the check-B lines, "TAGS <json list of the variant tags asserted>" and "BF16R WORKER OK"."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import test_bf16_domain_host as BH                # noqa: E402
import test_gpu_bf16_domain as D                  # noqa: E402
import test_gpu_igemm_domain as G                 # noqa: E402
from conftest import pkg                          # noqa: E402


def main():
    tile = int(os.environ.get("PNP_BF16R_TILE", "-1"))
    split = int(os.environ.get("PNP_BF16R_WSPLIT", "0"))
    assert (tile >= 0) != (split > 0), "set PNP_BF16R_TILE or PNP_BF16R_WSPLIT"
    K = pkg("kernels")
    dev = torch.device("cuda:0")
    for sw in (K.wino_mode, K.wino_wgrad_mode, K.x3_direct, K.x3_strided, K.x3_wgrad):
        sw(0)
    tags = set()
    if split:
        case = BH.WSPLIT_ROW
        g = BH.lib_geom(K, case)
        tags |= D.check_resident_row(K, dev, case, (2,), force_split=split, label="WSPLIT=%d " % split)
        L = BH.rplan(case, 2, force_split=split)["launches"][0]
        assert (L["ns"], L["per"], L["total"]) == (3, 22, 64), L
        x, _, dy, _, _ = G._operands(case, True)
        xh, dyh = K.cast_bf16(torch.from_numpy(x).to(dev)), K.cast_bf16(torch.from_numpy(dy).to(dev))
        nout = g.R * g.S * g.C * g.K
        assert G._splits_written(K, dev, split * nout * 4, nout, lambda: K.conv2d_wgrad_bf16r(xh, dyh, g)) == 3
    else:
        for case in BH.FORCED:
            g = BH.lib_geom(K, case)
            kinds = tuple(k for k in (0, 1) if BH.rplan(case, k, force_tile=tile) is not None)
            assert kinds == tuple(k for k in (0, 1) if K.bf16r_served(g, k)), (case, kinds)
            tags |= D.check_resident_row(K, dev, case, kinds, force_tile=tile, label="TILE=%d " % tile)
            if 0 not in kinds:
                continue
            # statistics partials of the forced tile: bm 256 x wm 4 on tile 0, bm 128 x wm 2 on tiles 1 and 2, rows past M masked
            x, w, _, _, _ = G._operands(case, False)
            xh, w_oi = K.cast_bf16(torch.from_numpy(x + np.float32(0.3)).to(dev)), K.filter_bf16(torch.from_numpy(w).to(dev))[1]
            shift = torch.from_numpy((0.2 * np.random.default_rng(tile).standard_normal(g.K)).astype(np.float32)).to(dev)
            (y, _, parts), names = D._launches(lambda: K.conv2d_fwd_bf16r(xh, w_oi, g, keep_prob=0.75, seed=7, stream_id=3, stat_shift=shift, want_stats=True))
            assert names == BH.rplan(case, 0, force_tile=tile)["symbols"], (case, names)
            assert parts[1] == BH.stats_parts(case, tile), (case, parts[1], BH.stats_parts(case, tile))
            P = g.N * g.OH * g.OW
            mean, var = K.bn_stats_finish(parts, shift, P)
            y64 = y.double().reshape(P, g.K)
            em, ev = G._rel(mean, y64.mean(0)), G._rel(var, y64.var(0, unbiased=False))
            print("forced tile %d statistics %s: %d parts, mean %.2e var %.2e" % (tile, BH.case_id(case), parts[1], em, ev))
            assert em < 1e-5 and ev < 1e-5, (case, em, ev)
    print("TAGS " + json.dumps(sorted(tags)))
    print("BF16R WORKER OK")


if __name__ == "__main__":
    main()
