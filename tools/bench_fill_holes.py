"""Cost of the hole filling (components.fill_holes, csrc/components.hip) on one GPU, at the operating point of
tools/bench_components.py: its seeded five-class blob volume of 256 x 256 x 200 voxels, filled after keep_largest(keep = 1) as the
pipeline does (the filter turns pockets of a wrong class into background holes), and unfiltered.  Records
  1. the wall time of components.fill_holes (ten launches + the one host read of the error counters), median of 7 synchronised
     repetitions, and the launches alone by HIP events, back to back,
  2. against the inference: segment_volume's wall time for a scan of the same shape in the same process (fp32 segmenter, random
     initialisation, B = 16), alone and with keep_largest=1, fill_holes=True — the condition is fill_holes < segment_volume / 10; the
     per-kernel figures of record come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_fill_holes.py
     --profile-step` run,
  3. against the hardware: the bytes the call must at least move over its event time, against the 6.3 TB/s achievable HBM figure,
  4. against the host, when scipy is there: scipy.ndimage.binary_fill_holes(vol > 0) on the same volume, and that it fills the same voxels.
Prints one JSON object and writes it to --out (default profiles/fill_holes_timing.json)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_components as BC  # noqa: E402  (the operating point: its volume, its timers)

C, K = BC.C, BC.K


def host_figure(vol):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    filled = ndimage.binary_fill_holes(vol > 0) & (vol == 0)
    return {"ms": (time.perf_counter() - t0) * 1e3, "voxels_filled": int(filled.sum()),
            "threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None}, filled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_holes_timing.json"))
    ap.add_argument("--profile-step", action="store_true", help="one warm-up, then ONE fill: for a rocprofv3 --kernel-trace run")
    ap.add_argument("--no-inference", action="store_true", help="leave out the segment_volume comparison")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ncls = 5
    raw = BC.blobs(BC.SHAPE, dev)
    vol, _ = C.keep_largest(raw, ncls)
    n = vol.numel()
    C.fill_holes(vol, ncls)                                       # warm-up: the workspace
    torch.cuda.synchronize()
    if a.profile_step:
        C.fill_holes(vol, ncls)
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": True, "voxels": n}))
        return
    out, stats = C.fill_holes(vol, ncls)
    res = {"device": torch.cuda.get_device_name(0), "shape": list(BC.SHAPE), "voxels": n, "num_cls": ncls, "input": "keep_largest(blobs, keep=1)",
           "class_histogram": torch.bincount(vol.reshape(-1).long(), minlength=ncls).tolist(), "stats": stats.cpu().tolist(),
           "workspace_bytes": int(K._lib.load().pnp_fill_holes_workspace_bytes(*BC.SHAPE, ncls))}
    # 1. the fill
    res["fill_holes"] = BC.wall(lambda: C.fill_holes(vol, ncls))
    buf = torch.empty_like(vol)
    mask = C.class_mask(ncls)
    res["fill_ms_back_to_back"] = BC.events(lambda: K.fill_holes(vol, ncls, mask, 0, buf), 20)
    res["fill_ms_back_to_back_max_size_8"] = BC.events(lambda: K.fill_holes(vol, ncls, mask, 8, buf), 10)
    res["keep_largest"] = BC.wall(lambda: C.keep_largest(raw, ncls))
    res["fill_holes_unfiltered_input"] = BC.wall(lambda: C.fill_holes(raw, ncls))
    res["stats_unfiltered_input"] = C.fill_holes(raw, ncls)[1].cpu().tolist()
    # 3. bytes per voxel the call must at least move: state (1 + 1) + tile (1 + 4) + border (1) + flatten (4 + 4) + prepare (4) + count (4)
    #    + contacts (4) + apply (1 + 4 + 1); the per-root rows and the gathers behind a root are not counted
    per_voxel = 38
    res["min_bytes"] = per_voxel * n
    res["fraction_of_achievable_hbm"] = per_voxel * n / (res["fill_ms_back_to_back"] * 1e-3) / BC.HBM_ACHIEVABLE
    # 4. the host
    hf = host_figure(vol.cpu().numpy())
    if hf is not None:
        res["host_scipy_binary_fill_holes"], host_filled = hf
        res["host_fills_the_same_voxels"] = bool(np.array_equal(host_filled, (out != vol).cpu().numpy()))
        res["host_over_device"] = res["host_scipy_binary_fill_holes"]["ms"] / res["fill_holes"]["median_ms"]
    # 2. the inference
    if not a.no_inference:
        vp = importlib.import_module(BC.PKG + ".volume_predict")
        ss = importlib.import_module(BC.PKG + ".source_segmenter")
        net = ss.Full_DRN(channels=3, n_class=ncls, batch_size=16, device=dev, seed=0, cost_kwargs=dict(BC.COST))
        fn = vp.segmenter_logits(net)
        rng = np.random.default_rng(0)
        scan = (rng.standard_normal(BC.SHAPE, dtype=np.float32) * 200 + 300).astype(np.int16)
        kw = dict(batch_size=16, num_cls=ncls, device=dev)
        vp.segment_volume(fn, scan[:, :, :16].copy(), **kw)
        res["segment_volume"] = BC.wall(lambda: vp.segment_volume(fn, scan, **kw), 5)
        res["segment_volume_keep_largest_1_fill_holes"] = BC.wall(lambda: vp.segment_volume(fn, scan, keep_largest=1, fill_holes=True, **kw), 5)
        res["fill_holes_over_segment_volume"] = res["fill_holes"]["median_ms"] / res["segment_volume"]["median_ms"]
        res["condition_under_a_tenth"] = bool(res["fill_holes_over_segment_volume"] < 0.1)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
