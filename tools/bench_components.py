"""Cost of the connected-component filter (components.py, csrc/components.hip) on one GPU: a seeded five-class blob volume of
256 x 256 x 200 voxels (the argmax of smoothed noise fields: a few large structures and a tail of small islands), keep = 1,
connectivity = 1.  Records
  1. the wall time of components.keep_largest (labelling + filter + the one host read of the error counters), median of synchronised
     repetitions, and the labelling and the filter alone by HIP events around back-to-back launches,
  2. against the inference: segment_volume's wall time for a scan of the same shape in the same process (fp32 segmenter, random
     initialisation, B = 16), with and without keep_largest=1 — the per-kernel figures of record come from a separate
     `rocprofv3 --kernel-trace --stats -- python tools/bench_components.py --profile-step` run,
  3. against the hardware: the bytes each stage must at least move (a model, listed per stage) over its event time, against the 6.3 TB/s
     achievable HBM figure,
  4. against the host, when scipy is there: scipy.ndimage.label per class plus bincount and the largest-label mask on the same volume.
Prints one JSON object and writes it to --out (default profiles/components_timing.json)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "medical-cross-modality-domain-adaptation_amd"
C = importlib.import_module(PKG + ".components")
K = importlib.import_module(PKG + ".kernels")

HBM_ACHIEVABLE = 6.3e12
COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}
SHAPE = (256, 256, 200)


def blobs(shape, dev, seed=11, ncls=5):
    """argmax of ncls noise fields: a coarse field upsampled 4 x (the structures) plus smoothed fine noise (the islands along their borders).
    Data generation only: torch's own kernels, outside every timed region."""
    g = torch.Generator(device=dev).manual_seed(seed)
    coarse = torch.randn((ncls, 1) + tuple(max(2, s // 4) for s in shape), generator=g, device=dev)
    f = torch.nn.functional.interpolate(coarse, size=shape, mode="trilinear", align_corners=False)
    fine = torch.randn((ncls, 1) + tuple(shape), generator=g, device=dev)
    f = f + 0.6 * torch.nn.functional.avg_pool3d(fine, 3, stride=1, padding=1)
    f[0] += 0.3
    return f[:, 0].argmax(0).to(torch.uint8).contiguous()


def events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn, reps=7):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(out)), "runs_ms": out}


def host_figure(vol, ncls):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    out = np.zeros_like(vol)
    found = []
    for c in range(1, ncls):
        lab, nl = ndimage.label(vol == c)
        found.append(int(nl))
        if nl:
            out[lab == int(np.argmax(np.bincount(lab.reshape(-1))[1:])) + 1] = c
    return {"ms": (time.perf_counter() - t0) * 1e3, "components": found, "threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_timing.json"))
    ap.add_argument("--profile-step", action="store_true", help="one warm-up, then ONE labelling + filter: for a rocprofv3 --kernel-trace run")
    ap.add_argument("--no-inference", action="store_true", help="leave out the segment_volume comparison")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ncls = 5
    vol = blobs(SHAPE, dev)
    n = vol.numel()
    C.keep_largest(vol, ncls)                                     # warm-up: the workspace
    torch.cuda.synchronize()
    if a.profile_step:
        C.keep_largest(vol, ncls)
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": True, "voxels": n}))
        return
    out, stats = C.keep_largest(vol, ncls)
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "voxels": n, "num_cls": ncls, "keep": 1, "connectivity": 1,
           "class_histogram": torch.bincount(vol.reshape(-1).long(), minlength=ncls).tolist(), "stats": stats.cpu().tolist()}
    # 1. the filter
    res["keep_largest"] = wall(lambda: C.keep_largest(vol, ncls))
    roots, _ = K.label_components(vol, ncls, 1)
    buf = torch.empty_like(vol)
    res["label_ms_back_to_back"] = events(lambda: K.label_components(vol, ncls, 1), 20)
    res["filter_ms_back_to_back"] = events(lambda: K.filter_components(vol, roots, ncls, C.class_mask(ncls), 1, 0, buf), 20)
    for conn in (2, 3):
        res["label_ms_back_to_back_connectivity_%d" % conn] = events(lambda: K.label_components(vol, ncls, conn), 10)
    res["filter_ms_back_to_back_keep_8"] = events(lambda: K.filter_components(vol, roots, ncls, C.class_mask(ncls), 8, 0, buf), 10)
    # 3. bytes each call must at least move: vol 1 B, parent / roots / sizes 4 B per voxel
    #    labelling: tile (1 + 4) + border (1) + flatten (4 + 4); filter: clear (4) + count (4) + rank (4) + apply (1 + 4 + 4 + 1)
    for name, per_voxel in (("label", 14), ("filter", 22)):
        ms = res["%s_ms_back_to_back" % name]
        res["%s_min_bytes" % name] = per_voxel * n
        res["%s_fraction_of_achievable_hbm" % name] = per_voxel * n / (ms * 1e-3) / HBM_ACHIEVABLE
    # 4. the host
    hf = host_figure(vol.cpu().numpy(), ncls)
    if hf is not None:
        res["host_scipy_label_bincount"], host_out = hf
        res["host_equals_device"] = bool(np.array_equal(host_out, out.cpu().numpy()))
        res["host_over_device"] = res["host_scipy_label_bincount"]["ms"] / res["keep_largest"]["median_ms"]
    # 2. the inference
    if not a.no_inference:
        vp = importlib.import_module(PKG + ".volume_predict")
        ss = importlib.import_module(PKG + ".source_segmenter")
        net = ss.Full_DRN(channels=3, n_class=ncls, batch_size=16, device=dev, seed=0, cost_kwargs=dict(COST))
        fn = vp.segmenter_logits(net)
        rng = np.random.default_rng(0)
        scan = (rng.standard_normal(SHAPE, dtype=np.float32) * 200 + 300).astype(np.int16)
        kw = dict(batch_size=16, num_cls=ncls, device=dev)
        vp.segment_volume(fn, scan[:, :, :16].copy(), **kw)
        res["segment_volume"] = wall(lambda: vp.segment_volume(fn, scan, **kw), 5)
        res["segment_volume_keep_largest_1"] = wall(lambda: vp.segment_volume(fn, scan, keep_largest=1, **kw), 5)
        res["keep_largest_over_segment_volume"] = res["keep_largest"]["median_ms"] / res["segment_volume"]["median_ms"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
