"""Cost of the label-free body crop (csrc/body.hip, body.py) on one GPU, on a seeded torso-like CT phantom of 256 x 256 x 200
voxels.  Records
  1. per call under HIP events (one event pair per call, median of --calls calls after a warm-up): pnp_volume_histogram (256 bins; it
     reads the volume twice: min / max, then the bins), pnp_volume_threshold_mask (reads 4 bytes, writes 1 per voxel), each with its bytes
     per second against the 6.3 TB/s achievable HBM figure, and the whole body.body_box call (two host synchronisations inside),
  2. the histogram on four value patterns that separate its two levels of atomics: `constant` (the bin pass returns at once: the
     min / max pass alone), `two_values` (every LDS add of a wave lands on one of two addresses, two global adds per workgroup),
     `uniform` (the LDS adds spread over all bins, 256 global adds per workgroup) and the normalised phantom itself; the per-kernel
     device times of record come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_body.py --kernels-only` run,
  3. the wall time of volume_predict.segment_volume (array in host memory to finished label volume, synchronised at the end, source
     segmenter with random weights, B = 16) with crop="body" against the same call with the box it found passed as crop=, alternating;
     the difference is the cost of finding the box.
Prints one JSON object and writes it to --out (default profiles/body_timing.json)."""
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
K = importlib.import_module(PKG + ".kernels")
body = importlib.import_module(PKG + ".body")

HBM_ACHIEVABLE = 6.3e12
COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}


def torso(shape=(256, 256, 200), seed=0):
    """air -1000 +- 10, an elliptic body of tissue 40 +- 20 with two lungs, a detached table plate, a few voxels of metal"""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    inside = ((x - 0.47 * X) / (0.35 * X)) ** 2 + ((y - 0.5 * Y) / (0.27 * Y)) ** 2 <= 1.0
    for cy in (0.36, 0.64):
        inside &= ~(((x - 0.42 * X) / (0.12 * X)) ** 2 + ((y - cy * Y) / (0.09 * Y)) ** 2 <= 1.0)
    v = rng.normal(-1000.0, 10.0, shape).astype(np.float32)
    t = np.broadcast_to(inside[:, :, None], shape).copy()
    t[:, :, :4] = False
    t[:, :, Z - 4:] = False
    v[t] = rng.normal(40.0, 20.0, int(t.sum())).astype(np.float32)
    x0 = int(0.9 * X)
    v[x0:x0 + 6, Y // 10:Y - Y // 10, :] = rng.normal(200.0, 10.0, (6, Y - 2 * (Y // 10), Z)).astype(np.float32)
    v[X // 2:X // 2 + 3, Y // 2:Y // 2 + 3, Z // 2] = 3000.0
    return v


def per_call(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": float(np.median(us)), "min_us": float(min(us)), "max_us": float(max(us)), "calls": calls}


def with_rate(row, nbytes):
    row["bytes"] = int(nbytes)
    row["bytes_per_s"] = nbytes / (row["median_us"] * 1e-6)
    row["share_of_6p3_TBps"] = row["bytes_per_s"] / HBM_ACHIEVABLE
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--predict-runs", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--kernels-only", action="store_true", help="parts 1 and 2 only, nothing written: for a `rocprofv3 --kernel-trace --stats` run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    raw = torso()
    n = raw.size
    vd = torch.from_numpy(raw).to(dev)
    vn, _ = K.volume_preprocess(vd, 98)
    res = {"device": torch.cuda.get_device_name(0), "volume": list(raw.shape), "nbins": 256}

    # 1. the two entry points on the normalised phantom, and the whole call
    rng, hist = K.volume_histogram(vn)
    k = body.otsu_bin(hist.cpu().numpy())
    mask = torch.empty(vn.shape, dtype=torch.uint8, device=dev)
    res["otsu_bin"] = k
    res["volume_histogram"] = with_rate(per_call(lambda: K.volume_histogram(vn), a.calls), 8 * n)
    res["volume_threshold_mask"] = with_rate(per_call(lambda: K.volume_threshold_mask(vn, rng, k, out=mask), a.calls), 5 * n)
    res["body_share_of_voxels"] = float(mask.sum().item()) / n
    box = body.body_box(vd)
    res["box"] = [list(b) for b in box]
    res["body_box"] = per_call(lambda: body.body_box(vd), a.calls)

    # 2. the histogram's two levels of atomics
    g = torch.Generator(device=dev).manual_seed(1)
    patterns = {"constant": torch.full((n,), 1.5, device=dev),
                "two_values": torch.where(torch.rand(n, device=dev, generator=g) < 0.7, torch.tensor(-1.0, device=dev), torch.tensor(2.0, device=dev)),
                "uniform": torch.rand(n, device=dev, generator=g),
                "normalised_phantom": vn.reshape(-1)}
    res["histogram_by_pattern"] = {name: with_rate(per_call(lambda t=t: K.volume_histogram(t), a.calls), 8 * n) for name, t in patterns.items()}
    res["histogram_by_pattern"]["constant"]["note"] = "the bin pass returns at once: min / max pass + launches"
    del patterns, mask
    if a.kernels_only:
        print(json.dumps(res))
        return

    # 3. prediction with the crop found on the device against the same box given by hand
    vp = importlib.import_module(PKG + ".volume_predict")
    ss = importlib.import_module(PKG + ".source_segmenter")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=a.batch_size, device=dev, seed=0, cost_kwargs=dict(COST))
    fn = vp.segmenter_logits(net)
    kw = dict(batch_size=a.batch_size, num_cls=5, device=dev, flip_correction=False)
    vp.segment_volume(fn, raw[:, :, :16], **kw)                       # warm-up: one batch
    found = []
    vp.segment_volume(fn, raw, crop="body", crop_box=found, **kw)     # warm-up of the crop's kernels
    torch.cuda.synchronize()
    times = {"crop_body": [], "crop_box": [], "no_crop": []}
    for _ in range(a.predict_runs):
        for name, crop in (("crop_body", "body"), ("crop_box", found[0]), ("no_crop", None)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vp.segment_volume(fn, raw, crop=crop, **kw)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    res["segment_volume_256x256x200"] = {name: {"median_ms": float(np.median(t)), "runs_ms": t} for name, t in times.items()}
    res["segment_volume_256x256x200"]["box"] = [list(b) for b in found[0]]
    res["segment_volume_256x256x200"]["finding_the_box_ms"] = float(np.median(times["crop_body"]) - np.median(times["crop_box"]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
