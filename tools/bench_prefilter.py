"""Timing of the anti-alias prefilter on one MI355X, one process:
  1. pnp_volume_smooth against a device-to-device copy of the same volume (one read + one write: the floor of ONE pass), the two
     alternating, HIP events around each call: 256x256x200 and 512x512x200 volumes, sigma = (0.93, 0.93, 1.58) (a CT of 0.35 x 0.35 x 0.6 mm
     on a 1 x 1 x 2.5 mm grid) and (0.5, 0.5, 0) (the 2 x resize); out of place and in place; median, min, max of --reps calls after --warmup;
     "copies_per_axis" = median / copy median / filtered axes;
  2. the one-time cost of VolumeSet.apply_prefilter for §13's set of 16 volumes of 256x256x200 (host clock, synchronised);
  3. segment_volume(..., sample_mm=1.0, prefilter="auto") against the same call without the prefilter on a 256x256x200 scan of
     0.35 x 0.35 x 0.6 mm voxels (sigma 0.93, 0.93, 0.33), random-initialised segmenter, median of 3 each, alternating.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_prefilter.py --profile-step` run (two calls per
case, nothing else).  Prints one JSON object and writes it to --out (default profiles/prefilter_timing.json)."""
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
vs = importlib.import_module(PKG + ".volume_source")
K = importlib.import_module(PKG + ".kernels")

SHAPES = [(256, 256, 200), (512, 512, 200)]
SIGMAS = [(0.93, 0.93, 1.58), (0.5, 0.5, 0.0)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # microseconds


def spread(us):
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)), "n": len(us)}


def kernel_cases(dev, reps, warmup):
    out = []
    for shape in SHAPES:
        v = torch.randn(shape, device=dev)
        dst, inplace = torch.empty_like(v), v.clone()
        for sig in SIGMAS:
            w = [vs.gaussian_weights(s) for s in sig]
            axes = sum(t is not None for t in w)
            calls = {"copy": lambda: dst.copy_(v), "smooth": lambda: K.volume_smooth(v, w, out=dst), "smooth_in_place": lambda: K.volume_smooth(inplace, w, out=inplace)}
            us = {k: [] for k in calls}
            for n in range(warmup + reps):
                for k, fn in calls.items():          # alternating
                    t = timed(fn)
                    if n >= warmup:
                        us[k].append(t)
            row = {"shape": list(shape), "sigma": list(sig), "radii": [0 if t is None else len(t) // 2 for t in w], "filtered_axes": axes,
                   "bytes_one_pass": 8 * v.numel()}
            for k in calls:
                row[k] = spread(us[k])
            cp = row["copy"]["median_us"]
            row["copy_tb_per_s"] = 8 * v.numel() / cp / 1e6
            row["copies_per_axis"] = row["smooth"]["median_us"] / cp / axes
            row["copies_per_axis_in_place"] = row["smooth_in_place"]["median_us"] / cp / axes
            out.append(row)
        K.drop_workspace("smooth")
    return out


def set_cost(dev, nvol=16, shape=(256, 256, 200), sig=(0.93, 0.93, 1.58)):
    images = [torch.randn(shape, device=dev) for _ in range(nvol)]
    labels = [torch.zeros(shape, dtype=torch.uint8, device=dev) for _ in range(nvol)]
    warm = vs.VolumeSet.from_device([images[0].clone()], labels[:1], ["w"], [0.0])
    warm.apply_prefilter([sig])
    vset = vs.VolumeSet.from_device(images, labels, ["v%02d" % i for i in range(nvol)], [0.0] * nvol)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vset.apply_prefilter([sig] * nvol)
    torch.cuda.synchronize()
    return {"volumes": nvol, "shape": list(shape), "sigma": list(sig), "ms": (time.perf_counter() - t0) * 1e3}


def predict_cost(dev, B=16):
    vp = importlib.import_module(PKG + ".volume_predict")
    ss = importlib.import_module(PKG + ".source_segmenter")
    bp = importlib.import_module("bench_predict")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, seed=0, cost_kwargs=dict(bp.COST))
    fn = vp.segmenter_logits(net)
    big = bp.scan((256, 256, 200), 0)
    kw = dict(batch_size=B, num_cls=5, device=dev, sample_mm=1.0, spacing=(0.35, 0.35, 0.6))
    vp.segment_volume(fn, bp.scan((256, 256, 16), 2), prefilter="auto", **kw)          # warm-up
    res = {"plain": [], "prefilter_auto": []}
    for _ in range(3):
        for name, pre in (("plain", None), ("prefilter_auto", "auto")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vp.segment_volume(fn, big, prefilter=pre, **kw)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 1e3)
    return {"spacing_mm": [0.35, 0.35, 0.6], "sample_mm": 1.0, "sigma": list(vs.prefilter_sigmas("auto", (256, 256, 200), (256, 256), (0.35, 0.35, 0.6), 1.0)),
            "plain_ms": {"median": float(np.median(res["plain"])), "runs": res["plain"]},
            "prefilter_auto_ms": {"median": float(np.median(res["prefilter_auto"])), "runs": res["prefilter_auto"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefilter_timing.json"))
    ap.add_argument("--no-predict", action="store_true", help="leave out the segment_volume comparison")
    ap.add_argument("--profile-step", action="store_true", help="two calls per case and nothing else: for a rocprofv3 --kernel-trace run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefilter.py needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda:0")
    if a.profile_step:
        rows = kernel_cases(dev, 2, 1)
        print(json.dumps({"profile_step": True, "cases": len(rows)}))
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "kernel": kernel_cases(dev, a.reps, a.warmup),
           "set_of_16": set_cost(dev)}
    if not a.no_predict:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        res["segment_volume_256x256x200"] = predict_cost(dev)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
