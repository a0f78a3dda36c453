"""Cost of multi-planar fusion (pnp_fuse_views in csrc/paste.hip, volume_predict.fuse_views) on one GPU at the size of a whole
scan: 256 x 256 x 200 voxels, 3 views, 5 classes, prob and entropy on — (3 * 5 + 5 + 1) * 4 + 1 = 85 bytes per voxel, 1.1 GB per launch,
far more than the chip's caches hold.  The views are the float32 softmax of seeded random logits, each set to 0 on a quarter of its
frames (mixed coverage).  Records, alternating in one process, HIP events around every single call, median (min ... max):
  1. pnp_fuse_views into separate outputs, and into the first view's buffer (prob == probs[0]: what segment_volume(axes=) launches);
  2. the same fusion written with torch ops on the same tensors — the thing the kernel replaces: per view the coverage mask from the
     class sum, the masked weighted sum, the division, argmax and entropy — with its result compared to the kernel's before it is timed;
  3. the achieved share of the 6.3 TB/s that a float4 copy reaches on this chip (DESIGN §13's yardstick), from the 85 bytes per voxel.
The per-kernel figure comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_fuse.py --profile-step` run.
Prints one JSON object and writes it to --out."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "medical-cross-modality-domain-adaptation_amd"
K = importlib.import_module(PKG + ".kernels")

HBM_COPY_BYTES_PER_S = 6.3e12


def one_call_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(min(v)), "max_us": 1e3 * float(max(v)), "calls": len(v)}


def torch_fusion(views, weights, ncls):
    """(label, prob, entropy) with torch ops: the rule of pnp_fuse_views, volume-sized temporaries and all"""
    acc = torch.zeros_like(views[0])
    wsum = torch.zeros_like(views[0][0])
    for p, w in zip(views, weights):
        cov = (p.sum(dim=0) > 0.5).to(p.dtype) * w
        acc += p * cov
        wsum += cov
    prob = torch.where(wsum > 0, acc / wsum.clamp_min(1e-30), torch.zeros_like(acc))
    label = prob.argmax(dim=0).to(torch.uint8)
    entropy = -(torch.where(prob > 0, prob * prob.clamp_min(1e-30).log(), torch.zeros_like(prob))).sum(dim=0) / math.log(ncls)
    return label, prob, entropy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_timing.json"))
    ap.add_argument("--shape", default="256,256,200")
    ap.add_argument("--profile-step", action="store_true", help="two warm-up launches and five timed ones: for a rocprofv3 --kernel-trace run")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = tuple(int(v) for v in a.shape.split(","))
    M, ncls = 3, 5
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    views = []
    for v in range(M):
        p = torch.softmax(3.0 * torch.randn((ncls,) + shape, device=dev, generator=gen), dim=0)
        p.movedim(1 + v, 1)[:, ::4] = 0.0                                   # a quarter of the frames along the view's own axis
        views.append(p.contiguous())
    weights = [1.0, 1.0, 2.0]
    n = int(np.prod(shape))
    label = torch.empty(shape, dtype=torch.uint8, device=dev)
    prob = torch.empty((ncls,) + shape, dtype=torch.float32, device=dev)
    ent = torch.empty(shape, dtype=torch.float32, device=dev)
    scratch = views[0].clone()                                              # the in-place launch overwrites its first view
    calls = {"fuse_views": lambda: K.fuse_views(views, weights, label=label, prob=prob, entropy=ent),
             "fuse_views_in_place": lambda: K.fuse_views([scratch] + views[1:], weights, label=label, prob=scratch, entropy=ent)}
    if a.profile_step:
        for _ in range(2 + 5):
            calls["fuse_views"]()
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": True, "launches": 7}))
        return
    # the two formulations agree before either is timed
    calls["fuse_views"]()
    tl, tp, th = torch_fusion(views, weights, ncls)
    covered = prob.sum(dim=0) > 0.5
    top = tp.topk(2, dim=0).values
    clear = (top[0] - top[1]) > 1e-5
    agree = {"max_abs_dP": float((prob - tp).abs().max()), "max_abs_dH": float((ent - th).abs().max()),
             "labels_differ_where_the_gap_is_clear": int(((label != tl) & clear & covered).sum()), "covered_share": float(covered.float().mean())}
    assert agree["max_abs_dP"] < 1e-5 and agree["max_abs_dH"] < 1e-4 and agree["labels_differ_where_the_gap_is_clear"] == 0, agree
    del tl, tp, th
    calls["torch_ops"] = lambda: torch_fusion(views, weights, ncls)
    times = {k: [] for k in calls}
    for rep in range(5 + 25):                                               # 5 warm-up rounds, then 25 alternating
        for k, f in calls.items():
            ms = one_call_ms(f)
            if rep >= 5:
                times[k].append(ms)
    bytes_moved = n * ((M * ncls + ncls + 1) * 4 + 1)
    res = {"device": torch.cuda.get_device_name(0), "volume": list(shape), "views": M, "num_cls": ncls, "bytes_per_voxel": bytes_moved // n,
           "bytes_moved": bytes_moved, "agreement_with_torch_ops": agree}
    res.update({k: stats(v) for k, v in times.items()})
    for k in ("fuse_views", "fuse_views_in_place"):
        rate = bytes_moved / (res[k]["median_us"] * 1e-6)
        res[k].update(bytes_per_s=rate, share_of_6p3_TBps=rate / HBM_COPY_BYTES_PER_S)
    res["torch_ops_over_fuse_views"] = res["torch_ops"]["median_us"] / res["fuse_views"]["median_us"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
