"""Cost of tiled whole-scan inference (volume_predict.segment_volume(tiles=), pnp_paste_tiles in csrc/paste.hip) on one GPU: a
seeded 512 x 512 x 200 scan of 0.5 mm voxels on a 1 mm grid, 256 x 256 planes, tiles=(2, 2), B = 16, num_cls = 5, the source segmenter's
fp32 forward (random initialisation) as logits_fn.  (The scan is exactly one plane wide, so tile_plan's "auto" is one plane and the four
planes asked for coincide: four gathers, four forwards and a paste in which every column is covered by all four members — the cost of any
2 x 2 plan, with the paste at its most expensive.)  Records
  1. the wall time per scan of segment_volume: the single plane and tiles=(2, 2);
  2. the yardstick of the kernel, alternating in one process, HIP events around every single launch, median (min ... max):
     pnp_paste_ensemble_fov at M = 4 with four full-cover maps, and pnp_paste_tiles at M = 4 with the same four maps and ramp = 1 — the
     same loads plus the window and the mask; then pnp_paste_tiles with the plan's own four maps and ramp.
The per-kernel figures (paste_tiles_kernel and the gathers beside the forwards' kernels) come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_tiles.py --profile-step` run.  Prints one JSON object and writes it to --out."""
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
vp = importlib.import_module(PKG + ".volume_predict")
ss = importlib.import_module(PKG + ".source_segmenter")
K = importlib.import_module(PKG + ".kernels")

COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}


def scan(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape, dtype=np.float32) * 200 + 300
    v[::7, ::5, ::3] += 3000
    return v.astype(np.int16)


def one_launch_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(min(v)), "max_us": 1e3 * float(max(v)), "launches": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_timing.json"))
    ap.add_argument("--profile-step", action="store_true", help="a 16-frame warm-up scan, then the scan once with tiles=(2, 2): for a "
                    "rocprofv3 --kernel-trace run")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, ncls, (X, Y, Z), (H, W) = a.batch_size, 5, (512, 512, 200), (256, 256)
    net = ss.Full_DRN(channels=3, n_class=ncls, batch_size=B, device=dev, seed=0, cost_kwargs=dict(COST))
    fn = vp.segmenter_logits(net)
    big = scan((X, Y, Z), 0)
    kw = dict(batch_size=B, num_cls=ncls, device=dev, spacing=(0.5, 0.5, 0.5), sample_mm=(1.0, 1.0, 0.5))
    vp.segment_volume(fn, scan((X, Y, 16), 2), tiles=(2, 2), **kw)                       # warm-up: 1 batch
    torch.cuda.synchronize()
    if a.profile_step:
        cov = []
        vp.segment_volume(fn, big, tiles=(2, 2), fov_stats=cov, **kw)                    # 13 batches of 4 gathers, 4 forwards, 1 paste
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": True, "batches": [1, 13], "members": 4, "coverage": cov}))
        return
    res = {"device": torch.cuda.get_device_name(0), "batch_size": B, "num_cls": ncls, "out_size": [H, W], "volume": [X, Y, Z]}

    def wall(**extra):
        out, cov = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vp.segment_volume(fn, big, fov_stats=cov, **extra, **kw)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": float(np.median(out)), "runs_ms": out, "coverage": cov[-1]}
    res["segment_volume_single_plane"] = wall()
    res["segment_volume_tiles_2x2"] = wall(tiles=(2, 2))
    # the yardstick: one fixed batch of four members
    whole, host = ((0, X), (0, Y), (0, Z)), {k: v for k, v in kw.items() if k != "device"}
    plan = vp.plan_view(vp.parse_request(tiles=(2, 2), **host), (X, Y, Z), 2, whole, kw["spacing"])          # what segment_volume ran above
    counts, ramp, plan_invs = plan.counts, plan.ramp, plan.invs
    # four full-cover maps: the resize map (every column inside the plane) and three small rotations about it at a scale that keeps the corners in
    views = [{}, {"scale": 0.9, "rotate": 3.0}, {"scale": 0.9, "rotate": -3.0}, {"scale": 0.95}]
    full = vp.plan_view(vp.parse_request(tta=views, batch_size=B, num_cls=ncls), (X, Y, Z), 2, whole).invs
    assert vp.coverage(full, X, Y, H, W) == 1.0
    members = [torch.randn((B, H, W, ncls), device=dev) * 3.0 for _ in range(4)]
    origin, strides = plan.origin, plan.strides
    out = torch.zeros((X, Y, Z), dtype=torch.uint8, device=dev)
    prob = torch.zeros((ncls, X, Y, Z), dtype=torch.float32, device=dev)
    ent = torch.zeros((X, Y, Z), dtype=torch.float32, device=dev)
    res.update(tile_counts=list(counts), ramp=ramp)
    for name, p, h in (("labels", None, None), ("prob_entropy", prob, ent)):
        calls = {"ensemble_fov_M4_full_cover": lambda: K.paste_ensemble(members, B, 50, full, (X, Y), out, origin, strides, prob=p, entropy=h, fov=True),
                 "tiles_M4_full_cover_ramp1": lambda: K.paste_tiles(members, B, 50, full, 1.0, (X, Y), out, origin, strides, prob=p, entropy=h),
                 "tiles_M4_plan": lambda: K.paste_tiles(members, B, 50, plan_invs, ramp, (X, Y), out, origin, strides, prob=p, entropy=h)}
        times = {k: [] for k in calls}
        for rep in range(5 + 25):                                                       # 5 warm-up rounds, then 25 alternating
            for k, f in calls.items():
                ms = one_launch_ms(f)
                if rep >= 5:
                    times[k].append(ms)
        res[name] = {k: stats(v) for k, v in times.items()}
        res[name]["tiles_over_ensemble_fov"] = res[name]["tiles_M4_full_cover_ramp1"]["median_us"] / res[name]["ensemble_fov_M4_full_cover"]["median_us"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
