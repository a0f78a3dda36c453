"""Cost of ensemble inference (volume_predict.py, pnp_paste_ensemble in csrc/paste.hip) on one GPU at the measured operating
point: M = 5 members (tta="default"), B = 16, 256 x 256 plane, one seeded 256 x 256 x 200 volume, num_cls = 5, the source segmenter's fp32
forward (random initialisation) as logits_fn.  Records
  1. the wall time per volume of segment_volume (array in host memory to the finished volumes on the device, synchronised once at the end):
     the default single-pass path, M = 5 labels only, M = 5 with prob + entropy,
  2. per batch by HIP events around back-to-back launches of one fixed batch: one gather, one forward, the ensemble paste (labels only /
     with prob + entropy; z fastest and z slowest), and the M = 1 ensemble launch next to pnp_paste_labels on the same logits — the per-kernel
     figures of record come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_ensemble.py --profile-step` run,
  3. the ensemble paste's bytes per second (reads M B H W ncls fp32; writes B X Y bytes, + 4 ncls B X Y with prob, + 4 B X Y with entropy)
     against the 6.3 TB/s achievable HBM figure,
  4. (M gathers + the ensemble paste) / (M forwards): the condition is < 0.10.
Prints one JSON object and writes it to --out (default profiles/ensemble_timing.json)."""
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
vs = importlib.import_module(PKG + ".volume_source")
ss = importlib.import_module(PKG + ".source_segmenter")
K = importlib.import_module(PKG + ".kernels")

HBM_ACHIEVABLE = 6.3e12
COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}


def scan(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape, dtype=np.float32) * 200 + 300
    v[::7, ::5, ::3] += 3000
    return v.astype(np.int16)


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


def wall(fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(out)), "runs_ms": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_timing.json"))
    ap.add_argument("--profile-step", action="store_true", help="one 16-frame warm-up volume, then the volume once labels-only and once with "
                    "prob + entropy, then one M = 1 batch through both entry points: for a rocprofv3 --kernel-trace run")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, ncls, (X, Y, Z) = a.batch_size, 5, (256, 256, 200)
    net = ss.Full_DRN(channels=3, n_class=ncls, batch_size=B, device=dev, seed=0, cost_kwargs=dict(COST))
    fn = vp.segmenter_logits(net)
    big = scan((X, Y, Z), 0)
    kw = dict(batch_size=B, num_cls=ncls, device=dev)
    vp.segment_volume(fn, scan((X, Y, 16), 2), tta="default", prob=True, entropy=True, **kw)          # warm-up: 1 batch
    torch.cuda.synchronize()
    plan = vp.plan_view(vp.parse_request(tta="default", batch_size=B, num_cls=ncls), (X, Y, Z), 2, ((0, X), (0, Y), (0, Z)))  # of the call above
    entries, M, maps, invs = [dict(e) for e in plan.entries], plan.members, plan.maps, plan.invs
    # one fixed batch: M gathers, M forwards
    v = torch.from_numpy(big.astype(np.float32)).to(dev)
    _, st = K.volume_preprocess(v, 98, out=v)
    vset = vs.VolumeSet.from_device([v], [torch.zeros(tuple(v.shape), dtype=torch.uint8, device=dev)], ["v"], [float(st[3].item())])
    src = vs.AugmentedSliceSource(vset, B, augment=None, num_cls=ncls)
    rec = np.zeros(B, dtype=vs.SAMPLE_DTYPE)
    rec["frame"] = 50 + np.arange(B)
    members = []
    for m in maps:
        rec["m"][:] = m
        members.append(fn(src.gather_records(rec, ncls, want_onehot=False)[0]).contiguous())
    origin, strides = plan.origin, plan.strides
    if a.profile_step:
        vp.segment_volume(fn, big, tta="default", **kw)                                  # 13 batches, labels only
        vp.segment_volume(fn, big, tta="default", prob=True, entropy=True, **kw)         # 13 batches, all three outputs
        out = torch.zeros((X, Y, Z), dtype=torch.uint8, device=dev)
        K.paste_ensemble(members[:1], B, 50, invs[:1], (X, Y), out, origin, strides)
        K.paste_labels(members[0], B, 50, invs[0], (X, Y), out, origin, strides)
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": True, "ensemble_batches": [1, 13, 13, 1], "members": M}))
        return
    res = {"device": torch.cuda.get_device_name(0), "batch_size": B, "num_cls": ncls, "out_size": [256, 256], "volume": [X, Y, Z], "members": M,
           "tta": entries}
    # 1. wall time per volume
    res["segment_volume_single_pass"] = wall(lambda: vp.segment_volume(fn, big, **kw))
    res["segment_volume_M5_labels"] = wall(lambda: vp.segment_volume(fn, big, tta="default", **kw))
    res["segment_volume_M5_prob_entropy"] = wall(lambda: vp.segment_volume(fn, big, tta="default", prob=True, entropy=True, **kw))
    # 2. stage by stage
    rec["m"][:] = maps[1]
    x = src.gather_records(rec, ncls, want_onehot=False)[0]
    res["gather_ms_incl_upload_and_allocation"] = events(lambda: src.gather_records(rec, ncls, want_onehot=False), 50)
    res["forward_ms"] = events(lambda: fn(x), 20)
    # 3. the ensemble paste alone
    read = M * B * 256 * 256 * ncls * 4
    for pattern, shape, axis in (("z_fastest", (X, Y, Z), 2), ("z_slowest", (Z, X, Y), 0)):
        o, s, _ = vp.file_layout(shape, True, axis, None)
        out = torch.zeros(shape, dtype=torch.uint8, device=dev)
        prob = torch.zeros((ncls,) + shape, dtype=torch.float32, device=dev)
        ent = torch.zeros(shape, dtype=torch.float32, device=dev)
        for name, p, h, written in (("labels", None, None, B * X * Y), ("prob_entropy", prob, ent, B * X * Y * (1 + 4 * ncls + 4))):
            ms = events(lambda: K.paste_ensemble(members, B, 50, invs, (X, Y), out, o, s, prob=p, entropy=h), 50)
            nbytes = read + written
            res["ensemble_M5_%s_%s" % (name, pattern)] = {"ms_back_to_back": ms, "strides": list(s), "bytes_read": read, "bytes_written": written,
                                                          "tb_per_s": nbytes / (ms * 1e-3) / 1e12, "fraction_of_achievable_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE}
    out = torch.zeros((X, Y, Z), dtype=torch.uint8, device=dev)
    res["ensemble_M1_labels_ms"] = events(lambda: K.paste_ensemble(members[:1], B, 50, invs[:1], (X, Y), out, origin, strides), 50)
    res["paste_labels_ms"] = events(lambda: K.paste_labels(members[0], B, 50, invs[0], (X, Y), out, origin, strides), 50)
    # 4. the condition
    for name in ("labels", "prob_entropy"):
        res["gathers_plus_paste_over_forwards_%s" % name] = ((M * res["gather_ms_incl_upload_and_allocation"] + res["ensemble_M5_%s_z_fastest" % name]["ms_back_to_back"])
                                                             / (M * res["forward_ms"]))
    src.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
