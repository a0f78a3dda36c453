"""Cost of the opt-in boundary term of the segmenter step: the training step of train_segmenter at B = 16 on one GPU with
bnd_weight = 0 (the reference's step) against bnd_weight > 0, alternating the two nets round by round so that the spread of one
configuration is visible next to the difference between the two; and the two kernels alone at 16 x 256 x 256 x 5 — the signed distance
transform (labels of four ellipses per slice, as in the tests; a second set where every other slice is background only) and the loss
pass with its gradient (microseconds, and GB/s over the bytes it has to move: logits and maps read once, gradient written once).  Kernel
times are device times: `--reps` calls recorded into one hipGraph and replayed between two events, rotating over buffers that together
exceed the Infinity Cache.  Prints one JSON object (and writes it to --out)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ss = importlib.import_module("medical-cross-modality-domain-adaptation_amd.source_segmenter")
K = importlib.import_module("medical-cross-modality-domain-adaptation_amd.kernels")

COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}


def blob_onehot(rng, B, empty_every=0):
    """[B, 256, 256, 5] one-hot labels: four ellipses per slice; with empty_every = n every n-th slice is background only"""
    yy, xx = np.mgrid[0:256, 0:256]
    lab = np.zeros((B, 256, 256), np.int64)
    for b in range(B):
        if empty_every and b % empty_every == 0:
            continue
        for c in range(1, 5):
            cy, cx = rng.integers(40, 216, 2)
            ry, rx = rng.integers(12, 40, 2)
            lab[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = c
    return np.stack([(lab == c) for c in range(5)], axis=-1).astype(np.float32)


def make(B, bnd, dev):
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(COST, **({"bnd_weight": bnd} if bnd else {})), device=dev)
    rng = np.random.default_rng(0)
    sd = net.store.state_dict()
    for k, a in sd.items():
        if "/Variable" in k:
            sd[k] = (rng.standard_normal(a.shape) * np.sqrt(2.0 / np.prod(a.shape[:-1]))).astype(np.float32)
    net.store.load_state_dict(sd)
    tr = ss.Trainer(net, None, None, num_cls=5, batch_size=B, optimizer="adam", opt_kwargs={"learning_rate": 1e-3})
    tr.opt = tr._get_optimizer(100)
    return tr


def time_steps(tr, x, y, steps, seed0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        tr.train_step(x, y, 0.75, seed0 + s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def graph_time_us(fn, nbuf, reps, replays=5):
    """fn(i) launches on buffer set i; -> (median, min, max) microseconds per call over `replays` replays of `reps` recorded calls"""
    for i in range(nbuf):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for r in range(reps):
            fn(r % nbuf)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_bench(dev, reps):
    B, C = 16, 5
    P = B * 256 * 256
    nbytes = P * C * 4
    nrot = 6                        # 6 x (21 MB labels + 21 MB maps + 21 MB logits + 21 MB gradient) = 503 MB: past the 256 MiB Infinity Cache
    rng = np.random.default_rng(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    ys = [torch.from_numpy(blob_onehot(rng, B)).to(dev) for _ in range(nrot)]
    ys_empty = [torch.from_numpy(blob_onehot(rng, B, empty_every=2)).to(dev) for _ in range(nrot)]
    zs = [torch.randn((P, C), device=dev, generator=gen) * 3.0 for _ in range(nrot)]
    phis = [K.signed_distance_2d(y).reshape(P, C) for y in ys]
    keep = [None] * nrot            # outputs stay alive inside the recording: every call its own output buffers

    def sdist(i):
        keep[i] = K.signed_distance_2d(ys[i])

    def sdist_empty(i):
        keep[i] = K.signed_distance_2d(ys_empty[i])

    def loss_grad(i):
        keep[i] = K.boundary_loss(zs[i], phis[i], 4, 0.01, want_grad=True)

    def loss_value(i):
        keep[i] = K.boundary_loss(zs[i], phis[i], 4)

    res = {"B": B, "P": P, "ncls": C, "max_abs_phi": float(max(float(q.abs().max()) for q in phis))}
    # the transform: labels read, maps written, one int16 per pixel and selected class written and read
    moved = {"signed_distance_2d": 2 * nbytes + 2 * P * 4 * 2, "signed_distance_2d_half_empty": 2 * nbytes + 2 * P * 4 * 2,
             "boundary_loss_value_and_grad": 3 * nbytes, "boundary_loss_value_only": 2 * nbytes}
    for name, fn in (("signed_distance_2d", sdist), ("signed_distance_2d_half_empty", sdist_empty), ("boundary_loss_value_and_grad", loss_grad),
                     ("boundary_loss_value_only", loss_value)):
        med, lo, hi = graph_time_us(fn, nrot, reps)
        res[name] = {"us": med, "us_min": lo, "us_max": hi, "bytes": moved[name], "gb_per_s": moved[name] / (med * 1e-6) / 1e9}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--bnd-weight", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=48, help="calls per recorded graph of the kernel measurement")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch_size
    res = {"batch_size": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "bnd_weight": a.bnd_weight,
           "device": torch.cuda.get_device_name(0)}
    if not a.kernel_only:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((B, 256, 256, 3), device=dev, generator=g)
        y = torch.from_numpy(blob_onehot(np.random.default_rng(1), B)).to(dev)
        trs = {"bnd0": make(B, 0.0, dev), "bnd": make(B, a.bnd_weight, dev)}
        for tr in trs.values():
            time_steps(tr, x, y, a.warmup, 100)
        ms = {k: [] for k in trs}
        for r in range(a.rounds):                   # alternate: bnd0, bnd, bnd0, bnd, ...
            for k, tr in trs.items():
                ms[k].append(time_steps(tr, x, y, a.steps, 200 + r * a.steps))
        for k in trs:
            res["train_step_ms_" + k] = {"rounds": ms[k], "median": float(np.median(ms[k])), "min": min(ms[k]), "max": max(ms[k])}
        res["bnd_value_last"] = float(trs["bnd"].net.bnd_value)
        res["added_ms"] = res["train_step_ms_bnd"]["median"] - res["train_step_ms_bnd0"]["median"]
        res["ratio_of_medians"] = res["train_step_ms_bnd"]["median"] / res["train_step_ms_bnd0"]["median"]
        res["peak_mem_gb"] = torch.cuda.max_memory_allocated() / 1e9
        del trs, tr
        torch.cuda.empty_cache()
    res["kernels"] = kernel_bench(dev, a.reps)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
