"""Cost of Fourier domain adaptation: (1) the launch set of pnp_fda_amplitude_swap at B = Bt = 16, 256 x 256 x 3 for each
--bands value, as device time per call of --reps calls recorded into one hipGraph, median / min / max over 5 replays; (2) the fp32 source
segmenter step at B = 16 without and with the amplitude swap of its batch in front of it, alternating the two round by round on one net
so that the spread of one configuration is visible next to the difference.  The stylised step's bands and pairs come from
fda.FdaStylizer.draw (beta 0.01 ... 0.09, the FDA paper's range) and its targets are one fixed device batch: the target feeder's copy
stream is not part of the figure.  Prints one JSON object (and writes it to --out)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_entropy import K, graph_time_us      # noqa: E402  (the package comes in through bench_entropy)

PKG = "medical-cross-modality-domain-adaptation_amd"
ss = importlib.import_module(PKG + ".source_segmenter")
fda = importlib.import_module(PKG + ".fda")


def kernel_bench(dev, reps, bands, B=16, H=256, W=256, C=3):
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randn((B, H, W, C), device=dev, generator=gen)
    tgt = torch.randn((B, H, W, C), device=dev, generator=gen) * 1.5 + 0.4
    pair = np.random.default_rng(0).integers(0, B, B)
    res = {"B": B, "Bt": B, "H": H, "W": W, "C": C}
    keep = [None]
    for b in bands:
        def call(i, b=b):
            keep[0] = K.fda_amplitude_swap(src, tgt, [b] * B, pair)
        med, lo, hi = graph_time_us(call, 1, reps)
        # FMAs of the four passes (real by complex: 2, complex by complex: 4; the analyses run on the B sources and the Bt = B targets)
        nb = b + 1
        fma = 2 * (2 * B) * H * W * C * nb + 4 * (2 * B) * C * nb * (2 * b + 1) * H + 4 * B * C * nb * (2 * b + 1) * H + 2 * B * H * W * C * nb
        res["band_%d" % b] = {"us": med, "us_min": lo, "us_max": hi, "gflop": 2 * fma / 1e9, "tflop_per_s": 2 * fma / (med * 1e-6) / 1e12,
                              "workspace_bytes": int(K._lib.load().pnp_fda_workspace_bytes(B, B, H, W, C, b))}
    return res


def step_bench(dev, B, steps, warmup, rounds):
    syn = importlib.import_module(PKG + ".synthetic")
    rng = np.random.default_rng(1)
    sl = [syn.make_slice(rng) for _ in range(B)]
    x = torch.from_numpy(np.stack([a for a, _ in sl])).to(dev)
    lab = torch.from_numpy(np.stack([l[:, :, 1] for _, l in sl])).to(dev)
    y = K.label_decomp(lab, 5)
    tgt = torch.from_numpy(np.stack([syn.make_slice(rng)[0] for _ in range(B)])).to(dev)
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, seed=3,
                      cost_kwargs={"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4})
    tr = ss.Trainer(net, None, None, num_cls=5, batch_size=B, optimizer="adam", opt_kwargs={"learning_rate": 1e-3})
    tr.opt = tr._get_optimizer(100)
    sty = fda.FdaStylizer(None, beta=(0.01, 0.09), prob=1.0)
    draws = [sty.draw(B, B, 256, 256) for _ in range(steps)]
    counter = [0]

    def run(on, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(n):
            bx = K.fda_amplitude_swap(x, tgt, *draws[s % len(draws)]) if on else x
            tr.train_step(bx, y, 0.75, counter[0])
            counter[0] += 1
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    run(False, warmup)
    run(True, warmup)
    ms = {"without": [], "with": []}
    for _ in range(rounds):                     # alternate: without, with, without, with, ...
        ms["without"].append(run(False, steps))
        ms["with"].append(run(True, steps))
    res = {k: {"rounds": v, "median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in ms.items()}
    res["difference_of_medians_ms"] = res["with"]["median"] - res["without"]["median"]
    res["bands_drawn"] = sorted({int(b) for d in draws for b in d[0]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=64, help="calls per recorded graph of the kernel measurement")
    ap.add_argument("--bands", default="2,12,23")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"batch_size": a.batch_size, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    res["kernels"] = kernel_bench(dev, a.reps, [int(b) for b in a.bands.split(",")], B=a.batch_size)
    if not a.kernel_only:
        res["segmenter_step_ms"] = step_bench(dev, a.batch_size, a.steps, a.warmup, a.rounds)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
