"""Cost of the opt-in entropy term of the generator step: the gen step of --phase train-gan at B = 16 on one GPU with
ent_weight = 0 (the reference's step) against ent_weight > 0, alternating the two nets round by round so that the spread of one
configuration is visible next to the difference between the two; and the entropy launch pair alone on logits [16 * 256 * 256, 5]
(microseconds and GB/s over the bytes it has to move: logits read once, gradient written once) next to the existing seg_loss_fwd +
seg_loss_bwd pair on the same logits.  Kernel times are device times: `--reps` calls recorded into one hipGraph and replayed between two
events, once on one buffer (the 42 MB stay in the Infinity Cache) and once rotating over buffers larger than it together (HBM).
Prints one JSON object (and writes it to --out)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
adv = importlib.import_module("medical-cross-modality-domain-adaptation_amd.adversarial")
K = importlib.import_module("medical-cross-modality-domain-adaptation_amd.kernels")

NETCFG = {"mr_front_trainable": False, "joint_trainable": False, "ct_front_trainable": True, "cls_trainable": True, "m_cls_trainable": True}


def make(B, ent, dev):
    ck = {"regularizer": 1e-4, "gan_regularizer": 1e-4, "miu_gen": 0.002, "miu_dis": 0.002, "lambda_mask_loss": 0.3}
    if ent:
        ck["ent_weight"] = ent
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=ck, network_config=dict(NETCFG), device=dev)
    rng = np.random.default_rng(0)
    sd = net.store.state_dict()
    for k, a in sd.items():
        if "Variable" in k:
            sd[k] = (rng.standard_normal(a.shape) * np.sqrt(2.0 / np.prod(a.shape[:-1]))).astype(np.float32)
    net.store.load_state_dict(sd)
    tr = adv.Trainer(net, None, None, None, None, num_cls=5, batch_size=B, opt_kwargs={"learning_rate": 3e-4},
                     train_config={"dis_sub_iter": 1, "gen_sub_iter": 1})
    tr._get_optimizer()
    return tr


def time_steps(tr, ct, steps, seed0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        tr.gen_step(ct, 0.75, seed0 + s)
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
    P, C = 16 * 256 * 256, 5
    nbytes = P * C * 4
    nrot = 8                        # 8 x (21 MB logits + 21 MB gradient [+ 21 MB labels]) = 336 MB and more: past the 256 MiB Infinity Cache
    gen = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn((P, C), device=dev, generator=gen) * 3.0 for _ in range(nrot)]
    ys = [torch.nn.functional.one_hot(torch.randint(0, C, (P,), device=dev, generator=gen), C).float().contiguous() for _ in range(nrot)]
    keep = [None] * nrot            # outputs stay alive inside the recording: every call its own gradient buffer

    def ent_grad(i):
        keep[i] = K.softmax_entropy(zs[i], 0.01, want_grad=True)

    def ent_value(i):
        keep[i] = K.softmax_entropy(zs[i])

    def seg_pair(i):
        out, ws = K.seg_loss_fwd(zs[i], ys[i], 1.0, 1.0)
        keep[i] = (out, K.seg_loss_bwd(zs[i], ys[i], ws, 1.0, 1.0, 1.0))

    res = {"P": P, "ncls": C}
    moved = {"entropy_value_and_grad": 2 * nbytes, "entropy_value_only": nbytes, "seg_loss_fwd_plus_bwd": 5 * nbytes}
    for name, fn in (("entropy_value_and_grad", ent_grad), ("entropy_value_only", ent_value), ("seg_loss_fwd_plus_bwd", seg_pair)):
        for mode, nbuf in (("one_buffer", 1), ("rotating", nrot)):
            med, lo, hi = graph_time_us(fn, nbuf, reps)
            res["%s_%s" % (name, mode)] = {"us": med, "us_min": lo, "us_max": hi, "bytes": moved[name], "gb_per_s": moved[name] / (med * 1e-6) / 1e9}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--ent-weight", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=64, help="calls per recorded graph of the kernel measurement")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch_size
    res = {"batch_size": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ent_weight": a.ent_weight,
           "device": torch.cuda.get_device_name(0)}
    if not a.kernel_only:
        g = torch.Generator(device=dev).manual_seed(1)
        ct = torch.randn((B, 256, 256, 3), device=dev, generator=g)
        trs = {"ent0": make(B, 0.0, dev), "ent": make(B, a.ent_weight, dev)}
        for tr in trs.values():
            time_steps(tr, ct, a.warmup, 100)
        ms = {k: [] for k in trs}
        for r in range(a.rounds):                   # alternate: ent0, ent, ent0, ent, ...
            for k, tr in trs.items():
                ms[k].append(time_steps(tr, ct, a.steps, 200 + r * a.steps))
        for k in trs:
            res["gen_step_ms_" + k] = {"rounds": ms[k], "median": float(np.median(ms[k])), "min": min(ms[k]), "max": max(ms[k])}
        res["ent_value_last"] = float(trs["ent"].net.ent_value)
        res["ratio_of_medians"] = res["gen_step_ms_ent"]["median"] / res["gen_step_ms_ent0"]["median"]
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
