"""Cost of the opt-in pseudo-label term of the generator step, after tools/bench_entropy.py: the joint step (one dis step and
one gen step) of --phase train-gan at B = 16 on one GPU with pl_weight = 0 (the reference's step) against pl_weight > 0, alternating the
two nets round by round so that the spread of one configuration is visible next to the difference between the two; the loss launch pair
alone on logits [--pixels, 5] (default 16 * 256 * 256) next to pnp_softmax_entropy with a gradient on the same logits in the same process
(the pseudo-label pass writes 5 more bytes per pixel: the class byte and the confidence); and the threshold update alone, all nine
launches.  Kernel times are device times: `--reps` calls recorded into one hipGraph and replayed between two events, once on one buffer
set (it stays in the Infinity Cache) and once rotating over sets larger than it together (HBM).  Prints one JSON object (and writes it
to --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_entropy import K, NETCFG, adv, graph_time_us      # noqa: E402  (the package comes in through bench_entropy)


def make(B, pl, dev):
    ck = {"regularizer": 1e-4, "gan_regularizer": 1e-4, "miu_gen": 0.002, "miu_dis": 0.002, "lambda_mask_loss": 0.3}
    if pl:
        ck.update(pl_weight=pl, pl_init=0.9, pl_portion=0.5, pl_momentum=0.9)
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


def time_steps(tr, mr, ct, steps, seed0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(steps):
        tr.dis_step(mr, ct, 0.75, seed0 + 2 * s)
        tr.gen_step(ct, 0.75, seed0 + 2 * s + 1)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def kernel_bench(dev, reps, P):
    C = 5
    nbytes = P * C * 4
    nrot = 8                        # at the default P: 8 x (21 MB logits + 21 MB gradient + 5 MB maps) = 376 MB: past the 256 MiB Infinity Cache
    gen = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn((P, C), device=dev, generator=gen) * 3.0 for _ in range(nrot)]
    tau = torch.tensor([0.9, 0.8, 0.85, 0.7, 0.75], device=dev)
    maps = [K.pseudo_label_loss(z, tau)[3:5] for z in zs]          # (labels, conf) of every buffer: the update's inputs
    taus = [tau.clone() for _ in range(nrot)]
    keep = [None] * nrot            # outputs stay alive inside the recording: every call its own buffers

    def pl_grad(i):
        keep[i] = K.pseudo_label_loss(zs[i], tau, None, 0.01, want_grad=True)

    def pl_value(i):
        keep[i] = K.pseudo_label_loss(zs[i], tau)

    def ent_grad(i):
        keep[i] = K.softmax_entropy(zs[i], 0.01, want_grad=True)

    def update(i):
        keep[i] = K.pseudo_label_update(maps[i][0], maps[i][1], taus[i], 0.5, 0.9)

    res = {"P": P, "ncls": C}
    # the update reads the byte and the float in each of its four rounds
    moved = {"pseudo_label_value_and_grad": 2 * nbytes + 5 * P, "pseudo_label_value_only": nbytes + 5 * P, "entropy_value_and_grad": 2 * nbytes,
             "pseudo_label_update": 4 * 5 * P}
    for name, fn in (("pseudo_label_value_and_grad", pl_grad), ("pseudo_label_value_only", pl_value), ("entropy_value_and_grad", ent_grad),
                     ("pseudo_label_update", update)):
        for mode, nbuf in (("one_buffer", 1), ("rotating", nrot)):
            med, lo, hi = graph_time_us(fn, nbuf, reps)
            res["%s_%s" % (name, mode)] = {"us": med, "us_min": lo, "us_max": hi, "bytes": moved[name], "gb_per_s": moved[name] / (med * 1e-6) / 1e9}
    for mode in ("one_buffer", "rotating"):
        res["loss_over_entropy_" + mode] = res["pseudo_label_value_and_grad_" + mode]["us"] / res["entropy_value_and_grad_" + mode]["us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pl-weight", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=64, help="calls per recorded graph of the kernel measurement")
    ap.add_argument("--pixels", type=int, default=16 * 256 * 256, help="P of the kernel measurement (2048 * 2048: the grid cap of the loss)")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch_size
    res = {"batch_size": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "pl_weight": a.pl_weight,
           "device": torch.cuda.get_device_name(0)}
    if not a.kernel_only:
        g = torch.Generator(device=dev).manual_seed(1)
        ct = torch.randn((B, 256, 256, 3), device=dev, generator=g)
        mr = torch.randn((B, 256, 256, 3), device=dev, generator=g)
        trs = {"pl0": make(B, 0.0, dev), "pl": make(B, a.pl_weight, dev)}
        for tr in trs.values():
            time_steps(tr, mr, ct, a.warmup, 100)
        ms = {k: [] for k in trs}
        for r in range(a.rounds):                   # alternate: pl0, pl, pl0, pl, ...
            for k, tr in trs.items():
                ms[k].append(time_steps(tr, mr, ct, a.steps, 200 + 2 * r * a.steps))
        for k in trs:
            res["joint_step_ms_" + k] = {"rounds": ms[k], "median": float(np.median(ms[k])), "min": min(ms[k]), "max": max(ms[k])}
        net = trs["pl"].net
        res["pl_value_last"], res["pl_share_last"] = float(net.pl_value), float(net.pl_share)
        res["pl_threshold_last"] = net.pl_threshold.tolist()
        res["difference_of_medians_ms"] = res["joint_step_ms_pl"]["median"] - res["joint_step_ms_pl0"]["median"]
        res["peak_mem_gb"] = torch.cuda.max_memory_allocated() / 1e9
        del trs, tr, net
        torch.cuda.empty_cache()
    res["kernels"] = kernel_bench(dev, a.reps, a.pixels)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
