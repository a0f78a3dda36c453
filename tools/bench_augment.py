"""Cost of the NIfTI training input (volume_source.py, csrc/augment.hip) on one GPU: a seeded set of 16 volumes of
256 x 256 x 200, batches of 16 slices of 256 x 256.  Records
  1. the preprocess time per volume (pnp_volume_preprocess, device-synchronised, in place),
  2. the sustained device-synchronised slices/s of ONE AugmentedSliceSource (parameter draw, upload and gather; default augmentation),
     against the fastest consumer of the project (the fp32 segmenter step, 1028 slices/s): the source must sustain at least 4x that,
  3. the gather kernel alone by HIP events around back-to-back launches of one fixed batch, as bytes written per second (the kernel is
     write-bound: 12 B image + 4 B label + 4 ncls B one-hot per pixel) against the 6.3 TB/s achievable HBM figure — the per-kernel figure
     of record comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py --profile-step` run,
  4. for scale, a CPU figure: the same batch (affine map, bilinear image, nearest label) built with numpy on 16 host threads.
With --sample-mm the source samples on a millimetre grid — the volumes get the voxel size of --voxel-mm, the gather is
pnp_aug_slices_z with a fractional frame step — and the host figure is left out; the default --out is then profiles/spacing_timing.json.
With --augment JSON the source uses those ranges; with one of the elastic / intensity keys the gather is pnp_aug_slices_warp, the
host figure is left out and the default --out is profiles/warp_timing.json.
Prints one JSON object and writes it to --out (default profiles/augment_timing.json)."""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "medical-cross-modality-domain-adaptation_amd"
vs = importlib.import_module(PKG + ".volume_source")
K = importlib.import_module(PKG + ".kernels")

FASTEST_CONSUMER = 1028.0      # slices/s, fp32 segmenter step at B = 16 (README / BASELINE)
HBM_ACHIEVABLE = 6.3e12


def make_volumes(nvol, shape, dev, seed=0):
    """intensity volumes with a bright tail and blocky labels, generated on the device (the host never holds the set)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    images, labels = [], []
    for _ in range(nvol):
        v = torch.randn(shape, device=dev, generator=g) * 200 + 300
        lab = (torch.rand((shape[0] // 16, shape[1] // 16, shape[2]), device=dev, generator=g) * 5).to(torch.uint8)
        lab = lab.repeat_interleave(16, 0).repeat_interleave(16, 1).contiguous()
        images.append(v + lab.float() * 150)
        labels.append(lab)
    return images, labels


def volume_set(images, labels, dev):
    """a VolumeSet over device tensors, timing the preprocess per volume"""
    self = vs.VolumeSet.__new__(vs.VolumeSet)
    self.device, self.names, self.percentile = dev, ["v%02d.nii.gz" % i for i in range(len(images))], 98
    self.images, self.labels, stats, ms = [], [], [], []
    for v, lab in zip(images, labels):
        K.volume_preprocess(v.clone(), 98)         # warm-up on a copy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, st = K.volume_preprocess(v, 98, out=v)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        self.images.append(v)
        self.labels.append(lab)
        stats.append(st)
    self.dims = [tuple(int(d) for d in v.shape) for v in self.images]
    host = torch.stack(stats).cpu().numpy()
    self.stats = [{"clip": float(r[0]), "mean": float(r[1]), "std": float(r[2]), "fill": float(r[3])} for r in host]
    self.set_fill(None)
    return self, ms


def host_batch(vols, labs, rec, H, W, fills, threads=16):
    """the same batch with numpy: one sample per task"""
    def one(b):
        v, z, m = int(rec["volume"][b]), int(rec["frame"][b]), rec["m"][b].astype(np.float64)
        vol, lab = vols[v], labs[v]
        X, Y = vol.shape[:2]
        i = np.arange(H, dtype=np.float64)[:, None]
        j = np.arange(W, dtype=np.float64)[None, :]
        sx, sy = m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]
        x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        tx, ty = (sx - x0)[..., None].astype(np.float32), (sy - y0)[..., None].astype(np.float32)
        fr = vol[:, :, z - 1:z + 2]

        def at(x, y):
            ok = (x >= 0) & (x < X) & (y >= 0) & (y < Y)
            return np.where(ok[..., None], fr[np.clip(x, 0, X - 1), np.clip(y, 0, Y - 1)], np.float32(fills[v]))
        a = at(x0, y0) * (1 - ty) + at(x0, y0 + 1) * ty
        c = at(x0 + 1, y0) * (1 - ty) + at(x0 + 1, y0 + 1) * ty
        img = a * (1 - tx) + c * tx
        lx, ly = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
        ok = (lx >= 0) & (lx < X) & (ly >= 0) & (ly < Y)
        return img, np.where(ok, lab[np.clip(lx, 0, X - 1), np.clip(ly, 0, Y - 1), z], 0).astype(np.float32)
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(len(rec))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    vs.add_sample_mm_flag(ap)
    ap.add_argument("--augment", default=None, metavar="JSON", help="augmentation ranges of the source (volume_source's --augment); default: DEFAULT_AUGMENT")
    ap.add_argument("--voxel-mm", default="0.8,0.8,1.6", help="with --sample-mm: the voxel size of every volume, slicing order")
    ap.add_argument("--profile-step", action="store_true", help="2 volumes, 20 batches, no host figure: for a rocprofv3 --kernel-trace run")
    a = ap.parse_args()
    sample_mm = vs.sample_mm_from_args(ap, a)
    a.no_augment = False            # (augment_from_args reads the pair of flags volume_source.add_augment_flags defines)
    try:
        augment = vs.augment_from_args(a)
    except ValueError as e:
        ap.error(str(e))
    warp = vs.uses_warp_entry(augment)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "warp_timing.json" if warp else "augment_timing.json" if sample_mm is None else "spacing_timing.json")
    dev = torch.device("cuda:0")
    shape, H, W, B, ncls = (256, 256, 200), 256, 256, a.batch_size, 5
    nvol = 2 if a.profile_step else a.volumes
    images, labels = make_volumes(nvol, shape, dev)
    vset, pre_ms = volume_set(images, labels, dev)
    vset.spacings = [vs.check_spacing(a.voxel_mm.split(","), "--voxel-mm")] * nvol
    src = vs.AugmentedSliceSource(vset, B, out_size=(H, W), augment=augment, seed=0, num_cls=ncls, sample_mm=sample_mm)
    entry = "pnp_aug_slices_warp" if warp else "pnp_aug_slices" if sample_mm is None else "pnp_aug_slices_z"
    if a.profile_step:
        for _ in range(20):
            src.next_device_batch()
        if warp:
            # the same records without warp and intensity through pnp_aug_slices_z, 20 launches: the two kernels side by side in one trace
            rz = np.zeros(B, dtype=vs.SAMPLE_Z_DTYPE)
            for f in rz.dtype.names:
                rz[f] = src.last_params[f]
            sz = torch.from_numpy(rz.view(np.uint8).copy()).to(dev)
            for _ in range(20):
                K.aug_slices_z(vset.table_host, vset.table_dev, nvol, sz, B, H, W, src._errors, ncls=ncls)
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": True, "errors": src.errors()}))
        return
    res = {"device": torch.cuda.get_device_name(0), "volumes": nvol, "volume_shape": list(shape), "batch_size": B, "out_size": [H, W],
           "num_cls": ncls, "augment": src.augment, "sample_mm": sample_mm, "voxel_mm": vset.spacings[0] if sample_mm else None,
           "gather_entry": entry, "preprocess_ms_per_volume": {"median": float(np.median(pre_ms)), "min": min(pre_ms), "max": max(pre_ms)}}
    # 2. the source, end to end, synchronised at the end of the timed region only (the trainers never synchronise on it either)
    for _ in range(a.warmup):
        src.next_device_batch()
    torch.cuda.synchronize()
    rates = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(a.batches):
            out = src.next_device_batch()
        torch.cuda.synchronize()
        rates.append(a.batches * B / (time.perf_counter() - t0))
    res["source_slices_per_s"] = {"median": float(np.median(rates)), "runs": rates}
    res["fastest_consumer_slices_per_s"] = FASTEST_CONSUMER
    res["source_over_fastest_consumer"] = float(np.median(rates)) / FASTEST_CONSUMER
    # per batch with a synchronisation after every batch (latency of one batch, not throughput)
    t0 = time.perf_counter()
    for _ in range(50):
        src.next_device_batch()
        torch.cuda.synchronize()
    res["batch_latency_ms_synchronised_each"] = (time.perf_counter() - t0) / 50 * 1e3
    # 3. the kernel alone
    rec = src.last_params.copy()
    reps = 50
    sd = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    if warp:
        cd = None if src.last_ctrl is None else torch.from_numpy(src.last_ctrl).to(dev)
        G = 0 if cd is None else cd.shape[1] - 3
        gather = lambda th, td, n, s, *rest, **kw: K.aug_slices_warp(th, td, n, s, cd, G, *rest, **kw)
    else:
        gather = K.aug_slices if sample_mm is None else K.aug_slices_z
    for want in (True, False):
        for _ in range(3):
            gather(vset.table_host, vset.table_dev, nvol, sd, B, H, W, src._errors, ncls=ncls, want_onehot=want)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            gather(vset.table_host, vset.table_dev, nvol, sd, B, H, W, src._errors, ncls=ncls, want_onehot=want)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        nbytes = B * H * W * (12 + 4 + (4 * ncls if want else 0))
        res["gather_kernel_onehot" if want else "gather_kernel_no_onehot"] = {
            "ms_back_to_back_incl_output_allocation": ms, "bytes_written": nbytes, "tb_per_s_written": nbytes / (ms * 1e-3) / 1e12,
            "fraction_of_achievable_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE}
    res["errors"] = src.errors()
    if sample_mm is not None or warp:
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    # 4. CPU figure for scale
    vols = [v.cpu().numpy() for v in vset.images[:4]]
    labs = [l.cpu().numpy() for l in vset.labels[:4]]
    rec4 = rec.copy()
    rec4["volume"] %= 4
    fills = [s["fill"] for s in vset.stats]
    host_batch(vols, labs, rec4, H, W, fills)
    t0 = time.perf_counter()
    for _ in range(3):
        host_batch(vols, labs, rec4, H, W, fills)
    dt = (time.perf_counter() - t0) / 3
    res["cpu_numpy_16_threads"] = {"note": "CPU figure: the same B = 16 batch built with numpy, one sample per task on 16 threads",
                                   "ms_per_batch": dt * 1e3, "slices_per_s": B / dt}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
