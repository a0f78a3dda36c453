"""-m gpu: csrc/augment.hip against the float64 restatement of tests/augment_ref.py — the exact clip quantile, the
moments and the normalised volume of pnp_volume_preprocess; image, label and one-hot of pnp_aug_slices over its domain; then the feature
through the product: train_segmenter / train_gan from NIfTI lists, the feeder hand-off, the numpy view and the tfrecord export.

Bounds (derived, not tuned):
  moments   1e-9 relative.  A sum is conditioned by sum|x|, so the mean is held to 1e-9 of mean|min(v, clip)| (which is 1e-9 of |mean|
            itself wherever the values do not cancel: every case below but `negative_and_zero_signs`), the std to 1e-9 of itself.
  output    4 * 2^-24 * max(1, max|out|): the float64 value rounded once, with margin.
  image     eps (Gx + Gy) + 4 * 2^-24 max|v|: bilinear-with-fill is Lipschitz in the coordinates with constants Gx, Gy = the largest gap
            between face-adjacent voxels (fill at the border included); eps = 4 float32 ulps at the largest coordinate term.
  label     no pixel excluded: the output is one of the (at most four) labels at floor(s + 0.5) for s -+ eps on either axis.
"""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


# ---- pnp_volume_preprocess -------------------------------------------------------------------------------------------------------------
def _pre_case(name):
    rng = np.random.default_rng(len(name))
    if name == "ties":
        return rng.integers(0, 4, 5000).astype(np.float32)
    if name == "constant":
        return np.full(777, 2.5, np.float32)
    if name == "negative_only":
        return (-np.abs(rng.standard_normal(3001)) * 100 - 1).astype(np.float32)
    if name == "negative_and_zero_signs":
        return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0, -2.0], np.float32), 4097)
    if name == "zeros_of_both_signs":
        return rng.choice(np.array([-0.0, 0.0], np.float32), 999)
    if name == "one":
        return np.array([-3.25], np.float32)
    if name == "two":
        return np.array([4.0, -1.0], np.float32)
    if name == "prime":
        return (rng.standard_normal(10007) * 300 + 1000).astype(np.float32)
    if name == "tiny_and_huge":
        return np.concatenate([rng.standard_normal(500) * 1e-30, rng.standard_normal(500) * 1e30, [0.0]]).astype(np.float32)
    if name == "volume":
        # an MMWHS-sized volume: CT-like intensities with a bright tail
        v = rng.standard_normal((256, 256, 200), dtype=np.float32) * 200 + 300
        v[::7, ::5, ::3] += 3000
        return v
    raise KeyError(name)


@pytest.mark.parametrize("name", ["ties", "constant", "negative_only", "negative_and_zero_signs", "zeros_of_both_signs", "one", "two", "prime",
                                  "tiny_and_huge", "volume"])
def test_preprocess_against_the_restatement(dev, name):
    K = pkg("kernels")
    v = _pre_case(name)
    ref, st = R.preprocess(v)
    vd = torch.from_numpy(v).to(dev)
    out, stats = K.volume_preprocess(vd)
    out2, stats2 = K.volume_preprocess(vd)
    got, s = out.cpu().numpy(), stats.cpu().numpy()
    print(name, "clip", s[0], st["clip"], "mean", s[1], st["mean"], "std", s[2], st["std"], "max|out - ref|", np.abs(got - ref).max())
    assert np.array_equal(got.view(np.uint32), out2.cpu().numpy().view(np.uint32)) and np.array_equal(s.view(np.uint64), stats2.cpu().numpy().view(np.uint64))
    assert s[0] == st["clip"]                                             # equal by value (-0.0 == +0.0)
    k = R.clip_index(v.size)
    assert s[0] == np.partition(v.ravel(), k)[k]
    scale = np.abs(np.minimum(v.astype(np.float64), st["clip"])).mean()
    assert abs(s[1] - st["mean"]) <= 1e-9 * scale
    if name != "negative_and_zero_signs" and scale > 0:
        assert abs(s[1] - st["mean"]) <= 1e-9 * abs(st["mean"])         # no cancellation: relative to the mean itself
    assert abs(s[2] - st["std"]) <= 1e-9 * st["std"]
    if st["std"] == 0:
        assert s[2] == 0 and not got.any() and s[3] == 0
    assert got.shape == v.shape and np.abs(got - ref).max() <= 4 * U * max(1.0, np.abs(ref).max())
    assert s[3] == got.min()
    # in place, and a percentile other than the default
    for pct in ((0, 50, 100) if v.size < (1 << 20) else ()):
        refp, stp = R.preprocess(v, pct)
        w = vd.clone()
        o, sp = K.volume_preprocess(w, pct, out=w)
        assert o is w and sp[0].item() == stp["clip"] and np.abs(w.cpu().numpy() - refp).max() <= 4 * U * max(1.0, np.abs(refp).max())


def test_preprocess_needs_contiguous_float32_on_the_device(dev):
    K, L = pkg("kernels"), pkg("_lib")
    with pytest.raises(L.PnpError):
        K.volume_preprocess(torch.zeros(8))
    with pytest.raises(L.PnpError):
        K.volume_preprocess(torch.zeros(8, dtype=torch.float64, device=dev))
    with pytest.raises(L.PnpError, match="percentile"):
        K.volume_preprocess(torch.zeros(8, device=dev), 101)


# ---- pnp_aug_slices --------------------------------------------------------------------------------------------------------------------
def _blob_volume(rng, shape, ncls_max=5):
    """smooth blobs of labels 1 .. ncls_max-1 on a noisy background; intensities depend on the label"""
    X, Y, Z = shape
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).astype(np.float64)
    lab = np.zeros(shape, np.uint8)
    for c in range(1, ncls_max):
        ctr = rng.uniform(0.2, 0.8, 3) * np.array(shape)
        rad = rng.uniform(0.15, 0.3) * min(X, Y)
        lab[(((g - ctr) / np.array([1, 1, max(Z / min(X, Y), 0.05) * 4])) ** 2).sum(-1) < rad ** 2] = c
    img = (rng.standard_normal(shape) * 40 + 100 + lab * 150.0).astype(np.float32)
    return img, lab


@pytest.fixture(scope="module")
def small_set(dev):
    """four small volumes: odd, non-square, below and above 256, Z = 3; labels up to 7 in the last one (beyond ncls = 5)"""
    vs = pkg("volume_source")
    rng = np.random.default_rng(11)
    shapes = [(37, 29, 5), (64, 80, 3), (300, 270, 4), (9, 261, 6)]
    pairs = [_blob_volume(rng, s, 8 if i == 3 else 5) for i, s in enumerate(shapes)]
    vset = vs.VolumeSet.from_arrays([p[0] for p in pairs], [p[1] for p in pairs], ["v%d.nii.gz" % i for i in range(4)], dev)
    host = [(v.cpu().numpy(), l.cpu().numpy()) for v, l in zip(vset.images, vset.labels)]
    return vset, host


def _records(vs, vset, out_hw, specs):
    rec = np.zeros(len(specs), dtype=vs.SAMPLE_DTYPE)
    for b, (v, z, kw) in enumerate(specs):
        rec["volume"][b], rec["frame"][b] = v, z
        X, Y, _ = vset.dims[v]
        rec["m"][b] = kw if isinstance(kw, np.ndarray) else vs.compose_matrix((X, Y), out_hw, **kw)
    return rec


def _check_batch(vset, host, rec, out_hw, x, label, onehot, ncls):
    K = pkg("kernels")
    H, W = out_hw
    xg, lg = x.cpu().numpy(), label.cpu().numpy()
    eps = R.coord_eps(rec["m"], H, W)
    worst = 0.0
    for b in range(len(rec)):
        v, z = int(rec["volume"][b]), int(rec["frame"][b])
        vol, lab = host[v]
        fill = np.float64(np.float32(vset.stats[v]["fill"]))
        sx, sy = R.coords(rec["m"][b], H, W)
        ref = R.gather_image(vol, z, sx, sy, fill)
        Gx, Gy = R.adjacent_gap(vol, fill)
        bound = eps * (Gx + Gy) + 4 * U * max(float(np.abs(vol).max()), abs(fill))
        err = float(np.abs(xg[b] - ref).max())
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
        cand = R.label_candidates(lab, z, sx, sy, eps)
        assert np.all((lg[b][None] == cand).any(axis=0)), (b, int((~(lg[b][None] == cand).any(axis=0)).sum()))
    if onehot is not None:
        assert torch.equal(onehot, K.label_decomp(label, ncls))
        assert np.array_equal(onehot.cpu().numpy(), R.onehot(lg, ncls))
    print("image error / bound, worst sample: %.3f (eps %.3e)" % (worst, eps))


CASES = {
    # out size, ncls, [(volume, frame, compose_matrix kwargs | six entries)]
    "mixed_B6": ((32, 48), 5, [(0, 1, {}), (0, 3, {"rotate": 90.0}), (1, 1, {"rotate": 33.0, "scale": 1.3, "translate": (2.5, -4.0)}),
                               (1, 1, {"flip": True, "rotate": -12.5}), (0, 2, {"scale": 0.2, "rotate": 5.0}),
                               (0, 1, np.array([0, 0, -0.75, 0, 0, 28.25], np.float32))]),      # every pixel between the border and the fill
    "tail_17x23_B3": ((17, 23), 3, [(3, 1, {"rotate": 7.0}), (3, 4, {"scale": 0.7, "translate": (0.0, 30.0)}), (0, 2, {"rotate": 180.0})]),
    "above_256_B1": ((256, 256), 5, [(2, 2, {"rotate": 0.0, "scale": 1.0})]),
    "above_256_rot_B2": ((260, 250), 32, [(2, 1, {"rotate": 45.0, "scale": 0.8}), (2, 2, {"rotate": 270.0, "flip": True})]),
    "one_pixel_B1": ((1, 1), 1, [(0, 1, {})]),
    "labels_beyond_ncls_B2": ((40, 300), 5, [(3, 2, {}), (3, 3, {"rotate": 3.0})]),
    "far_outside_B2": ((16, 16), 5, [(0, 1, np.array([1e6, 0, -3e7, 0, 1e6, 5], np.float32)), (1, 1, np.array([0, -3e9, 1e10, 1e-3, 0, 0], np.float32))]),
    "B16": ((8, 12), 5, [(b % 4, 1, {"rotate": 23.0 * b, "scale": 0.5 + 0.1 * b, "translate": (b - 8.0, 0.5 * b), "flip": bool(b & 1)}) for b in range(16)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_gather_against_the_restatement(dev, small_set, case):
    vs = pkg("volume_source")
    vset, host = small_set
    out_hw, ncls, specs = CASES[case]
    src = vs.AugmentedSliceSource(vset, len(specs), out_size=out_hw, augment=None, num_cls=ncls)
    rec = _records(vs, vset, out_hw, specs)
    x, label, onehot = src.gather_records(rec, ncls, True)
    assert x.shape == (len(specs),) + out_hw + (3,) and label.shape == (len(specs),) + out_hw and onehot.shape == label.shape + (ncls,)
    _check_batch(vset, host, rec, out_hw, x, label, onehot, ncls)
    x2, label2, none = src.gather_records(rec, ncls, False)
    assert none is None and torch.equal(x, x2) and torch.equal(label, label2)
    assert src.errors() == 0
    if case == "far_outside_B2":
        fill = np.float32(vset.stats[0]["fill"])
        assert np.all(x[0].cpu().numpy() == fill) and np.all(x[1].cpu().numpy() == np.float32(vset.stats[1]["fill"])) and not label.any()
    if case == "labels_beyond_ncls_B2":
        assert float(label.max()) >= 5 and bool((onehot.sum(-1) == 0).any())
    if case == "mixed_B6":
        assert float((x[4] == np.float32(vset.stats[0]["fill"])).float().mean()) > 0.5       # scale 0.2: most of the output is outside


def test_identity_on_a_256_volume_is_the_raw_frames(dev):
    vs = pkg("volume_source")
    rng = np.random.default_rng(2)
    img, lab = _blob_volume(rng, (256, 256, 5))
    vset = vs.VolumeSet.from_arrays([img], [lab], ["whole.nii"], dev)
    src = vs.AugmentedSliceSource(vset, 3, augment=None)
    rec = _records(vs, vset, (256, 256), [(0, 1, {}), (0, 3, {}), (0, 2, {})])
    assert np.array_equal(rec["m"][0], np.array([1, 0, 0, 0, 1, 0], np.float32))
    x, label, onehot = src.gather_records(rec, 5, True)
    v = vset.images[0]
    for b, z in enumerate((1, 3, 2)):
        assert torch.equal(x[b].view(torch.int32), v[:, :, z - 1:z + 2].contiguous().view(torch.int32))
        assert torch.equal(label[b], vset.labels[0][:, :, z].float())
    assert torch.equal(onehot, pkg("kernels").label_decomp(label, 5))
    # the source's own draws with augment=None are these identity maps
    xs, oh, fids = src.next_device_batch()
    for b, fid in enumerate(fids):
        name, z = fid.split("#")
        assert name == "whole.nii" and torch.equal(xs[b], v[:, :, int(z) - 1:int(z) + 2])
    assert src.errors() == 0
    src.close()


def test_out_of_range_samples_are_refused_without_a_fault(dev, small_set):
    vs, L = pkg("volume_source"), pkg("_lib")
    vset, host = small_set
    out_hw = (10, 14)
    src = vs.AugmentedSliceSource(vset, 7, out_size=out_hw, augment=None)
    ident = np.array([1, 0, 0, 0, 1, 0], np.float32)
    specs = [(0, 0, ident), (0, 4, ident), (0, 2, ident), (-1, 1, ident), (4, 1, ident), (1, 2, ident), (1, 1, ident)]
    rec = _records(vs, vset, out_hw, [(v if 0 <= v < 4 else 0, z, m) for v, z, m in specs])
    rec["volume"] = [s[0] for s in specs]
    x, label, onehot = src.gather_records(rec, 5, True)
    bad = [0, 1, 3, 4, 5]                      # frame 0, frame Z - 1, volume -1, volume nvol, frame Z - 1 of a Z = 3 volume
    for b in bad:
        v = int(rec["volume"][b])
        fill = np.float32(vset.stats[v]["fill"]) if 0 <= v < 4 else np.float32(0)
        assert bool((x[b] == float(fill)).all()) and not label[b].any() and bool((onehot[b, :, :, 0] == 1).all()) and not onehot[b, :, :, 1:].any()
    good = [2, 6]
    _check_batch(vset, host, rec[good], out_hw, x[good], label[good], None, 5)
    assert src.errors() == len(bad)
    src.gather_records(rec[:2], 5, False)
    assert src.errors() == len(bad) + 2        # the counter is added to, never reset
    with pytest.raises(L.PnpError, match="refused 7 samples"):
        src.close()


# ---- through the product ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nii_lists(tmp_path_factory):
    """three 256 x 256 x 6 blob volumes written with nifti.save, a training and a validation list"""
    nifti = pkg("nifti")
    root = tmp_path_factory.mktemp("nii")
    rng = np.random.default_rng(5)
    lines = []
    for n in range(3):
        img, lab = _blob_volume(rng, (256, 256, 6))
        nifti.save(nifti.Nifti1Image(img, np.diag([1.0, 1.0, 2.0, 1.0])), str(root / ("s%d_image.nii.gz" % n)))
        nifti.save(nifti.Nifti1Image(lab.astype(np.int16), np.diag([1.0, 1.0, 2.0, 1.0])), str(root / ("s%d_label.nii.gz" % n)))
        lines.append("s%d_image.nii.gz s%d_label.nii.gz" % (n, n))
    (root / "train_list").write_text("\n".join(lines) + "\n")
    (root / "val_list").write_text(lines[2] + "\n")
    return str(root / "train_list"), str(root / "val_list"), str(root)


def test_train_segmenter_and_gan_from_nifti_lists(dev, nii_lists, tmp_path, monkeypatch):
    ts, tg, ss, nifti = pkg("train_segmenter"), pkg("train_gan"), pkg("source_segmenter"), pkg("nifti")
    train_list, val_list, root = nii_lists
    seen = []
    orig = ss.Trainer.train_step

    def spy(self, batch_x, batch_y, dropout, step):
        if not seen:
            seen.append((batch_x.clone(), batch_y.clone()))
        return orig(self, batch_x, batch_y, dropout, step)
    monkeypatch.setattr(ss.Trainer, "train_step", spy)
    fids = []
    feed_next = pkg("feeder").DeviceFeeder.next

    def next_spy(self):
        r = feed_next(self)
        fids.append((self.source, r[2]))
        return r
    monkeypatch.setattr(pkg("feeder").DeviceFeeder, "next", next_spy)

    out = str(tmp_path / "seg_plain")
    tr = ts.main(["--nii-train", train_list, "--nii-val", val_list, "--no-augment", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out])
    assert len(tr.step_times) == 3 and np.isfinite(tr.loss_dict["train"][1]) and np.isfinite(tr.loss_dict["val"][2])
    ck = os.path.join(out, "checkpoint.npz")
    assert os.path.exists(ck)
    # the first batch the trainer saw: the host-built frames of the normalised volumes, bit for bit
    bx, by = seen[0]
    src, first = next((s, f) for s, f in fids if s is tr.train_list)
    assert tr.train_list.augment is None and tr.val_list.augment is None and len(first) == 2
    for b, fid in enumerate(first):
        name, z = fid.split("#")
        z = int(z)
        n = src.volumes.names.index(name)
        raw_y = np.asarray(nifti.load(os.path.join(root, name.replace("image", "label"))).get_data())
        raw_y = np.flip(np.flip(raw_y, axis=0), axis=1)                  # the flip of volume_eval.test_eval
        norm = src.volumes.images[n].cpu().numpy()
        assert np.array_equal(bx[b].cpu().numpy().view(np.uint32), norm[:, :, z - 1:z + 2].view(np.uint32))
        assert np.array_equal(by[b].cpu().numpy(), R.onehot(raw_y[:, :, z], 5))
        raw = np.flip(np.flip(np.asarray(nifti.load(os.path.join(root, name)).get_data()), axis=0), axis=1)
        ref, _ = R.preprocess(raw)
        assert np.abs(norm - ref).max() <= 4 * U * max(1.0, np.abs(ref).max())
    assert tr.train_list.errors() == 0

    # augmented (the default ranges), then two critic iterations of the GAN's pre-train phase from four NIfTI lists
    out2 = str(tmp_path / "seg_aug")
    tr2 = ts.main(["--nii-train", train_list, "--nii-val", val_list, "--augment", '{"rotate": 20, "scale": 0.2, "translate": 8, "flip": 0.5}',
                   "--batch-size", "2", "--iters", "2", "--epochs", "1", "--output", out2])
    assert tr2.train_list.augment["rotate"] == 20.0 and tr2.val_list.augment is None
    assert np.isfinite(tr2.loss_dict["train"][1]) and os.path.exists(os.path.join(out2, "checkpoint.npz"))
    out3 = str(tmp_path / "gan")
    t3 = tg.main("pre-train", ["--mr-nii-train", train_list, "--mr-nii-val", val_list, "--ct-nii-train", train_list, "--ct-nii-val", val_list,
                               "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out3, "--baseline", ck])
    assert t3.global_step == 2 and np.isfinite(float(t3.net.dis_loss))
    assert t3.mr_train_list.augment == pkg("volume_source").DEFAULT_AUGMENT and t3.ct_val_list.augment is None


def test_numpy_view_feeder_and_export(dev, nii_lists, tmp_path):
    vs, tfr, F = pkg("volume_source"), pkg("tfrecord"), pkg("feeder")
    train_list, _, _ = nii_lists
    vset = vs.VolumeSet(vs.read_pairs(train_list), dev)
    mk = lambda seed=3, shard=None: vs.AugmentedSliceSource(vset, 4, out_size=(64, 48), seed=seed, shard=shard)
    a, b, c = mk(), mk(), mk()
    x, onehot, fids = a.next_device_batch()
    batch, fids_b = b.next_batch(4)
    assert fids == fids_b and batch.shape == (4, 64, 48, 4) and batch.dtype == np.float32
    assert np.array_equal(batch[..., 0:3], x.cpu().numpy()) and np.array_equal(R.onehot(batch[..., 3], 5), onehot.cpu().numpy())
    assert all(f.split("#")[0] in vset.names and 1 <= int(f.split("#")[1]) <= 4 for f in fids)
    other = mk(shard=(1, 2)).next_batch(4)
    assert other[1] != fids or not np.array_equal(other[0], batch)      # ranks differ
    # the feeder hands the same batches over, in order, with the one-hot of ITS num_cls
    feed = F.DeviceFeeder(c, 4, 3, dev)
    try:
        fx, fy, ff = feed.next()
        torch.cuda.current_stream().synchronize()
        assert ff == fids and torch.equal(fx, x) and fy.shape == (4, 64, 48, 3) and torch.equal(fy, onehot[..., :3])
        x2, _, fids2 = a.next_device_batch()
        fx2, _, ff2 = feed.next()
        assert ff2 == fids2 and torch.equal(fx2, x2)
    finally:
        feed.close()
    # the export writes what a source of the same seed delivers
    outdir = str(tmp_path / "export")
    files = vs.main(["--export", "5", outdir, "--list", train_list, "--seed", "9"])
    assert len(files) == 5 and open(os.path.join(outdir, "slice_list")).read().split() == files
    ref = vs.AugmentedSliceSource(vset, 16, seed=9)
    want = np.concatenate([ref.next_batch(5)[0]])
    for f, w in zip(files, want):
        assert np.array_equal(tfr.read_slice(f, verify=True), w)
