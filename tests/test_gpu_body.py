"""-m gpu: the label-free body crop on the device (csrc/body.hip, body.py) against the numpy restatement tests/body_ref.py.
Every comparison is an equality of integers or of float bits.

  pnp_volume_histogram / pnp_volume_threshold_mask over n (one lane .. more than one pass of the capped grid of 1024 workgroups x 256 lanes
  x 4 voxels), base offsets of 0, 1 and 3 elements (the head / body / tail walk), nbins in {2, 256, 1024} and six kinds of values;
  body.body_box on the torso phantoms; VolumeSet(crop="body") and image-only lists; segment_volume(crop="body") against the explicit box;
  train_gan's pre-train phase with an unlabelled CT training list, and predict --crop-body."""
import json
import os

import numpy as np
import pytest
import torch

import body_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

GRID_PASS = 1024 * 256 * 4                     # voxels one pass of the capped grid covers (csrc/body.hip: kMaxBlocks x kThreads x 4)
SIZES = [1, 63, 64, 65, 255, 257, 4099, GRID_PASS + 3]
KINDS = ("normal", "two", "constant", "ramp", "negative", "outlier")
GUARD = 64


def _values(kind, n, nbins, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        v = rng.standard_normal(n)
    elif kind == "two":
        v = np.where(rng.random(n) < 0.3, -1.25, 7.5)
        v[0] = -1.25
        v[-1] = 7.5
    elif kind == "constant":
        v = np.full(n, 3.75)
    elif kind == "ramp":                         # exactly on the bin edges lo + j (hi - lo) / nbins, j = 0 .. nbins: the last is hi itself
        j = np.arange(n) % (nbins + 1) if n > nbins else (np.arange(n) * nbins) // max(n - 1, 1)
        v = -2.0 + j * (8.0 / nbins)             # a power-of-two step: exact in float32
        rng.shuffle(v)
    elif kind == "negative":
        v = -1.0 - np.abs(rng.standard_normal(n)) * 100.0
    else:
        v = rng.standard_normal(n)
        v[n // 2] = 1e30
    return v.astype(np.float32)


def _on_device(dev, v, off):
    buf = torch.zeros(v.size + off + 4, dtype=torch.float32, device=dev)
    t = buf[off:off + v.size]
    t.copy_(torch.from_numpy(v))
    assert t.data_ptr() % 16 == (4 * off) % 16 and t.is_contiguous()
    return t


@pytest.mark.parametrize("n", SIZES)
def test_histogram_and_mask_equal_the_restatement(dev, n):
    K = pkg("kernels")
    for ki, kind in enumerate(KINDS):
        for nbins in (2, 256, 1024):
            v = _values(kind, n, nbins, 100 * ki + nbins + n % 97)
            (lo, hi), want = R.histogram(v, nbins)
            assert int(want.sum()) == n
            masks = {k: R.mask(v, lo, hi, k, nbins) for k in (0, 127, 254, 255)} if nbins == 256 else {}
            for off in (0, 1, 3):
                vd = _on_device(dev, v, off)
                rng, hist = K.volume_histogram(vd, nbins)
                got_r, got_h = rng.cpu().numpy(), hist.cpu().numpy()
                what = (kind, n, nbins, off)
                assert got_r.view(np.uint32).tolist() == np.array([lo, hi], np.float32).view(np.uint32).tolist(), what
                assert got_h.shape == (nbins,) and np.array_equal(got_h.astype(np.int64), want), what
                assert int(got_h.astype(np.int64).sum()) == n, what
                for k, m in masks.items():
                    # the mask sits between guards, at an address that is (off = 1) or is not a multiple of 4 behind the walk's head
                    buf = torch.full((n + 2 * GUARD + 4,), 0xA5, dtype=torch.uint8, device=dev)
                    out = buf[GUARD + (off & 1):GUARD + (off & 1) + n]
                    res = K.volume_threshold_mask(vd, rng, k, nbins, out=out)
                    assert res.data_ptr() == out.data_ptr()
                    b = buf.cpu().numpy()
                    assert np.array_equal(b[GUARD + (off & 1):GUARD + (off & 1) + n], m), what + (k,)
                    assert (b[:GUARD + (off & 1)] == 0xA5).all() and (b[GUARD + (off & 1) + n:] == 0xA5).all(), what + (k,)
            if n == 4099 and kind == "normal" and nbins == 256:          # a fresh output tensor, and two runs are one result
                vd = _on_device(dev, v, 0)
                r1, h1 = K.volume_histogram(vd, nbins)
                r2, h2 = K.volume_histogram(vd, nbins)
                assert torch.equal(h1, h2) and torch.equal(r1, r2)
                assert np.array_equal(K.volume_threshold_mask(vd, r1, 127, nbins).cpu().numpy(), masks[127])


def test_wrappers_refuse(dev):
    K, L = pkg("kernels"), pkg("_lib")
    v = torch.zeros(64, device=dev)
    rng, _ = K.volume_histogram(v)
    for bad in (lambda: K.volume_histogram(torch.zeros(8)), lambda: K.volume_histogram(v.double()), lambda: K.volume_histogram(v, 1),
                lambda: K.volume_histogram(v, 1025), lambda: K.volume_histogram(v[::2]), lambda: K.volume_threshold_mask(torch.zeros(8), rng, 1),
                lambda: K.volume_threshold_mask(v, rng.cpu(), 1), lambda: K.volume_threshold_mask(v, rng, 256), lambda: K.volume_threshold_mask(v, rng, -1),
                lambda: K.volume_threshold_mask(v, rng, 1, out=torch.zeros(63, dtype=torch.uint8, device=dev)),
                lambda: K.volume_threshold_mask(v.double(), rng, 1)):
        with pytest.raises(L.PnpError):
            bad()


# ---- body_box --------------------------------------------------------------------------------------------------------------------------
def _reference_box(dev, v, margin=0, percentile=98, info=None):
    """the restatement's chain on the DEVICE's normalised copy of v, brought to the host"""
    K = pkg("kernels")
    vn, _ = K.volume_preprocess(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev), percentile)
    return R.box_of_normalised(vn.cpu().numpy(), margin=margin, info=info)


CASES = [((48, 40, 12), kind, seed) for kind in ("ct", "mr") for seed in range(3)] + [((45, 37, 11), "ct", 3)]


@pytest.fixture(scope="module")
def phantoms():
    return {c: R.phantom(*c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%d" % ("x".join(str(n) for n in c[0]), c[1], c[2]))
def test_body_box_on_the_phantoms(dev, phantoms, case):
    body = pkg("body")
    v, true_box = phantoms[case]
    vd = torch.from_numpy(v).to(dev)
    got = body.body_box(vd)
    info = {}
    assert got == _reference_box(dev, v, info=info) == true_box, (got, true_box, info.get("k"))
    assert torch.equal(vd.cpu(), torch.from_numpy(v))                                # the input is not modified
    assert body.body_box(vd) == got                                                  # two runs, one result
    assert body.body_box(vd, margin=3) == _reference_box(dev, v, margin=3) == R.grow(true_box, 3, v.shape)
    assert R.grow(true_box, 3, v.shape)[2] == (0, v.shape[2])                        # ... and that margin is clamped in z
    if case[1] == "ct":
        assert int(info["stats"][1][0]) == 2 and int(info["stats"][1][1] - info["stats"][1][2]) == 2 * 32 * case[0][2]        # the table went


def test_body_box_of_a_constant_volume_and_refusals(dev):
    body, L = pkg("body"), pkg("_lib")
    assert body.body_box(torch.full((9, 7, 5), -3.5, device=dev)) == ((0, 9), (0, 7), (0, 5))
    assert body.body_box(torch.full((9, 7, 5), -3.5, device=dev), margin=2) == ((0, 9), (0, 7), (0, 5))
    v = torch.zeros((9, 7, 5), device=dev)
    with pytest.raises(L.PnpError):
        body.body_box(v.cpu())
    for bad in (lambda: body.body_box(v.double()), lambda: body.body_box(v.permute(1, 0, 2)), lambda: body.body_box(v, margin=-1),
                lambda: body.body_box(v, connectivity=4), lambda: body.body_box(v[0])):
        with pytest.raises(ValueError):
            bad()


# ---- VolumeSet ---------------------------------------------------------------------------------------------------------------------------
def _label_of(shape, box):
    """four classes in blocks inside the body's box"""
    lab = np.zeros(shape, np.int16)
    (x0, x1), (y0, y1), (z0, z1) = box
    xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
    lab[x0 + 3:xm, y0 + 3:ym, z0:z1] = 1
    lab[xm:x1 - 3, y0 + 3:ym, z0:z1] = 2
    lab[x0 + 3:xm, ym:y1 - 3, z0:z1] = 3
    lab[xm:x1 - 3, ym:y1 - 3, z0:z1] = 4
    return lab


@pytest.fixture(scope="module")
def nii(tmp_path_factory):
    """phantoms written with nifti.save: two MR and two CT scans with labels, and the four lists of a GAN run whose CT training list names
    the images alone"""
    nifti = pkg("nifti")
    root = tmp_path_factory.mktemp("body_nii")
    aff = np.diag([1.0, 1.0, 2.0, 1.0])
    files = {}
    for kind in ("mr", "ct"):
        for seed in range(2):
            v, box = R.phantom((48, 40, 12), kind, seed)
            name = "%s%d" % (kind, seed)
            nifti.save(nifti.Nifti1Image(v, aff), str(root / (name + "_image.nii.gz")))
            nifti.save(nifti.Nifti1Image(_label_of(v.shape, box), aff), str(root / (name + "_label.nii.gz")))
            files[name] = (v, _label_of(v.shape, box), box)
    pair = lambda n: "%s_image.nii.gz %s_label.nii.gz" % (n, n)
    (root / "mr_train").write_text(pair("mr0") + "\n" + pair("mr1") + "\n")
    (root / "mr_val").write_text(pair("mr1") + "\n")
    (root / "ct_train").write_text("ct0_image.nii.gz\nct1_image.nii.gz\n")           # unlabelled target scans
    (root / "ct_val").write_text(pair("ct1") + "\n")
    (root / "ct_mixed").write_text(pair("ct0") + "\nct1_image.nii.gz\n")
    return str(root), files


@pytest.mark.parametrize("margin", [0, 2])
def test_volume_set_with_body_crop_equals_the_host_crop(dev, nii, margin):
    vs, body = pkg("volume_source"), pkg("body")
    root, files = nii
    pairs = vs.read_pairs(os.path.join(root, "mr_train")) + vs.read_pairs(os.path.join(root, "ct_val"))
    got = vs.VolumeSet(pairs, dev, crop="body" if margin == 0 else ("body", margin))
    imgs, labs, boxes = [], [], []
    for name in ("mr0", "mr1", "ct1"):
        v, lab, true_box = files[name]
        img, l8 = vs.prepare_pair(v, lab, True, 2, None)                             # the flips of the default path
        box = _reference_box(dev, img, margin=margin)
        flipped = ((48 - true_box[0][1], 48 - true_box[0][0]), (40 - true_box[1][1], 40 - true_box[1][0]), true_box[2])
        assert box == R.grow(flipped, margin, img.shape)
        sl = tuple(slice(a, b) for a, b in box)
        imgs.append(img[sl])
        labs.append(l8[sl])
        boxes.append(box)
    want = vs.VolumeSet.from_arrays(imgs, labs, got.names, dev)
    assert got.boxes == boxes and got.dims == want.dims and got.has_labels == [True] * 3 and want.boxes is None
    for a, b, la, lb in zip(got.images, want.images, got.labels, want.labels):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(la, lb)
    assert got.stats == want.stats
    # without the option nothing changes: no boxes, the whole volumes
    plain = vs.VolumeSet(pairs[:1], dev)
    assert plain.boxes is None and plain.dims == [(48, 40, 12)] and plain.has_labels == [True]
    # the label crop records its box as well, and is what it was
    lc = vs.VolumeSet(pairs[:1], dev, crop=1)
    assert lc.boxes == [tuple((s.start, s.stop) for s in vs.label_bounding_box(vs.prepare_pair(*files["mr0"][:2], True, 2, None)[1], 1))]
    assert lc.dims == [tuple(b - a for a, b in lc.boxes[0])]


def test_volume_set_body_boxes_of_three_axes_are_one_box_permuted(dev, nii):
    vs, body = pkg("volume_source"), pkg("body")
    root, files = nii
    got = vs.VolumeSet(vs.read_pairs(os.path.join(root, "ct_val")), dev, axis=(0, 1, 2), crop="body")
    one = got.boxes[2]                                                               # axis 2: the file order after the flips
    assert got.boxes == [body.permute_box(one, a) for a in (0, 1, 2)] and len(set(got.boxes)) == 3
    assert got.dims == [tuple(b - a for a, b in box) for box in got.boxes]
    single = vs.VolumeSet(vs.read_pairs(os.path.join(root, "ct_val")), dev, crop="body")
    assert single.boxes == [one] and torch.equal(single.images[0].view(torch.int32), got.images[2].view(torch.int32))


def test_image_only_list(dev, nii):
    vs = pkg("volume_source")
    root, files = nii
    pairs = vs.read_pairs(os.path.join(root, "ct_train"), labels="optional")
    assert [p[1] for p in pairs] == [None, None]
    vset = vs.VolumeSet(pairs, dev, crop=("body", 2))
    assert vset.has_labels == [False, False] and all(l.dtype == torch.uint8 and not bool(l.any()) for l in vset.labels)
    assert [tuple(l.shape) for l in vset.labels] == vset.dims == [tuple(b - a for a, b in box) for box in vset.boxes]
    src = vs.AugmentedSliceSource(vset, 3, out_size=(32, 24), seed=1)
    assert src.labelled is False
    x, onehot, fids = src.next_device_batch()
    assert onehot.shape == (3, 32, 24, 5) and bool((onehot[..., 0] == 1).all()) and not bool(onehot[..., 1:].any())
    src.close()
    with pytest.raises(ValueError, match="unlabelled"):
        vs.AugmentedSliceSource(vset, 3, sampling={"foreground": 0.5})
    with pytest.raises(ValueError, match="has no label"):
        vs.VolumeSet(pairs, dev, crop=2)
    mixed = vs.VolumeSet(vs.read_pairs(os.path.join(root, "ct_mixed"), labels="optional"), dev)
    assert mixed.has_labels == [True, False] and mixed.boxes is None and bool(mixed.labels[0].any()) and not bool(mixed.labels[1].any())
    assert vs.AugmentedSliceSource(mixed, 2, out_size=(16, 16)).labelled is False
    fa = vs.VolumeSet.from_arrays([files["ct0"][0], files["ct1"][0]], [files["ct0"][1], None], ["a", "b"], dev)
    assert fa.has_labels == [True, False] and not bool(fa.labels[1].any()) and bool(fa.labels[0].any())
    assert vs.AugmentedSliceSource(vs.VolumeSet(vs.read_pairs(os.path.join(root, "ct_val")), dev), 2, out_size=(16, 16)).labelled is True


# ---- segment_volume ----------------------------------------------------------------------------------------------------------------------
def _stub(ncls=5):
    """logits from the three channels and the pixel position: deterministic torch arithmetic, the same for equal inputs (the stub of
    tests/test_gpu_volume_axes.py)"""
    def fn(x):
        Bn, H, W, _ = x.shape
        i = torch.arange(H, device=x.device, dtype=torch.float32).view(1, H, 1)
        j = torch.arange(W, device=x.device, dtype=torch.float32).view(1, 1, W)
        out = torch.stack([x[..., 0] * (0.5 + c) - x[..., 1] * (0.3 * c) + x[..., 2] * 0.7 + torch.sin(0.4 * i * (c + 1) + 0.3 * j) for c in range(ncls)], dim=-1)
        return out.contiguous()
    return fn


COMMON = dict(out_size=(24, 20), batch_size=4)


@pytest.mark.parametrize("kw", [{}, {"sample_mm": 2.0, "spacing": (1.0, 1.0, 2.0)}], ids=["plain", "sample_mm"])
def test_segment_volume_body_crop_equals_the_explicit_box(dev, phantoms, kw):
    vp = pkg("volume_predict")
    image, true_box = phantoms[((48, 40, 12), "ct", 1)]
    b = []
    got = vp.segment_volume(_stub(), image, crop=("body", 1), crop_box=b, device=dev, **COMMON, **kw)
    flipped = ((48 - true_box[0][1], 48 - true_box[0][0]), (40 - true_box[1][1], 40 - true_box[1][0]), true_box[2])
    assert len(b) == 1 and b[0] == R.grow(flipped, 1, image.shape)
    want = vp.segment_volume(_stub(), image, crop=b[0], device=dev, **COMMON, **kw)
    assert torch.equal(got, want) and bool(got.any())
    g = got.cpu().numpy()
    inside = np.zeros(image.shape, bool)
    (x0, x1), (y0, y1), (z0, z1) = R.grow(true_box, 1, image.shape)                  # the same voxels in file order
    inside[x0:x1, y0:y1, z0:z1] = True
    assert not g[~inside].any() and g[inside].any()
    b0 = []
    assert torch.equal(vp.segment_volume(_stub(), image, crop="body", crop_box=b0, device=dev, **COMMON, **kw),
                       vp.segment_volume(_stub(), image, crop=flipped, device=dev, **COMMON, **kw)) and b0 == [flipped]
    e = []
    vp.segment_volume(_stub(), image, crop=flipped, crop_box=e, device=dev, **COMMON, **kw)            # any crop reports its box
    assert e == [flipped]


def test_segment_volume_body_crop_with_axes(dev, phantoms):
    vp = pkg("volume_predict")
    image, true_box = phantoms[((48, 40, 12), "mr", 0)]
    b = []
    got = vp.segment_volume(_stub(), image, axes=(0, 1, 2), crop="body", crop_box=b, device=dev, **COMMON)
    assert len(b) == 1
    want = vp.segment_volume(_stub(), image, axes=(0, 1, 2), crop=b[0], device=dev, **COMMON)
    assert torch.equal(got.label, want.label) and bool(got.label.any()) and got.prob is None and want.prob is None
    assert b[0] == ((48 - true_box[0][1], 48 - true_box[0][0]), (40 - true_box[1][1], 40 - true_box[1][0]), true_box[2])


# ---- through the command lines -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint(dev, nii, tmp_path_factory):
    """a source segmenter trained for two iterations on the body-cropped MR phantoms: train_segmenter --crop-body"""
    ts = pkg("train_segmenter")
    root, _ = nii
    out = str(tmp_path_factory.mktemp("body_seg"))
    tr = ts.main(["--nii-train", os.path.join(root, "mr_train"), "--nii-val", os.path.join(root, "mr_val"), "--crop-body", "2", "--batch-size", "2",
                  "--iters", "2", "--epochs", "1", "--output", out])
    assert tr.train_list.volumes.boxes is not None and tr.train_list.volumes.dims[0] == (33, 27, 12) and np.isfinite(tr.loss_dict["train"][1])
    ck = os.path.join(out, "checkpoint.npz")
    assert os.path.exists(ck)
    return ck


def test_train_gan_pre_train_with_an_unlabelled_ct_list(dev, nii, checkpoint, tmp_path):
    tg = pkg("train_gan")
    root, _ = nii
    out = str(tmp_path / "gan")
    lists = [os.path.join(root, n) for n in ("mr_train", "mr_val", "ct_train", "ct_val")]
    t = tg.main("pre-train", ["--mr-nii-train", lists[0], "--mr-nii-val", lists[1], "--ct-nii-train", lists[2], "--ct-nii-val", lists[3],
                              "--crop-body", "2", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out, "--baseline", checkpoint])
    assert t.global_step == 2 and np.isfinite(float(t.net.dis_loss))
    assert t.ct_train_list.labelled is False and t.ct_val_list.labelled is True and t.mr_train_list.labelled is True
    assert t.ct_train_list.volumes.has_labels == [False, False] and all(v.boxes is not None for v in (t.ct_train_list.volumes, t.mr_val_list.volumes))
    rows = [json.loads(line) for line in open(os.path.join(out, "metrics.jsonl"))]
    train_rows, val_rows = [r for r in rows if r["kind"] == "train_eval"], [r for r in rows if r["kind"] == "val_eval"]
    assert train_rows and val_rows
    for r in train_rows:
        assert "ct_dice" in r and r["ct_dice"] is None and isinstance(r["mr_dice"], float) and np.isfinite(r["mr_dice"])
    for r in val_rows:
        assert isinstance(r["ct_dice"], float) and np.isfinite(r["ct_dice"]) and isinstance(r["mr_dice"], float)
    assert t.loss_dict["train"][1] is None and isinstance(t.loss_dict["val"][1], float)


def test_predict_with_crop_body(dev, nii, checkpoint, tmp_path, capsys):
    pr, nifti = pkg("predict"), pkg("nifti")
    root, files = nii
    image = os.path.join(root, "ct0_image.nii.gz")
    out = str(tmp_path / "pred")
    res = pr.main(["--model", checkpoint, "--net", "segmenter", "--images", image, "--out", out, "--batch-size", "2", "--crop-body", "1"])
    true_box = files["ct0"][2]
    flipped = ((48 - true_box[0][1], 48 - true_box[0][0]), (40 - true_box[1][1], 40 - true_box[1][0]), true_box[2])
    box = R.grow(flipped, 1, (48, 40, 12))
    assert res["crop_box"] == [[list(b) for b in box]]
    assert "body box  %s" % " x ".join("[%d, %d)" % b for b in box) in capsys.readouterr().out
    pred = nifti.load(res["paths"][0])
    assert res["paths"] == [os.path.join(out, "pred_ct0_image.nii.gz")] and pred.shape == (48, 40, 12) and pred.get_data().dtype == np.uint8
    assert np.allclose(pred.affine, np.diag([1.0, 1.0, 2.0, 1.0]))
    inside = np.zeros((48, 40, 12), bool)
    (x0, x1), (y0, y1), (z0, z1) = R.grow(true_box, 1, (48, 40, 12))
    inside[x0:x1, y0:y1, z0:z1] = True
    assert not pred.get_data()[~inside].any()
