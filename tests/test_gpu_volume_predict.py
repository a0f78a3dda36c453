"""-m gpu: volume inference through the product (volume_predict.py, predict.py) with the real networks, randomly
initialised, B = 2: segment_volume against Full_DRN.evaluate on the same slices, against tests/paste_ref.py on a volume whose in-plane size
and file order differ from the network's, the crop box, the adapted net's adapter, Trainer.predict_volumes and the command line.

Rule for comparisons with the networks' own compact_pred: softmax_argmax_kernel takes the argmax of expf(l) / sum, about 3 ulps of relative
error per probability, so it can misorder only logit gaps below about 8 * 2^-24; a difference is allowed only at pixels whose two largest
logits differ by less than 1e-6, and such pixels must be at most 1e-4 of all pixels.  The comparison with paste_ref uses the bound of
tests/test_gpu_paste.py on the logits captured from the device."""
import os

import numpy as np
import pytest
import torch

import paste_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

B = 2
COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}
ADV_COST = {"regularizer": 1e-4, "gan_regularizer": 1e-4, "miu_gen": 0.002, "miu_dis": 0.002, "lambda_mask_loss": 0.3}
NETCFG = {"mr_front_trainable": False, "joint_trainable": False, "ct_front_trainable": True, "cls_trainable": True, "m_cls_trainable": True}


def _random_state(net, seed, logits_fn):
    """He-scaled conv weights, BN statistics off the identity; then the logits convolution is rescaled so that the logits of a probe batch
    peak at 10: softmax_argmax_kernel, the other side of the comparisons, overflows expf above 88"""
    rng = np.random.default_rng(seed)
    sd = net.store.state_dict()
    for k, a in sd.items():
        if "Variable" in k:
            sd[k] = (rng.standard_normal(a.shape) * np.sqrt(2.0 / np.prod(a.shape[:-1])) * 0.9).astype(np.float32)
        elif k.endswith("moving_mean"):
            sd[k] = (0.05 * rng.standard_normal(a.shape)).astype(np.float32)
        elif k.endswith("moving_variance"):
            sd[k] = (1.0 + 0.2 * rng.random(a.shape)).astype(np.float32)
        elif k.endswith("gamma"):
            sd[k] = (1.0 + 0.05 * rng.standard_normal(a.shape)).astype(np.float32)
    net.store.load_state_dict(sd)
    probe = torch.from_numpy((1.5 * rng.standard_normal((B, 256, 256, 3))).astype(np.float32)).to(net.device)
    peak = float(logits_fn(net)(probe).abs().max())
    last = [k for k in sd if "output" in k and "Variable" in k]
    assert len(last) == 1 and np.isfinite(peak) and peak > 0, (last, peak)
    sd[last[0]] = (sd[last[0]] * (10.0 / peak)).astype(np.float32)
    net.store.load_state_dict(sd)
    return net


@pytest.fixture(scope="module")
def seg(dev):
    ss = pkg("source_segmenter")
    return _random_state(ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, seed=0, cost_kwargs=dict(COST)), 5, pkg("volume_predict").segmenter_logits)


def _scan(shape, seed):
    """a smooth-ish int16 scan with a bright tail: blobs over noise"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    v = 400 * np.exp(-4 * (g[0] ** 2 + g[1] ** 2 + 0.5 * g[2] ** 2)) + 60 * rng.standard_normal(shape) + 100 * np.sin(5 * g[0]) * np.cos(3 * g[1])
    return v.astype(np.int16)


def _to_slicing(a, flip, axis):
    if flip:
        a = np.flip(np.flip(a, 0), 1)
    return np.moveaxis(a, axis, -1)


def _to_file(a, flip, axis):
    a = np.moveaxis(a, -1, axis)
    if flip:
        a = np.flip(np.flip(a, 0), 1)
    return a


def _allowed_differences(mine, theirs, logits, what):
    """mine / theirs [..]: labels; logits [.., ncls]: differences only where the two largest logits are closer than 1e-6, and few of those"""
    top = np.sort(logits.astype(np.float64), axis=-1)
    close = (top[..., -1] - top[..., -2]) < 1e-6
    diff = mine != theirs
    print("%s: %d of %d labels differ, %d pixels with a top-2 gap < 1e-6, max|logit| %.3f" % (what, int(diff.sum()), diff.size, int(close.sum()),
                                                                                         float(np.abs(logits).max())))
    assert not np.any(diff & ~close), "%s: %d labels differ at pixels with a clear maximum" % (what, int((diff & ~close).sum()))
    assert close.sum() <= 1e-4 * close.size, "%s: %d near-tied pixels: the comparison would be vacuous" % (what, int(close.sum()))


def _network_labels(net, frames_s, dev):
    """compact_pred and logits of Full_DRN.evaluate on the slices (z - 1, z, z + 1) of the normalised volume frames_s [X, Y, Z'], z = 1 .. Z' - 2"""
    preds, logits = [], []
    zs = list(range(1, frames_s.shape[2] - 1))
    for k in range(0, len(zs), B):
        x = torch.stack([frames_s[:, :, z - 1:z + 2] for z in zs[k:k + B]]).contiguous()
        y = torch.zeros(tuple(x.shape[:3]) + (5,), device=dev)
        y[..., 0] = 1.0
        net.evaluate(x, y, keep_prob=1.0, main_bn=False, adapt_bn=False)
        preds.append(net.compact_pred.cpu().numpy())
        logits.append(net.logits.detach().cpu().numpy())
    return np.concatenate(preds), np.concatenate(logits)            # [Z' - 2, X, Y], [Z' - 2, X, Y, 5]


def test_native_size_volume_matches_the_networks_own_prediction(dev, seg):
    vp, vs, K = pkg("volume_predict"), pkg("volume_source"), pkg("kernels")
    image = _scan((256, 256, 6), 0)
    fn = vp.segmenter_logits(seg)
    skip = vp.segment_volume(fn, image, edge="skip", batch_size=B, device=dev)
    assert skip.dtype == torch.uint8 and tuple(skip.shape) == image.shape and skip.is_cuda
    skip = skip.cpu().numpy()
    assert not skip[:, :, 0].any() and not skip[:, :, 5].any()
    img_s, _ = vs.prepare_pair(image, np.zeros(image.shape, np.uint8))
    v, _ = K.volume_preprocess(torch.from_numpy(img_s).to(dev))
    pred, logits = _network_labels(seg, v, dev)                     # frames 1 .. 4
    mine = np.moveaxis(_to_slicing(skip, True, 2)[:, :, 1:5], 2, 0)
    _allowed_differences(mine, pred, logits, "skip, frames 1..4")
    assert len(np.unique(pred)) > 1, "a constant prediction shows nothing"
    rep = vp.segment_volume(fn, image, edge="replicate", batch_size=B, device=dev).cpu().numpy()
    assert np.array_equal(rep[:, :, 1:5], skip[:, :, 1:5])
    # the edge frames of "replicate": the slices (f0, f0, f1) and (f4, f5, f5)
    padded = torch.cat([v[:, :, :1], v, v[:, :, -1:]], dim=2)
    edge = torch.stack([padded[:, :, 0:3], padded[:, :, 5:8]]).contiguous()
    y = torch.zeros((2, 256, 256, 5), device=dev)
    y[..., 0] = 1.0
    seg.evaluate(edge, y, keep_prob=1.0, main_bn=False, adapt_bn=False)
    mine = np.moveaxis(_to_slicing(rep, True, 2)[:, :, [0, 5]], 2, 0)
    _allowed_differences(mine, seg.compact_pred.cpu().numpy(), seg.logits.detach().cpu().numpy(), "replicate, frames 0 and 5")


def test_other_size_and_file_order_against_the_restatement(dev, seg):
    """200 x 232 x 5 in slicing order, stored with the slicing axis in the middle and flipped: batches of 2, 2 and 1 frames"""
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    image = _scan((200, 5, 232), 1)
    captured = []
    inner = vp.segmenter_logits(seg)

    def fn(x):
        out = inner(x)
        captured.append(out.detach().clone())
        return out
    got = vp.segment_volume(fn, image, flip_correction=True, axis=1, edge="replicate", batch_size=B, device=dev).cpu().numpy()
    assert got.shape == image.shape and len(captured) == 3
    X, Y, Z = 200, 232, 5
    inv = vp.invert_matrix(vs.compose_matrix((X, Y), (256, 256)))
    got_s = _to_slicing(got, True, 1)
    bad = differ = 0
    for k, lg in enumerate(captured):
        lg = lg.cpu().numpy()
        nb = min(B, Z - k * B)
        lab, r = R.labels(lg, inv, X, Y, nb)
        mine = np.moveaxis(got_s[:, :, k * B:k * B + nb], 2, 0)
        ok = np.take_along_axis(R.admissible(r, R.delta(lg[:nb], inv, X, Y)), mine[..., None].astype(np.int64), axis=-1)[..., 0]
        bad += int((~ok).sum())
        differ += int((mine != lab).sum())
    print("200 x 232 x 5: %d of %d labels differ from the float64 argmax, %d outside the bound" % (differ, X * Y * Z, bad))
    assert bad == 0
    assert len(np.unique(got)) > 1


def test_crop_box(dev, seg):
    vp = pkg("volume_predict")
    image = _scan((200, 5, 232), 2)
    fn = vp.segmenter_logits(seg)
    box = ((10, 150), (21, 200), (1, 5))
    kw = dict(flip_correction=True, axis=1, edge="replicate", batch_size=B, device=dev)
    got = vp.segment_volume(fn, image, crop=box, **kw).cpu().numpy()
    got_s = _to_slicing(got, True, 1)
    inside = np.zeros(got_s.shape, bool)
    inside[tuple(slice(a, b) for a, b in box)] = True
    assert not got_s[~inside].any()
    cropped_file = np.ascontiguousarray(_to_file(_to_slicing(image, True, 1)[tuple(slice(a, b) for a, b in box)], True, 1))
    alone = vp.segment_volume(fn, cropped_file, **kw).cpu().numpy()
    assert np.array_equal(got_s[tuple(slice(a, b) for a, b in box)], _to_slicing(alone, True, 1))
    assert len(np.unique(alone)) > 1
    # a margin around a label's bounding box is the same box
    label = np.zeros(image.shape, np.uint8)
    label_s = _to_slicing(label, True, 1)          # a view: writes land in `label`
    label_s[12:148, 23:198, 2:4] = 3
    margin = vp.segment_volume(fn, image, label=label, crop=2, **kw).cpu().numpy()
    same = vp.segment_volume(fn, image, crop=((10, 150), (21, 200), (0, 5)), **kw).cpu().numpy()
    assert np.array_equal(margin, same) and same.any()
    with pytest.raises(ValueError, match="a label is needed"):
        vp.segment_volume(fn, image, crop=2, **kw)


def test_adapted_nets_adapter(dev):
    adv, vp, K = pkg("adversarial"), pkg("volume_predict"), pkg("kernels")
    net = _random_state(adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(ADV_COST), network_config=dict(NETCFG), device=dev, seed=1), 9,
                        vp.adapted_logits)
    image = _scan((256, 256, 4), 3)
    got = vp.segment_volume(vp.adapted_logits(net), image, flip_correction=False, edge="skip", batch_size=B, device=dev).cpu().numpy()
    v, _ = K.volume_preprocess(torch.from_numpy(image.astype(np.float32)).to(dev))
    x = torch.stack([v[:, :, 0:3], v[:, :, 1:4]]).contiguous()
    y = torch.zeros((2, 256, 256, 5), device=dev)
    y[..., 0] = 1.0
    pred, _ = net.predict_ct(x, y)
    with torch.no_grad():
        logits = net._graph(None, x, 1.0, mr_front_bn=False, joint_bn=False, ct_front_bn=False, critics=False)["ct_logits"]
    _allowed_differences(np.moveaxis(got[:, :, 1:3], 2, 0), pred.cpu().numpy(), logits.cpu().numpy(), "adapted net")
    assert not got[:, :, 0].any() and not got[:, :, 3].any() and len(np.unique(got)) > 1


def test_trainer_method_and_command_line(dev, seg, tmp_path):
    ss, nifti, pr = pkg("source_segmenter"), pkg("nifti"), pkg("predict")
    aff_a = np.array([[0.0, -1.5, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, 3.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    aff_b = np.diag([0.8, 0.8, 2.5, 1.0])
    a, b, la = str(tmp_path / "a.nii.gz"), str(tmp_path / "b.nii"), str(tmp_path / "a_label.nii.gz")
    nifti.save(nifti.Nifti1Image(_scan((40, 36, 4), 4), aff_a), a)
    nifti.save(nifti.Nifti1Image(_scan((33, 47, 3), 5), aff_b), b)
    lab = np.zeros((40, 36, 4), np.int16)
    lab[8:30, 5:25, 1:4] = 1
    lab[12:20, 10:18, 1:3] = 3
    lab[9, 6, 1] = 7                                    # >= num_cls: 0 in the written ground truth
    nifti.save(nifti.Nifti1Image(lab, aff_a), la)
    tr = ss.Trainer(seg, train_list=[], val_list=[], num_cls=5, batch_size=B)
    out1 = str(tmp_path / "plain")
    paths = tr.predict_volumes([a, b], out1)
    assert paths == [os.path.join(out1, "pred_a.nii.gz"), os.path.join(out1, "pred_b.nii")] and sorted(os.listdir(out1)) == ["pred_a.nii.gz", "pred_b.nii"]
    for p, shape, aff in ((paths[0], (40, 36, 4), aff_a), (paths[1], (33, 47, 3), aff_b)):
        got = nifti.load(p)
        assert got.shape == shape and got.get_data().dtype == np.uint8 and np.allclose(got.affine, aff) and got.get_data().max() < 5
    out2 = str(tmp_path / "labelled")
    assert tr.predict_volumes([a], out2, label_list=[la], crop=2, edge="skip") == [os.path.join(out2, "pred_a.nii.gz")]
    assert sorted(os.listdir(out2)) == ["dense_pred_a.nii.gz", "gth_dense_pred_a.nii.gz", "pred_a.nii.gz"]
    gth = nifti.load(os.path.join(out2, "gth_dense_pred_a.nii.gz")).get_data()
    assert gth[9, 6, 1] == 0 and np.array_equal(gth[10:], lab[10:]) and gth.dtype == np.uint8
    cropped = nifti.load(os.path.join(out2, "pred_a.nii.gz")).get_data()
    assert cropped[6:32, 3:27, 1:3].any() and not cropped[:, :, 0].any() and not cropped[:, :, 3].any() and not cropped[:6].any() and not cropped[32:].any() and not cropped[:, :3].any() and not cropped[:, 27:].any()
    # the command line builds its own net from a checkpoint of this one: the same labels as the method
    ckpt = seg.save(str(tmp_path / "ckpt.npz"))
    ckpt = ckpt if isinstance(ckpt, str) and os.path.isfile(ckpt) else str(tmp_path / "ckpt.npz")
    out3 = str(tmp_path / "cli")
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", a, "--labels", la, "--out", out3, "--batch-size", str(B), "--score",
                   "--json", str(tmp_path / "score.json")])
    assert res["paths"] == [os.path.join(out3, "pred_a.nii.gz")] and os.path.isfile(str(tmp_path / "score.json"))
    assert np.array_equal(nifti.load(res["paths"][0]).get_data(), nifti.load(paths[0]).get_data())
    score = res["score"]
    assert score["num_cls"] == 5 and len(score["subjects"]) == 1 and set(score["organs"]) and len(score["subjects"][0]["dice"]) == 5
    for r in score["organs"].values():
        assert {"dice_mean", "dice_std", "assd_mean", "hd95_mean", "undefined"} <= set(r)
