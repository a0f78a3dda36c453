"""-m gpu: the connected-component filter where a user meets it — segment_volume(keep_largest=), the ensemble path, the
predict and evaluate command lines — with the real segmenter, randomly initialised, B = 2, on a 256 x 256 x 6 volume.  Labels are integers:
every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import components_ref as R
import test_gpu_volume_predict as P
from conftest import pkg

pytestmark = pytest.mark.gpu

B = P.B


@pytest.fixture(scope="module")
def seg(dev):
    ss = pkg("source_segmenter")
    return P._random_state(ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, seed=0, cost_kwargs=dict(P.COST)), 5,
                           pkg("volume_predict").segmenter_logits)


@pytest.fixture(scope="module")
def image():
    return P._scan((256, 256, 6), 0)


@pytest.fixture(scope="module")
def plain(dev, seg, image):
    vp = pkg("volume_predict")
    return vp.segment_volume(vp.segmenter_logits(seg), image, batch_size=B, device=dev)


def test_segment_volume_option_equals_filtering_its_result(dev, seg, image, plain):
    vp, C = pkg("volume_predict"), pkg("components")
    fn = vp.segmenter_logits(seg)
    host = plain.cpu().numpy()
    stats = []
    got = vp.segment_volume(fn, image, batch_size=B, device=dev, keep_largest=1, component_stats=stats)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == image.shape and len(stats) == 1
    want, want_stats = C.keep_largest(plain)
    assert np.array_equal(plain.cpu().numpy(), host)
    assert torch.equal(got, want) and torch.equal(stats[0], want_stats)
    ref_out, ref_stats, _ = R.keep_largest(host, 5)
    assert np.array_equal(got.cpu().numpy(), ref_out) and np.array_equal(stats[0].cpu().numpy(), ref_stats)
    print("components per class", ref_stats[:, 0].tolist(), "voxels", ref_stats[:, 1].tolist(), "->", ref_stats[:, 2].tolist())
    assert ref_stats[:, 0].max() > 1 and ref_stats[:, 2].sum() < ref_stats[:, 1].sum(), "a prediction without islands shows nothing"
    opts = {"keep": 2, "min_size": 5, "connectivity": 3, "classes": [1, 2]}
    got = vp.segment_volume(fn, image, batch_size=B, device=dev, keep_largest=opts)
    assert np.array_equal(got.cpu().numpy(), R.keep_largest(host, 5, 2, 5, 3, [1, 2])[0])
    assert torch.equal(vp.segment_volume(fn, image, batch_size=B, device=dev, keep_largest=None), plain)


def test_ensemble_path_filters_the_label_only(dev, seg, image):
    vp, C = pkg("volume_predict"), pkg("components")
    fn = vp.segmenter_logits(seg)
    base = vp.segment_volume(fn, image, batch_size=B, device=dev, prob=True, entropy=True)
    got = vp.segment_volume(fn, image, batch_size=B, device=dev, prob=True, entropy=True, keep_largest={"keep": 1, "connectivity": 2})
    assert isinstance(got, vp.Ensemble)
    assert torch.equal(got.prob, base.prob) and torch.equal(got.entropy, base.entropy)
    want, _ = C.keep_largest(base.label, connectivity=2)
    assert torch.equal(got.label, want) and not torch.equal(got.label, base.label)


def test_predict_command_line(dev, seg, tmp_path, capsys):
    ss, nifti, pr = pkg("source_segmenter"), pkg("nifti"), pkg("predict")
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(P._scan((40, 36, 4), 4), np.eye(4)), a)
    tr = ss.Trainer(seg, train_list=[], val_list=[], num_cls=5, batch_size=B)
    unfiltered = nifti.load(tr.predict_volumes([a], str(tmp_path / "plain"))[0]).get_data()
    want, want_stats, _ = R.keep_largest(np.ascontiguousarray(unfiltered), 5)
    method = nifti.load(tr.predict_volumes([a], str(tmp_path / "method"), keep_largest=1)[0]).get_data()
    assert np.array_equal(method, want)
    ckpt = seg.save(str(tmp_path / "ckpt.npz"))
    ckpt = ckpt if isinstance(ckpt, str) and os.path.isfile(ckpt) else str(tmp_path / "ckpt.npz")
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", a, "--out", str(tmp_path / "cli"), "--batch-size", str(B), "--keep-largest"])
    assert np.array_equal(nifti.load(res["paths"][0]).get_data(), want)
    assert res["component_stats"] == [want_stats.tolist()]
    assert "components  class 1: %d components" % want_stats[1, 0] in capsys.readouterr().out


def test_evaluate_with_a_planted_island(dev, tmp_path, capsys):
    """the prediction is the ground truth plus a 2 x 2 x 2 island of class 1 far from the structure: unfiltered, the island sets HD;
    filtered, prediction and ground truth coincide"""
    nifti, ev = pkg("nifti"), pkg("evaluate")
    gt = np.zeros((40, 36, 12), np.uint8)
    gt[8:20, 6:18, 2:9] = 1
    gt[24:32, 20:30, 3:8] = 2
    pred = gt.copy()
    pred[36:38, 2:4, 9:11] = 1
    pf, gf = str(tmp_path / "dense_pred_s.nii.gz"), str(tmp_path / "gth_dense_pred_s.nii.gz")
    nifti.save(nifti.Nifti1Image(pred, np.eye(4)), pf)
    nifti.save(nifti.Nifti1Image(gt, np.eye(4)), gf)
    raw = ev.evaluate([(pf, gf)])
    fil = ev.evaluate([(pf, gf)], keep_largest=1)
    assert "keep_largest" not in raw and "component_stats" not in raw["subjects"][0]
    assert fil["keep_largest"] == {"keep": 1} and fil["subjects"][0]["component_stats"][1] == [2, 12 * 12 * 7 + 8, 12 * 12 * 7, 12 * 12 * 7]
    assert raw["subjects"][0]["hd"][1] > 15.0 and fil["subjects"][0]["hd"][1] == 0.0
    assert raw["subjects"][0]["dice"][1] < 1.0 and fil["subjects"][0]["dice"][1] == 1.0
    assert raw["subjects"][0]["hd"][2] == fil["subjects"][0]["hd"][2] == 0.0
    out = str(tmp_path / "score.json")
    assert ev.main(["--pred-dir", str(tmp_path), "--keep-largest", "--connectivity", "3", "--json", out]) == 0
    saved = json.load(open(out))
    assert saved["keep_largest"] == {"keep": 1, "min_size": 0, "connectivity": 3} and saved["subjects"][0]["hd"][1] == 0.0
    assert saved["subjects"][0]["component_stats"][1][0] == 2
    assert "predictions filtered" in capsys.readouterr().out
