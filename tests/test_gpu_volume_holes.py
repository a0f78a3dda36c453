"""-m gpu: the hole filling where a user meets it — segment_volume(fill_holes=) on the plain, ensemble and multi-planar
paths, together with keep_largest, Trainer.predict_volumes and the predict and evaluate command lines.  segment_volume runs a stub network
whose argmax is a planted pattern with holes: the scan's grey level encodes the class, the stub answers -(x - level of class c)^2 on the
centre channel.  Labels are integers: every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import holes_ref as R
import test_gpu_volume_predict as P
from conftest import pkg

pytestmark = pytest.mark.gpu

LEVELS = np.array([0, 300, 600, 900, 1200], dtype=np.float64)
N = 40                                                  # a cube with out_size = (N, N): every view's plane is the volume's own grid
COMMON = dict(out_size=(N, N), batch_size=4, percentile=100)


def _pattern():
    """class 1: a block with a 3 x 3 x 3 background hole and a 2 x 2 x 2 pocket of class 3; class 2: a block with a 2 x 3 x 4 hole that also
    touches a pocket of class 4; class 3: a larger structure elsewhere; a background notch that is open to the outside"""
    L = np.zeros((N, N, N), np.uint8)
    L[4:20, 4:20, 4:20] = 1
    L[8:11, 8:11, 8:11] = 0
    L[14:16, 14:16, 14:16] = 3
    L[22:36, 22:36, 10:30] = 2
    L[26:28, 26:29, 15:19] = 0
    L[28:30, 26:29, 15:19] = 4
    L[4:16, 24:36, 24:36] = 3
    L[8:10, 24:27, 28:30] = 0                           # reaches the structure's surface at y = 24: no cavity
    return L


@pytest.fixture(scope="module")
def planted():
    L = _pattern()
    image = LEVELS[L].astype(np.int16)
    centres = (LEVELS - image.mean()) / image.std()     # volume_preprocess at percentile 100: the z-score of the whole box

    def fn(x):
        c = torch.tensor(centres, device=x.device, dtype=torch.float32).view(1, 1, 1, -1)
        return (-4.0 * (x[..., 1:2] - c) ** 2).contiguous()
    return L, image, fn


@pytest.fixture(scope="module")
def plain(dev, planted):
    _, image, fn = planted
    out = pkg("volume_predict").segment_volume(fn, image, device=dev, **COMMON)
    host = out.cpu().numpy()
    _, stats, info = R.fill_holes(host, 5)
    assert info["cavities"] >= 2 and stats[0, 1] > 0, "a prediction without holes shows nothing"
    return out, host


def test_the_stub_predicts_the_planted_pattern(planted, plain):
    assert np.array_equal(plain[1], planted[0])


def test_segment_volume_option_equals_filling_its_result(dev, planted, plain):
    vp, C = pkg("volume_predict"), pkg("components")
    _, image, fn = planted
    unfilled, host = plain
    stats = []
    got = vp.segment_volume(fn, image, device=dev, fill_holes=True, hole_stats=stats, **COMMON)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == image.shape and len(stats) == 1
    want, want_stats = C.fill_holes(unfilled)
    assert np.array_equal(unfilled.cpu().numpy(), host)
    assert torch.equal(got, want) and torch.equal(stats[0], want_stats)
    ref_out, ref_stats, _ = R.fill_holes(host, 5)
    assert np.array_equal(got.cpu().numpy(), ref_out) and np.array_equal(stats[0].cpu().numpy(), ref_stats)
    assert ref_stats.tolist() == [[2, 27 + 24, 0, 0], [1, 27, 27, 0], [1, 24, 24, 0], [0] * 4, [0] * 4]
    assert (ref_out[8:11, 8:11, 8:11] == 1).all() and (ref_out[26:28, 26:29, 15:19] == 2).all() and not ref_out[8:10, 24:27, 28:30].any()
    assert (ref_out[14:16, 14:16, 14:16] == 3).all(), "a class inside a class is never touched"
    opts = {"max_size": 24, "classes": [1, 2]}
    got = vp.segment_volume(fn, image, device=dev, fill_holes=opts, **COMMON)
    assert np.array_equal(got.cpu().numpy(), R.fill_holes(host, 5, 24, [1, 2])[0]) and not got[8:11, 8:11, 8:11].any()
    got = vp.segment_volume(fn, image, device=dev, fill_holes=24, **COMMON)
    assert np.array_equal(got.cpu().numpy(), R.fill_holes(host, 5, 24)[0])
    for off in (None, False):
        assert torch.equal(vp.segment_volume(fn, image, device=dev, fill_holes=off, **COMMON), unfilled)


def test_keep_largest_runs_first(dev, planted, plain):
    """keep_largest(keep=1) empties the class-3 pocket (the larger class-3 structure stays), fill_holes then closes it with class 1; in the
    other order the pocket would be anatomy for the fill and a hole after the filter"""
    vp, C = pkg("volume_predict"), pkg("components")
    _, image, fn = planted
    unfilled, host = plain
    cs, hs = [], []
    got = vp.segment_volume(fn, image, device=dev, keep_largest=1, fill_holes=True, component_stats=cs, hole_stats=hs, **COMMON)
    kept, kept_stats, _ = __import__("components_ref").keep_largest(host, 5)
    want, want_stats, _ = R.fill_holes(kept, 5)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cs[0].cpu().numpy(), kept_stats) and np.array_equal(hs[0].cpu().numpy(), want_stats)
    assert (want[14:16, 14:16, 14:16] == 1).all() and want_stats[1].tolist() == [2, 27 + 8, 27, 0]
    other = C.keep_largest(C.fill_holes(unfilled)[0])[0]
    assert not other[14:16, 14:16, 14:16].any() and not torch.equal(other, got)


def test_ensemble_path_fills_the_label_only(dev, planted):
    vp, C = pkg("volume_predict"), pkg("components")
    _, image, fn = planted
    base = vp.segment_volume(fn, image, device=dev, prob=True, entropy=True, **COMMON)
    got = vp.segment_volume(fn, image, device=dev, prob=True, entropy=True, fill_holes={"classes": [1]}, **COMMON)
    assert isinstance(got, vp.Ensemble)
    assert torch.equal(got.prob, base.prob) and torch.equal(got.entropy, base.entropy)
    want, _ = C.fill_holes(base.label, classes=[1])
    assert torch.equal(got.label, want) and not torch.equal(got.label, base.label)
    assert np.array_equal(want.cpu().numpy(), R.fill_holes(base.label.cpu().numpy(), 5, 0, [1])[0])


def test_axes_fill_once_on_the_fused_label(dev, planted):
    vp = pkg("volume_predict")
    _, image, fn = planted
    base = vp.segment_volume(fn, image, device=dev, axes=(0, 1, 2), **COMMON)
    hs = []
    got = vp.segment_volume(fn, image, device=dev, axes=(0, 1, 2), fill_holes=True, hole_stats=hs, **COMMON)
    want, want_stats, info = R.fill_holes(base.label.cpu().numpy(), 5)
    assert info["cavities"] >= 2 and len(hs) == 1, "once, on the fused label: one stats tensor, not one per view"
    assert np.array_equal(got.label.cpu().numpy(), want) and np.array_equal(hs[0].cpu().numpy(), want_stats)


@pytest.fixture(scope="module")
def seg(dev):
    ss = pkg("source_segmenter")
    return P._random_state(ss.Full_DRN(channels=3, n_class=5, batch_size=P.B, device=dev, seed=0, cost_kwargs=dict(P.COST)), 5,
                           pkg("volume_predict").segmenter_logits)


def test_trainer_and_predict_command_line(dev, seg, tmp_path, capsys):
    ss, nifti, pr, C = pkg("source_segmenter"), pkg("nifti"), pkg("predict"), pkg("components")
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(P._scan((40, 36, 8), 4), np.eye(4)), a)
    tr = ss.Trainer(seg, train_list=[], val_list=[], num_cls=5, batch_size=P.B)
    unfilled = np.ascontiguousarray(nifti.load(tr.predict_volumes([a], str(tmp_path / "plain"))[0]).get_data())
    want, want_stats, info = R.fill_holes(unfilled, 5)
    print("cavities", info["cavities"], "ties", info["ties"], "voxels", int(want_stats[0, 1]))
    assert want_stats[0, 1] > 0, "a prediction without holes shows nothing"
    hs = []
    method = nifti.load(tr.predict_volumes([a], str(tmp_path / "method"), fill_holes=True, hole_stats=hs)[0]).get_data()
    assert np.array_equal(method, want) and np.array_equal(hs[0].cpu().numpy(), want_stats)
    ckpt = seg.save(str(tmp_path / "ckpt.npz"))
    ckpt = ckpt if isinstance(ckpt, str) and os.path.isfile(ckpt) else str(tmp_path / "ckpt.npz")
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", a, "--out", str(tmp_path / "cli"), "--batch-size", str(P.B), "--fill-holes"])
    assert np.array_equal(nifti.load(res["paths"][0]).get_data(), want)
    assert res["hole_stats"] == [want_stats.tolist()] and "component_stats" not in res
    assert "holes  %s" % C.fill_stats_line(want_stats) in capsys.readouterr().out
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", a, "--out", str(tmp_path / "cli2"), "--batch-size", str(P.B),
                   "--fill-holes", "1", "--fill-classes", "2,3"])
    assert np.array_equal(nifti.load(res["paths"][0]).get_data(), R.fill_holes(unfilled, 5, 1, [2, 3])[0])


def test_evaluate_with_a_planted_hole(dev, tmp_path, capsys):
    """the prediction is the ground truth with a 3 x 3 x 3 hole in class 1: unfilled, the hole costs Dice and adds an inner surface; filled,
    prediction and ground truth coincide"""
    nifti, ev = pkg("nifti"), pkg("evaluate")
    gt = np.zeros((40, 36, 12), np.uint8)
    gt[8:20, 6:18, 2:9] = 1
    gt[24:32, 20:30, 3:8] = 2
    pred = gt.copy()
    pred[12:15, 10:13, 4:7] = 0
    pf, gf = str(tmp_path / "dense_pred_s.nii.gz"), str(tmp_path / "gth_dense_pred_s.nii.gz")
    nifti.save(nifti.Nifti1Image(pred, np.eye(4)), pf)
    nifti.save(nifti.Nifti1Image(gt, np.eye(4)), gf)
    raw = ev.evaluate([(pf, gf)])
    fil = ev.evaluate([(pf, gf)], fill_holes=True)
    assert "fill_holes" not in raw and "hole_stats" not in raw["subjects"][0]
    assert fil["fill_holes"] == {} and "keep_largest" not in fil and "component_stats" not in fil["subjects"][0]
    assert fil["subjects"][0]["hole_stats"] == [[1, 27, 0, 0], [1, 27, 27, 0], [0] * 4, [0] * 4, [0] * 4]
    assert raw["subjects"][0]["dice"][1] < 1.0 and fil["subjects"][0]["dice"][1] == 1.0
    assert raw["subjects"][0]["assd"][1] > 0.0 and fil["subjects"][0]["assd"][1] == 0.0
    assert raw["subjects"][0]["dice"][2] == fil["subjects"][0]["dice"][2] == 1.0
    small = ev.evaluate([(pf, gf)], fill_holes=26)
    assert small["fill_holes"] == {"max_size": 26} and small["subjects"][0]["hole_stats"][0] == [1, 27, 1, 27] and small["subjects"][0]["dice"][1] < 1.0
    out = str(tmp_path / "score.json")
    assert ev.main(["--pred-dir", str(tmp_path), "--fill-holes", "--fill-classes", "1", "--keep-largest", "--json", out]) == 0
    saved = json.load(open(out))
    assert saved["fill_holes"] == {"classes": [1]} and saved["keep_largest"]["keep"] == 1 and saved["subjects"][0]["dice"][1] == 1.0
    assert saved["subjects"][0]["hole_stats"][1] == [1, 27, 27, 0] and saved["subjects"][0]["component_stats"][1][0] == 1
    assert "holes filled" in capsys.readouterr().out
