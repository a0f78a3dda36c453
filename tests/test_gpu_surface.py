"""-m gpu: the surface-distance kernels (csrc/surface.hip) against the float64 reference (tests/surface_ref.py): the exact squared EDT
(bit-exact with unit spacing), the per-class metrics of surface.surface_metrics, determinism, one 256x256x200 pair with a closed-form
answer, Trainer.test_eval(surface=True) of both trainers and the evaluate CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surface_ref as R
from conftest import PKG, ROOT, pkg
from test_gpu_volume import COST, NETCFG, _expected, _he, _volume

pytestmark = pytest.mark.gpu

DIST = ("asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95")


def _pairmin_dev(dev):
    """the reference's brute-force pairwise minimum in float64 on the device (volumes of the trainer tests are too large for numpy)"""
    def pm(pa, pb, chunk=256):
        a = torch.from_numpy(pa).to(dev)
        b = torch.from_numpy(pb).to(dev)
        out = torch.empty(len(pa), dtype=torch.float64, device=dev)
        for i in range(0, len(pa), chunk):
            ac = a[i:i + chunk]
            d2 = (ac[:, None, 0] - b[None, :, 0]) ** 2
            d2 += (ac[:, None, 1] - b[None, :, 1]) ** 2
            d2 += (ac[:, None, 2] - b[None, :, 2]) ** 2
            out[i:i + chunk] = d2.min(dim=1).values.sqrt()
        return out.cpu().numpy()
    return pm


def _same(m, ref, rtol_sum, exact_max, num_cls):
    for k in ("n_border_pred", "n_border_gt"):
        np.testing.assert_array_equal(m[k][1:], ref[k][1:], err_msg=k)
    for k in DIST:
        assert np.isnan(m[k][0]), k
        np.testing.assert_array_equal(np.isnan(m[k]), np.isnan(ref[k]), err_msg=k)
        ok = ~np.isnan(ref[k])
        if exact_max and k in ("hd", "hd95"):
            np.testing.assert_array_equal(m[k][ok], ref[k][ok], err_msg=k)
        else:
            np.testing.assert_allclose(m[k][ok], ref[k][ok], rtol=rtol_sum, atol=0, err_msg=k)


@pytest.mark.parametrize("shape", [(37, 29, 23), (1, 64, 5), (200, 3, 3), (1024, 2, 3)])
def test_edt_against_reference(dev, shape):
    K = pkg("kernels")
    rng = np.random.default_rng(sum(shape))
    mask = (rng.random(shape) < 0.01)
    mask.flat[rng.integers(0, mask.size)] = True
    md = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    got = K.edt_sq(md).cpu().numpy()
    ref = R.edt_sq(mask)
    assert np.array_equal(got, ref.astype(np.float32)) and np.array_equal(got.astype(np.float64), ref)       # unit spacing: bit-exact
    sp = (0.7, 1.3, 2.5)
    got = K.edt_sq(md, sp).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, R.edt_sq(mask, sp), rtol=1e-6, atol=0)
    empty = K.edt_sq(torch.zeros(shape, dtype=torch.uint8, device=dev)).cpu().numpy()
    assert np.all(np.isposinf(empty))


@pytest.fixture(scope="module")
def blobs():
    shape = (96, 80, 40)
    return R.ellipsoids(shape, 5, 1), R.ellipsoids(shape, 5, 2)


def test_metrics_against_reference(dev, blobs):
    S = pkg("surface")
    p, g = blobs
    m = S.surface_metrics(p, g, 5)
    _same(m, R.metrics(p, g, 5, pairmin=_pairmin_dev(dev)), 1e-12, True, 5)
    sp = (0.8, 1.1, 2.5)
    m = S.surface_metrics(torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev), 5, sp)
    _same(m, R.metrics(p, g, 5, sp, pairmin=_pairmin_dev(dev)), 1e-6, False, 5)


def test_metrics_edge_cases(dev, blobs):
    S = pkg("surface")
    p, g = blobs
    p = p.copy()
    g = g.copy()
    p[0, :, :] = 1                       # objects touching the volume edge
    g[:, :, -1] = 2
    p[p == 4] = 0                        # class 4 empty in the prediction
    m = S.surface_metrics(p, g, 5)
    ref = R.metrics(p, g, 5, pairmin=_pairmin_dev(dev))
    _same(m, ref, 1e-12, True, 5)
    assert m["n_border_pred"][4] == 0 and m["n_border_gt"][4] > 0 and all(np.isnan(m[k][4]) for k in DIST)
    same = S.surface_metrics(g, g, 5)
    for k in DIST:
        assert np.all(same[k][1:4] == 0.0), k
    sw = S.surface_metrics(g, p, 5)      # swapped arguments: directions swap
    np.testing.assert_array_equal(sw["asd_pred_gt"][1:4], m["asd_gt_pred"][1:4])
    np.testing.assert_array_equal(sw["n_border_pred"][1:], m["n_border_gt"][1:])
    np.testing.assert_array_equal(sw["hd95"][1:4], m["hd95"][1:4])


def test_binary_wrappers(dev):
    S = pkg("surface")
    big = np.zeros((9, 9, 9), bool)
    small = np.zeros_like(big)
    big[2:7, 2:7, 2:7] = True
    small[3:6, 3:6, 3:6] = True
    assert S.asd(small, big) == 1.0
    assert abs(S.asd(big, small) - (8 * 3 ** 0.5 + 36 * 2 ** 0.5 + 54) / 98) < 1e-14
    assert S.hd(small, big) == 3 ** 0.5 and S.hd95(big, small) == 3 ** 0.5
    assert S.assd(small, big) == S.assd(big, small)
    with pytest.raises(RuntimeError):
        S.hd(np.zeros_like(big), big)


def test_determinism(dev, blobs):
    K = pkg("kernels")
    p, g = (torch.from_numpy(v).to(dev) for v in blobs)
    a = K.surface_distances(p, g, 5, (0.8, 1.1, 2.5)).cpu().numpy()
    b = K.surface_distances(p, g, 5, (0.8, 1.1, 2.5)).cpu().numpy()
    assert a.tobytes() == b.tobytes()


BOXES = [(1, (20, 120), (30, 100), (10, 60)), (2, (140, 230), (20, 90), (40, 43)), (3, (30, 200), (130, 240), (80, 150)),
         (4, (210, 250), (150, 250), (160, 190))]


def _boxes(shape, dz):
    v = np.zeros(shape, np.int32)
    for c, (x0, x1), (y0, y1), (z0, z1) in BOXES:
        v[x0:x1, y0:y1, z0 + dz:z1 + dz] = c
    return v


def test_scale_closed_form(dev):
    """256 x 256 x 200, 4 classes: boxes against the same boxes shifted by +1 in z — every distance is 0 or 1"""
    S = pkg("surface")
    m = S.surface_metrics(_boxes((256, 256, 200), 0), _boxes((256, 256, 200), 1), 5)
    for c, (x0, x1), (y0, y1), (z0, z1) in BOXES:
        nx, ny, nz = x1 - x0, y1 - y0, z1 - z0
        nb = nx * ny * nz - (nx - 2) * (ny - 2) * (nz - 2)
        ones = nx * ny + (nx - 2) * (ny - 2)                # the whole bottom (top) slice + the interior of the top (bottom) slice
        assert m["n_border_pred"][c] == nb and m["n_border_gt"][c] == nb
        assert m["asd_pred_gt"][c] == ones / nb and m["asd_gt_pred"][c] == ones / nb and m["hd"][c] == 1.0
        pooled = np.r_[np.zeros(2 * (nb - ones)), np.ones(2 * ones)]
        assert m["hd95"][c] == np.percentile(pooled, 95)


def _csv_rows(path):
    lines = open(path).read().strip().split("\n")
    assert lines[0].startswith("subject,organ,label,")
    return [l.split(",") for l in lines[1:]]


def _check_rows(rows, subject, m, names):
    mine = [r for r in rows if r[0] == subject]
    assert [r[1] for r in mine] == names
    for r in mine:
        c = int(r[2])
        vals = [float(x) for x in r[3:]]
        want = [m["n_border_pred"][c], m["n_border_gt"][c], m["asd_pred_gt"][c], m["asd_gt_pred"][c], m["assd"][c], m["hd"][c], m["hd95"][c]]
        np.testing.assert_array_equal(vals, want)


def test_segmenter_test_eval_surface(dev, tmp_path):
    ss, L, S = pkg("source_segmenter"), pkg("lib"), pkg("surface")
    B = 2

    def run(out, surface):
        net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, cost_kwargs={"cross_flag": True, "miu_cross": 1.0, "dice_flag": True,
                                                                                       "miu_dice": 1.0, "regularizer": 1e-4}, seed=3)
        _he(net, 5)
        tr = ss.Trainer(net, None, None, num_cls=5, batch_size=B, test_nii_list=[img], test_label_list=[lab], optimizer="adam",
                        opt_kwargs={"learning_rate": 1e-3})
        return tr, tr.test_eval(None, out, flip_correction=True, save_result=True, surface=surface)

    img, lab, raw, laby = _volume(tmp_path, 6, 0)
    _, (d0, s0) = run(str(tmp_path / "off"), False)
    tr, (d1, s1) = run(str(tmp_path / "on"), True)
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1)
    assert not os.path.exists(str(tmp_path / "off" / "surface.csv"))
    folder = tmp_path / "on" / "test_pred"
    pred = L.read_nii_image(str(folder / "dense_pred_img_0.nii.gz"))
    gth = L.read_nii_image(str(folder / "gth_dense_pred_img_0.nii.gz"))
    m = S.surface_metrics(pred, gth, 5)
    names = [o for o, i in sorted(ss.contour_map.items(), key=lambda kv: kv[1]) if i > 0]
    _check_rows(_csv_rows(str(tmp_path / "on" / "surface.csv")), "img_0.nii.gz", m, names)
    assert len(tr.surface_eval_list) == 1
    ref = R.metrics(pred, gth, 5, pairmin=_pairmin_dev(dev))
    _same(m, ref, 1e-12, True, 5)


def test_adversarial_test_eval_surface(dev, tmp_path):
    adv = pkg("adversarial")
    B = 2
    vols = [_volume(tmp_path, 5, s) for s in (1, 2)]

    def run(out, surface):
        net = adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(COST), network_config=dict(NETCFG), device=dev, seed=1)
        _he(net, 7)
        tr = adv.Trainer(net, None, None, None, None, num_cls=5, batch_size=B, test_nii_list=[v[0] for v in vols],
                         test_label_list=[v[1] for v in vols], opt_kwargs={"learning_rate": 3e-4})
        np.random.seed(11)
        return net, tr, tr.test_eval(None, out, surface=surface)

    _, _, (d0, s0) = run(str(tmp_path / "off"), False)
    net, tr, (d1, s1) = run(str(tmp_path / "on"), True)
    assert np.array_equal(d0, d1) and np.array_equal(s0, s1)

    def predict_one(x):
        p, _ = net.predict_ct(torch.from_numpy(x).to(dev), torch.zeros((B, 256, 256, 5), device=dev))
        return p.cpu().numpy()

    rows = _csv_rows(str(tmp_path / "on" / "surface.csv"))
    names = [o for o, i in sorted(adv.contour_map.items(), key=lambda kv: kv[1]) if i > 0]
    np.random.seed(11)
    for img, lab, raw, laby in vols:
        frames = [1, 2, 3]
        np.random.shuffle(frames)
        vol_pred, _ = _expected(predict_one, raw, laby, B, [frames[0:2], frames[2:4]])
        gt = np.flip(np.flip(laby, 0), 1)
        ref = R.metrics(vol_pred, gt, 5, pairmin=_pairmin_dev(dev))
        sub = os.path.basename(img)
        mine = [r for r in rows if r[0] == sub]
        assert [r[1] for r in mine] == names
        for r in mine:
            c = int(r[2])
            vals = np.array([float(x) for x in r[3:]])
            want = np.array([ref[k][c] for k in ("n_border_pred", "n_border_gt", "asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95")])
            np.testing.assert_array_equal(np.isnan(vals), np.isnan(want))
            ok = ~np.isnan(want)
            np.testing.assert_allclose(vals[ok], want[ok], rtol=1e-12, atol=0)
            assert vals[5] == want[5] or np.isnan(want[5])
    assert len(tr.surface_eval_list) == 2


def test_evaluate_cli(dev, tmp_path):
    L, S, E = pkg("lib"), pkg("surface"), pkg("evaluate")
    shape = (40, 36, 24)
    aff = np.diag([1.25, 1.25, 2.0, 1.0])
    preds, gts = [], []
    for s in range(2):
        p, g = R.ellipsoids(shape, 5, 30 + s).astype(np.float64), R.ellipsoids(shape, 5, 40 + s).astype(np.float64)
        preds.append(L.write_nii(p, "p%d.nii.gz" % s, str(tmp_path), affine=aff))
        gts.append(L.write_nii(g, "g%d.nii.gz" % s, str(tmp_path), affine=aff))
    out = str(tmp_path / "res.json")
    cmd = [sys.executable, "-m", PKG + ".evaluate", "--pred"] + preds + ["--gt"] + gts + ["--spacing", "header", "--json", out]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(out))
    for s in range(2):
        p, g = L.read_nii_image(preds[s]), L.read_nii_image(gts[s])
        m = S.surface_metrics(p, g, 5, (1.25, 1.25, 2.0))
        sub = res["subjects"][s]
        for k in ("assd", "hd95"):
            np.testing.assert_array_equal([np.nan if v is None else v for v in sub[k]], m[k])
        np.testing.assert_allclose(sub["dice"], E.dice_3d(p, g, 5, dev), rtol=0, atol=0)
        pi, gi = p.astype(int), g.astype(int)
        for c in range(1, 5):
            tot = (pi == c).sum() + (gi == c).sum()
            assert abs(sub["dice"][c] - 2.0 * ((pi == c) & (gi == c)).sum() / tot) < 1e-15
    assert "la_blood" in res["organs"] and "dice_mean" in res["organs"]["la_blood"]
