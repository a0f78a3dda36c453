"""not gpu: the host side of volume inference (volume_predict.py, predict.py) — the restatement of tests/paste_ref.py pinned
to scipy.ndimage.map_coordinates(order=1, mode="nearest") + np.argmax, the inverse maps, the file layout, that the label bound of
tests/test_gpu_paste.py is not vacuous on the committed seeds, every argument refusal of pnp_paste_labels (decided on the host before any
HIP call: the buffers are small host buffers, never read), the CLI's argument errors and the affine of a written prediction."""
import ctypes

import numpy as np
import pytest

import paste_ref as R
from conftest import pkg


def _inv(case, which):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (H, W), (X, Y) = R.CASES[case][:2]
    return vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), **R.MAPS[which]))


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(R.MAPS))
@pytest.mark.parametrize("case", ["upsample", "downsample", "identity"])
def test_restatement_is_scipy_nearest_plus_argmax(case, which):
    nd = pytest.importorskip("scipy.ndimage")
    (H, W), (X, Y) = R.CASES[case][:2]
    logits = R.case_logits(case, 5)
    inv = _inv(case, which)
    pi, pj = R.coords(inv, X, Y)
    lab, r = R.labels(logits, inv, X, Y)
    for b in range(logits.shape[0]):
        ref = np.stack([nd.map_coordinates(logits[b, :, :, c].astype(np.float64), [pi, pj], order=1, mode="nearest") for c in range(5)], -1)
        np.testing.assert_allclose(r[b], ref, rtol=0, atol=1e-12)
        assert np.array_equal(lab[b], np.argmax(ref, -1))
    if case == "identity" and which == "resize":
        assert np.array_equal(lab, np.argmax(logits, -1))


def test_first_maximum_and_nan_coordinate():
    plane = np.zeros((1, 4, 4, 4), np.float32)
    plane[..., 1] = plane[..., 3] = 2.0
    lab, _ = R.labels(plane, [1, 0, 0, 0, 1, 0], 4, 4)
    assert np.all(lab == 1)
    plane = np.random.default_rng(0).standard_normal((4, 4, 3))
    r = R.interpolate(plane, np.array([[np.nan, 9.0]]), np.array([[2.0, -3.0]]))
    assert np.array_equal(r[0, 0], plane[0, 2]) and np.array_equal(r[0, 1], plane[3, 0])


# ---- inverse maps ----------------------------------------------------------------------------------------------------------------------
def test_invert_matrix_is_exact_for_permutations():
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    for n in (8, 9, 256):
        assert np.array_equal(vp.invert_matrix(vs.compose_matrix((n, n + 3), (n, n + 3))), np.array([1, 0, 0, 0, 1, 0], np.float32))
        for kw in ({"rotate": 90.0}, {"rotate": 180.0}, {"rotate": -90.0}, {"rotate": 270.0}, {"flip": True}, {"rotate": 90.0, "flip": True}):
            m = vs.compose_matrix((n, n), (n, n), **kw)
            inv = vp.invert_matrix(m)
            assert inv.dtype == np.float32 and np.array_equal(inv, np.round(inv)) and set(np.abs(inv[[0, 1, 3, 4]])) == {0.0, 1.0}, (kw, inv)
            # p -> s -> p is the identity on the whole grid, exactly
            i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
            sx, sy = m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]
            assert np.array_equal(inv[0] * sx + inv[1] * sy + inv[2], i) and np.array_equal(inv[3] * sx + inv[4] * sy + inv[5], j), kw
    with pytest.raises(ValueError, match="singular"):
        vp.invert_matrix([1, 2, 0, 2, 4, 0])


def test_invert_matrix_composes_to_the_identity():
    """a resize plus a 13 degree rotation: M o M^-1 is the identity within float64 rounding before the one rounding to float32, and the
    float32 entries are that inverse rounded once"""
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    m32 = vs.compose_matrix((180, 210), (256, 256), rotate=13.0, translate=(1.5, -2.25))
    m = m32.astype(np.float64)
    inv = vp.invert_matrix(m32, dtype=np.float64)
    A, t = m[[0, 1, 3, 4]].reshape(2, 2), m[[2, 5]]
    Bm, u = inv[[0, 1, 3, 4]].reshape(2, 2), inv[[2, 5]]
    eps = 2.0 ** -52
    # each entry of the inverse carries a few roundings (determinant, quotient); products of entries around 1, offsets around 256
    assert np.abs(A @ Bm - np.eye(2)).max() <= 16 * eps * np.abs(A).max() * np.abs(Bm).max()
    assert np.abs(A @ u + t).max() <= 16 * eps * 256 * np.abs(A).max() * np.abs(Bm).max()
    got = vp.invert_matrix(m32)
    assert got.dtype == np.float32 and np.array_equal(got, inv.astype(np.float32))


# ---- the file layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_file_layout_addresses_what_prepare_pair_views(flip, axis):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    shape = (5, 6, 7)
    arr = np.arange(np.prod(shape)).reshape(shape)
    sl, _ = vs.prepare_pair(arr, np.zeros(shape, np.uint8), flip, axis, None)
    for box in (None, ((1, 4), (2, 5), (0, 3))):
        origin, (sx, sy, sz), (X, Y, Z) = vp.file_layout(shape, flip, axis, box)
        want = sl if box is None else sl[tuple(slice(a, b) for a, b in box)]
        assert (X, Y, Z) == want.shape
        idx = R.written_index(X, Y, Z, 0, origin, (sx, sy, sz))          # [Z, X, Y]
        assert np.array_equal(arr.ravel()[idx].astype(np.float32), np.moveaxis(want, 2, 0))


def test_crop_boxes():
    vp = pkg("volume_predict")
    lab = np.zeros((6, 7, 8), np.uint8)
    lab[2:4, 3:6, 1:3] = 2
    assert vp._box_of(None, None, lab.shape) == ((0, 6), (0, 7), (0, 8))
    assert vp._box_of(1, lab, lab.shape) == ((1, 5), (2, 7), (0, 4))
    assert vp._box_of(((0, 6), (1, 2), (3, 8)), None, lab.shape) == ((0, 6), (1, 2), (3, 8))
    for bad in (((0, 7), (0, 7), (0, 8)), ((2, 2), (0, 7), (0, 8)), ((0, 6), (0, 7)), ((-1, 3), (0, 7), (0, 8))):
        with pytest.raises(ValueError):
            vp._box_of(bad, None, lab.shape)
    with pytest.raises(ValueError, match="a label is needed"):
        vp._box_of(2, None, lab.shape)


# ---- the bound of the GPU test is not vacuous ------------------------------------------------------------------------------------------
def test_admissible_sets_are_single_classes_almost_everywhere():
    """over N(0, 1) logits the top-2 gap has O(1) density and 2 delta ~ 1e-5: the share of voxels at which the bound admits more than one
    class must be <= 1e-3 over everything tests/test_gpu_paste.py runs (and the rotated map must reach the clamp on all four sides)"""
    multi = total = 0
    for case in sorted(R.CASES):
        (H, W), (X, Y), B, nb = R.CASES[case][:4]
        for which in sorted(R.MAPS):
            for ncls in ((1, 2, 5, 8) if case == "upsample" else (5,)):
                logits, inv = R.case_logits(case, ncls), _inv(case, which)
                _, r = R.labels(logits, inv, X, Y, nb)
                d = R.delta(logits[:nb], inv, X, Y)
                assert d < 1e-4, (case, which, d)
                if ncls > 1:
                    multi += int((R.admissible(r, d).sum(-1) > 1).sum())
                    total += r.shape[0] * X * Y
    assert total > 40000 and multi <= 1e-3 * total, (multi, total)
    pi, pj = R.coords(_inv("upsample", "rotated"), 37, 23)
    assert pi.min() < 0 and pi.max() > 15 and pj.min() < 0 and pj.max() > 23


# ---- argument refusals of pnp_paste_labels ---------------------------------------------------------------------------------------------
def test_paste_refusals_before_any_hip_call(built):
    L = built._lib
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    ident = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)

    def refused(msg, logits=ptr, B=2, H=8, W=8, ncls=5, nb=2, z0=1, inv=ident, X=4, Y=5, vol=ptr, elems=4 * 5 * 6, origin=0, s=(30, 6, 1)):
        rc = lib.pnp_paste_labels(logits, B, H, W, ncls, nb, z0, inv, X, Y, vol, elems, origin, s[0], s[1], s[2], None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())

    refused(b"null pointer", logits=None)
    refused(b"null pointer", inv=None)
    refused(b"null pointer", vol=None)
    refused(b"logits [0, 8, 8]", B=0)
    refused(b"logits [2, 0, 8]", H=0)
    refused(b"logits [2, 8, -1]", W=-1)
    refused(b"source extents 0 x 5", X=0)
    refused(b"source extents 4 x -2", Y=-2)
    refused(b"output plane 4097 x 8 above 4096", H=4097)
    refused(b"output plane 8 x 4097 above 4096", W=4097)
    refused(b"source extents 4097 x 5 above 4096", X=4097, elems=1 << 40, s=(1 << 20, 6, 1))
    refused(b"source extents 4 x 4097 above 4096", Y=4097, elems=1 << 40, s=(1 << 20, 6, 1))
    refused(b"ncls 0 outside [1, 8]", ncls=0)
    refused(b"ncls 9 outside [1, 8]", ncls=9)
    refused(b"nb = 0 outside [1, B = 2]", nb=0)
    refused(b"nb = 3 outside [1, B = 2]", nb=3)
    refused(b"z0 = -1 is negative", z0=-1)
    refused(b"vol_elems = 0", elems=0)
    # the extreme corners: frames 5 and 6 of a 6-frame volume; one element short; a negative stride without its origin; an origin below 0
    refused(b"outside [0, 120)", z0=5)
    refused(b"outside [0, 119)", z0=4, elems=119)
    refused(b"outside [0, 120)", s=(30, 6, -1), z0=0)
    refused(b"outside [0, 120)", s=(-30, 6, 1))
    refused(b"outside [0, 120)", origin=-1, z0=0)
    refused(b"outside [0, 120)", s=(1 << 62, 6, 1))
    # collisions: y's stride shorter than the nb frames of a column; equal strides; a zero stride
    refused(b"collide", s=(30, 1, 1))
    refused(b"collide", s=(6, 6, 1))
    refused(b"collide", s=(30, 0, 1))
    refused(b"collide", s=(4, 1, 30), z0=0)          # |sx| = 4 < Y = 5 bytes of a row
    refused(b"collide", s=(30, 6, 0))
    refused(b"collide", s=(-30, -1, 1), origin=118, z0=0)
    refused(b"collide", s=(1 << 40, 1 << 40, 1), elems=1 << 62, X=2, Y=2)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path):
    nifti = pkg("nifti")
    out = {}
    for name in ("a.nii.gz", "b.nii.gz", "la.nii.gz", "lb.nii.gz"):
        out[name] = str(tmp_path / name)
        nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16)), out[name])
    model = tmp_path / "m.npz"
    np.savez(str(model), x=np.zeros(1))
    return out, str(model)


def test_cli_arguments(tmp_path):
    pr = pkg("predict")
    f, model = _files(tmp_path)
    base = ["--model", model, "--net", "segmenter", "--out", str(tmp_path / "o")]
    a, images, labels, opt = pr.parse_args(base + ["--images", f["a.nii.gz"], f["b.nii.gz"]])
    assert images == [f["a.nii.gz"], f["b.nii.gz"]] and labels is None
    assert opt == {"edge": "replicate", "axis": 2, "flip_correction": True, "batch_size": 16, "crop": None}
    a, images, labels, opt = pr.parse_args(base + ["--images", f["a.nii.gz"], "--labels", f["la.nii.gz"], "--crop-margin", "3", "--edge", "skip",
                                                   "--axis", "1", "--no-flip-correction", "--batch-size", "4", "--score", "--spacing", "header"])
    assert labels == [f["la.nii.gz"]] and opt == {"edge": "skip", "axis": 1, "flip_correction": False, "batch_size": 4, "crop": 3} and a.score
    _, _, _, opt = pr.parse_args(base + ["--images", f["a.nii.gz"], "--crop", "0:4,1:3,0:2"])
    assert opt["crop"] == ((0, 4), (1, 3), (0, 2))
    lst = tmp_path / "list"
    lst.write_text("# pairs\na.nii.gz la.nii.gz\n%s lb.nii.gz\n" % f["b.nii.gz"])
    _, images, labels, _ = pr.parse_args(base + ["--list", str(lst)])
    assert images == [f["a.nii.gz"], f["b.nii.gz"]] and labels == [f["la.nii.gz"], f["lb.nii.gz"]]
    lst.write_text("a.nii.gz\nb.nii.gz\n")
    assert pr.parse_args(base + ["--list", str(lst)])[2] is None


def test_cli_argument_errors(tmp_path):
    pr = pkg("predict")
    f, model = _files(tmp_path)
    base = ["--model", model, "--net", "segmenter", "--out", str(tmp_path / "o")]
    img = ["--images", f["a.nii.gz"]]
    mixed = tmp_path / "mixed"
    mixed.write_text("a.nii.gz la.nii.gz\nb.nii.gz\n")
    three = tmp_path / "three"
    three.write_text("a.nii.gz la.nii.gz b.nii.gz\n")
    empty = tmp_path / "empty"
    empty.write_text("# nothing\n")
    for argv in (base,                                                          # neither --images nor --list
                 base + img + ["--list", str(mixed)],                           # both
                 ["--net", "segmenter", "--out", "o"] + img,                    # no --model
                 ["--model", model, "--net", "unet", "--out", "o"] + img,       # unknown net
                 ["--model", str(tmp_path / "missing.npz"), "--net", "adapted", "--out", "o"] + img,
                 base + ["--images", str(tmp_path / "missing.nii.gz")],
                 base + img + ["--labels", f["la.nii.gz"], f["lb.nii.gz"]],     # 2 labels for 1 image
                 base + img + ["--score"],                                      # --score without labels
                 base + img + ["--crop-margin", "2"],                           # a margin without labels
                 base + img + ["--labels", f["la.nii.gz"], "--crop-margin", "-1"],
                 base + img + ["--labels", f["la.nii.gz"], "--crop-margin", "2", "--crop", "0:1,0:1,0:1"],
                 base + img + ["--crop", "0:1,0:1"], base + img + ["--crop", "0:1,0:1,3:3"], base + img + ["--crop", "a:1,0:1,0:1"],
                 base + img + ["--json", "x.json"], base + img + ["--edge", "mirror"], base + img + ["--axis", "3"],
                 base + img + ["--batch-size", "0"],
                 base + ["--list", str(mixed)], base + ["--list", str(three)], base + ["--list", str(empty)],
                 base + ["--list", str(tmp_path / "nolist")]):
        with pytest.raises(SystemExit):
            pr.parse_args(argv)


def test_written_prediction_keeps_the_inputs_affine(tmp_path, monkeypatch):
    """predict_volumes with the device part replaced: what reaches the disk is uint8, of the input's shape, with the input's affine"""
    import torch
    vp, nifti = pkg("volume_predict"), pkg("nifti")
    aff = np.array([[0.0, -1.5, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, 3.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    rng = np.random.default_rng(0)
    img, lab = tmp_path / "scan.nii.gz", tmp_path / "scan_label.nii"
    nifti.save(nifti.Nifti1Image(rng.integers(-100, 900, (7, 5, 4)).astype(np.int16), aff), str(img))
    gt = rng.integers(0, 8, (7, 5, 4)).astype(np.int16)
    nifti.save(nifti.Nifti1Image(gt, aff), str(lab))
    seen = {}

    def fake(logits_fn, image, label=None, **kw):
        seen.update(kw, label=label)
        return torch.from_numpy((np.asarray(image) % 5).astype(np.uint8))
    monkeypatch.setattr(vp, "segment_volume", fake)
    paths = vp.predict_volumes(None, [str(img)], str(tmp_path / "out"), label_list=[str(lab)], num_cls=5, device="cpu", edge="skip")
    assert paths == [str(tmp_path / "out" / "pred_scan.nii.gz")] and seen["edge"] == "skip" and np.array_equal(seen["label"], gt)
    for name in ("pred_scan.nii.gz", "dense_pred_scan.nii.gz", "gth_dense_pred_scan.nii.gz"):
        got = nifti.load(str(tmp_path / "out" / name))
        assert got.shape == (7, 5, 4) and got.get_data().dtype == np.uint8 and np.allclose(got.affine, aff), name
    assert np.array_equal(nifti.load(paths[0]).get_data(), nifti.load(str(img)).get_data() % 5)
    assert np.array_equal(nifti.load(str(tmp_path / "out" / "gth_dense_pred_scan.nii.gz")).get_data(), np.where(gt > 4, 0, gt))
    assert pkg("evaluate").pairs_of_dir(str(tmp_path / "out")) == [(str(tmp_path / "out" / "dense_pred_scan.nii.gz"),
                                                                   str(tmp_path / "out" / "gth_dense_pred_scan.nii.gz"))]
