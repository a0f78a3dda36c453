"""not gpu: the host side of ensemble inference — the restatement of tests/ensemble_ref.py pinned to
scipy.ndimage.map_coordinates(order=1, mode="nearest") + scipy.special.softmax, every new host refusal of pnp_paste_ensemble by its text
(decided before any HIP call: the buffers are small host buffers, never read), the tta validation, the CLI's new argument errors, the
prob_ / entropy_ files of a stubbed prediction, and that the label bound of tests/test_gpu_ensemble.py is not vacuous on its cases."""
import ctypes
import json

import numpy as np
import pytest

import ensemble_ref as E
import paste_ref as R
from conftest import pkg


def _invs(case, M):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (H, W), (X, Y) = R.CASES[case][:2]
    return [vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), **E.MAPS[m])) for m in range(M)]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["upsample", "downsample", "identity"])
def test_restatement_is_scipy_nearest_plus_softmax(case):
    nd, sp = pytest.importorskip("scipy.ndimage"), pytest.importorskip("scipy.special")
    (H, W), (X, Y), B = R.CASES[case][:3]
    M, ncls = 4, 5
    logits = [E.smooth_logits(case, ncls, m) for m in range(M)]
    invs = _invs(case, M)
    res = E.ensemble(logits, invs, X, Y)
    probs = []
    for lg, inv in zip(logits, invs):
        pi, pj = R.coords(inv, X, Y)
        r = np.stack([np.stack([nd.map_coordinates(lg[b, :, :, c].astype(np.float64), [pi, pj], order=1, mode="nearest") for c in range(ncls)], -1)
                      for b in range(B)])
        probs.append(sp.softmax(r, axis=-1))
    P = np.mean(probs, axis=0)
    np.testing.assert_allclose(res.prob, P, rtol=0, atol=1e-12)
    assert np.array_equal(res.label, np.argmax(P, -1))
    H_ref = -(P * np.log(P)).sum(-1) / np.log(ncls)
    np.testing.assert_allclose(res.entropy, H_ref, rtol=0, atol=1e-12)
    assert res.entropy.min() >= 0 and res.entropy.max() <= 1 + 1e-12 and len(np.unique(res.label)) > 1


def test_restatement_edge_cases():
    """first maximum; ncls = 1: P = 1, entropy 0; a zero probability contributes 0 to the entropy; the paste of all three allocations"""
    ident = [1, 0, 0, 0, 1, 0]
    two = np.zeros((1, 4, 4, 4), np.float32)
    two[..., 1] = two[..., 3] = 2.0
    res = E.ensemble([two, two], [ident, ident], 4, 4)
    assert np.all(res.label == 1)
    one = E.ensemble([np.ones((2, 4, 4, 1), np.float32)], [ident], 4, 4)
    assert np.all(one.prob == 1.0) and np.all(one.entropy == 0.0) and np.all(one.label == 0)
    assert E.entropy(np.array([[0.0, 1.0], [0.5, 0.5]])).tolist() == [0.0, 1.0]
    elems, origin, strides = R.layout("sub_box", 4, 4, 5)
    vol, prob, ent = np.full(elems, 0xAB, np.uint8), np.full(4 * elems, -7.0, np.float32), np.full(elems, -7.0, np.float32)
    big = E.ensemble([two], [ident], 4, 4)
    idx = E.paste(vol, prob, ent, big, 1, origin, strides)
    assert (vol != 0xAB).sum() == 16 and (ent != -7.0).sum() == 16 and (prob != -7.0).sum() == 64
    assert np.allclose(prob.reshape(4, elems)[:, idx.ravel()].sum(0), 1.0) and np.all(vol[idx] == 1)
    assert E.entropy_bound(1e-6, 1) == 0.0 and 0 < E.entropy_bound(1e-6, 5) < 1e-4


# ---- the label bound of the GPU test is not vacuous ------------------------------------------------------------------------------------
def test_admissible_sets_are_single_classes_almost_everywhere():
    """per class count, over everything tests/test_gpu_ensemble.py compares with a bound: the voxels at which more than one class lies
    within 2 delta_p of the largest mean probability are at most 1e-3 of all (the cap of §14)"""
    multi, total = {}, {}
    for case, M, ncls in E.SWEEP:
        if ncls == 1:
            continue
        (H, W), (X, Y), B, nb = R.CASES[case][:4]
        logits, invs = [E.smooth_logits(case, ncls, m) for m in range(M)], _invs(case, M)
        res = E.ensemble(logits, invs, X, Y, nb)
        dp = E.delta_p(logits, invs, X, Y, nb)
        assert E.K_ROUND * E.U < dp < 1e-4, (case, M, ncls, dp)
        multi[ncls] = multi.get(ncls, 0) + int((E.admissible(res.prob, dp).sum(-1) > 1).sum())
        total[ncls] = total.get(ncls, 0) + nb * X * Y
    print({n: (multi[n], total[n], multi[n] / total[n]) for n in sorted(total)})
    assert sorted(total) == [2, 5, 8]
    for n in total:
        assert total[n] > 5000 and multi[n] <= 1e-3 * total[n], (n, multi[n], total[n])


# ---- argument refusals of pnp_paste_ensemble -------------------------------------------------------------------------------------------
def test_ensemble_refusals_before_any_hip_call(built):
    L = built._lib
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    addr = ctypes.addressof(buf)

    def refused(msg, M=2, members=None, inv=True, B=2, H=8, W=8, ncls=5, nb=2, z0=1, X=4, Y=5, vol=ptr, elems=4 * 5 * 6, origin=0, s=(30, 6, 1),
                no_array=False):
        members = [addr] * max(M, 1) if members is None else members
        arr = None if no_array else (ctypes.c_void_p * len(members))(*members)
        maps = (ctypes.c_float * (6 * len(members)))(*([1, 0, 0, 0, 1, 0] * len(members))) if inv else None
        rc = lib.pnp_paste_ensemble(M, arr, maps, B, H, W, ncls, nb, z0, X, Y, vol, elems, origin, s[0], s[1], s[2], None, None, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())
        assert lib.pnp_last_error().startswith(b"pnp_paste_ensemble:"), lib.pnp_last_error()

    # the new ones
    refused(b"M = 0 members outside [1, 8]", M=0)
    refused(b"M = 9 members outside [1, 8]", M=9)
    refused(b"M = -1 members outside [1, 8]", M=-1)
    refused(b"member 1 of 2 is a null pointer", members=[addr, None])
    refused(b"member 0 of 3 is a null pointer", M=3, members=[None, addr, addr])
    refused(b"null inv", inv=False)
    refused(b"null pointer", no_array=True)
    refused(b"null pointer", vol=None)
    refused(b"ncls * vol_elems = 5 * 4611686018427387904 overflows int64", elems=1 << 62)
    refused(b"ncls * vol_elems = 2 * 4611686018427387904 overflows int64", elems=1 << 62, ncls=2)
    # everything pnp_paste_labels refuses, under this entry point's name
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
    refused(b"outside [0, 120)", z0=5)
    refused(b"outside [0, 119)", z0=4, elems=119)
    refused(b"outside [0, 120)", s=(30, 6, -1), z0=0)
    refused(b"outside [0, 120)", s=(-30, 6, 1))
    refused(b"outside [0, 120)", origin=-1, z0=0)
    refused(b"outside [0, 120)", s=(1 << 62, 6, 1))
    refused(b"collide", s=(30, 1, 1))
    refused(b"collide", s=(6, 6, 1))
    refused(b"collide", s=(30, 0, 1))
    refused(b"collide", s=(4, 1, 30), z0=0)
    refused(b"collide", s=(30, 6, 0))
    refused(b"collide", s=(-30, -1, 1), origin=118, z0=0)
    refused(b"collide", s=(1 << 40, 1 << 40, 1), elems=1 << 60, X=2, Y=2)
    # and the older entry point still speaks under its own name
    ident = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)
    assert lib.pnp_paste_labels(ptr, 2, 8, 8, 5, 2, 1, ident, 4, 5, ptr, 120, 0, 30, 1, 1, None) == -1
    assert lib.pnp_last_error().startswith(b"pnp_paste_labels: strides 30 1 1 let two voxels of a 4 x 5 x 2 box collide")


# ---- tta and members -------------------------------------------------------------------------------------------------------------------
def test_tta_validation():
    vp = pkg("volume_predict")
    assert vp.tta_entries(None) == [{}]
    assert vp.tta_entries("default") == [{}, {"rotate": 7.5}, {"rotate": -7.5}, {"scale": 0.95}, {"scale": 1.05}]
    got = vp.tta_entries([{"rotate": 5, "translate": [1, 2]}, {"flip": True, "scale": 2}])
    assert got == [{"rotate": 5.0, "translate": (1.0, 2.0)}, {"flip": True, "scale": 2.0}]
    for bad, text in (([], "empty"), ("best", "default"), ({"rotate": 1.0}, "list of dicts"), ([3.0], "dict"), ([{"rot": 1.0}], "unknown keys"),
                      ([{"scale": 0.0}], "positive"), ([{"scale": -1.0}], "positive"), ([{"rotate": float("nan")}], "finite"),
                      ([{"rotate": "a"}], "tta\\[0\\]"), ([{"translate": (1.0,)}], "two finite"), ([{"translate": 3.0}], "tta\\[0\\]"),
                      ([{}, {"flip": 1}], "tta\\[1\\].*bool")):
        with pytest.raises(ValueError, match=text):
            vp.tta_entries(bad)
    f, g = (lambda x: x), (lambda x: x)
    assert vp.ensemble_members(f, None) == ([f], [{}])
    fns, entries = vp.ensemble_members([f, g], [{}, {"rotate": 3.0}, {"flip": True}, {"scale": 1.1}])
    assert fns == [f, g] and len(entries) == 4                                    # 8 members: the most
    with pytest.raises(ValueError, match="2 callables x 5 tta entries = 10 members, at most 8"):
        vp.ensemble_members([f, g], "default")
    with pytest.raises(ValueError, match="1 callables x 9 tta entries = 9 members, at most 8"):
        vp.ensemble_members(f, [{"rotate": float(k)} for k in range(9)])
    with pytest.raises(ValueError, match="empty list"):
        vp.ensemble_members([], None)


def test_segment_volume_refuses_bad_ensembles_before_any_device_work():
    """the members are validated before the device is looked at: device='cpu' would raise PnpError, a bad tta raises ValueError first"""
    vp, L = pkg("volume_predict"), pkg("_lib")
    image = np.zeros((8, 8, 4), np.int16)
    f = lambda x: x
    with pytest.raises(ValueError, match="unknown keys"):
        vp.segment_volume(f, image, tta=[{"shear": 1.0}], device="cpu")
    with pytest.raises(ValueError, match="at most 8"):
        vp.segment_volume([f, f], image, tta="default", device="cpu")
    with pytest.raises(L.PnpError, match="no CPU fallback"):
        vp.segment_volume(f, image, prob=True, device="cpu")


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path):
    nifti = pkg("nifti")
    img = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16)), img)
    models = []
    for name in ("m.npz", "m2.npz", "m3.npz"):
        np.savez(str(tmp_path / name), x=np.zeros(1))
        models.append(str(tmp_path / name))
    return img, models


def test_cli_ensemble_arguments(tmp_path):
    pr = pkg("predict")
    img, (m, m2, m3) = _files(tmp_path)
    base = ["--model", m, "--net", "segmenter", "--out", str(tmp_path / "o"), "--images", img]
    a, _, _, opt = pr.parse_args(base)
    assert opt == {"edge": "replicate", "axis": 2, "flip_correction": True, "batch_size": 16, "crop": None} and a.ensemble is None      # the default path
    a, _, _, opt = pr.parse_args(base + ["--tta", "default", "--prob", "--entropy"])
    assert opt["tta"] == [{}, {"rotate": 7.5}, {"rotate": -7.5}, {"scale": 0.95}, {"scale": 1.05}] and opt["prob"] is True and opt["entropy"] is True
    a, _, _, opt = pr.parse_args(base + ["--tta", '[{}, {"rotate": 7.5}, {"rotate": -7.5}, {"scale": 1.05}]', "--entropy", "--ensemble", m2])
    assert a.ensemble == [m2] and len(opt["tta"]) == 4 and "prob" not in opt                # 2 x 4 = 8 members: the most
    _, _, _, opt = pr.parse_args(base + ["--tta", json.dumps([{}, {"rotate": 4, "translate": [1, -1]}, {"flip": True}]), "--prob"])
    assert opt["tta"] == [{}, {"rotate": 4.0, "translate": (1.0, -1.0)}, {"flip": True}] and opt["prob"] is True and "entropy" not in opt
    a, _, _, opt = pr.parse_args(base + ["--ensemble", m2, m3])
    assert a.ensemble == [m2, m3] and "tta" not in opt and "prob" not in opt


def test_cli_ensemble_argument_errors(tmp_path):
    pr = pkg("predict")
    img, (m, m2, m3) = _files(tmp_path)
    base = ["--model", m, "--net", "segmenter", "--out", str(tmp_path / "o"), "--images", img]
    for extra in (["--tta", "best"],                                                    # neither `default` nor JSON
                  ["--tta", "{not json"],
                  ["--tta", "[]"],                                                      # no member
                  ["--tta", '{"rotate": 5}'],                                           # a dict, not a list
                  ["--tta", '[{"shear": 2}]'],                                          # unknown key
                  ["--tta", '[{"scale": 0}]'],
                  ["--tta", '[{"rotate": "x"}]'],
                  ["--tta", json.dumps([{"rotate": float(k)} for k in range(9)])],      # 9 members
                  ["--tta", "default", "--ensemble", m2],                               # 2 x 5 = 10 members
                  ["--ensemble", m2, m3, m2, m3, m2, m3, m2, m3],                       # 9 checkpoints
                  ["--ensemble", str(tmp_path / "missing.npz")],
                  ["--ensemble"],
                  ["--tta"]):
        with pytest.raises(SystemExit):
            pr.parse_args(base + extra)


# ---- the files ---------------------------------------------------------------------------------------------------------------------------
def test_written_probability_and_entropy_files(tmp_path, monkeypatch):
    """predict_volumes with the device part replaced: prob_ is float32 [*shape, ncls] with the class axis last, entropy_ float32 of the
    input's shape, both with the input's affine; a field that is None writes no file; a plain tensor (the default path) writes pred_ alone"""
    import torch
    vp, nifti = pkg("volume_predict"), pkg("nifti")
    aff = np.array([[0.0, -1.5, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, 3.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    rng = np.random.default_rng(0)
    img = tmp_path / "scan.nii.gz"
    nifti.save(nifti.Nifti1Image(rng.integers(-100, 900, (7, 5, 4)).astype(np.int16), aff), str(img))
    P = rng.random((3, 7, 5, 4)).astype(np.float32)
    Hn = rng.random((7, 5, 4)).astype(np.float32)
    seen = {}

    def fake(logits_fn, image, label=None, **kw):
        seen.update(kw)
        lab = torch.from_numpy((np.asarray(image) % 3).astype(np.uint8))
        if not kw.get("prob") and not kw.get("entropy") and kw.get("tta") is None:
            return lab
        return vp.Ensemble(lab, torch.from_numpy(P) if kw.get("prob") else None, torch.from_numpy(Hn) if kw.get("entropy") else None)
    monkeypatch.setattr(vp, "segment_volume", fake)
    out = tmp_path / "out"
    paths = vp.predict_volumes(None, [str(img)], str(out), num_cls=3, device="cpu", tta="default", prob=True, entropy=True)
    assert paths == [str(out / "pred_scan.nii.gz")] and seen["tta"] == "default" and seen["prob"] is True
    assert sorted(p.name for p in out.iterdir()) == ["entropy_scan.nii.gz", "pred_scan.nii.gz", "prob_scan.nii.gz"]
    pred, prob, ent = (nifti.load(str(out / (k + "_scan.nii.gz"))) for k in ("pred", "prob", "entropy"))
    assert pred.shape == (7, 5, 4) and pred.get_data().dtype == np.uint8 and np.allclose(pred.affine, aff)
    assert prob.shape == (7, 5, 4, 3) and prob.get_data().dtype == np.float32 and np.allclose(prob.affine, aff)
    assert np.array_equal(prob.get_data(), np.moveaxis(P, 0, -1))
    assert ent.shape == (7, 5, 4) and ent.get_data().dtype == np.float32 and np.allclose(ent.affine, aff) and np.array_equal(ent.get_data(), Hn)
    out2 = tmp_path / "out2"
    vp.predict_volumes(None, [str(img)], str(out2), num_cls=3, device="cpu", entropy=True)
    assert sorted(p.name for p in out2.iterdir()) == ["entropy_scan.nii.gz", "pred_scan.nii.gz"]
    out3 = tmp_path / "out3"
    vp.predict_volumes(None, [str(img)], str(out3), num_cls=3, device="cpu")
    assert sorted(p.name for p in out3.iterdir()) == ["pred_scan.nii.gz"]
