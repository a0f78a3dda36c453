"""-m gpu: multi-planar inference and training through the product (volume_predict.segment_volume(axes=), volume_source.VolumeSet(axis=
a sequence), predict --axes).

Inference: a (12, 10, 16) volume — three distinct extents — with a stub logits_fn; segment_volume(axes=(0, 1, 2)) against the three existing
single-axis calls fused by tests/fuse_ref.py under that file's bounds, with the double flip on and off and both edge modes; the millimetre
grid with anisotropic voxels (one field-of-view share per view), keep_largest on the fused label only, axes=(2,) bit for bit the
single-axis ensemble path, and with edge="skip" the frames one view skips labelled from the other views.
Training: VolumeSet(axis=(0, 1, 2)) of two NIfTI pairs holds the six entries of the three single-axis sets, pair-major, bit for bit; a
source on it serves all three orientations; a set built with axis=2 is the set the constructor built before it took a sequence.
The command line: predict --axes 0,1,2 writes the three files on the input's grid."""
import os

import numpy as np
import pytest
import torch

import fuse_ref as F
from conftest import pkg

pytestmark = pytest.mark.gpu

SHAPE = (12, 10, 16)
COMMON = dict(out_size=(10, 4), batch_size=3)


def _stub(ncls=5):
    """logits from the three channels and the pixel position: deterministic torch arithmetic, the same for equal inputs (the stub of
    tests/test_gpu_spacing.py)"""
    def fn(x):
        Bn, H, W, _ = x.shape
        i = torch.arange(H, device=x.device, dtype=torch.float32).view(1, H, 1)
        j = torch.arange(W, device=x.device, dtype=torch.float32).view(1, 1, W)
        out = torch.stack([x[..., 0] * (0.5 + c) - x[..., 1] * (0.3 * c) + x[..., 2] * 0.7 + torch.sin(0.4 * i * (c + 1) + 0.3 * j) for c in range(ncls)], dim=-1)
        return out.contiguous()
    return fn


def _scan(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (400 * np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + 0.5 * g[2] ** 2)) + 60 * rng.standard_normal(shape)).astype(np.int16)


def _views(dev, image, axes, **kw):
    vp = pkg("volume_predict")
    return [vp.segment_volume(_stub(), image, axis=a, prob=True, device=dev, **COMMON, **kw) for a in axes]


def _against_the_restatement(res, views, weights, what):
    M = len(views)
    probs = [v.prob.cpu().numpy() for v in views]
    ref = F.fuse(probs, weights)
    dp = F.delta_p(M)
    lab, P, H = res.label.cpu().numpy(), res.prob.cpu().numpy(), res.entropy.cpu().numpy()
    assert lab.shape == SHAPE and P.shape == (5,) + SHAPE and H.shape == SHAPE and lab.dtype == np.uint8
    unc = ~ref.covered
    assert not lab[unc].any() and not P[:, unc].any() and not H[unc].any()
    e1, e2 = float(np.abs(P - ref.prob).max()), float(np.abs(H - ref.entropy).max())
    adm = F.admissible(np.moveaxis(ref.prob, 0, -1), dp)
    ok = np.take_along_axis(adm, lab[..., None].astype(np.int64), axis=-1)[..., 0]
    multi = int(((adm.sum(-1) > 1) & ref.covered).sum())
    hb = F.entropy_bound(dp, 5)
    print("%s: max|dP| %.3g (bound %.3g), max|dH| %.3g (bound %.3g), %d labels differ from the float64 argmax, %d voxels admit more than one "
          "class, %d of %d covered" % (what, e1, dp, e2, hb, int((lab != ref.label).sum()), multi, int(ref.covered.sum()), lab.size))
    assert e1 <= dp and e2 <= hb and bool(ok[ref.covered].all()) and multi <= 2, what
    assert len(np.unique(lab)) > 1, "a constant prediction shows nothing"
    return ref


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("edge", ["replicate", "skip"])
def test_three_views_against_single_axis_calls_fused_by_the_restatement(dev, flip, edge):
    vp = pkg("volume_predict")
    image = _scan(SHAPE, 1)
    kw = dict(flip_correction=flip, edge=edge)
    views = _views(dev, image, (0, 1, 2), **kw)
    res = vp.segment_volume(_stub(), image, axes=(0, 1, 2), prob=True, entropy=True, device=dev, **COMMON, **kw)
    assert isinstance(res, vp.Ensemble)
    ref = _against_the_restatement(res, views, None, "flip %s, edge %s" % (flip, edge))
    if edge == "skip":
        # a view leaves the first and last frame along its own axis at 0; only a voxel on the border along ALL three axes has no view
        corners = np.zeros(SHAPE, bool)
        corners[np.ix_((0, -1), (0, -1), (0, -1))] = True
        assert np.array_equal(~ref.covered, corners)
        P2 = views[2].prob.cpu().numpy()
        assert not P2[:, :, :, 0].any() and not P2[:, :, :, -1].any()               # view 2 skipped these frames ...
        lab = res.label.cpu().numpy()
        assert lab[1:-1, 1:-1, 0].any() and lab[1:-1, 1:-1, -1].any()                # ... and they are labelled from views 0 and 1
        two = F.fuse([v.prob.cpu().numpy() for v in views[:2]], None)
        assert np.abs(res.prob.cpu().numpy()[:, :, :, 0] - two.prob[:, :, :, 0]).max() <= F.delta_p(2)
    else:
        assert ref.covered.all()
    # weights, a subset of the axes in another order, and only what was asked for
    w = (1.0, 1.0, 2.0)
    res_w = vp.segment_volume(_stub(), image, axes=(0, 1, 2), axis_weights=w, prob=True, entropy=True, device=dev, **COMMON, **kw)
    _against_the_restatement(res_w, views, w, "weights %r" % (w,))
    res_s = vp.segment_volume(_stub(), image, axes=[2, 0], device=dev, **COMMON, **kw)
    assert isinstance(res_s, vp.Ensemble) and res_s.prob is None and res_s.entropy is None
    sub = F.fuse([views[2].prob.cpu().numpy(), views[0].prob.cpu().numpy()], None)
    adm = F.admissible(np.moveaxis(sub.prob, 0, -1), F.delta_p(2))
    got = res_s.label.cpu().numpy()
    assert bool(np.take_along_axis(adm, got[..., None].astype(np.int64), axis=-1)[..., 0][sub.covered].all()) and not got[~sub.covered].any()


def test_explicit_box_and_margin(dev):
    """a box in the slicing order of axis 2, re-expressed per view: outside it all three outputs are 0, inside it the views' fusion"""
    vp = pkg("volume_predict")
    image = _scan(SHAPE, 2)
    box = ((2, 11), (1, 8), (3, 14))
    views = [vp.segment_volume(_stub(), image, axis=a, crop=vp.view_box(box, a), prob=True, device=dev, **COMMON) for a in (0, 1, 2)]
    res = vp.segment_volume(_stub(), image, axes=(0, 1, 2), crop=box, prob=True, entropy=True, device=dev, **COMMON)
    ref = _against_the_restatement(res, views, None, "explicit box")
    inside = np.zeros(SHAPE, bool)
    inside[tuple(slice(a, b) for a, b in box)] = True
    assert np.array_equal(ref.covered, np.flip(np.flip(inside, 0), 1))               # the box is in slicing order: after the double flip
    label = np.zeros(SHAPE, np.uint8)
    label[3:9, 2:7, 5:12] = 1
    views = [vp.segment_volume(_stub(), image, label=label, axis=a, crop=1, prob=True, device=dev, **COMMON) for a in (0, 1, 2)]
    res = vp.segment_volume(_stub(), image, label=label, axes=(0, 1, 2), crop=1, prob=True, entropy=True, device=dev, **COMMON)
    ref = _against_the_restatement(res, views, None, "margin")
    grown = np.zeros(SHAPE, bool)
    grown[2:10, 1:8, 4:13] = True
    assert np.array_equal(ref.covered, grown)


def test_millimetre_grid_with_anisotropic_voxels(dev):
    vp = pkg("volume_predict")
    image = _scan(SHAPE, 3)
    kw = dict(spacing=(0.8, 1.1, 0.6), sample_mm=1.0)
    singles, views = [], []
    for a in (0, 1, 2):
        st = []
        views.append(vp.segment_volume(_stub(), image, axis=a, prob=True, device=dev, fov_stats=st, **COMMON, **kw))
        singles += st
    stats = []
    res = vp.segment_volume(_stub(), image, axes=(0, 1, 2), prob=True, entropy=True, device=dev, fov_stats=stats, **COMMON, **kw)
    assert len(stats) == 3 and stats == singles and min(stats) < 1.0
    ref = _against_the_restatement(res, views, None, "sample_mm = 1.0, voxels of 0.8 x 1.1 x 0.6 mm")
    assert ref.covered.any() and not ref.covered.all()


def test_keep_largest_runs_once_on_the_fused_label(dev):
    vp, components = pkg("volume_predict"), pkg("components")
    image = _scan(SHAPE, 4)
    plain = vp.segment_volume(_stub(), image, axes=(0, 1, 2), prob=True, entropy=True, device=dev, **COMMON)
    cs = []
    kept = vp.segment_volume(_stub(), image, axes=(0, 1, 2), prob=True, entropy=True, keep_largest=1, component_stats=cs, device=dev, **COMMON)
    want, stats = components.keep_largest(plain.label.clone(), num_cls=5, keep=1)
    assert torch.equal(kept.label, want) and len(cs) == 1 and torch.equal(cs[0], stats)
    assert not torch.equal(kept.label, plain.label), "the filter removed nothing: the case shows nothing"
    assert torch.equal(kept.prob, plain.prob) and torch.equal(kept.entropy, plain.entropy)


@pytest.mark.parametrize("edge", ["replicate", "skip"])
def test_one_axis_is_the_single_axis_ensemble_path_bit_for_bit(dev, edge):
    vp = pkg("volume_predict")
    image = _scan(SHAPE, 5)
    want = vp.segment_volume(_stub(), image, axis=2, prob=True, entropy=True, edge=edge, device=dev, **COMMON)
    got = vp.segment_volume(_stub(), image, axes=(2,), prob=True, entropy=True, edge=edge, device=dev, **COMMON)
    assert torch.equal(got.label, want.label) and len(torch.unique(want.label)) > 1
    assert torch.equal(got.prob.view(torch.int32), want.prob.view(torch.int32))
    assert torch.equal(got.entropy.view(torch.int32), want.entropy.view(torch.int32))
    fused = vp.fuse_views([want], prob=True, entropy=True)                      # the public helper: the same launch on a finished prediction
    assert torch.equal(fused.label, want.label) and torch.equal(fused.prob.view(torch.int32), want.prob.view(torch.int32))
    assert torch.equal(fused.entropy.view(torch.int32), want.entropy.view(torch.int32))
    with pytest.raises(ValueError, match="no probabilities"):
        vp.fuse_views([vp.Ensemble(want.label, None, None)])
    with pytest.raises(ValueError, match="positive finite"):
        vp.fuse_views([want, want.prob.clone()], weights=(1.0, 0.0))


# ---- training --------------------------------------------------------------------------------------------------------------------------
def _pairs(tmp_path):
    nifti = pkg("nifti")
    pairs = []
    for n, (shape, vox) in enumerate((((9, 8, 7), (0.5, 0.7, 2.0)), ((6, 10, 8), (1.5, 0.9, 0.6)))):
        img = _scan(shape, 20 + n)
        lab = np.zeros(shape, np.int16)
        lab[1:-2, 2:-1, 1:-1] = 1 + n
        aff = np.diag(vox + (1.0,))
        fi, fl = str(tmp_path / ("s%d_image.nii.gz" % n)), str(tmp_path / ("s%d_label.nii.gz" % n))
        nifti.save(nifti.Nifti1Image(img, aff), fi)
        nifti.save(nifti.Nifti1Image(lab, aff), fl)
        pairs.append((fi, fl))
    return pairs


def test_volume_set_on_three_axes(dev, tmp_path):
    vs = pkg("volume_source")
    pairs = _pairs(tmp_path)
    multi = vs.VolumeSet(pairs, dev, axis=(0, 1, 2))
    singles = [vs.VolumeSet(pairs, dev, axis=a) for a in (0, 1, 2)]
    assert len(multi) == 6 and multi.axes == (0, 1, 2)
    assert multi.names == ["s0_image.nii.gz@0", "s0_image.nii.gz@1", "s0_image.nii.gz@2", "s1_image.nii.gz@0", "s1_image.nii.gz@1", "s1_image.nii.gz@2"]
    for p in range(2):
        for a in range(3):
            k, one = 3 * p + a, singles[a]
            assert multi.dims[k] == one.dims[p] and multi.spacings[k] == one.spacings[p]
            assert torch.equal(multi.images[k].view(torch.int32), one.images[p].view(torch.int32)) and torch.equal(multi.labels[k], one.labels[p])
    assert multi.dims[:3] == [(8, 7, 9), (9, 7, 8), (9, 8, 7)] and len(set(multi.spacings)) == 6
    assert np.allclose(multi.spacings[0], (0.7, 2.0, 0.5), rtol=1e-6) and np.allclose(multi.spacings[5], (1.5, 0.9, 0.6), rtol=1e-6)
    # a one-element sequence keeps the plain names
    assert vs.VolumeSet(pairs, dev, axis=(1,)).names == singles[1].names == ["s0_image.nii.gz", "s1_image.nii.gz"]
    for bad in ((), (0, 0), (0, 3)):
        with pytest.raises(ValueError, match="axes"):
            vs.VolumeSet(pairs, dev, axis=bad)
    # a source on it serves every orientation
    src = vs.AugmentedSliceSource(multi, 8, out_size=(16, 12), seed=3, num_cls=3)
    seen = set()
    for _ in range(4):
        x, onehot, fids = src.next_device_batch()
        assert tuple(x.shape) == (8, 16, 12, 3) and tuple(onehot.shape) == (8, 16, 12, 3) and bool(torch.isfinite(x).all())
        seen |= {f.split("#")[0] for f in fids}
        assert all(f.split("#")[0] in multi.names for f in fids)
    assert {n.split("@")[1] for n in seen} == {"0", "1", "2"} and {n.split("@")[0] for n in seen} == {"s0_image.nii.gz", "s1_image.nii.gz"}
    assert src.errors() == 0
    src.close()
    # sources_from_lists forwards the axes to both sets
    (tmp_path / "list").write_text("".join("%s %s\n" % p for p in pairs))
    tr, va = vs.sources_from_lists(str(tmp_path / "list"), str(tmp_path / "list"), dev, 4, 3, axes=(0, 2))
    assert tr.volumes.names == va.volumes.names == ["s0_image.nii.gz@0", "s0_image.nii.gz@2", "s1_image.nii.gz@0", "s1_image.nii.gz@2"]
    tr, va = vs.sources_from_lists(str(tmp_path / "list"), str(tmp_path / "list"), dev, 4, 3)
    assert tr.volumes.names == va.volumes.names == ["s0_image.nii.gz", "s1_image.nii.gz"]


def test_a_single_axis_set_is_what_it_was(dev, tmp_path):
    """axis=2 (and the default): the names, and for a seed the first batch, of a set assembled by hand the way the constructor did
    before it took a sequence — nifti.load, prepare_pair, upload and pnp_volume_preprocess through from_arrays, slicing_spacing"""
    vs, nifti = pkg("volume_source"), pkg("nifti")
    pairs = _pairs(tmp_path)
    arrays, spacings = [], []
    for fi, fl in pairs:
        image = nifti.load(fi)
        arrays.append(vs.prepare_pair(image.get_data(), nifti.load(fl).get_data(), True, 2, None))
        spacings.append(vs.slicing_spacing(image.affine, 2, fi))
    by_hand = vs.VolumeSet.from_arrays([a[0] for a in arrays], [a[1] for a in arrays], [os.path.basename(p[0]) for p in pairs], dev, spacings=spacings)
    for kw in ({}, {"axis": 2}, {"axis": np.int64(2)}):
        got = vs.VolumeSet(pairs, dev, **kw)
        assert got.names == by_hand.names == ["s0_image.nii.gz", "s1_image.nii.gz"] and got.dims == by_hand.dims
        assert got.spacings == by_hand.spacings
        a, b = (vs.AugmentedSliceSource(s, 6, out_size=(16, 12), seed=11, num_cls=3) for s in (got, by_hand))
        (xa, ha, fa), (xb, hb, fb) = a.next_device_batch(), b.next_device_batch()
        assert fa == fb and torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ha, hb)
        assert a.last_params.tobytes() == b.last_params.tobytes() and a.errors() == 0 and b.errors() == 0


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_predict_command_line(dev, tmp_path):
    ss, nifti, pr = pkg("source_segmenter"), pkg("nifti"), pkg("predict")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=2, device=dev, seed=0,
                      cost_kwargs={"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4})
    ck = net.save(str(tmp_path / "ckpt.npz"))
    ck = ck if isinstance(ck, str) and os.path.isfile(ck) else str(tmp_path / "ckpt.npz")
    aff = np.array([[0.0, -1.5, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, 3.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    shape = (7, 5, 6)
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(_scan(shape, 6), aff), a)
    base = ["--model", ck, "--net", "segmenter", "--images", a, "--batch-size", "2"]
    with pytest.raises(SystemExit):
        pr.main(base + ["--out", str(tmp_path / "refused"), "--axes", "0,1,2", "--axis", "0"])
    assert not os.path.exists(str(tmp_path / "refused"))
    out = str(tmp_path / "out")
    res = pr.main(base + ["--out", out, "--axes", "0,1,2", "--axis-weights", "1,1,2", "--prob", "--entropy"])
    assert res["paths"] == [os.path.join(out, "pred_a.nii.gz")]
    assert sorted(os.listdir(out)) == ["entropy_a.nii.gz", "pred_a.nii.gz", "prob_a.nii.gz"]
    pred, prob, ent = (nifti.load(os.path.join(out, k + "_a.nii.gz")) for k in ("pred", "prob", "entropy"))
    assert pred.shape == shape and pred.get_data().dtype == np.uint8 and np.allclose(pred.affine, aff) and pred.get_data().max() < 5
    assert prob.shape == shape + (5,) and prob.get_data().dtype == np.float32 and np.allclose(prob.affine, aff)
    assert ent.shape == shape and ent.get_data().dtype == np.float32 and np.allclose(ent.affine, aff)
    P, H = prob.get_data(), ent.get_data()
    assert np.abs(P.sum(-1) - 1).max() <= 5 * 2.0 ** -23 + 5 * F.delta_p(3) and H.min() >= 0 and H.max() <= 1 + 1e-6
    top = np.sort(P, -1)
    clear = top[..., -1] - top[..., -2] > 1e-6                     # the file's label is the argmax of the file's probabilities
    assert np.array_equal(np.argmax(P, -1)[clear], pred.get_data()[clear])
    out2 = str(tmp_path / "plain")                                  # and the default command line still writes the label file alone
    pr.main(base + ["--out", out2])
    assert os.listdir(out2) == ["pred_a.nii.gz"]
