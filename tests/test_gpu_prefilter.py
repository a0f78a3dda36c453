"""-m gpu: the anti-alias prefilter — pnp_volume_smooth against the float64 restatement of tests/prefilter_ref.py, then
VolumeSet.apply_prefilter, the training and the prediction path and the command lines.

Bounds (derived, not tuned):
  kernel     prefilter_ref.bound: (n_x + n_y + n_z + 6) 2^-24 max|v|, n_a = 2 R_a + 1 over the filtered axes — every pass is one fmaf chain of
             n_a non-negative weights that sum to 1 (one rounding of at most 2^-24 max|v| per tap), the restatement uses the same float32
             weights.  No voxel excluded.
  whole path the gather's own image bound (spacing_ref.image_bound, §17), evaluated on the smoothed volume, plus the kernel bound: the
             gather is Lipschitz 1 in the voxel values (bilinear weights sum to 1).
"""
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import prefilter_ref as R
import spacing_ref as S
from conftest import pkg

pytestmark = pytest.mark.gpu

SHAPES = [(13, 11, 7), (9, 17, 5), (6, 5, 1), (70, 3, 33), (130, 67, 70)]
SIGMAS = [(0.3, 1.0, 2.2), (8, 0, 0.93), (2.2, 2.2, 8), (0, 0, 1), (1, 0, 0)]


def _weights(sigmas):
    vs = pkg("volume_source")
    return [vs.gaussian_weights(s) for s in sigmas]


def _volume(shape, kind):
    rng = np.random.default_rng(sum(shape) + 7 * len(kind))
    if kind == "spike":
        v = rng.standard_normal(shape).astype(np.float32)
        v[tuple(n // 2 for n in shape)] = 1e4
        return v
    return (rng.standard_normal(shape) * 3).astype(np.float32)


_REFS = {}


def _ref(shape, kind, sigmas):
    """computed once per case, shared, never changed"""
    key = (shape, kind, sigmas)
    if key not in _REFS:
        ref = R.smooth(_volume(shape, kind), sigmas)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["normal", "spike"])
def test_kernel_against_the_restatement(dev, shape, kind):
    """largest measured share of the bound: DESIGN.md §19"""
    K = pkg("kernels")
    v = _volume(shape, kind)
    vd = torch.from_numpy(v).to(dev)
    top = float(np.abs(v).max())
    worst = 0.0
    for sigmas in SIGMAS:
        got = K.volume_smooth(vd, _weights(sigmas))
        assert got.shape == vd.shape and got.data_ptr() != vd.data_ptr()
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - _ref(shape, kind, sigmas)).max())
        bound = R.bound(sigmas, top)
        print("pnp_volume_smooth %s %s sigma %s: error / bound %.4f" % (shape, kind, sigmas, err / bound))
        worst = max(worst, err / bound)
        assert err <= bound, (shape, kind, sigmas, err, bound)
        assert torch.equal(vd.cpu(), torch.from_numpy(v))                        # src is unchanged by the out-of-place call
    print("pnp_volume_smooth %s %s: worst error / bound %.4f" % (shape, kind, worst))


# ---- 2. in place, run to run, all radii 0 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_in_place_and_rerun_are_bitwise_the_out_of_place_result(dev, shape):
    K = pkg("kernels")
    v = torch.from_numpy(_volume(shape, "normal")).to(dev)
    for sigmas in SIGMAS + [(1, 1, 0), (0, 2.2, 0)]:
        w = _weights(sigmas)
        keep = v.clone()
        a = K.volume_smooth(v, w)
        assert torch.equal(v.view(torch.int32), keep.view(torch.int32))
        b = K.volume_smooth(v, w)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), sigmas     # run to run
        c = v.clone()
        assert K.volume_smooth(c, w, out=c) is c
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), sigmas     # in place
        assert not torch.equal(a, v)


def test_all_radii_zero(dev):
    K = pkg("kernels")
    v = torch.from_numpy(_volume((13, 11, 7), "normal")).to(dev)
    v.view(-1)[5] = float("nan")                                                 # a copy keeps every bit pattern
    keep = v.clone()
    for w in ([None, None, None], _weights((0.1, 0.0, 0.12))):
        assert all(t is None for t in w)
        out = K.volume_smooth(v, w)
        assert out.data_ptr() != v.data_ptr() and torch.equal(out.view(torch.int32), keep.view(torch.int32))
        assert K.volume_smooth(v, w, out=v) is v and torch.equal(v.view(torch.int32), keep.view(torch.int32))


def test_wrapper_refuses_what_is_not_a_volume(dev):
    K, L = pkg("kernels"), pkg("_lib")
    v = torch.zeros((4, 4, 4), device=dev)
    w = np.array([0.25, 0.5, 0.25], np.float32)
    for args in ((v[0], [w, None, None]), (v, [w, None]), (v, [w[:2], None, None]), (v.cpu(), [w, None, None]), (v.double(), [w, None, None])):
        with pytest.raises(L.PnpError):
            K.volume_smooth(*args)
    with pytest.raises(L.PnpError, match="not finite"):
        K.volume_smooth(v, [np.array([0.25, np.inf, 0.25], np.float32), None, None])
    with pytest.raises(L.PnpError, match="partially"):
        flat = torch.zeros(128, device=dev)
        K.volume_smooth(flat[:64].view(4, 4, 4), [w, None, None], out=flat[32:96].view(4, 4, 4))


# ---- 3. a linear field -------------------------------------------------------------------------------------------------------------------
def test_linear_field_is_preserved_away_from_the_borders(dev):
    """a symmetric kernel whose weights sum to 1 preserves f = a x + b y + c z + d wherever no tap is clamped: the kernel bound holds
    against f itself (the float32 weights are exactly symmetric, so the first moment is exactly 0; their sums miss 1 by 4e-9 .. 2e-8,
    well inside the bound's 6 units of slack: 0.02 of the bound in float64)."""
    K = pkg("kernels")
    shape, sigmas = (40, 36, 30), (2.2, 1, 0.5)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    f = (0.8 * g[0] - 0.5 * g[1] + 0.3 * g[2] + 20).astype(np.float32)
    got = K.volume_smooth(torch.from_numpy(f).to(dev), _weights(sigmas)).cpu().numpy().astype(np.float64)
    Rs = [R.radius(s) for s in sigmas]
    assert Rs == [9, 4, 2]
    inner = tuple(slice(r, n - r) for r, n in zip(Rs, shape))
    top = float(np.abs(f).max())
    bound = R.bound(sigmas, top)
    err = float(np.abs(got - f.astype(np.float64))[inner].max())
    print("linear field: error / bound %.3f" % (err / bound))
    assert err <= bound and got[inner].size > 5000
    assert np.abs(got - f)[0].max() > 100 * bound                                # at the border the clamp does change it: the slice matters


# ---- 4. VolumeSet.apply_prefilter ------------------------------------------------------------------------------------------------------------
def _small_set(dev, spacings=None):
    vs = pkg("volume_source")
    rng = np.random.default_rng(23)
    shapes = [(13, 11, 7), (9, 17, 5)]
    host = [((rng.standard_normal(s) * 2).astype(np.float32), rng.integers(0, 5, s).astype(np.uint8)) for s in shapes]
    vset = vs.VolumeSet.from_device([torch.from_numpy(v).to(dev) for v, _ in host], [torch.from_numpy(l).to(dev) for _, l in host],
                                    ["a", "b"], [-1.5, 0.25], spacings=spacings)
    return vset, host


def test_apply_prefilter(dev):
    vs = pkg("volume_source")
    vset, host = _small_set(dev)
    assert vset.sigmas == [None, None]
    vset.set_fill(-9.0)
    stats = [dict(s) for s in vset.stats]
    sig = [(1.0, 0.0, 0.5), (0.0, 2.2, 0.0)]
    vset.apply_prefilter(sig)
    assert vset.sigmas == sig
    for n, (v, lab) in enumerate(host):
        assert torch.equal(vset.labels[n].cpu(), torch.from_numpy(lab))
        err = float(np.abs(vset.images[n].cpu().numpy() - R.smooth(v, sig[n])).max())
        assert 0 < err <= R.bound(sig[n], np.abs(v).max())
        assert vset._table_host_np["image"][n] == vset.images[n].data_ptr() and vset._table_host_np["fill"][n] == np.float32(-9.0)
    assert vset.stats == stats
    ptrs, imgs = [v.data_ptr() for v in vset.images], [v.clone() for v in vset.images]
    vset.apply_prefilter([tuple(s) for s in sig])                                # the same values: nothing happens
    assert [v.data_ptr() for v in vset.images] == ptrs and all(torch.equal(a, b) for a, b in zip(vset.images, imgs))
    with pytest.raises(ValueError, match="twice"):
        vset.apply_prefilter([(1.0, 0.0, 0.5), (0.0, 2.0, 0.0)])
    with pytest.raises(ValueError, match="2 volumes"):
        vset.apply_prefilter(sig[:1])
    assert all(torch.equal(a, b) for a, b in zip(vset.images, imgs))
    assert not any(k[1] == "smooth" for k in pkg("kernels")._ws_cache)           # the scratch volume was given back


def test_sigmas_below_the_threshold_change_nothing(dev):
    vs = pkg("volume_source")
    plain, _ = _small_set(dev)
    vset, host = _small_set(dev)
    vset.apply_prefilter([(0.1, 0.12, 0.0), (0.0, 0.0, 0.124)])
    assert vset.sigmas == [(0.1, 0.12, 0.0), (0.0, 0.0, 0.124)]
    for n, (v, _) in enumerate(host):
        assert torch.equal(vset.images[n].cpu().view(torch.int32), torch.from_numpy(v).view(torch.int32))
    rec = np.zeros(4, dtype=vs.SAMPLE_DTYPE)
    rec["volume"], rec["frame"] = [0, 1, 0, 1], [1, 3, 5, 2]
    for b in range(4):
        rec["m"][b] = vs.compose_matrix(vset.dims[rec["volume"][b]][:2], (16, 12), rotate=20.0 * b, scale=1.1)
    a = vs.AugmentedSliceSource(plain, 4, out_size=(16, 12), augment=None).gather_records(rec, 5, True)
    b = vs.AugmentedSliceSource(vset, 4, out_size=(16, 12), augment=None).gather_records(rec, 5, True)
    for got, want in zip(b, a):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # a source built without the option leaves a set alone
    src = vs.AugmentedSliceSource(plain, 4, out_size=(4, 4), augment=None, prefilter=None)
    assert src.prefilter is None and plain.sigmas == [None, None]
    assert vs.AugmentedSliceSource(plain, 4, out_size=(4, 4), augment=None, prefilter="off").prefilter is None and plain.sigmas == [None, None]


def test_source_computes_the_sigmas_per_volume(dev):
    vs = pkg("volume_source")
    vset, host = _small_set(dev, spacings=[(0.35, 0.35, 0.6), (1.0, 0.5, 1.6)])
    src = vs.AugmentedSliceSource(vset, 2, out_size=(8, 8), augment=None, sample_mm=(1.0, 1.0, 2.5), prefilter="auto")
    want = [R.auto_sigmas(d, (8, 8), sp, (1.0, 1.0, 2.5)) for d, sp in zip(vset.dims, vset.spacings)]
    assert src.prefilter == "auto" and vset.sigmas == want and want[1][0] == 0.0 and want[1][1] == 0.5
    for n, (v, _) in enumerate(host):
        assert np.abs(vset.images[n].cpu().numpy() - R.smooth(v, want[n])).max() <= R.bound(want[n], np.abs(v).max())
    # without sample_mm: the resize's rule, (X / H, Y / W, 1)
    vset2, host2 = _small_set(dev)
    vs.AugmentedSliceSource(vset2, 2, out_size=(4, 8), augment=None, prefilter="auto")
    assert vset2.sigmas == [((13 / 4 - 1) / 2, (11 / 8 - 1) / 2, 0.0), ((9 / 4 - 1) / 2, (17 / 8 - 1) / 2, 0.0)]
    # a second source on the same set with other sigmas would filter it twice
    with pytest.raises(ValueError, match="twice"):
        vs.AugmentedSliceSource(vset2, 2, out_size=(8, 8), augment=None, prefilter="auto")


# ---- 5. the whole path, training side ----------------------------------------------------------------------------------------------------
def test_stripes_through_the_training_source(dev):
    """the stripe volume of tests/test_prefilter_host.py (a cosine of period 1.0 mm on voxels of 0.35 mm under pixels of 1 mm): the batch
    of the source without the option shows the stripes at full amplitude, the batch of the source with prefilter="auto" is the
    restatement's — the float64 gather of the float64-smoothed volume — and small"""
    vs = pkg("volume_source")
    vol = R.stripes()
    rng = np.random.default_rng(4)
    lab = rng.integers(0, 5, R.STRIPE_SHAPE).astype(np.uint8)
    sp = (R.STRIPE_MM,) * 3

    def source(prefilter):
        vset = vs.VolumeSet.from_device([torch.from_numpy(vol).to(dev)], [torch.from_numpy(lab).to(dev)], ["stripes"], [0.0], spacings=[sp])
        return vs.AugmentedSliceSource(vset, 2, out_size=R.STRIPE_OUT, augment=None, sample_mm=R.STRIPE_SAMPLE_MM, prefilter=prefilter)
    rec = np.zeros(2, dtype=vs.SAMPLE_Z_DTYPE)
    rec["frame"], rec["dz"] = [2, 4], np.float32(R.STRIPE_SAMPLE_MM[2] / sp[2])
    rec["m"][:] = R.stripe_map(vs.compose_matrix)
    plain, filt = source(None), source("auto")
    sig = R.auto_sigmas(R.STRIPE_SHAPE, R.STRIPE_OUT, sp, R.STRIPE_SAMPLE_MM)
    assert filt.volumes.sigmas == [sig] and plain.volumes.sigmas == [None]
    xa, la, oa = plain.gather_records(rec, 5, True)
    xb, lb, ob = filt.gather_records(rec, 5, True)
    assert plain.errors() == 0 and filt.errors() == 0
    assert float(xa.abs().max()) >= 0.9
    smooth = R.smooth(vol, sig)
    sx, sy = A.coords(rec["m"][0], *R.STRIPE_OUT)
    bound = S.image_bound(smooth, 0.0, rec["m"], *R.STRIPE_OUT) + R.bound(sig, 1.0)
    xg = xb.cpu().numpy().astype(np.float64)
    for b in range(2):
        ref = S.gather_image_z(smooth, int(rec["frame"][b]), rec["dz"][b], sx, sy, 0.0)
        err = float(np.abs(xg[b] - ref).max())
        print("stripes, filtered batch %d: error %.3e, bound %.3e, max|x| %.4f" % (b, err, bound, np.abs(xg[b]).max()))
        assert err <= bound
    assert float(np.abs(xg).max()) <= 0.2
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(oa.view(torch.int32), ob.view(torch.int32))
    assert len(torch.unique(la)) == 5


# ---- 6. the whole path, prediction side ----------------------------------------------------------------------------------------------------
def _capturing_stub(seen, ncls=5):
    def fn(x):
        seen.append(x.detach().clone())
        Bn, H, W, _ = x.shape
        i = torch.arange(H, device=x.device, dtype=torch.float32).view(1, H, 1)
        j = torch.arange(W, device=x.device, dtype=torch.float32).view(1, 1, W)
        return torch.stack([x[..., 0] * (0.5 + c) - x[..., 1] * (0.3 * c) + x[..., 2] * 0.7 + torch.sin(0.4 * i * (c + 1) + 0.3 * j) for c in range(ncls)],
                           dim=-1).contiguous()
    return fn


def _scan(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (400 * np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + 0.5 * g[2] ** 2)) + 60 * rng.standard_normal(shape)).astype(np.int16)


@pytest.mark.parametrize("edge", ["replicate", "skip"])
def test_without_the_option_the_prediction_is_todays_bit_for_bit(dev, edge):
    vp = pkg("volume_predict")
    image = _scan((16, 12, 6), 1)
    for extra in ({}, {"spacing": (0.5, 0.5, 1.0), "sample_mm": 1.0}):
        common = dict(edge=edge, batch_size=4, out_size=(8, 6), device=dev, **extra)
        seen = [[], [], [], []]
        want = vp.segment_volume(_capturing_stub(seen[0]), image, **common)
        for n, pre in enumerate((None, (0, 0, 0), "off"), 1):
            got = vp.segment_volume(_capturing_stub(seen[n]), image, prefilter=pre, **common)
            assert torch.equal(got, want) and len(seen[n]) == len(seen[0])
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(seen[n], seen[0]))
        assert len(torch.unique(want)) > 1
        seen_f = []
        vp.segment_volume(_capturing_stub(seen_f), image, prefilter="auto", **common)          # 2 voxels per pixel: sigma 0.5 in the plane
        assert not torch.equal(seen_f[0], seen[0][0])


@pytest.mark.parametrize("with_mm", [True, False])
def test_prediction_reads_the_smoothed_volume(dev, with_mm):
    """edge="replicate", flip_correction off so that the slicing order is the array order.  The slices the stub receives equal the float64
    gather of the float64-smoothed, normalised box.  Without sample_mm the default path pads the volume with copies of its edge frames
    AFTER smoothing: frames -1 and Z of the restatement are copies of the smoothed frames 0 and Z - 1."""
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    image = _scan((40, 24, 5), 3).astype(np.float32)
    X, Y, Z = image.shape
    H, W, B = 14, 12, 4
    spacing = (0.35, 0.5, 1.0)
    opts = dict(spacing=spacing, sample_mm=(1.0, 1.0, 1.5)) if with_mm else {}
    seen = []
    vp.segment_volume(_capturing_stub(seen), image, flip_correction=False, edge="replicate", batch_size=B, out_size=(H, W), device=dev,
                      prefilter="auto", **opts)
    got = torch.cat(seen)[:Z].cpu().numpy().astype(np.float64)
    norm, _ = A.preprocess(image)
    fill = float(norm.min())
    sig = R.auto_sigmas((X, Y, Z), (H, W), spacing, (1.0, 1.0, 1.5)) if with_mm else R.auto_sigmas((X, Y, Z), (H, W))
    assert R.radius(sig[0]) > 0 and (R.radius(sig[2]) > 0) == with_mm
    smooth = R.smooth(norm.astype(np.float32), sig)
    if with_mm:
        m = vs.compose_matrix((X, Y), (H, W), spacing_xy=spacing[:2], pixel_mm=(1.0, 1.0))
        dz, vol, shift = np.float32(1.5 / spacing[2]), smooth, 0
    else:
        m = vs.compose_matrix((X, Y), (H, W))
        dz, vol, shift = np.float32(1.0), np.concatenate([smooth[:, :, :1], smooth, smooth[:, :, -1:]], axis=2), 1
    # the map, the frame step, the frames and the padding stated here by hand are the ones of the plan that ran
    plan = vp.plan_view(vp.parse_request(flip_correction=False, batch_size=B, out_size=(H, W), prefilter="auto", **opts), image.shape, 2,
                        ((0, X), (0, Y), (0, Z)), opts.get("spacing"))
    assert len(plan.maps) == 1 and np.array_equal(plan.maps[0], m) and plan.padded == (not with_mm) and plan.frames == (shift, Z, -shift)
    assert (plan.dz == dz if with_mm else plan.dz is None) and (plan.taps[2] is not None) == with_mm and plan.taps[0] is not None
    sx, sy = A.coords(m, H, W)
    top = float(np.abs(norm).max())
    # the normalised volume itself is the device's float32 (§13: 4 u max|v| against the float64 restatement); smoothing and gather are Lipschitz 1
    bound = S.image_bound(vol, fill, m[None], H, W) + R.bound(sig, top) + 4 * R.U * top
    worst = 0.0
    for z in range(Z):
        ref = S.gather_image_z(vol, z + shift, dz, sx, sy, fill)
        worst = max(worst, float(np.abs(got[z] - ref).max()))
    print("segment_volume prefilter=auto, sample_mm %s: error %.3e, bound %.3e" % (with_mm, worst, bound))
    assert worst <= bound
    # and it is not the unsmoothed volume that was read
    raw = norm if with_mm else np.concatenate([norm[:, :, :1], norm, norm[:, :, -1:]], axis=2)
    assert np.abs(got[0] - S.gather_image_z(raw, shift, dz, sx, sy, fill)).max() > 100 * bound


# ---- 7. end to end through the command lines -------------------------------------------------------------------------------------------------
def test_command_lines(dev, tmp_path):
    ts, pr, nifti = pkg("train_segmenter"), pkg("predict"), pkg("nifti")
    aff = np.diag([0.6, 0.9, 2.0, 1.0])
    lines = []
    for n in range(2):
        img = _scan((48, 40, 5), 10 + n)
        lab = np.zeros(img.shape, np.int16)
        lab[10:30, 8:28, 1:4] = 1 + n
        nifti.save(nifti.Nifti1Image(img, aff), str(tmp_path / ("s%d_image.nii.gz" % n)))
        nifti.save(nifti.Nifti1Image(lab, aff), str(tmp_path / ("s%d_label.nii.gz" % n)))
        lines.append("s%d_image.nii.gz s%d_label.nii.gz" % (n, n))
    (tmp_path / "train_list").write_text("\n".join(lines) + "\n")
    (tmp_path / "val_list").write_text(lines[1] + "\n")
    out = str(tmp_path / "seg")
    tr = ts.main(["--nii-train", str(tmp_path / "train_list"), "--nii-val", str(tmp_path / "val_list"), "--sample-mm", "1.0", "--prefilter", "auto",
                  "--batch-size", "2", "--iters", "2", "--epochs", "1", "--output", out])
    want = ((1.0 / 0.6 - 1) / 2, (1.0 / 0.9 - 1) / 2, 0.0)
    assert tr.train_list.prefilter == "auto" == tr.val_list.prefilter
    for src, n in ((tr.train_list, 2), (tr.val_list, 1)):
        assert len(src.volumes.sigmas) == n and all(np.allclose(s, want, rtol=1e-6, atol=0) for s in src.volumes.sigmas)
    assert tr.train_list.errors() == 0 and tr.val_list.errors() == 0 and np.isfinite(tr.loss_dict["train"][1])
    ckpt = os.path.join(out, "checkpoint.npz")
    assert os.path.exists(ckpt)
    image = str(tmp_path / "s0_image.nii.gz")
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", image, "--out", str(tmp_path / "pred"), "--batch-size", "2", "--sample-mm", "1.0",
                   "--prefilter", "auto"])
    got, src = nifti.load(res["paths"][0]), nifti.load(image)
    assert res["paths"] == [str(tmp_path / "pred" / "pred_s0_image.nii.gz")]
    assert got.shape == src.shape == (48, 40, 5) and got.get_data().dtype == np.uint8 and np.allclose(got.affine, aff) and got.get_data().max() < 5
