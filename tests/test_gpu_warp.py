"""-m gpu: pnp_aug_slices_warp against the float64 restatement of tests/warp_ref.py, then the feature through the product.

Bounds (derived, not tuned; u = 2^-24):
  image     (eps_affine + eps_warp)(Gx + Gy) + 4 u max|v|: §13's bound with the coordinate error of the displacement added.
            eps_affine = augment_ref.coord_eps; eps_warp = c u max|P| plus one float32 ulp at the coordinate, c = 26 + 6.1 G:
              6.1 G  the rounding of t: rh = fl(G / H) and g = fl((i + 0.5) rh) round once each, |dg| <= 2.01 u G, the spline's slope in g is
                     at most 1.5 max|P| (sum_a |B'_a| <= 1.5, held in test_warp_host.py), two axes;
              18     the polynomial weights: sum_a |dB_a| <= 9 u per axis (B0: 7/6, B3: 4/6, B1: 3.5, B2: 3.2), weights of the other axis sum to 1;
              8      the 16 products: two fmaf chains of four terms with non-negative weights summing to 1, 4 u max|P| each.
            (Operation by operation at warp_ref.warp_c.)  The same tables and volumes on every device give the same bound.
  label     no pixel excluded: one of the labels at floor(s + 0.5) for s -+ (eps_affine + eps_warp) on either axis, s the displaced coordinate.
  gain/bias 1 float32 ulp of fl32(gain base + bias) (the kernel's fmaf rounds once: it is expected to be exact).
  noise     c' u sigma with c' = 184 when the value without noise is 0 (gain = bias = 0), from |n| <= sqrt(48 ln 2) = 5.77, the rounding of
            2 pi u2 and 3 / 3 / 4 ulp for logf / sqrtf / cosf (warp_ref.NOISE_C: OpenCL's full-profile limits; the device library's own
            figures are not documented on the build machine, so the measured error is printed and recorded in DESIGN.md §18).  On top of
            another value the final fmaf also rounds at |out|: half an ulp there is added, nothing else.
"""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
import warp_ref as Wr
from conftest import pkg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(37, 29, 5), (64, 80, 3), (9, 261, 6)]


def _blob_volume(rng, shape, ncls_max=5):
    """test_gpu_augment.py's: smooth blobs of labels 1 .. ncls_max-1 on a noisy background; intensities depend on the label"""
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
    vs = pkg("volume_source")
    rng = np.random.default_rng(11)
    pairs = [_blob_volume(rng, s, 8 if i == 2 else 5) for i, s in enumerate(SHAPES)]
    vset = vs.VolumeSet.from_arrays([p[0] for p in pairs], [p[1] for p in pairs], ["v%d.nii.gz" % i for i in range(3)], dev)
    host = [(v.cpu().numpy(), l.cpu().numpy()) for v, l in zip(vset.images, vset.labels)]
    gaps = [R.adjacent_gap(v, np.float64(np.float32(st["fill"]))) for (v, _), st in zip(host, vset.stats)]      # computed once, shared
    return vset, host, gaps


@pytest.fixture()
def errors(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _records(vs, rng, B, out_hw, frames="inner", dz=1.0, volumes=None):
    """B records with rotation, scale, translation and flip in the map; identity intensity, warp = 0"""
    rec = np.zeros(B, dtype=vs.SAMPLE_W_DTYPE)
    for b in range(B):
        v = int(rng.integers(0, 3)) if volumes is None else volumes[b % len(volumes)]
        X, Y, Z = SHAPES[v]
        rec["volume"][b] = v
        rec["frame"][b] = int(rng.integers(1, Z - 1)) if frames == "inner" else int(rng.integers(0, Z))
        rec["dz"][b] = dz if np.isscalar(dz) else dz[b % len(dz)]
        rec["m"][b] = vs.compose_matrix((X, Y), out_hw, rotate=rng.uniform(-40, 40), scale=np.exp(rng.uniform(-0.3, 0.3)),
                                        translate=tuple(rng.uniform(-3, 3, 2)), flip=bool(rng.integers(2)))
    rec["gain"] = 1.0
    return rec


def _table(rng, B, G, sigma=2.0):
    return np.clip(rng.standard_normal((B, G + 3, G + 3, 2)) * sigma, -3 * sigma, 3 * sigma).astype(np.float32)


def _warp(dev, vset, rec, ctrl, out_hw, errors, ncls=5, want_onehot=True):
    K = pkg("kernels")
    sd = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    cd = None if ctrl is None else torch.from_numpy(np.ascontiguousarray(ctrl, dtype=np.float32)).to(dev)
    G = 0 if ctrl is None else ctrl.shape[1] - 3
    return K.aug_slices_warp(vset.table_host, vset.table_dev, len(vset), sd, cd, G, len(rec), out_hw[0], out_hw[1], errors, ncls=ncls,
                             want_onehot=want_onehot)


def _narrow(vs, rec, dtype):
    out = np.zeros(len(rec), dtype=dtype)
    for f in dtype.names:
        out[f] = rec[f]
    return out


def _bits(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


def _reference(small_set, rec, ctrl, out_hw, b):
    """(float64 image [H, W, 3] before the intensity map, image bound, displaced coordinates, eps) of sample b (dz = 1, inner frame)"""
    vset, host, gaps = small_set
    H, W = out_hw
    v, z = int(rec["volume"][b]), int(rec["frame"][b])
    assert rec["dz"][b] == 1.0 and 1 <= z <= SHAPES[v][2] - 2
    vol, _ = host[v]
    fill = np.float64(np.float32(vset.stats[v]["fill"]))
    table = ctrl[b] if (ctrl is not None and rec["warp"][b]) else None
    sx, sy = Wr.coords(rec["m"][b], table, H, W)
    eps = R.coord_eps(rec["m"], H, W)
    if table is not None:
        eps += Wr.warp_eps(table, max(float(np.abs(sx).max()), float(np.abs(sy).max())))
    Gx, Gy = gaps[v]
    bound = eps * (Gx + Gy) + 4 * U * max(float(np.abs(vol).max()), abs(fill))
    return R.gather_image(vol, z, sx, sy, fill), bound, (sx, sy), eps


def _check_batch(small_set, rec, ctrl, out_hw, x, label, onehot, ncls, skip=None):
    """image within the bound, label among the candidates, one-hot = label_decomp; skip: [B, H, W] bool of pixels judged elsewhere"""
    K = pkg("kernels")
    vset, host, _ = small_set
    xg, lg = x.cpu().numpy(), label.cpu().numpy()
    worst = 0.0
    for b in range(len(rec)):
        ref, bound, (sx, sy), eps = _reference(small_set, rec, ctrl, out_hw, b)
        keep = np.ones(out_hw, dtype=bool) if skip is None else ~skip[b]
        err = float(np.abs(xg[b] - ref)[keep].max()) if keep.any() else 0.0
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
        cand = R.label_candidates(host[int(rec["volume"][b])][1], int(rec["frame"][b]), sx, sy, eps)
        hit = (lg[b][None] == cand).any(axis=0)
        assert np.all(hit[keep]), (b, int((~hit[keep]).sum()))
    if onehot is not None:
        assert torch.equal(onehot, K.label_decomp(label, ncls))
        assert np.array_equal(onehot.cpu().numpy(), R.onehot(lg, ncls))
    return worst


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_hw,B", [((32, 48), 6), ((17, 23), 3), ((1, 1), 1)])
def test_identity_records_are_the_affine_gathers_bit_for_bit(dev, small_set, errors, out_hw, B):
    vs, K = pkg("volume_source"), pkg("kernels")
    vset = small_set[0]
    rng = np.random.default_rng(B)
    up = lambda r: torch.from_numpy(r.view(np.uint8).copy()).to(dev)
    # any frame, fractional steps: pnp_aug_slices_z
    rec = _records(vs, rng, B, out_hw, frames="any", dz=[0.37, 1.0, 2.5])
    want = K.aug_slices_z(vset.table_host, vset.table_dev, 3, up(_narrow(vs, rec, vs.SAMPLE_Z_DTYPE)), B, out_hw[0], out_hw[1], errors, ncls=5)
    assert _bits(_warp(dev, vset, rec, None, out_hw, errors), want)
    assert _bits(_warp(dev, vset, rec, _table(rng, B, 4), out_hw, errors), want)          # the warp instance with warp = 0 in every record
    x, label, none = _warp(dev, vset, rec, None, out_hw, errors, want_onehot=False)
    assert none is None and _bits((x, label), want[:2])
    # dz = 1 on inner frames: pnp_aug_slices
    rec = _records(vs, rng, B, out_hw)
    want = K.aug_slices(vset.table_host, vset.table_dev, 3, up(_narrow(vs, rec, vs.SAMPLE_DTYPE)), B, out_hw[0], out_hw[1], errors, ncls=5)
    assert _bits(_warp(dev, vset, rec, None, out_hw, errors), want) and _bits(_warp(dev, vset, rec, _table(rng, B, 16), out_hw, errors), want)
    assert int(errors.item()) == 0


# ---- 2. zero and constant tables ---------------------------------------------------------------------------------------------------------
def test_zero_and_constant_control_tables(dev, small_set, errors):
    vs = pkg("volume_source")
    vset = small_set[0]
    out_hw, B, G = (17, 23), 3, 4
    rng = np.random.default_rng(2)
    rec = _records(vs, rng, B, out_hw)
    plain = _warp(dev, vset, rec, None, out_hw, errors)
    rec["warp"] = 1
    assert _bits(_warp(dev, vset, rec, np.zeros((B, G + 3, G + 3, 2), np.float32), out_hw, errors), plain)
    ctrl = np.zeros((B, G + 3, G + 3, 2), np.float32)
    ctrl[..., 0], ctrl[..., 1] = np.float32(2.75), np.float32(-1.5)
    x, label, onehot = _warp(dev, vset, rec, ctrl, out_hw, errors)
    worst = _check_batch(small_set, rec, ctrl, out_hw, x, label, onehot, 5)
    print("constant table: image error / bound %.3f" % worst)
    assert not _bits((x,), plain[:1]) and int(errors.item()) == 0


# ---- 3. random tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_hw,B", [((32, 48), 6), ((17, 23), 3), ((3, 5), 16), ((5, 300), 4)])
@pytest.mark.parametrize("G", [1, 3, 4, 16])
def test_random_tables_against_the_restatement(dev, small_set, errors, G, out_hw, B):
    vs = pkg("volume_source")
    vset = small_set[0]
    rng = np.random.default_rng([G, out_hw[0], B])
    rec = _records(vs, rng, B, out_hw)
    rec["warp"] = [(b % 3) != 1 for b in range(B)]                 # warped and plain samples in one batch
    ctrl = _table(rng, B, G)
    ncls = 5 if G != 3 else 8
    x, label, onehot = _warp(dev, vset, rec, ctrl, out_hw, errors, ncls=ncls)
    assert x.shape == (B,) + out_hw + (3,) and label.shape == (B,) + out_hw and onehot.shape == (B,) + out_hw + (ncls,)
    worst = _check_batch(small_set, rec, ctrl, out_hw, x, label, onehot, ncls)
    print("G=%d %s B=%d: image error / bound, worst sample: %.3f (c = %.1f)" % (G, out_hw, B, worst, Wr.warp_c(G)))
    again = _warp(dev, vset, rec, ctrl, out_hw, errors, ncls=ncls)
    assert _bits(again, (x, label, onehot)) and int(errors.item()) == 0
    # the warp does something: a warped sample differs from its plain gather
    rec0 = rec.copy()
    rec0["warp"] = 0
    x0 = _warp(dev, vset, rec0, ctrl, out_hw, errors, ncls=ncls, want_onehot=False)[0]
    assert not torch.equal(x0[0], x[0]) and torch.equal(x0[1], x[1])


# ---- 4. non-finite and huge control points -------------------------------------------------------------------------------------------------
def test_non_finite_and_huge_control_points_end_as_fill(dev, small_set, errors):
    """The compare-before-convert rule (§13's far_outside case, for the displacement): a NaN, an infinity or 1e30 among the 16 points a pixel
    reads puts it outside the slice — fill / label 0 — and nothing is refused.  G = 4 on 32 x 48 keeps every pixel's t at least 1/64 from a
    cell border (asserted), so the reference and the kernel agree on which points a pixel reads."""
    vs = pkg("volume_source")
    vset = small_set[0]
    out_hw, B, G = (32, 48), 4, 4
    for n in out_hw:
        _, t = Wr.cells(n, G)
        assert min(t.min(), 1 - t.max()) >= 1 / 64
    rng = np.random.default_rng(4)
    rec = _records(vs, rng, B, out_hw, volumes=[0, 1, 0, 1])
    rec["warp"] = 1
    clean = _table(rng, B, G)
    ctrl = clean.copy()                                              # a point in row k is read by the cells k - 3 .. k of that axis
    ctrl[0, 0, 0, 0] = np.nan
    ctrl[0, 6, 6, 1] = np.inf
    ctrl[1, 0, 6, 0], ctrl[1, 1, 6, 0] = np.inf, -np.inf            # both in the support of cell (0, 3): inf - inf
    ctrl[2, 6, 0, 0] = 1e30
    ctrl[2, 0, 3, 1] = -1e30
    bad = ~np.isfinite(ctrl).all(axis=-1) | (np.abs(ctrl) > 1e20).any(axis=-1)
    ref_ctrl = np.where(bad[..., None], np.float32(0), ctrl)       # what the other pixels read is unchanged by the zeroed entries
    reach = np.stack([Wr.support_holds(ctrl[b], out_hw[0], out_hw[1], bad[b]) for b in range(B)])
    assert reach[:3].any(axis=(1, 2)).all() and not reach[:3].all(axis=(1, 2)).any() and not reach[3].any()
    x, label, onehot = _warp(dev, vset, rec, ctrl, out_hw, errors)
    xg, lg = x.cpu().numpy(), label.cpu().numpy()
    for b in range(B):
        fill = np.float32(vset.stats[int(rec["volume"][b])]["fill"])
        assert np.all(xg[b][reach[b]] == fill) and not lg[b][reach[b]].any(), b
    worst = _check_batch(small_set, rec, ref_ctrl, out_hw, x, label, onehot, 5, skip=reach)
    print("pixels reached by a non-finite point: %d of %d; the others: image error / bound %.3f" % (int(reach.sum()), reach.size, worst))
    assert int(errors.item()) == 0


# ---- 5. gain and bias ----------------------------------------------------------------------------------------------------------------------
def test_gain_and_bias(dev, small_set, errors):
    vs = pkg("volume_source")
    vset = small_set[0]
    out_hw, B, G = (17, 23), 5, 4
    rng = np.random.default_rng(5)
    rec = _records(vs, rng, B, out_hw)
    rec["warp"] = 1
    ctrl = _table(rng, B, G)
    base = _warp(dev, vset, rec, ctrl, out_hw, errors)
    rec["gain"] = [1.25, 0.8, 1.0, 0.0, -1.5]
    rec["bias"] = [0.3, -0.2, 0.5, 0.25, 0.0]
    got = _warp(dev, vset, rec, ctrl, out_hw, errors)
    assert _bits(got, _warp(dev, vset, rec, ctrl, out_hw, errors))
    assert _bits(got[1:], base[1:])                                 # label and one-hot do not see the intensity
    b64, g = base[0].cpu().numpy().astype(np.float64), got[0].cpu().numpy()
    want = (rec["gain"].astype(np.float64)[:, None, None, None] * b64 + rec["bias"].astype(np.float64)[:, None, None, None]).astype(np.float32)
    ulps = np.abs(g.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print("gain / bias: worst distance from fl32(gain base + bias): %.2f ulp" % float(ulps.max()))
    assert float(ulps.max()) <= 1.0
    assert np.all(g[3] == np.float32(0.25))                         # gain 0: the bias everywhere, fill pixels included
    assert int(errors.item()) == 0


# ---- 6. noise ------------------------------------------------------------------------------------------------------------------------------
def test_noise(dev, small_set, errors):
    vs = pkg("volume_source")
    vset = small_set[0]
    out_hw, B = (17, 23), 4
    H, W = out_hw
    rng = np.random.default_rng(6)
    rec = _records(vs, rng, B, out_hw)
    rec["seed"] = [7, 0xFFFFFFFF, 123456789, 7]
    sig = np.array([0.1, 1.0, 0.013, 0.1], np.float32)
    nref = np.stack([Wr.noise_field(H, W, int(s)) for s in rec["seed"]])
    assert np.abs(nref).max() <= np.sqrt(48 * np.log(2))
    base = _warp(dev, vset, rec, None, out_hw, errors)
    # (a) on top of zero (gain = bias = 0): the noise alone, held to c' u sigma
    z = rec.copy()
    z["gain"], z["noise"] = 0.0, sig
    alone = _warp(dev, vset, z, None, out_hw, errors)
    a = alone[0].cpu().numpy().astype(np.float64)
    err = np.abs(a - sig.astype(np.float64)[:, None, None, None] * nref) / sig.astype(np.float64)[:, None, None, None]
    print("noise alone: worst |out - sigma n| = %.2f u sigma (bound c' = %.0f)" % (float(err.max()) / U, Wr.NOISE_C))
    assert float(err.max()) <= Wr.NOISE_C * U
    assert _bits(alone[1:], base[1:])
    # (b) on top of the image: the same noise, and the final fmaf rounds once more at |out| (half an ulp there)
    rec["noise"] = sig
    got = _warp(dev, vset, rec, None, out_hw, errors)
    g, b0 = got[0].cpu().numpy(), base[0].cpu().numpy()
    diff = g.astype(np.float64) - b0.astype(np.float64)
    bound = Wr.NOISE_C * U * sig.astype(np.float64)[:, None, None, None] + 0.5 * np.spacing(np.abs(g)).astype(np.float64)
    derr = np.abs(diff - sig.astype(np.float64)[:, None, None, None] * nref)
    print("noise on the image: worst error / bound %.3f" % float((derr / bound).max()))
    assert np.all(derr <= bound)
    # the same seed twice: identical bits; samples 0 and 3 share seed and sigma: the same noise on different images
    assert _bits(got, _warp(dev, vset, rec, None, out_hw, errors))
    assert np.array_equal(alone[0][0].cpu().numpy(), alone[0][3].cpu().numpy())
    # different seeds, pixels and channels differ
    assert not np.array_equal(a[0] / 0.1, a[1]) and np.abs(a[0] / np.float64(sig[0]) - a[1] / np.float64(sig[1])).std() > 0.5
    assert np.abs(a[1][..., 0] - a[1][..., 1]).std() > 0.5 and np.abs(a[1][1:] - a[1][:-1]).std() > 0.5       # (|N(0, 2)| has std 0.85)
    n1 = a[1].ravel()                                               # sigma 1: the normal itself, 1173 values
    assert abs(n1.mean()) <= 5 / np.sqrt(n1.size) and abs(n1.var() - 1) <= 5 * np.sqrt(2.0 / n1.size)
    # noise = 0 adds nothing, whatever the seed
    rec["noise"] = 0.0
    assert _bits(_warp(dev, vset, rec, None, out_hw, errors), base)
    assert int(errors.item()) == 0


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_samples_and_host_errors(dev, small_set, errors):
    vs, K, L = pkg("volume_source"), pkg("kernels"), pkg("_lib")
    vset = small_set[0]
    out_hw, B = (10, 14), 6
    rng = np.random.default_rng(7)
    rec = _records(vs, rng, B, out_hw, volumes=[0, 1, 2])
    rec["gain"], rec["bias"], rec["noise"], rec["seed"] = 1.5, 0.25, 0.5, np.arange(B)
    alone = _warp(dev, vset, rec[[0, 5]], None, out_hw, errors)
    assert int(errors.item()) == 0
    rec["warp"][1] = 1                      # a warp without a table (G = 0)
    rec["volume"][2] = 3                    # volume nvol
    rec["frame"][3] = SHAPES[0][2]          # frame Z
    rec["volume"][4] = -1
    x, label, onehot = _warp(dev, vset, rec, None, out_hw, errors)
    assert int(errors.item()) == 4          # once each
    for b in (1, 2, 3, 4):
        v = int(rec["volume"][b])
        fill = np.float32(vset.stats[v]["fill"]) if 0 <= v < 3 else np.float32(0)
        # plain fill: neither gain, bias nor noise touch a refused sample
        assert bool((x[b] == float(fill)).all()) and not label[b].any() and bool((onehot[b, :, :, 0] == 1).all()) and not onehot[b, :, :, 1:].any(), b
    assert _bits((x[[0, 5]], label[[0, 5]], onehot[[0, 5]]), alone)
    # with a table the same record is served
    rec2 = rec[[1]].copy()
    _warp(dev, vset, rec2, _table(rng, 1, 2), out_hw, errors)
    assert int(errors.item()) == 4
    # host-side refusals raise before any launch
    sd = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    cd = torch.zeros(B * 7 * 7 * 2, dtype=torch.float32, device=dev)
    call = lambda ctrl, G, samples=sd, H=10: K.aug_slices_warp(vset.table_host, vset.table_dev, 3, samples, ctrl, G, B, H, 14, errors, ncls=5)
    with pytest.raises(L.PnpError, match="G = 17 outside"):
        call(torch.zeros(B * 20 * 20 * 2, dtype=torch.float32, device=dev), 17)
    with pytest.raises(L.PnpError, match="null exactly when G == 0"):
        call(None, 4)
    with pytest.raises(L.PnpError, match="control table must be contiguous float32"):
        call(cd[:-2], 4)
    with pytest.raises(L.PnpError, match="8-byte aligned"):
        call(torch.zeros(B * 7 * 7 * 2 + 1, dtype=torch.float32, device=dev)[1:], 4)
    with pytest.raises(L.PnpError, match="not B = 6 records"):
        call(cd, 4, samples=sd[:-56])
    with pytest.raises(L.PnpError, match="output size 0 x 14"):
        call(cd, 4, H=0)
    assert int(errors.item()) == 4


# ---- 8. through the product ------------------------------------------------------------------------------------------------------------------
AUG = {"rotate": 10, "elastic": 2.0, "elastic_grid": 4, "contrast": 0.2, "brightness": 0.3, "noise": 0.1}


def test_source_with_the_new_keys(dev, small_set):
    vs = pkg("volume_source")
    vset, host, gaps = small_set
    out_hw, B = (32, 32), 4
    mk = lambda aug=AUG, seed=3, shard=None: vs.AugmentedSliceSource(vset, B, out_size=out_hw, augment=aug, seed=seed, shard=shard)
    a, b = mk(), mk()
    xa, oa, fa = a.next_device_batch()
    xb, ob, fb = b.next_device_batch()
    assert fa == fb and torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(oa, ob)
    rec, ctrl = a.last_params, a.last_ctrl
    assert rec.dtype == vs.SAMPLE_W_DTYPE and ctrl.shape == (B, 7, 7, 2) and ctrl.dtype == np.float32 and np.all(rec["warp"] == 1) and np.all(rec["dz"] == 1)
    assert np.array_equal(ctrl, b.last_ctrl) and np.ptp(rec["gain"]) > 0 and np.ptp(rec["noise"]) > 0
    # the batch is the reference rebuilt from the records and the control table
    xg = xa.cpu().numpy()
    worst = 0.0
    for s in range(B):
        ref, ibound, (sx, sy), eps = _reference(small_set, rec, ctrl, out_hw, s)
        g, bi, sg = (np.float64(rec[k][s]) for k in ("gain", "bias", "noise"))
        want = Wr.intensity(ref, g, bi, sg, Wr.noise_field(out_hw[0], out_hw[1], int(rec["seed"][s])))
        # the image bound scaled by the gain, the noise bound, and the two fmaf roundings at the size of the result
        bound = abs(g) * ibound + Wr.NOISE_C * U * sg + 2 * U * float(np.abs(want).max())
        err = float(np.abs(xg[s] - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (s, err, bound)
        lab = oa[s].argmax(-1).cpu().numpy()
        cand = R.label_candidates(host[int(rec["volume"][s])][1], int(rec["frame"][s]), sx, sy, eps)
        valid = oa[s].sum(-1).cpu().numpy() > 0
        assert np.all((lab[None] == cand).any(axis=0)[valid])
    print("source batch against the reference: error / bound %.3f" % worst)
    # the numpy view and other ranks
    batch, fids = mk().next_batch(B)
    assert fids == fa and np.array_equal(batch[..., :3], xg)
    other = mk(shard=(1, 2))
    xo, _, fo = other.next_device_batch()
    assert fo != fa or not torch.equal(xo, xa)
    assert not np.array_equal(other.last_ctrl, ctrl)
    # the classic fields of the stream are those of the source without the new keys, which calls what it called before
    plain = mk(aug={"rotate": 10})
    plain.next_device_batch()
    assert plain.last_params.dtype == vs.SAMPLE_DTYPE and plain.last_ctrl is None and not plain.warp
    for f in ("volume", "frame", "m"):
        assert plain.last_params[f].tobytes() == rec[f].tobytes()
    # intensity only: no table is uploaded
    inten = mk(aug={"contrast": 0.2, "noise": 0.05})
    inten.next_device_batch()
    assert inten.last_ctrl is None and inten.last_params.dtype == vs.SAMPLE_W_DTYPE and not inten.last_params["warp"].any()
    with pytest.raises(ValueError, match="folds"):
        mk(aug={"elastic": 5.0})
    for src in (a, b, other, plain, inten):
        assert src.errors() == 0
        src.close()


def test_train_segmenter_with_elastic_augmentation(dev, tmp_path):
    ts, vs, nifti = pkg("train_segmenter"), pkg("volume_source"), pkg("nifti")
    rng = np.random.default_rng(5)
    lines = []
    for n in range(2):
        img, lab = _blob_volume(rng, (256, 256, 4))
        nifti.save(nifti.Nifti1Image(img, np.diag([1.0, 1.0, 2.0, 1.0])), str(tmp_path / ("s%d_image.nii.gz" % n)))
        nifti.save(nifti.Nifti1Image(lab.astype(np.int16), np.diag([1.0, 1.0, 2.0, 1.0])), str(tmp_path / ("s%d_label.nii.gz" % n)))
        lines.append("s%d_image.nii.gz s%d_label.nii.gz" % (n, n))
    (tmp_path / "train_list").write_text("\n".join(lines) + "\n")
    (tmp_path / "val_list").write_text(lines[1] + "\n")
    tr = ts.main(["--nii-train", str(tmp_path / "train_list"), "--nii-val", str(tmp_path / "val_list"), "--augment", '{"elastic": 2}',
                  "--batch-size", "2", "--iters", "2", "--epochs", "1", "--output", str(tmp_path / "seg")])
    assert tr.train_list.augment["elastic"] == 2.0 and tr.train_list.warp and tr.val_list.augment is None and not tr.val_list.warp
    assert tr.train_list.last_params.dtype == vs.SAMPLE_W_DTYPE and tr.train_list.last_ctrl.shape == (2, 7, 7, 2)
    assert tr.val_list.last_params is None or tr.val_list.last_params.dtype == vs.SAMPLE_DTYPE
    assert np.isfinite(tr.loss_dict["train"][1]) and tr.train_list.errors() == 0 and os.path.exists(os.path.join(str(tmp_path / "seg"), "checkpoint.npz"))
