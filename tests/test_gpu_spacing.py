"""-m gpu: sampling on a millimetre grid — pnp_aug_slices_z, pnp_paste_labels_fov and pnp_paste_ensemble_fov against the
float64 restatements of tests/spacing_ref.py, then the feature through segment_volume and the command lines.

Bounds (derived, not tuned):
  image     spacing_ref.image_bound: §13's eps (Gx + Gy) + 4 u max|v| plus the z term eps_z Gz + 4 u max|v| (eps_z: 4 float32 ulps at the
            largest frame coordinate, Gz: the largest gap between voxels adjacent along z; the lerp rounds three times).  No pixel excluded.
  label     §13's candidate rule, at the centre frame.
  linear field   restated at test_linear_field_on_two_grids.
  paste     the written set is compared EXACTLY with the float64 coverage: every geometry keeps its coordinates at least 1e-3 plane pixels
            from the coverage border (asserted), hundreds of times the float32 coordinate error; covered bytes are compared bit for bit
            with the entry without _fov and held to paste_ref.admissible / ensemble_ref's bounds against float64.
"""
import os

import numpy as np
import pytest
import torch

import augment_ref as A
import ensemble_ref as E
import paste_ref as P
import spacing_ref as S
from conftest import pkg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(13, 11, 7), (9, 17, 5), (6, 5, 1)]
SPACINGS = [(0.7, 1.3, 2.0), (1.2, 0.9, 1.0), (0.5, 0.5, 3.0)]
FILLS = [-1.75, 0.5, -3.0]


@pytest.fixture(scope="module")
def small_set(dev):
    """three small volumes, one of a single frame, handed over as they are (from_device: nothing is normalised)"""
    vs = pkg("volume_source")
    rng = np.random.default_rng(17)
    host = [((rng.standard_normal(s) * 2).astype(np.float32), rng.integers(0, 7, s).astype(np.uint8)) for s in SHAPES]
    vset = vs.VolumeSet.from_device([torch.from_numpy(v).to(dev) for v, _ in host], [torch.from_numpy(l).to(dev) for _, l in host],
                                    ["v%d" % i for i in range(3)], FILLS, spacings=SPACINGS, min_frames=1)
    assert vset.spacings == SPACINGS
    return vset, host


MAPS = ({"rotate": 33.0, "scale": 1.3, "flip": True, "translate": (0.8, -1.1)},      # rotated / scaled / flipped
        {"rotate": -12.5, "scale": 0.45},                                           # most of the plane outside the slice
        {})                                                                         # the plain millimetre grid: partly outside already


def _records(vs, specs, out_hw, pixel_mm=(1.0, 1.1)):
    """specs: [(volume, frame, dz, compose_matrix keywords | six entries)]"""
    rec = np.zeros(len(specs), dtype=vs.SAMPLE_Z_DTYPE)
    for b, (v, z, dz, kw) in enumerate(specs):
        rec["volume"][b], rec["frame"][b], rec["dz"][b] = v, z, dz
        vv = min(max(v, 0), len(SHAPES) - 1)
        rec["m"][b] = kw if isinstance(kw, np.ndarray) else pkg("volume_source").compose_matrix(SHAPES[vv][:2], out_hw, spacing_xy=SPACINGS[vv][:2],
                                                                                                pixel_mm=pixel_mm, **kw)
    return rec


def _check_batch(host, rec, out_hw, x, label, onehot, ncls):
    H, W = out_hw
    xg, lg = x.cpu().numpy(), label.cpu().numpy()
    eps = A.coord_eps(rec["m"], H, W)
    worst = 0.0
    for b in range(len(rec)):
        v, z, dz = int(rec["volume"][b]), int(rec["frame"][b]), float(rec["dz"][b])
        vol, lab = host[v]
        fill = np.float64(np.float32(FILLS[v]))
        sx, sy = A.coords(rec["m"][b], H, W)
        ref = S.gather_image_z(vol, z, dz, sx, sy, fill)
        bound = S.image_bound(vol, fill, rec["m"], H, W)
        err = float(np.abs(xg[b] - ref).max())
        worst = max(worst, err / bound)
        assert err <= bound, (b, v, z, dz, err, bound)
        cand = A.label_candidates(lab, z, sx, sy, eps)
        assert np.all((lg[b][None] == cand).any(axis=0)), (b, int((~(lg[b][None] == cand).any(axis=0)).sum()))
    if onehot is not None:
        assert np.array_equal(onehot.cpu().numpy(), A.onehot(lg, ncls))
    return worst


# ---- 1. the gather against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_hw,B", [((16, 12), 3), ((5, 3), 1)])
def test_gather_against_the_restatement(dev, small_set, out_hw, B):
    vs = pkg("volume_source")
    vset, host = small_set
    src = vs.AugmentedSliceSource(vset, B, out_size=out_hw, augment=None, num_cls=5, sample_mm=1.0)
    worst, outside, n = 0.0, 0.0, 0
    for dz in (0.0, 0.37, 1.0, 2.5, 7.9):
        for where in (0, 1, 2):                         # centre frame 0, the middle, Z - 1
            for k, kw in enumerate(MAPS):
                vols = range(3) if B == 3 else [(n + k) % 3]
                specs = [(v, (0, SHAPES[v][2] // 2, SHAPES[v][2] - 1)[where], dz, kw) for v in vols]
                rec = _records(vs, specs, out_hw)
                x, label, onehot = src.gather_records(rec, 5, True)
                assert x.shape == (B,) + out_hw + (3,) and label.shape == (B,) + out_hw and onehot.shape == (B,) + out_hw + (5,)
                worst = max(worst, _check_batch(host, rec, out_hw, x, label, onehot, 5))
                outside += float(np.mean([float((x[k2, ..., 1] == FILLS[sp[0]]).float().mean()) for k2, sp in enumerate(specs)]))
                n += 1
    print("pnp_aug_slices_z %s B=%d: image error / bound, worst sample of %d batches: %.3f" % (out_hw, B, n, worst))
    assert src.errors() == 0
    assert 0.02 < outside / n < 0.9                     # the maps are partly out of the slice, and not only


# ---- 2. dz = 1 is pnp_aug_slices, bit for bit --------------------------------------------------------------------------------------------
def test_unit_step_is_the_three_frame_gather_bit_for_bit(dev, small_set):
    vs = pkg("volume_source")
    vset, host = small_set
    two = vs.VolumeSet.from_device(vset.images[:2], vset.labels[:2], vset.names[:2], FILLS[:2])
    out_hw = (16, 12)
    rng = np.random.default_rng(3)
    specs = []
    for v in (0, 1):
        for z in range(1, SHAPES[v][2] - 1):
            m = vs.compose_matrix(SHAPES[v][:2], out_hw, rotate=rng.uniform(-180, 180), scale=np.exp(rng.uniform(-0.5, 0.5)),
                                  translate=tuple(rng.uniform(-3, 3, 2)), flip=bool(rng.integers(2)))
            specs.append((v, z, 1.0, m))
    rec_z = _records(vs, specs, out_hw)
    rec = np.zeros(len(specs), dtype=vs.SAMPLE_DTYPE)
    for f in ("volume", "frame", "m"):
        rec[f] = rec_z[f]
    a = vs.AugmentedSliceSource(two, len(specs), out_size=out_hw, augment=None, num_cls=5).gather_records(rec, 5, True)
    srcz = vs.AugmentedSliceSource(two, len(specs), out_size=out_hw, augment=None, num_cls=5, sample_mm=2.0)
    b = srcz.gather_records(rec_z, 5, True)
    for got, want in zip(b, a):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert srcz.errors() == 0
    # at frame 0 / Z - 1 the missing neighbour is the edge frame itself: today's edge padding (segment_volume's padded copy)
    v = vset.images[0]
    padded = torch.cat([v[:, :, :1], v, v[:, :, -1:]], dim=2).contiguous()
    pad = vs.VolumeSet.from_device([padded], [torch.zeros_like(padded, dtype=torch.uint8)], ["p"], FILLS[:1])
    m = vs.compose_matrix(SHAPES[0][:2], out_hw, rotate=20.0)
    rec = np.zeros(2, dtype=vs.SAMPLE_DTYPE)
    rec["frame"], rec["m"] = [1, SHAPES[0][2]], m
    want = vs.AugmentedSliceSource(pad, 2, out_size=out_hw, augment=None).gather_records(rec, 5, False)[0]
    got = srcz.gather_records(_records(vs, [(0, 0, 1.0, m), (0, SHAPES[0][2] - 1, 1.0, m)], out_hw), 5, False)[0]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- 3. refused samples ------------------------------------------------------------------------------------------------------------------
def test_refused_samples_are_counted_once_and_delivered_as_fill(dev, small_set):
    vs, L = pkg("volume_source"), pkg("_lib")
    vset, host = small_set
    out_hw = (10, 14)
    ident = np.array([1, 0, 0, 0, 1, 0], np.float32)
    specs = [(0, 3, 0.5, ident), (0, -1, 1.0, ident), (0, 7, 1.0, ident), (1, 2, np.nan, ident), (1, 2, -1.0, ident), (3, 0, 1.0, ident),
             (-1, 0, 1.0, ident), (1, 2, np.inf, ident), (2, 0, 4.0, ident), (1, 4, 1.5, ident)]
    rec = _records(vs, specs, out_hw)
    src = vs.AugmentedSliceSource(vset, len(specs), out_size=out_hw, augment=None, sample_mm=1.0)
    x, label, onehot = src.gather_records(rec, 5, True)
    bad = [1, 2, 3, 4, 5, 6, 7]          # frame -1, frame Z, dz NaN, dz -1, volume nvol, volume -1, dz inf
    for b in bad:
        v = int(rec["volume"][b])
        fill = np.float32(FILLS[v]) if 0 <= v < 3 else np.float32(0)
        assert bool((x[b] == float(fill)).all()) and not label[b].any() and bool((onehot[b, :, :, 0] == 1).all()) and not onehot[b, :, :, 1:].any(), b
    good = [0, 8, 9]                     # the neighbours in the batch are what they are without the refused ones
    _check_batch(host, rec[good], out_hw, x[good], label[good], None, 5)
    alone = src.gather_records(rec[good], 5, False)[0]
    assert torch.equal(alone.view(torch.int32), x[good].view(torch.int32))
    assert src.errors() == len(bad)
    with pytest.raises(L.PnpError, match="refused 7 samples"):
        src.close()
    # the wrapper refuses a table of the other record type (it would be read past its end)
    K = pkg("kernels")
    short = torch.zeros(2 * 32, dtype=torch.uint8, device=dev)
    with pytest.raises(L.PnpError, match="not B = 2 records"):
        K.aug_slices_z(vset.table_host, vset.table_dev, 3, short, 2, 4, 4, src._errors)


# ---- 4. a linear field on two grids: the feature's point -----------------------------------------------------------------------------------
def test_linear_field_on_two_grids(dev):
    """f(mm) = a x + b y + c z + d, millimetres from the volume's centre, sampled on two grids of different voxel size.  Trilinear
    interpolation reproduces a linear field, so with one sample_mm both gathers give f at the pixel's physical position, and the outer
    channels differ from the centre one by -+ c frame_mm.
    Bound per value: eps (|a| sx + |b| sy) + eps_z |c| sz + 10 u max|f|
      eps, eps_z   the coordinate roundings of §13 / §17 in voxels, times the field's gradient per voxel;
      10 u max|f|  counted roundings, each at most u max|f| = 2^-24 max|f|: the voxel stored as float32 (1); the z-lerp's difference and
                   fmaf (3, derived at spacing_ref.image_bound); 1 - t twice (2); per bilinear step one product and one fmaf, the two
                   y-steps running side by side (2 + 2).
    The pixel's physical position is taken from the six float32 entries the kernel gets (test_spacing_host.py holds those to the
    formula)."""
    vs = pkg("volume_source")
    a, b, c, d = 0.8, -0.5, 0.3, 20.0
    grids = [((40, 40, 41), (0.6, 0.6, 2.0), 22), ((40, 44, 41), (1.2, 0.9, 1.0), 24)]          # frames 22 / 24: both z = +4 mm
    sample_mm, out_hw = (0.5, 0.45, 1.5), (32, 32)
    vols = []
    for (X, Y, Z), (sx, sy, sz), _ in grids:
        g = np.meshgrid((np.arange(X) - (X - 1) / 2) * sx, (np.arange(Y) - (Y - 1) / 2) * sy, (np.arange(Z) - (Z - 1) / 2) * sz, indexing="ij")
        vols.append((a * g[0] + b * g[1] + c * g[2] + d).astype(np.float32))
    top = max(float(np.abs(v).max()) for v in vols)
    vset = vs.VolumeSet.from_device([torch.from_numpy(v).to(dev) for v in vols], [torch.zeros(v.shape, dtype=torch.uint8, device=dev) for v in vols],
                                    ["fine", "coarse"], [0.0, 0.0], spacings=[g[1] for g in grids])
    src = vs.AugmentedSliceSource(vset, 2, out_size=out_hw, augment=None, sample_mm=sample_mm)
    kw = {"rotate": 20.0, "scale": 1.05, "translate": (1.0, -0.6)}
    rec = np.zeros(2, dtype=vs.SAMPLE_Z_DTYPE)
    for n, ((X, Y, Z), sp, frame) in enumerate(grids):
        rec[n] = (n, frame, np.float32(sample_mm[2] / sp[2]), vs.compose_matrix((X, Y), out_hw, spacing_xy=sp[:2], pixel_mm=sample_mm[:2], **kw))
    x = src.gather_records(rec, 5, False)[0].cpu().numpy().astype(np.float64)
    assert src.errors() == 0
    fields, worst = [], 0.0
    for n, ((X, Y, Z), (sx, sy, sz), frame) in enumerate(grids):
        cx, cy = A.coords(rec["m"][n], *out_hw)
        assert cx.min() >= 0 and cx.max() <= X - 1 and cy.min() >= 0 and cy.max() <= Y - 1          # every corner inside the volume
        lo, hi = S.frame_positions(frame, rec["dz"][n], Z)
        assert 0 < lo < frame < hi < Z - 1
        zmm = (np.array([lo, frame, hi]) - (Z - 1) / 2) * sz
        want = (a * (cx - (X - 1) / 2) * sx + b * (cy - (Y - 1) / 2) * sy + d)[..., None] + c * zmm
        bound = A.coord_eps(rec["m"][n:n + 1], *out_hw) * (abs(a) * sx + abs(b) * sy) + S.z_eps(Z) * abs(c) * sz + 10 * U * top
        err = float(np.abs(x[n] - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (n, err, bound)
        # channels 0 / 2 = channel 1 -+ c frame_mm (dz is frame_mm / sz rounded to float32: relative 2^-24 of the step)
        step = 2 * bound + abs(c) * sample_mm[2] * U
        assert np.abs(x[n][..., 0] - (x[n][..., 1] - c * sample_mm[2])).max() <= step and np.abs(x[n][..., 2] - (x[n][..., 1] + c * sample_mm[2])).max() <= step
        fields.append((want, bound))
    # the two scans show the network the same picture: the plane's physical positions agree up to the rounding of the map entries
    same = float(np.abs(fields[0][0] - fields[1][0]).max())
    assert same <= fields[0][1] + fields[1][1], same
    assert np.abs(x[0] - x[1]).max() <= 2 * (fields[0][1] + fields[1][1])
    assert np.ptp(x[0][..., 1]) > 5.0                   # the field varies over the plane: the comparison is not vacuous
    print("linear field: error / bound %.3f; the two grids differ by %.3e (max|f| %.1f)" % (worst, float(np.abs(x[0] - x[1]).max()), top))


# ---- 5. pnp_paste_labels_fov -------------------------------------------------------------------------------------------------------------
def _geometry(case):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (X, Y), sp, px, (H, W), kw, _, _ = S.GEOMETRIES[case]
    return (X, Y), (H, W), vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), spacing_xy=sp, pixel_mm=px, **kw))


def _paste_labels_case(dev, XY, HW, inv, kind, B, nb, z0, Z, seed):
    K = pkg("kernels")
    (X, Y), (H, W) = XY, HW
    assert S.border_margin(inv, X, Y, H, W) >= 1e-3          # no input is exempt from the exact comparison below
    cov = S.covered(inv, X, Y, H, W)
    logits = S.smooth_plane_logits(B, H, W, 5, seed)
    lg = torch.from_numpy(logits).to(dev)
    elems, origin, strides = P.layout(kind, X, Y, Z)
    got = torch.full((elems,), 0xAB, dtype=torch.uint8, device=dev)
    full = torch.full((elems,), 0xAB, dtype=torch.uint8, device=dev)
    K.paste_labels(lg, nb, z0, inv, (X, Y), got, origin, strides, fov=True)
    K.paste_labels(lg, nb, z0, inv, (X, Y), full, origin, strides)
    got, full = got.cpu().numpy(), full.cpu().numpy()
    idx = P.written_index(X, Y, nb, z0, origin, strides)                      # [nb, X, Y]
    want_written = np.zeros(elems, dtype=bool)
    want_written[idx[:, cov].ravel()] = True
    assert np.array_equal(got != 0xAB, want_written), (int((got != 0xAB).sum()), int(want_written.sum()))
    assert np.array_equal(got[want_written], full[want_written])              # covered bytes: pnp_paste_labels', bit for bit
    assert np.all(got[~want_written] == 0xAB)
    _, r = P.labels(logits, inv, X, Y, nb)
    adm = P.admissible(r, P.delta(logits[:nb], inv, X, Y))
    lab = got[idx]                                                            # [nb, X, Y]
    ok = np.take_along_axis(adm, np.minimum(lab, 4)[..., None].astype(np.int64), axis=-1)[..., 0]
    assert np.all(ok[:, cov]) and np.all(lab[:, cov] < 5)
    return float(cov.mean())


@pytest.mark.parametrize("case", sorted(S.GEOMETRIES))
def test_paste_labels_fov_writes_the_covered_columns_only(dev, case):
    XY, HW, inv = _geometry(case)
    share = _paste_labels_case(dev, XY, HW, inv, "c", 8, 7, 1, 9, case)        # nb = 7: head bytes, a packed dword, tail bytes; z0 unaligned
    print("geometry %d: %.1f %% covered" % (case, 100 * share))
    assert abs(share - S.GEOMETRIES[case][6]) < 0.005


@pytest.mark.parametrize("kind", ["c", "zfirst_flipped", "sub_box"])
def test_paste_labels_fov_in_every_layout(dev, kind):
    """an 11 x 9 grid at (0.7, 1.3) mm under an 8 x 8 plane of 1 mm pixels, rotated: small enough for paste_ref's sub_box; nb = 5, z0 = 1"""
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    inv = vp.invert_matrix(vs.compose_matrix((11, 9), (8, 8), rotate=10.0, spacing_xy=(0.7, 1.3), pixel_mm=(1.0, 1.0)))
    share = _paste_labels_case(dev, (11, 9), (8, 8), inv, kind, 6, 5, 1, 7, 40)
    assert 0.3 < share < 0.9


# ---- 6. pnp_paste_ensemble_fov -----------------------------------------------------------------------------------------------------------
def _ensemble_case(dev, invs, XY, HW, kind, seed, M=None):
    K = pkg("kernels")
    (X, Y), (H, W) = XY, HW
    B, nb, z0, Z, ncls = 6, 5, 1, 7, 5
    M = len(invs) if M is None else M
    logits = [S.smooth_plane_logits(B, H, W, ncls, [seed, m]) for m in range(M)]
    lg = [torch.from_numpy(l).to(dev) for l in logits]
    elems, origin, strides = P.layout(kind, X, Y, Z)
    out = {}
    for fov in (True, False):
        vol = torch.full((elems,), 0xAB, dtype=torch.uint8, device=dev)
        prob = torch.full((ncls * elems,), -7.0, dtype=torch.float32, device=dev)
        ent = torch.full((elems,), -7.0, dtype=torch.float32, device=dev)
        K.paste_ensemble(lg, nb, z0, invs, (X, Y), vol, origin, strides, prob=prob, entropy=ent, fov=fov)
        out[fov] = (vol.cpu().numpy(), prob.cpu().numpy().reshape(ncls, elems), ent.cpu().numpy())
    return logits, out, P.written_index(X, Y, nb, z0, origin, strides), elems


@pytest.mark.parametrize("kind", ["c", "zfirst_flipped"])
def test_paste_ensemble_fov_covers_the_intersection(dev, kind):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    XY, HW = (23, 19), (16, 16)
    invs = []
    for case in (1, 2, 5):               # the maps of geometries 1, 2 and 5 on one 16 x 16 plane (members share their logits' shape)
        _, sp, px, _, kw, _, _ = S.GEOMETRIES[case]
        invs.append(vp.invert_matrix(vs.compose_matrix(XY, HW, spacing_xy=sp, pixel_mm=px, **kw)))
    assert S.border_margin(invs, *XY, *HW) >= 1e-3
    cov = S.covered(invs, *XY, *HW)
    each = [S.covered(i, *XY, *HW) for i in invs]
    assert np.array_equal(cov, each[0] & each[1] & each[2]) and cov.sum() < min(e.sum() for e in each) and cov.sum() > 50
    logits, out, idx, elems = _ensemble_case(dev, invs, XY, HW, kind, 60)
    written = np.zeros(elems, dtype=bool)
    written[idx[:, cov].ravel()] = True
    (vol, prob, ent), (fvol, fprob, fent) = out[True], out[False]
    assert np.array_equal(vol != 0xAB, written) and np.array_equal(ent != -7.0, written) and np.array_equal((prob != -7.0).all(axis=0), written)
    assert np.array_equal((prob != -7.0).any(axis=0), written)
    assert np.array_equal(vol[written], fvol[written])
    assert np.array_equal(prob[:, written].view(np.uint32), fprob[:, written].view(np.uint32))
    assert np.array_equal(ent[written].view(np.uint32), fent[written].view(np.uint32))
    # and the covered values are the ensemble's, against float64 (§15's bounds)
    ref = E.ensemble(logits, invs, *XY, nb=5)
    dp = E.delta_p(logits, invs, *XY, nb=5)
    lab = vol[idx]
    ok = np.take_along_axis(E.admissible(ref.prob, dp), np.minimum(lab, 4)[..., None].astype(np.int64), axis=-1)[..., 0]
    assert np.all(ok[:, cov])
    gp = np.moveaxis(prob[:, idx], 0, -1)
    assert np.abs(gp - ref.prob)[:, cov].max() <= dp
    assert np.abs(ent[idx] - ref.entropy)[:, cov].max() <= E.entropy_bound(dp, 5)


def test_identical_members_equal_one_member(dev):
    XY, HW, inv = _geometry(5)
    K = pkg("kernels")
    logits = torch.from_numpy(S.smooth_plane_logits(6, *HW, 5, 70)).to(dev)
    elems, origin, strides = P.layout("c", *XY, 7)
    res = []
    for M in (1, 2, 4, 8):
        vol = torch.full((elems,), 0xAB, dtype=torch.uint8, device=dev)
        prob = torch.full((5 * elems,), -7.0, dtype=torch.float32, device=dev)
        ent = torch.full((elems,), -7.0, dtype=torch.float32, device=dev)
        K.paste_ensemble([logits] * M, 5, 1, [inv] * M, XY, vol, origin, strides, prob=prob, entropy=ent, fov=True)
        res.append((vol, prob, ent))
    for vol, prob, ent in res[1:]:
        assert torch.equal(vol, res[0][0]) and torch.equal(prob.view(torch.int32), res[0][1].view(torch.int32))
        assert torch.equal(ent.view(torch.int32), res[0][2].view(torch.int32))
    # M = 1 agrees with pnp_paste_labels_fov on what is written, and where
    lab = torch.full((elems,), 0xAB, dtype=torch.uint8, device=dev)
    K.paste_labels(logits, 5, 1, inv, XY, lab, origin, strides, fov=True)
    assert torch.equal(lab == 0xAB, res[0][0] == 0xAB) and float((lab != res[0][0]).float().mean()) < 0.01


# ---- 7. the whole path with a stub network -------------------------------------------------------------------------------------------------
def _stub(ncls=5, favourite=None):
    """logits from the three channels and the pixel position: deterministic torch arithmetic, the same for equal inputs"""
    def fn(x):
        Bn, H, W, _ = x.shape
        i = torch.arange(H, device=x.device, dtype=torch.float32).view(1, H, 1)
        j = torch.arange(W, device=x.device, dtype=torch.float32).view(1, 1, W)
        out = torch.stack([x[..., 0] * (0.5 + c) - x[..., 1] * (0.3 * c) + x[..., 2] * 0.7 + torch.sin(0.4 * i * (c + 1) + 0.3 * j) for c in range(ncls)], dim=-1)
        if favourite is not None:
            out[..., favourite] += 100.0
        return out.contiguous()
    return fn


def _scan(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (400 * np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + 0.5 * g[2] ** 2)) + 60 * rng.standard_normal(shape)).astype(np.int16)


@pytest.mark.parametrize("edge", ["replicate", "skip"])
def test_identity_case_is_the_default_path_bit_for_bit(dev, edge):
    vp = pkg("volume_predict")
    image = _scan((16, 12, 6), 1)
    common = dict(edge=edge, batch_size=4, out_size=(16, 12), device=dev)
    stats = []
    want = vp.segment_volume(_stub(), image, **common)
    got = vp.segment_volume(_stub(), image, spacing=(1.0, 1.0, 1.0), sample_mm=1.0, fov_stats=stats, **common)
    assert torch.equal(got, want) and len(torch.unique(want)) > 1 and stats == [1.0]
    # anisotropic voxels sampled at their own size, another axis and crop: still the default path
    opts = dict(axis=0, crop=((1, 11), (2, 6), (0, 16)), edge=edge, batch_size=3, out_size=(10, 4), device=dev)
    want = vp.segment_volume(_stub(), image, **opts)
    got = vp.segment_volume(_stub(), image, spacing=(2.5, 0.4, 0.9), sample_mm=(0.4, 0.9, 2.5), **opts)
    assert torch.equal(got, want) and bool(want.any())
    # the ensemble path: two exact views, probabilities and entropy
    ens = dict(tta=[{}, {"flip": True}], prob=True, entropy=True)
    want = vp.segment_volume(_stub(), image, **common, **ens)
    got = vp.segment_volume(_stub(), image, spacing=(1.0, 1.0, 1.0), sample_mm=1.0, **common, **ens)
    assert torch.equal(got.label, want.label) and torch.equal(got.prob.view(torch.int32), want.prob.view(torch.int32))
    assert torch.equal(got.entropy.view(torch.int32), want.entropy.view(torch.int32)) and float(want.prob.sum()) > 0


def test_voxels_outside_the_field_of_view_stay_zero(dev):
    """a 48 x 40 scan at 0.5 mm under a 16 x 16 plane of 1 mm pixels: 16 of 24 x 20 mm are seen.  The stub always answers class 3, so
    the label volume is 3 inside the field of view and 0 outside it, exactly."""
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    image = _scan((48, 40, 4), 2)
    stats = []
    res = vp.segment_volume(_stub(favourite=3), image, spacing=(0.5, 0.5, 2.0), sample_mm=(1.0, 1.0, 2.0), out_size=(16, 16), batch_size=3,
                            device=dev, prob=True, entropy=True, fov_stats=stats)
    inv = vp.invert_matrix(vs.compose_matrix((48, 40), (16, 16), spacing_xy=(0.5, 0.5), pixel_mm=(1.0, 1.0)))
    assert S.border_margin(inv, 48, 40, 16, 16) >= 1e-3
    cov = S.covered(inv, 48, 40, 16, 16)
    assert stats == [cov.mean()] and 0.2 < stats[0] < 0.6
    # the plan of this request knows both before anything runs
    req = vp.parse_request(spacing=(0.5, 0.5, 2.0), sample_mm=(1.0, 1.0, 2.0), out_size=(16, 16), batch_size=3, prob=True, entropy=True)
    plan = vp.plan_view(req, image.shape, 2, ((0, 48), (0, 40), (0, 4)), (0.5, 0.5, 2.0))
    assert len(plan.invs) == 1 and np.array_equal(plan.invs[0], inv) and plan.coverage == stats[0] and plan.frames == (0, 4, 0) and not plan.padded
    cov_file = np.flip(np.flip(cov, 0), 1)[:, :, None]                       # slicing order -> the file's (the double flip)
    label, prob, ent = res.label.cpu().numpy(), res.prob.cpu().numpy(), res.entropy.cpu().numpy()
    assert np.array_equal(label, np.where(cov_file, 3, 0) * np.ones((1, 1, 4), np.uint8))
    assert np.all(prob.sum(axis=0)[np.broadcast_to(cov_file, label.shape)] > 0.999) and not prob[:, ~np.broadcast_to(cov_file, label.shape)].any()
    assert not ent[~np.broadcast_to(cov_file, label.shape)].any()
    # the label path alone
    lab = vp.segment_volume(_stub(favourite=3), image, spacing=(0.5, 0.5, 2.0), sample_mm=(1.0, 1.0, 2.0), out_size=(16, 16), batch_size=3, device=dev)
    assert np.array_equal(lab.cpu().numpy(), label)
    # a single frame is enough in this mode
    one = vp.segment_volume(_stub(favourite=2), image[:, :, :1], spacing=(0.5, 0.5, 2.0), sample_mm=1.0, out_size=(16, 16), batch_size=3, device=dev)
    assert np.array_equal(one.cpu().numpy(), np.where(cov_file, 2, 0).astype(np.uint8))


# ---- 8. end to end through the command lines -------------------------------------------------------------------------------------------------
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
    tr = ts.main(["--nii-train", str(tmp_path / "train_list"), "--nii-val", str(tmp_path / "val_list"), "--sample-mm", "1.5", "--batch-size", "2",
                  "--iters", "2", "--epochs", "1", "--output", out])
    assert tr.train_list.sample_mm == (1.5, 1.5, 1.5) == tr.val_list.sample_mm
    assert np.allclose(tr.train_list.volumes.spacings, [(0.6, 0.9, 2.0)] * 2, rtol=1e-6, atol=0)      # the header keeps float32 zooms
    assert tr.train_list.last_params.dtype.itemsize == 36 and np.all(tr.train_list.last_params["dz"] == np.float32(0.75))
    assert tr.train_list.errors() == 0 and tr.val_list.errors() == 0 and np.isfinite(tr.loss_dict["train"][1])
    ckpt = os.path.join(out, "checkpoint.npz")
    assert os.path.exists(ckpt)
    image = str(tmp_path / "s0_image.nii.gz")
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", image, "--out", str(tmp_path / "pred"), "--batch-size", "2", "--sample-mm", "1.0"])
    got, src = nifti.load(res["paths"][0]), nifti.load(image)
    assert res["paths"] == [str(tmp_path / "pred" / "pred_s0_image.nii.gz")]
    assert got.shape == src.shape == (48, 40, 5) and got.get_data().dtype == np.uint8 and np.allclose(got.affine, aff) and got.get_data().max() < 5
