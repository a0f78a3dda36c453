"""-m gpu: tiled whole-scan inference (volume_predict.segment_volume(tiles=)) end to end — a scan wider than the plane is
covered by overlapping planes, the label, probability and entropy volumes are tiles_ref driven through the same plan (the logits of
every member captured as the device produced them), the result agrees with the untiled one inside the single plane's field of view, and
the option reaches Trainer.predict_volumes and the predict command line.

The scan is 40 x 36 x 5 voxels of 0.5 mm under 16 x 16 planes of 1 mm pixels: 20 x 18 mm against 16 mm, two planes per axis whose centres
lie whole pixels from the box's centre, so every plane samples the same millimetre grid.  The logits_fn is pointwise (the classes are
bands of the centre channel's intensity): a grid point has the same logits in whichever plane it lies, up to the gather's rounding.

Where the tiled result must equal the untiled one: inside the single plane's field of view, at the columns that every plane covering
them — and the single plane — INTERPOLATES.  In the outer half pixel of a plane (coordinates in [-0.5, 0) or (n - 1, n - 0.5]) the
kernel's clamp replicates the plane's edge pixel instead, by contract, and the window gives that value the weight 0.5 / ramp
and not 0: there a covering plane contributes other logits than the single plane reads, and the blend may differ from the untiled label
with a clear maximum (58 of the 1200 voxels there did when this was written).  In that zone the assertion is weaker, not absent: where
the single plane itself interpolates, the tiled probabilities differ from the untiled ones by at most lambda, the share of the column's
weight that the clamping planes carry (every softmax lies in [0, 1]), so the label may differ only where the untiled top-2 gap is at most
2 lambda + 2 delta_p.  Only in the single plane's OWN outer half pixel (the rim of its field of view, 124 of 1024 columns), where the
untiled path is the one that replicates, nothing ties the two, and differences are counted and printed (54 of the 58).  Everywhere else the labels are
equal but for top-2 gaps under the bound, which are held to the 5 % cap."""
import os

import numpy as np
import pytest
import torch

import ensemble_ref as E
import tiles_ref as T
from conftest import pkg
from test_gpu_volume_predict import COST, _random_state, _to_slicing

pytestmark = pytest.mark.gpu

XYZ, VOX, HW, MM = (40, 36, 5), 0.5, (16, 16), 1.0
CENTRES = (-1.2, -0.4, 0.2, 0.9, 1.8)


def _scan(shape, seed):
    """smooth blobs over a little noise (int16, slicing order of `shape`)"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    v = 400 * np.exp(-3 * (g[0] ** 2 + g[1] ** 2 + 0.5 * g[2] ** 2)) + 150 * np.sin(4 * g[0] + g[2]) * np.cos(3 * g[1]) + 10 * rng.standard_normal(shape)
    return v.astype(np.int16)


def _bands(captured=None):
    """pointwise logits: class c answers -4 (v - CENTRES[c])^2 of the centre channel"""
    def fn(x):
        c = torch.tensor(CENTRES, device=x.device, dtype=torch.float32).view(1, 1, 1, -1)
        out = (-4.0 * (x[..., 1:2] - c) ** 2).contiguous()
        if captured is not None:
            captured.append(out.detach().clone())
        return out
    return fn


def _plan(entries=({},), tiles="auto", overlap=0.25):
    """the maps of the box XYZ, built by hand: (inverse maps in member order for one callable, ramp, counts) — and held equal to the plan
    that segment_volume runs (parse_request + plan_view), so the restatement below is driven through the maps the device got"""
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    (X, Y), (H, W) = XYZ[:2], HW
    extent, plane = (X * VOX, Y * VOX), (H * MM, W * MM)
    offs, counts = vp.tile_plan(extent, plane, tiles, overlap)
    ramp = vp.tile_ramp(extent, plane, counts, (MM, MM))
    invs = []
    for ti, tj in offs:
        for e in entries:
            t = e.get("translate", (0.0, 0.0))
            invs.append(vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), **dict(e, translate=(t[0] + ti, t[1] + tj)), spacing_xy=(VOX, VOX), pixel_mm=(MM, MM))))
    req = vp.parse_request(tta=list(entries), tiles=tiles, tile_overlap=overlap, out_size=HW, spacing=_spacing(2), sample_mm=MM)
    plan = vp.plan_view(req, XYZ, 2, tuple((0, n) for n in XYZ), _spacing(2))
    assert plan.counts == counts and plan.ramp == ramp and plan.kind == "tiles" and plan.members == len(invs)
    assert all(np.array_equal(a, b) for a, b in zip(plan.invs, invs))
    return invs, ramp, counts


def _clamp_zone(invs, X, Y, H, W):
    """[M, X, Y] bool: the columns that map m covers with a coordinate in the outer half pixel of its plane, where the clamp replicates
    the edge pixel"""
    import paste_ref as R
    out = []
    for inv, cov in zip(invs, T.member_covers(invs, X, Y, H, W)):
        pi, pj = R.coords(inv, X, Y)
        out.append(cov & ((pi < 0) | (pi > H - 1) | (pj < 0) | (pj > W - 1)))
    return np.stack(out)


def _file(image_s, axis, flip):
    """the file array whose slicing order is image_s"""
    a = np.moveaxis(image_s, -1, axis)
    return np.ascontiguousarray(np.flip(np.flip(a, 0), 1) if flip else a)


def _spacing(axis):
    sp = [VOX, VOX]
    sp.insert(axis, 2.0)
    return tuple(sp)


@pytest.mark.parametrize("axis,flip,B", [(2, True, 2), (0, False, 4)], ids=["z-fastest", "slicing-axis-first-unflipped"])
def test_tiled_volume_against_the_restatement_and_the_untiled_path(dev, axis, flip, B):
    vp = pkg("volume_predict")
    X, Y, Z = XYZ
    H, W = HW
    image = _file(_scan(XYZ, 3), axis, flip)
    common = dict(flip_correction=flip, axis=axis, batch_size=B, out_size=HW, device=dev, spacing=_spacing(axis), sample_mm=(MM, MM, 2.0))
    # untiled: part of the box is lost, and the rim stays 0
    stats = []
    untiled = []
    plain = vp.segment_volume(_bands(untiled), image, fov_stats=stats, **common)
    plain_s = _to_slicing(plain.cpu().numpy(), flip, axis)
    single_inv = vp.invert_matrix(pkg("volume_source").compose_matrix((X, Y), HW, spacing_xy=(VOX, VOX), pixel_mm=(MM, MM)))
    single = T.member_covers([single_inv], X, Y, H, W)[0]
    assert stats[0] == single.mean() and 0.5 < stats[0] < 1.0 and not plain_s[~single].any() and plain_s[single].any()
    # tiled
    captured, stats = [], []
    res = vp.segment_volume(_bands(captured), image, tiles="auto", prob=True, entropy=True, fov_stats=stats, **common)
    invs, ramp, counts = _plan()
    assert counts == (2, 2) and ramp == 12.0 and stats == [1.0] and len(captured) == 4 * -(-Z // B)
    lab_s = _to_slicing(res.label.cpu().numpy(), flip, axis)
    prob_s = np.stack([_to_slicing(p, flip, axis) for p in res.prob.cpu().numpy()], axis=-1).astype(np.float64)       # [X, Y, Z, ncls]
    ent_s = _to_slicing(res.entropy.cpu().numpy(), flip, axis).astype(np.float64)
    assert T.edge_columns(invs, X, Y, H, W).mean() == 0.0
    zone = _clamp_zone(invs + [single_inv], X, Y, H, W)
    own, clamped = zone[-1], zone.any(axis=0)                # the single plane's own outer half pixel; any plane's
    near = total = bad = differ = outer = rim = 0
    for k in range(0, Z, B):
        nb = min(B, Z - k)
        logits = [t.cpu().numpy() for t in captured[4 * (k // B):4 * (k // B) + 4]]
        ref = T.tiles(logits, invs, X, Y, ramp, nb)
        assert ref.covered.all() and set(np.unique((ref.weights > 0).sum(0)).tolist()) == {1, 2, 4}
        dp = T.delta_p_tiles(logits, invs, X, Y, nb)
        mine = np.moveaxis(lab_s[:, :, k:k + nb], 2, 0)
        P = np.moveaxis(prob_s[:, :, k:k + nb], 2, 0)
        Hn = np.moveaxis(ent_s[:, :, k:k + nb], 2, 0)
        ok = np.take_along_axis(E.admissible(ref.prob, dp), mine[..., None].astype(np.int64), axis=-1)[..., 0]
        bad += int((~ok).sum())
        differ += int((mine != ref.label).sum())
        err, herr = float(np.abs(P - ref.prob).max()), float(np.abs(Hn - ref.entropy).max())
        print("frames %d..%d: max|dP| %.3g (bound %.3g), max|dH| %.3g (bound %.3g)" % (k, k + nb - 1, err, dp, herr, E.entropy_bound(dp, 5)))
        assert err <= dp and herr <= E.entropy_bound(dp, 5) and np.abs(P.sum(-1) - 1.0).max() <= 5 * 2.0 ** -23
        # inside the single plane's field of view: the untiled label, but for the voxels whose reference top-2 gap is under the bound
        top = np.sort(ref.prob, axis=-1)
        tied = (top[..., -1] - top[..., -2] <= 2.0 * dp)[:, single]
        same = (mine == np.moveaxis(plain_s[:, :, k:k + nb], 2, 0))[:, single]
        edge = np.broadcast_to(clamped[single][None], same.shape)
        # in the zone: |P - P_untiled| <= lambda, the weight share of the planes that clamp there (not where the single plane clamps itself)
        lam = ((ref.weights * zone[:-1]).sum(axis=0) / ref.weights.sum(axis=0))[single]
        P0 = np.sort(E.softmax(E.member_logits([untiled[k // B].cpu().numpy()], [single_inv], X, Y, nb)[0]), axis=-1)
        loose = ((P0[..., -1] - P0[..., -2])[:, single] <= 2.0 * lam[None] + 2.0 * dp) | np.broadcast_to(own[single][None], same.shape)
        assert np.all(same | tied | (edge & loose)), "%d voxels differ from the untiled path with a clear maximum" % int((~same & ~tied & ~(edge & loose)).sum())
        rim += int((~same & ~tied & np.broadcast_to(own[single][None], same.shape)).sum())
        near += int((tied & ~edge).sum())
        total += int((~edge).sum())
        outer += int((~same & ~tied & edge).sum())
    print("%d of %d labels differ from the float64 argmax, %d outside the bound; inside the single plane: %d of %d interpolated voxels with a top-2 gap "
          "under the bound; %d columns of %d in a plane's outer half pixel, %d voxels there differ from the untiled label with a clear maximum "
          "(all within the weight share of the clamping planes, but for %d in the single plane's own outer half pixel)"
          % (differ, X * Y * Z, bad, near, total, int(clamped[single].sum()), int(single.sum()), outer, rim))
    assert bad == 0 and near <= 0.05 * total and clamped[single].mean() <= 0.25
    assert (lab_s[~single] != 0).any() and len(np.unique(lab_s)) >= 3
    # the same plan given explicitly
    again = vp.segment_volume(_bands(), image, tiles=(2, 2), prob=True, entropy=True, **common)
    assert torch.equal(again.label, res.label) and torch.equal(again.prob, res.prob) and torch.equal(again.entropy, res.entropy)


def test_tiles_with_views_and_the_component_filter(dev):
    """2 x 2 tiles x 2 views = 8 members, keep_largest=1: the label is the filter applied to the unfiltered tiled label, prob is unchanged"""
    vp, comp = pkg("volume_predict"), pkg("components")
    image = _file(_scan(XYZ, 4), 2, True)
    common = dict(batch_size=3, out_size=HW, device=dev, spacing=_spacing(2), sample_mm=MM, tiles="auto", tta=[{}, {"flip": True}], prob=True)
    captured, stats = [], []
    raw = vp.segment_volume(_bands(captured), image, fov_stats=stats, **common)
    assert len(captured) == 8 * 2 and stats == [1.0] and raw.entropy is None
    kept = vp.segment_volume(_bands(), image, keep_largest=1, **common)
    want, _ = comp.keep_largest(raw.label.clone(), num_cls=5, keep=1)
    assert torch.equal(kept.label, want) and torch.equal(kept.prob, raw.prob) and not torch.equal(kept.label, raw.label)
    # the members are tile-major, then view: against the restatement on the first batch
    invs, ramp, _ = _plan(entries=({}, {"flip": True}))
    X, Y, _ = XYZ
    logits = [t.cpu().numpy() for t in captured[:8]]
    ref = T.tiles(logits, invs, X, Y, ramp, 3)
    dp = T.delta_p_tiles(logits, invs, X, Y, 3)
    mine = np.moveaxis(_to_slicing(raw.label.cpu().numpy(), True, 2)[:, :, :3], 2, 0)
    assert np.take_along_axis(E.admissible(ref.prob, dp), mine[..., None].astype(np.int64), axis=-1).all()


def test_keyword_errors(dev):
    vp = pkg("volume_predict")
    image = _file(_scan(XYZ, 5), 2, True)
    with pytest.raises(ValueError, match="tiles needs sample_mm"):
        vp.segment_volume(_bands(), image, tiles="auto", out_size=HW, device=dev)
    with pytest.raises(ValueError, match="cannot cover"):
        vp.segment_volume(_bands(), image, tiles=(1, 2), out_size=HW, device=dev, spacing=_spacing(2), sample_mm=MM)
    with pytest.raises(ValueError, match="at most 64"):
        vp.segment_volume([_bands()] * 4, image, tiles=(3, 3), tta=[{}, {"flip": True}], out_size=HW, device=dev, spacing=_spacing(2), sample_mm=MM)


def test_trainer_method_and_command_line(dev, tmp_path):
    """a 70 x 66 x 2 scan of 4 mm voxels is 280 x 264 mm against the network's 256 mm plane: untiled the rim stays 0, with tiles="auto" it
    is labelled — through Trainer.predict_volumes and through `predict --sample-mm 1.0 --tiles auto`, which agree"""
    ss, nifti, pr, vp = pkg("source_segmenter"), pkg("nifti"), pkg("predict"), pkg("volume_predict")
    seg = _random_state(ss.Full_DRN(channels=3, n_class=5, batch_size=2, device=dev, seed=0, cost_kwargs=dict(COST)), 5, vp.segmenter_logits)
    a = str(tmp_path / "wide.nii.gz")
    nifti.save(nifti.Nifti1Image(_scan((70, 66, 2), 6), np.diag([4.0, 4.0, 4.0, 1.0])), a)
    tr = ss.Trainer(seg, train_list=[], val_list=[], num_cls=5, batch_size=2)
    plain = nifti.load(tr.predict_volumes([a], str(tmp_path / "plain"), sample_mm=1.0)[0]).get_data()
    tiled = nifti.load(tr.predict_volumes([a], str(tmp_path / "tiled"), sample_mm=1.0, tiles="auto")[0]).get_data()
    rim = np.ones((70, 66, 2), bool)
    rim[3:-3, 1:-1] = False                                   # 12 mm = 3 voxels and 4 mm = 1 voxel on either side lie outside the centred plane
    assert tiled.shape == plain.shape == (70, 66, 2) and tiled.dtype == np.uint8 and tiled.max() < 5
    assert not plain[rim].any() and plain.any() and tiled[rim].any()
    ckpt = seg.save(str(tmp_path / "ckpt.npz"))
    ckpt = ckpt if isinstance(ckpt, str) and os.path.isfile(ckpt) else str(tmp_path / "ckpt.npz")
    res = pr.main(["--model", ckpt, "--net", "segmenter", "--images", a, "--out", str(tmp_path / "cli"), "--batch-size", "2", "--sample-mm", "1.0",
                   "--tiles", "auto"])
    assert np.array_equal(nifti.load(res["paths"][0]).get_data(), tiled)
