"""Inference of whole NIfTI volumes onto their own grid: image.nii.gz in, label volume of the same shape and axis order
out.  Unlike Trainer.test_eval (volume_eval.py, kept quirk for quirk from the reference) it takes any in-plane size, needs no ground
truth, predicts every frame and keeps the volume on the device from upload to the finished label volume.

  segment_volume(logits_fn, image, ...)   one volume: orientation and crop like volume_source.prepare_pair, pnp_volume_preprocess, then per
                                          batch of ascending frames the gather (pnp_aug_slices with the un-augmented compose_matrix map),
                                          logits_fn, and pnp_paste_labels with the inverse map straight into the file's array order
  invert_matrix(m)                        the inverse of a compose_matrix map: source voxel (x, y) -> output-plane coordinates
  segmenter_logits / adapted_logits       the logits_fn of source_segmenter.Full_DRN and of the CT path of adversarial.Full_DRN
  predict_volumes(...)                    files in, pred_<basename> files out (what both trainers' predict_volumes call)

The label of a voxel is the argmax of the bilinearly interpolated LOGITS (not probabilities): no exp, and for an identity map exactly
argmax(logits).

Ensemble inference (opt-in): with a list of callables (checkpoints), tta= (views of the same slice) or prob= / entropy=,
segment_volume gathers once per distinct map, runs one forward per member and makes ONE pnp_paste_ensemble launch per batch, which
interpolates every member's logits through that member's own inverse map, averages the softmax and writes the label, the mean
probabilities and the normalised entropy in the file's array order.  With the defaults nothing of this is reached.

Hole filling (opt-in): fill_holes= runs components.fill_holes on the finished label volume, on the device, after keep_largest.
Connected-component filtering (opt-in): keep_largest= runs components.keep_largest on the finished label volume, on the
device, before it is returned.

Millimetre grid (opt-in): with sample_mm= the plane has a fixed pixel size and is centred on the (cropped) volume, the
outer channels lie frame_mm from the centre frame (pnp_aug_slices_z; its clamp is the edge replication, so nothing is padded) and the
paste writes only the voxel columns inside the plane's field of view (pnp_paste_labels_fov / pnp_paste_ensemble_fov); the rest stays 0.

Anti-alias prefilter (opt-in): with prefilter= the normalised box is low-passed on the device (pnp_volume_smooth) before
anything samples it, with volume_source.prefilter_sigmas' rule — the setting the network was trained with.

Tiles (opt-in, needs sample_mm): with tiles= the crop box is covered by several overlapping planes of the same millimetre
grid (tile_plan), every plane is predicted, and ONE pnp_paste_tiles launch per batch blends them over their union with a window that
trusts a plane's centre more than its border.  Without the option nothing of this is reached.

Multi-planar fusion (opt-in): with axes= the scan is predicted once per listed slicing axis by the single-axis path above
(every other option applies to each view), and ONE pnp_fuse_views launch averages the views' probability volumes over the views that
cover a voxel (check_axes, view_box, fuse_views).  Without the option nothing of this is reached.
"""
import collections
import logging
import math
import os

import numpy as np

from . import _lib
from .volume_source import (SAMPLE_DTYPE, SAMPLE_Z_DTYPE, AugmentedSliceSource, VolumeSet, check_axes, check_prefilter, check_sample_mm,
                            check_spacing, compose_matrix, gaussian_weights, label_bounding_box, prefilter_sigmas, prepare_pair, slicing_order)

EDGES = ("replicate", "skip")
MAX_MEMBERS = 8                          # pnp_paste_ensemble's
MAX_TILE_MEMBERS = 64                    # pnp_paste_tiles'
TTA_KEYS = ("rotate", "scale", "translate", "flip")      # compose_matrix's keywords
DEFAULT_TTA = ({}, {"rotate": 7.5}, {"rotate": -7.5}, {"scale": 0.95}, {"scale": 1.05})
Ensemble = collections.namedtuple("Ensemble", ("label", "prob", "entropy"))


def invert_matrix(m, dtype=np.float32):
    """six float32 entries (m00, m01, m02, m10, m11, m12) of s = A p + t  ->  the six entries of p = A^-1 s - A^-1 t, inverted in float64
    and rounded once to `dtype` (float32: what the kernel gets; float64: unrounded).  The identity, quarter turns and the flip of a square
    slice come back as exact 0 / +-1 entries."""
    a00, a01, t0, a10, a11, t1 = (float(v) for v in np.asarray(m, dtype=np.float32).astype(np.float64))
    det = a00 * a11 - a01 * a10
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("invert_matrix: the map %r is singular" % (list(m),))
    b00, b01, b10, b11 = a11 / det, -a01 / det, -a10 / det, a00 / det
    out = np.array([b00, b01, -(b00 * t0 + b01 * t1), b10, b11, -(b10 * t0 + b11 * t1)], dtype=np.float64) + 0.0      # (-0.0 -> 0.0)
    return out.astype(dtype)


def coverage(inv, X, Y, H, W, mode="all"):
    """the share of the X * Y voxel columns that lie inside the field of view of EVERY given map (mode="all": pnp_paste_*_fov's columns)
    or of AT LEAST ONE of them (mode="any": pnp_paste_tiles' columns); inv: six entries, or a list of such.  The rule — unclamped plane
    coordinates in [-0.5, H - 0.5] x [-0.5, W - 0.5] — is evaluated in float64 on the host from the float32 entries the kernel gets"""
    if mode not in ("all", "any"):
        raise ValueError("coverage: mode must be 'all' or 'any', got %r" % (mode,))
    maps = np.asarray(inv, dtype=np.float32).astype(np.float64).reshape(-1, 6)
    x = np.arange(int(X), dtype=np.float64)[:, None]
    y = np.arange(int(Y), dtype=np.float64)[None, :]
    ok = np.full((int(X), int(Y)), mode == "all", dtype=bool)
    for m in maps:
        pi, pj = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        inside = (pi >= -0.5) & (pi <= H - 0.5) & (pj >= -0.5) & (pj <= W - 0.5)
        ok = ok & inside if mode == "all" else ok | inside
    return float(ok.mean())


def check_tiles(tiles):
    """None, "auto" or (ni, nj) with both counts >= 1 -> None / "auto" / a pair of ints; anything else is a ValueError"""
    if tiles is None or (isinstance(tiles, str) and tiles == "auto"):
        return tiles
    try:
        t = tuple(tiles)
        ok = not isinstance(tiles, str) and len(t) == 2 and all(isinstance(n, (int, np.integer)) and not isinstance(n, bool) and n >= 1 for n in t)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("tiles must be None, 'auto' or (ni, nj) with counts >= 1, got %r" % (tiles,))
    return int(t[0]), int(t[1])


def _axis_overlap_mm(L, F, n):
    """what two neighbouring planes of extent F share when n of them, evenly spaced, lie flush in a box of extent L (n > 1)"""
    return F - (L - F) / (n - 1)


def tile_plan(extent_mm, fov_mm, tiles="auto", overlap=0.25):
    """-> (offsets_mm, (ni, nj)): the planes that cover a box of extent_mm = (Li, Lj) with a field of view of fov_mm = (Fi, Fj) each.
    Per in-plane axis n = 1 if L <= F, else ceil((L - o) / (F - o)) with o = overlap * F (overlap in [0, 0.5]: the least share of a plane
    that its neighbour repeats); tiles = (ni, nj) overrides both counts.  The centres are evenly spaced, the first and the last plane lie
    flush with the box's edges, a single plane is centred.  offsets_mm lists (ti, tj), the plane centres relative to the box's centre in
    millimetres, tile-major (i outer, j inner): what is added to compose_matrix's `translate`.  ValueError: an overlap outside [0, 0.5],
    extents that are not positive and finite, counts with n * F < L (they cannot cover the box)."""
    tiles = check_tiles(tiles)
    if tiles is None:
        raise ValueError("tile_plan: tiles must be 'auto' or (ni, nj)")
    overlap = float(overlap)
    if not 0.0 <= overlap <= 0.5:
        raise ValueError("tile overlap %r outside [0, 0.5]" % (overlap,))
    L, F = tuple(float(v) for v in extent_mm), tuple(float(v) for v in fov_mm)
    if len(L) != 2 or len(F) != 2 or not all(0.0 < v < math.inf for v in L + F):
        raise ValueError("tile_plan: extent_mm %r and fov_mm %r must be two positive finite numbers each" % (extent_mm, fov_mm))
    counts, centres = [], []
    for a in range(2):
        if tiles == "auto":
            o = overlap * F[a]
            n = 1 if L[a] <= F[a] else int(math.ceil((L[a] - o) / (F[a] - o)))
        else:
            n = tiles[a]
            if n * F[a] < L[a]:
                raise ValueError("tiles: %d planes of %g mm cannot cover %g mm along axis %d" % (n, F[a], L[a], a))
        counts.append(n)
        centres.append([0.0] if n == 1 else [(L[a] - F[a]) * (k / (n - 1.0) - 0.5) for k in range(n)])
    return [(ti, tj) for ti in centres[0] for tj in centres[1]], (counts[0], counts[1])


def tile_ramp(extent_mm, fov_mm, counts, pixel_mm):
    """the window's rise in plane pixels for tile_plan's planes: max(1, the overlap of two neighbouring planes in plane pixels), the
    smallest over the axes that have more than one plane; 1 if none has (or if neighbours only abut)"""
    over = [_axis_overlap_mm(float(L), float(F), int(n)) / float(p) for L, F, n, p in zip(extent_mm, fov_mm, counts, pixel_mm) if n > 1]
    return max(1.0, min(over)) if over else 1.0


def file_layout(shape, flip_correction=True, axis=2, box=None):
    """where voxel (x, y, z) of the slicing order (double flip, `axis` moved last, optional box ((x0, x1), (y0, y1), (z0, z1))) lies in
    the C-order array of the file's `shape`: (origin, (sx, sy, sz), (X, Y, Z)) in elements.  Taken from the strides numpy itself gives the
    view that prepare_pair builds, so the two cannot disagree."""
    probe = np.empty(tuple(int(n) for n in shape), dtype=np.uint8)          # never touched: only its address arithmetic is used
    v = probe
    if flip_correction:
        v = np.flip(np.flip(v, axis=0), axis=1)
    v = np.moveaxis(v, axis, -1)
    if box is not None:
        v = v[tuple(slice(int(a), int(b)) for a, b in box)]
    origin = v.__array_interface__["data"][0] - probe.__array_interface__["data"][0]
    return int(origin), tuple(int(s) for s in v.strides), tuple(int(n) for n in v.shape)


def _box_of(crop, label, dims):
    if crop is None:
        return tuple((0, n) for n in dims)
    if isinstance(crop, (int, np.integer)):
        if label is None:
            raise ValueError("crop=%d is a margin around the label's bounding box: a label is needed" % crop)
        if crop < 0:
            raise ValueError("crop margin %d is negative" % crop)
        return tuple((s.start, s.stop) for s in label_bounding_box(label, int(crop)))
    box = tuple((int(a), int(b)) for a, b in crop)
    if len(box) != 3 or any(not 0 <= a < b <= n for (a, b), n in zip(box, dims)):
        raise ValueError("crop box %r does not lie inside the volume %r (slicing order, half-open)" % (crop, tuple(dims)))
    return box


def view_box(box, axis):
    """an explicit crop box ((x0, x1), (y0, y1), (z0, z1)) given in the slicing order of the default axis (2: the array's own order after
    the flips) -> the same voxel set in the slicing order of `axis`: the ranges permuted as prepare_pair's moveaxis(axis, -1) permutes
    the array's axes"""
    if axis not in (0, 1, 2):
        raise ValueError("view_box: axis %r is not one of 0, 1, 2" % (axis,))
    b = [(int(lo), int(hi)) for lo, hi in box]
    if len(b) != 3:
        raise ValueError("crop box %r: three ranges expected" % (box,))
    return tuple(b[:axis] + b[axis + 1:] + [b[axis]])


def fuse_views(views, weights=None, prob=True, entropy=False):
    """views: the Ensemble tuples (their .prob is used) or bare probability tensors [num_cls, *shape] of several predictions of ONE scan on
    one device — segment_volume(prob=True) results for different slicing axes, or for groups of checkpoints that do not fit one call's
    member limit -> Ensemble(label, prob, entropy) by one pnp_fuse_views launch: per voxel the weighted mean over the
    views that cover it (whose probabilities are not all 0 there), its first strict maximum and its normalised entropy; a voxel that no
    view covers is 0 in all three.  weights: None or one positive finite number per view.  The inputs are left as they are; prob /
    entropy: whether those two are computed (None otherwise)."""
    from . import kernels as K
    probs = []
    for n, v in enumerate(views):
        p = v.prob if isinstance(v, Ensemble) else v
        if p is None:
            raise ValueError("fuse_views: view %d carries no probabilities (predict it with prob=True)" % n)
        probs.append(p)
    if not probs:
        raise ValueError("fuse_views: no view")
    if weights is not None:
        weights = _check_weights(weights, len(probs))
    label, p, h = K.fuse_views(probs, weights, prob=bool(prob), entropy=bool(entropy))
    return Ensemble(label, p, h)


def _check_weights(weights, n):
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError("fuse_views: weights must be %d positive finite numbers, got %r" % (n, weights))
    if len(w) != n or not all(0.0 < v < math.inf for v in w):
        raise ValueError("fuse_views: weights must be %d positive finite numbers, got %r" % (n, weights))
    return w


def tta_entries(tta):
    """None -> [{}]; "default" -> DEFAULT_TTA; a list of dicts of compose_matrix's keywords -> a list of validated copies.  Raises ValueError
    for an empty list, an entry that is no dict, unknown keys and values compose_matrix cannot take (checked here, on the host)."""
    if tta is None:
        return [{}]
    if isinstance(tta, str):
        if tta != "default":
            raise ValueError("tta: the only named set is 'default', got %r" % tta)
        return [dict(e) for e in DEFAULT_TTA]
    if isinstance(tta, dict) or not isinstance(tta, (list, tuple)):
        raise ValueError("tta must be None, 'default' or a list of dicts, got %r" % (tta,))
    if len(tta) == 0:
        raise ValueError("tta: an empty list has no member")
    out = []
    for n, e in enumerate(tta):
        if not isinstance(e, dict):
            raise ValueError("tta[%d]: a dict of %s expected, got %r" % (n, TTA_KEYS, e))
        unknown = sorted(set(e) - set(TTA_KEYS))
        if unknown:
            raise ValueError("tta[%d]: unknown keys %s (known: %s)" % (n, unknown, list(TTA_KEYS)))
        e = dict(e)
        try:
            for k in ("rotate", "scale"):
                if k in e:
                    e[k] = float(e[k])
                    if not np.isfinite(e[k]):
                        raise ValueError("%s is not finite" % k)
            if "scale" in e and not e["scale"] > 0.0:
                raise ValueError("scale must be positive")
            if "translate" in e:
                t = tuple(float(v) for v in e["translate"])
                if len(t) != 2 or not all(np.isfinite(t)):
                    raise ValueError("translate must be two finite numbers")
                e["translate"] = t
            if "flip" in e:
                if not isinstance(e["flip"], (bool, np.bool_)):
                    raise ValueError("flip must be a bool")
                e["flip"] = bool(e["flip"])
        except (TypeError, ValueError) as err:
            raise ValueError("tta[%d] = %r: %s" % (n, tta[n], err))
        out.append(e)
    return out


def ensemble_members(logits_fn, tta, limit=MAX_MEMBERS):
    """-> (callables, entries): the members are callables x entries, callable-major; more than `limit` is a ValueError"""
    fns = list(logits_fn) if isinstance(logits_fn, (list, tuple)) else [logits_fn]
    if not fns:
        raise ValueError("logits_fn: an empty list has no member")
    entries = tta_entries(tta)
    if len(fns) * len(entries) > limit:
        raise ValueError("%d callables x %d tta entries = %d members, at most %d" % (len(fns), len(entries), len(fns) * len(entries), limit))
    return fns, entries


def segment_volume(logits_fn, image, *, label=None, flip_correction=True, axis=2, crop=None, edge="replicate", batch_size=16, percentile=98,
                   out_size=(256, 256), num_cls=5, device="cuda", tta=None, prob=False, entropy=False, keep_largest=None, component_stats=None,
                   spacing=None, sample_mm=None, fov_stats=None, prefilter=None, tiles=None, tile_overlap=0.25, axes=None, axis_weights=None, crop_box=None,
                   fill_holes=None, hole_stats=None):
    """-> uint8 label volume of `image`'s shape and axis order, a device tensor (`.cpu().numpy()` is the caller's).
      logits_fn  x [B, H, W, 3] -> logits [B, H, W, num_cls] (device tensors; segmenter_logits / adapted_logits); a list of them is a
                 checkpoint ensemble
      tta        None, "default" (DEFAULT_TTA) or a list of dicts of compose_matrix's keywords: the views of every slice
      prob, entropy   also return the mean class probabilities [num_cls, *image.shape] / the entropy normalised by log(num_cls) (float32)
    With a list of callables, tta, prob or entropy the result is Ensemble(label, prob, entropy) (a field not asked for is None; outside the
    crop box all three are 0) and every batch ends in one pnp_paste_ensemble launch; with the defaults it is the label
    tensor alone, through pnp_paste_labels.
      label      optional ground truth of the same shape: only its bounding box is used (crop = a margin in voxels)
      crop       None, a margin around the label's bounding box, or a box ((x0, x1), (y0, y1), (z0, z1)) in slicing order; outside it: 0.
                 "body" or ("body", margin): the label-free body crop of DESIGN.md §24 — the prepared full volume is uploaded,
                 body.body_box finds the patient's bounding box on the device (two host synchronisations), the crop is taken on the device
                 and everything after that is the path of an explicit box: the result equals crop=<that box> bit for bit.  With axes the
                 box is found once, in the default axis's order, and handed to the views through view_box.
      crop_box   optional list: the box used, ((x0, x1), (y0, y1), (z0, z1)) in slicing order (with axes: of the default axis), is appended
      keep_largest   None, an int K (keep the K largest 3-D components of every class) or a dict of components.keep_largest's keywords
                 (keep, min_size, connectivity, classes): applied in place to the finished label volume on the device.  On
                 the ensemble path only Ensemble.label is filtered: prob and entropy are returned as computed, also where the label became 0.
      component_stats   optional list: the filter's int64 [num_cls, 4] stats tensor is appended to it
      fill_holes     None / False, True (holes of any size), a positive int (the largest hole filled, in voxels) or a dict of
                 components.fill_holes' keywords (max_size, classes): every enclosed background hole of the finished label volume takes
                 the class that touches it most, in place on the device, after keep_largest.  On the ensemble and tiles
                 paths only Ensemble.label changes; with axes it runs once, on the fused label.
      hole_stats     optional list: the fill's int64 [num_cls, 4] stats tensor is appended to it
      sample_mm  None, or a number / (pi_mm, pj_mm, frame_mm): sample on that millimetre grid.  Needs `spacing`, the voxel
                 size in mm per ARRAY axis of `image` (surface.spacing_of(affine)).  The plane is centred on the crop box; a voxel column
                 outside its field of view (for any member) stays 0 in label, prob and entropy, like outside the crop box; tta
                 entries' translate is in mm; the edge frames are replicated by the gather's clamp, nothing is padded
      fov_stats  optional list: with sample_mm the share of the box's voxel columns inside the field of view is appended (coverage)
      prefilter  None / "off", "auto" or sigmas in voxels (a number or (sx, sy, sz), slicing order): the anti-alias prefilter of DESIGN.md
                 §19.  The normalised box is smoothed in place (pnp_volume_smooth) after pnp_volume_preprocess and before the edge frames
                 are padded (the padding copies smoothed frames), with volume_source.prefilter_sigmas' sigmas from the box extents,
                 out_size, spacing and sample_mm; tta scales are ignored.  "auto" with spacing but without sample_mm is the plain resize's
                 rule.  The fill stays the unsmoothed minimum.  Use the setting the network was trained with.
      tiles      None, "auto" or (ni, nj): cover the crop box with ni x nj overlapping planes of the millimetre grid (needs
                 sample_mm) instead of the one centred plane.  tile_plan places them (tile_overlap in [0, 0.5]: the least share of a plane
                 that its neighbour repeats); every batch gathers once per (tile, view), a tile's offset added in mm to the entry's
                 translate, runs every callable on every gather and ends in ONE pnp_paste_tiles launch, which writes the columns that at
                 least one member covers and blends the covering members' softmax with a window that rises over the planes' overlap.
                 Members = callables x tiles x tta entries (in that order, callable-major), at most 64.  The result is the Ensemble tuple
                 with the ensemble path's rules for prob, entropy, keep_largest and the short last batch; fov_stats gets the share of the
                 columns that at least one member covers.  ALL members' logits of a batch are alive at once: members x 4 B H W num_cls
                 bytes — 21 MB per member at the defaults, 1.3 GB at the limit of 64 members — beside one forward's activations.  On an
                 MI355X (288 GB) no member count needs a smaller batch_size; where that product nears the free memory, halve batch_size.
      axes       None, or a sequence of distinct slicing axes from 0, 1, 2 (check_axes): multi-planar fusion.  `axis` must
                 then be left at its default.  Every listed axis is predicted by the single-axis path with prob=True and every other option
                 unchanged (tta, lists of callables, tiles, sample_mm, prefilter, edge, batch_size; the member limits hold per view), and
                 ONE pnp_fuse_views launch averages the views into the first view's probability buffer: per voxel over the views that
                 wrote it (a view leaves 0 outside its field of view, on the edge frames it skips and outside the crop box), weighted by
                 axis_weights (None: all 1).  The result is always the Ensemble tuple (prob / entropy None unless asked for);
                 keep_largest runs once, on the fused label, never on a view; fov_stats gets one share per view, in axes order.  crop: None
                 and a margin work as they are (a label's bounding box is the same voxel set in every orientation); an explicit box is
                 given in the slicing order of the default axis (2) and re-expressed per view (view_box).  sample_mm and spacing keep their
                 meaning per view (slicing_order moves each view's axis last): with an anisotropic scan a single number — an isotropic
                 grid — is the sensible sample_mm.  Peak memory is len(axes) probability volumes: 262 MB per view at 256 x 256 x 200 x 5.
      edge       "replicate": the normalised volume is padded with a copy of its first and last frame, every frame is predicted;
                 "skip": frames 1 .. Z - 2 only (the reference's frame set), the two edge frames stay 0
    Frames run in ascending order, batch_size at a time; the last, short batch repeats its last frame and pastes nb < B slices.  Nothing
    synchronises between batches; the gather's error counter is read once at the end."""
    import torch
    from . import kernels as K
    if edge not in EDGES:
        raise ValueError("edge must be one of %s, got %r" % (EDGES, edge))
    from . import components
    post = components.parse_option(keep_largest, num_cls)
    holes = components.parse_fill_option(fill_holes, num_cls)
    body_margin = _body_margin(crop)                            # None unless crop is "body" / ("body", margin)
    if axes is not None or axis_weights is not None:
        if axes is None:
            raise ValueError("axis_weights %r goes with axes" % (axis_weights,))
        if axis != 2:
            raise ValueError("axes=%r and axis=%r exclude each other: leave axis at its default" % (axes, axis))
        axes, axis_weights = check_axes(axes, axis_weights)
        if body_margin is not None:                             # found once, in the slicing order of axis 2; the views get it as a box
            full = _upload_prepared(image, flip_correction, 2, device)
            from . import body
            crop = body.body_box(full, percentile=int(percentile), margin=body_margin)
            del full
        explicit = crop is not None and not isinstance(crop, (int, np.integer))          # a box, in the slicing order of axis 2
        if crop_box is not None:
            if explicit:
                crop_box.append(tuple((int(a), int(b)) for a, b in crop))
            else:
                lab2 = None if label is None else prepare_pair(image, label, flip_correction, 2, None)[1]
                crop_box.append(_box_of(crop, lab2, file_layout(np.shape(image), flip_correction, 2)[2]))
        views = []
        for a in axes:
            one = segment_volume(logits_fn, image, label=label, flip_correction=flip_correction, axis=a,
                                 crop=view_box(crop, a) if explicit else crop, edge=edge, batch_size=batch_size, percentile=percentile,
                                 out_size=out_size, num_cls=num_cls, device=device, tta=tta, prob=True, spacing=spacing, sample_mm=sample_mm,
                                 fov_stats=fov_stats, prefilter=prefilter, tiles=tiles, tile_overlap=tile_overlap)
            views.append(one.prob)
            if len(views) == 1:
                fused = one.label                       # the first view's label buffer takes the fused labels
            del one
        _, out_p, out_e = K.fuse_views(views, axis_weights, label=fused, prob=views[0] if prob else None, entropy=bool(entropy))
        del views
        _filter_components(fused, post, num_cls, component_stats)
        _fill_holes(fused, holes, num_cls, hole_stats)
        return Ensemble(fused, out_p, out_e)
    B, H, W = int(batch_size), int(out_size[0]), int(out_size[1])
    if B < 1:
        raise ValueError("batch_size must be at least 1")
    mm = check_sample_mm(sample_mm)
    pre = check_prefilter(prefilter)
    if mm is not None:
        if spacing is None:
            raise ValueError("sample_mm needs spacing: the voxel size in mm per array axis of the image (surface.spacing_of(affine))")
        vox = slicing_order(spacing, axis, "spacing")          # as prepare_pair moves `axis` last
        geom = {"spacing_xy": vox[:2], "pixel_mm": mm[:2]}
    else:
        geom = {}
    tiles = check_tiles(tiles)
    if tiles is not None:
        if mm is None:
            raise ValueError("tiles needs sample_mm: the planes of a tiled prediction share one millimetre grid")
        if not 0.0 <= float(tile_overlap) <= 0.5:
            raise ValueError("tile overlap %r outside [0, 0.5]" % (tile_overlap,))
    ensemble = tiles is not None or isinstance(logits_fn, (list, tuple)) or tta is not None or bool(prob) or bool(entropy)
    if ensemble:
        fns, entries = ensemble_members(logits_fn, tta, MAX_MEMBERS if tiles is None else MAX_TILE_MEMBERS)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.PnpError("segment_volume: pnp kernels need a CUDA/HIP device (got %s) — there is no CPU fallback" % (device,))
    image = np.asarray(image)
    img, lab = prepare_pair(image, np.zeros(image.shape, np.uint8) if label is None else label, flip_correction, axis, None)
    full = None
    if body_margin is not None:
        from . import body
        full = torch.from_numpy(img).to(device)
        box = body.body_box(full, percentile=int(percentile), margin=body_margin)
    else:
        box = _box_of(crop, None if label is None else lab, img.shape)
    if crop_box is not None:
        crop_box.append(box)
    origin, strides, (X, Y, Z) = file_layout(image.shape, flip_correction, axis, box)
    if edge == "skip" and Z < 3:
        raise ValueError("edge='skip' needs at least 3 frames, the box has %d" % Z)
    ramp = None
    if tiles is not None:                               # the plan, before any device work: tile-major, then view
        extent, plane_mm = (X * vox[0], Y * vox[1]), (H * mm[0], W * mm[1])
        offsets, counts = tile_plan(extent, plane_mm, tiles, tile_overlap)
        if len(fns) * len(offsets) * len(entries) > MAX_TILE_MEMBERS:
            raise ValueError("%d callables x %d x %d tiles x %d tta entries = %d members, at most %d" % (
                len(fns), counts[0], counts[1], len(entries), len(fns) * len(offsets) * len(entries), MAX_TILE_MEMBERS))
        ramp = tile_ramp(extent, plane_mm, counts, mm[:2])
        shifted = []
        for ti, tj in offsets:
            for e in entries:
                t = e.get("translate", (0.0, 0.0))
                shifted.append(dict(e, translate=(t[0] + ti, t[1] + tj)))
        entries = shifted
    out = torch.zeros(tuple(image.shape), dtype=torch.uint8, device=device)

    if full is not None:                                # the body crop, taken on the device
        v = full[tuple(slice(a, b) for a, b in box)].contiguous()
        del full
    else:
        v = torch.from_numpy(np.ascontiguousarray(img[tuple(slice(a, b) for a, b in box)])).to(device)
    _, stats = K.volume_preprocess(v, int(percentile), out=v)
    fill = float(stats[3].item())                       # the one read before the loop: the fill enters the gather's descriptor table
    if pre is not None:
        taps = [gaussian_weights(s) for s in prefilter_sigmas(pre, (X, Y, Z), (H, W), vox if mm is not None else None, mm)]
        if any(t is not None for t in taps):
            K.volume_smooth(v, taps, out=v)
            K.drop_workspace("smooth")
    if mm is not None:
        first, count, shift = (0, Z, 0) if edge == "replicate" else (1, Z - 2, 0)       # pnp_aug_slices_z clamps: its own replication
    elif edge == "replicate":
        v = torch.cat([v[:, :, :1], v, v[:, :, -1:]], dim=2).contiguous()          # statistics: of the unpadded volume, above
        first, count, shift = 1, Z, -1                  # centre frames 1 .. Z of the padded volume are output frames 0 .. Z - 1
    else:
        first, count, shift = 1, Z - 2, 0
    vs = VolumeSet.from_device([v], [torch.zeros(tuple(v.shape), dtype=torch.uint8, device=device)], ["volume"], [fill], percentile,
                               min_frames=3 if mm is None else 1)
    src = AugmentedSliceSource(vs, B, out_size=(H, W), augment=None, num_cls=num_cls, sample_mm=mm)
    rec = np.zeros(B, dtype=SAMPLE_DTYPE if mm is None else SAMPLE_Z_DTYPE)
    if mm is not None:
        rec["dz"] = np.float32(mm[2] / vox[2])
    fov = mm is not None
    # one batch loop for every path: the default one is one callable, one map and pnp_paste_labels[_fov] (the maximum of the interpolated
    # logits, not the M = 1 ensemble kernel's maximum of their softmax)
    if ensemble:
        maps = [compose_matrix((X, Y), (H, W), **e, **geom) for e in entries]
    else:
        fns, maps = [logits_fn], [compose_matrix((X, Y), (H, W), **geom)]
    invs = [invert_matrix(m) for m in maps] * len(fns)                      # callable-major, like the members
    if fov and fov_stats is not None:
        fov_stats.append(coverage(invs, X, Y, H, W, mode="all" if ramp is None else "any"))
    out_p = torch.zeros((int(num_cls),) + tuple(image.shape), dtype=torch.float32, device=device) if prob else None
    out_e = torch.zeros(tuple(image.shape), dtype=torch.float32, device=device) if entropy else None
    if not ensemble:
        paste = lambda members, nb, z: K.paste_labels(members[0], nb, z, invs[0], (X, Y), out, origin, strides, fov=fov)
    elif ramp is not None:
        paste = lambda members, nb, z: K.paste_tiles(members, nb, z, invs, ramp, (X, Y), out, origin, strides, prob=out_p, entropy=out_e)
    else:
        paste = lambda members, nb, z: K.paste_ensemble(members, nb, z, invs, (X, Y), out, origin, strides, prob=out_p, entropy=out_e, fov=fov)
    for k in range(0, count, B):
        nb = min(B, count - k)
        rec["frame"] = np.minimum(first + k + np.arange(B), first + k + nb - 1)
        xs = []
        for m in maps:                                                      # one gather per distinct map, shared by the callables
            rec["m"][:] = m
            xs.append(src.gather_records(rec, num_cls, want_onehot=False)[0])
        members = []
        for fn in fns:
            for x in xs:
                logits = fn(x)
                if tuple(logits.shape) != (B, H, W, int(num_cls)):
                    raise ValueError("logits_fn returned %s, expected %s" % (tuple(logits.shape), (B, H, W, int(num_cls))))
                members.append(logits.detach().contiguous())
        paste(members, nb, first + k + shift)
    src.close()
    _filter_components(out, post, num_cls, component_stats)
    _fill_holes(out, holes, num_cls, hole_stats)
    return Ensemble(out, out_p, out_e) if ensemble else out


def _body_margin(crop):
    """the margin of crop="body" / ("body", margin), None for every other crop; a malformed body crop is a ValueError"""
    if isinstance(crop, str) or (isinstance(crop, (tuple, list)) and len(crop) > 0 and isinstance(crop[0], str)):
        from . import body
        return body.parse_crop(crop)[1]
    return None


def _upload_prepared(image, flip_correction, axis, device):
    """prepare_pair's image (flips, `axis` last, finite check) on the device, whole"""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.PnpError("segment_volume: pnp kernels need a CUDA/HIP device (got %s) — there is no CPU fallback" % (device,))
    image = np.asarray(image)
    return torch.from_numpy(prepare_pair(image, np.zeros(image.shape, np.uint8), flip_correction, axis, None)[0]).to(device)


def _filter_components(label, post, num_cls, component_stats):
    """components.keep_largest on the finished label volume, in place; post: components.parse_option's keywords or None (nothing runs)"""
    if post is None:
        return
    from . import components
    _, stats = components.keep_largest(label, num_cls=num_cls, out=label, **post)
    if component_stats is not None:
        component_stats.append(stats)


def _fill_holes(label, holes, num_cls, hole_stats):
    """components.fill_holes on the finished label volume, in place; holes: components.parse_fill_option's keywords or None (nothing runs)"""
    if holes is None:
        return
    from . import components
    _, stats = components.fill_holes(label, num_cls=num_cls, out=label, **holes)
    if hole_stats is not None:
        hole_stats.append(stats)


def segmenter_logits(net):
    """logits_fn of source_segmenter.Full_DRN: every BN in inference mode, no dropout"""
    import torch

    def fn(x):
        with torch.no_grad():
            return net.forward(x, 1.0, main_bn=False, adapt_bn=False)
    return fn


def adapted_logits(net):
    """logits_fn of the CT path of adversarial.Full_DRN (adapt_* front + shared second half), critics pruned"""
    import torch

    def fn(x):
        with torch.no_grad():
            return net._graph(None, x, 1.0, mr_front_bn=False, joint_bn=False, ct_front_bn=False, critics=False)["ct_logits"]
    return fn


def predict_volumes(logits_fn, nii_list, output_path, label_list=None, num_cls=5, device="cuda", **options):
    """every image of nii_list -> <output_path>/pred_<basename>: uint8 NIfTI on the input's grid with the input's affine.  With
    label_list (same order) also the dense_pred_<name>.nii.gz / gth_dense_pred_<name>.nii.gz pair that `evaluate --pred-dir` reads (the
    ground truth with labels >= num_cls set to 0).  options: segment_volume's; with crop="body" / ("body", margin) the box
    found for every image is logged (crop_box=[] also collects them, one per image); with prob= / entropy= also prob_<basename> (float32,
    [*shape, num_cls]) and entropy_<basename> (float32) on the same grid with the same affine; with keep_largest= every label volume written
    is the filtered one (component_stats=[]: one stats tensor per volume is appended), with fill_holes= its enclosed holes are filled after
    that (hole_stats=[] likewise); prefilter= is segment_volume's (the
    setting the network was trained with); tiles= / tile_overlap= are segment_volume's (the share logged is then the union
    of the planes); axes= / axis_weights= are segment_volume's (every image is predicted once per listed slicing axis and
    the views are fused; one share is then logged per view); with sample_mm= every image's voxel size is read
    from its affine, the share of its voxel columns inside the field of view is logged, and a share below 1 is a warning (the voxels
    outside stay 0: choose crop / out_size / sample_mm so that the structure lies inside).  Returns the pred_* paths."""
    from . import nifti
    nii_list = list(nii_list)
    if label_list is not None and len(label_list) != len(nii_list):
        raise ValueError("%d labels for %d images" % (len(label_list), len(nii_list)))
    os.makedirs(output_path, exist_ok=True)
    paths = []
    for n, fid in enumerate(nii_list):
        img = nifti.load(fid)
        gt = None if label_list is None else np.asarray(nifti.load(label_list[n]).get_data())
        extra = {}
        if options.get("sample_mm") is not None:
            from .surface import spacing_of
            extra = {"spacing": check_spacing(spacing_of(img.affine), str(fid)), "fov_stats": []}
        if _body_margin(options.get("crop")) is not None:
            extra["crop_box"] = options["crop_box"] if options.get("crop_box") is not None else []
        res = segment_volume(logits_fn, img.get_data(), label=gt, num_cls=num_cls, device=device,
                             **{k: v for k, v in options.items() if k not in extra}, **extra)
        if "crop_box" in extra:
            logging.info("%s: body box %s of the volume %s (slicing order, half-open)" % (
                fid, " x ".join("[%d, %d)" % b for b in extra["crop_box"][-1]), tuple(img.get_data().shape)))
        for share in extra.get("fov_stats", ()):
            log = logging.warning if share < 1.0 else logging.info
            log("%s: %.1f %% of the voxel columns lie inside the field of view (pixels of %s mm)%s" % (
                fid, 100.0 * share, " x ".join("%g" % v for v in check_sample_mm(options["sample_mm"])[:2]),
                "; the rest stays 0" if share < 1.0 else ""))
        base = os.path.basename(str(fid))
        soft = res if isinstance(res, Ensemble) else Ensemble(res, None, None)
        pred = soft.label.cpu().numpy()
        paths.append(nifti.save(nifti.Nifti1Image(pred, img.affine), os.path.join(output_path, "pred_" + base)))
        if soft.prob is not None:            # class-major planes on the device -> the class axis last in the file
            p = np.ascontiguousarray(np.moveaxis(soft.prob.cpu().numpy(), 0, -1), dtype=np.float32)
            nifti.save(nifti.Nifti1Image(p, img.affine), os.path.join(output_path, "prob_" + base))
        if soft.entropy is not None:
            nifti.save(nifti.Nifti1Image(soft.entropy.cpu().numpy().astype(np.float32, copy=False), img.affine), os.path.join(output_path, "entropy_" + base))
        if gt is not None:
            dense = "dense_pred_" + base.split(".")[0] + ".nii.gz"
            nifti.save(nifti.Nifti1Image(pred, img.affine), os.path.join(output_path, dense))
            g = np.where(gt > num_cls - 1, 0, gt).astype(np.uint8)
            nifti.save(nifti.Nifti1Image(g, img.affine), os.path.join(output_path, "gth_" + dense))
    return paths
