"""Inference of whole NIfTI volumes onto their own grid: image.nii.gz in, label volume of the same shape and axis order
out.  Unlike Trainer.test_eval (volume_eval.py, kept quirk for quirk from the reference) it takes any in-plane size, needs no ground
truth, predicts every frame and keeps the volume on the device from upload to the finished label volume.

  segment_volume(logits_fn, image, ...)   one volume: orientation and crop like volume_source.prepare_pair, pnp_volume_preprocess, then per
                                          batch of ascending frames the gather (pnp_aug_slices with the un-augmented compose_matrix map),
                                          logits_fn, and pnp_paste_labels with the inverse map straight into the file's array order.
                                          It composes the three below, which tests and tools read as well:
  parse_request(n_callables, ...)         the options, checked once: everything that needs no image (host)
  plan_view(request, shape, axis, box, spacing)   the geometry of one view: layout, maps, member order, frames, coverage (host, numpy only)
  run_view(plan, fns, volume, out, ...)   the device work of one view from its plan
  invert_matrix(m)                        the inverse of a compose_matrix map: source voxel (x, y) -> output-plane coordinates
  segmenter_logits / adapted_logits       the logits_fn of source_segmenter.Full_DRN and of the CT path of adversarial.Full_DRN
  predict_volumes(...)                    files in, pred_<basename> files out
  trainer_predict_volumes(...)            the body of both trainers' predict_volumes

The label of a voxel is the argmax of the bilinearly interpolated LOGITS (not probabilities): no exp, and for an identity map exactly
argmax(logits).

Ensemble inference (opt-in): with a list of callables (checkpoints), tta= (views of the same slice) or prob= / entropy=,
segment_volume gathers once per distinct map, runs one forward per member and makes ONE pnp_paste_ensemble launch per batch, which
interpolates every member's logits through that member's own inverse map, averages the softmax and writes the label, the mean
probabilities and the normalised entropy in the file's array order.  With the defaults nothing of this is reached.

Post-processing (opt-in): keep_largest= runs components.keep_largest and then fill_holes= components.fill_holes on the
finished label volume, on the device, before it is returned.

Millimetre grid (opt-in): with sample_mm= the plane has a fixed pixel size and is centred on the (cropped) volume, the
outer channels lie frame_mm from the centre frame (pnp_aug_slices_z; its clamp is the edge replication, so nothing is padded) and the
paste writes only the voxel columns inside the plane's field of view (pnp_paste_labels_fov / pnp_paste_ensemble_fov); the rest stays 0.

Anti-alias prefilter (opt-in): with prefilter= the normalised box is low-passed on the device (pnp_volume_smooth) before
anything samples it, with volume_source.prefilter_sigmas' rule — the setting the network was trained with.

Tiles (opt-in, needs sample_mm): with tiles= the crop box is covered by several overlapping planes of the same millimetre
grid (tile_plan), every plane is predicted, and ONE pnp_paste_tiles launch per batch blends them over their union with a window that
trusts a plane's centre more than its border.  Without the option nothing of this is reached.

Multi-planar fusion (opt-in): with axes= the scan gets one plan and one run per listed slicing axis (every other option
applies to each view), and ONE pnp_fuse_views launch averages the views' probability volumes over the views that cover a voxel
(check_axes, view_box, fuse_views).  Without the option nothing of this is reached.
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


Request = collections.namedtuple("Request", (
    "edge", "B", "H", "W", "num_cls", "percentile", "flip_correction", "axis", "crop", "body_margin", "sample_mm", "prefilter", "tiles",
    "tile_overlap", "entries", "n_callables", "member_limit", "ensemble", "prob", "entropy", "keep_largest", "fill_holes", "axes", "axis_weights"))
ViewPlan = collections.namedtuple("ViewPlan", (
    "request", "axis", "box", "origin", "strides", "dims", "vox", "geom", "counts", "offsets", "ramp", "entries", "maps", "invs", "kind", "fov",
    "coverage", "frames", "padded", "min_frames", "rec_dtype", "dz", "sigmas", "taps", "members", "logits_bytes"))


def parse_request(n_callables=None, *, flip_correction=True, axis=2, crop=None, edge="replicate", batch_size=16, percentile=98, out_size=(256, 256),
                  num_cls=5, tta=None, prob=False, entropy=False, keep_largest=None, spacing=None, sample_mm=None, prefilter=None, tiles=None,
                  tile_overlap=0.25, axes=None, axis_weights=None, fill_holes=None):
    """segment_volume's options, checked once -> Request: everything about a prediction that needs no image and no device.  n_callables:
    None for a bare logits_fn, the length of a list of them (a list, also of one, is a checkpoint ensemble).  Every ValueError an option can
    earn on its own is raised here, in this order: edge, keep_largest, fill_holes, crop, axes / axis_weights, batch_size, sample_mm,
    prefilter, spacing, tiles / tile_overlap, the members.
      ensemble      a list of callables, tta, prob, entropy, tiles or axes: the result is the Ensemble tuple
      entries       tta_entries(tta): the views of every slice; members = callables x entries, at most member_limit (MAX_MEMBERS, with
                    tiles MAX_TILE_MEMBERS and then counted again with the planes, by plan_view)
      keep_largest, fill_holes   components.parse_option / parse_fill_option's keywords, or None
      body_margin   the margin of crop="body" / ("body", margin), None for every other crop
      sample_mm     check_sample_mm's triple or None; it needs `spacing`, which is checked here and ordered per view by plan_view
      axes, axis_weights   check_axes' tuples, or None: `axis` must then be left at its default"""
    from . import components
    if edge not in EDGES:
        raise ValueError("edge must be one of %s, got %r" % (EDGES, edge))
    post = components.parse_option(keep_largest, num_cls)
    holes = components.parse_fill_option(fill_holes, num_cls)
    body_margin = _body_margin(crop)
    if axes is not None or axis_weights is not None:
        if axes is None:
            raise ValueError("axis_weights %r goes with axes" % (axis_weights,))
        if axis != 2:
            raise ValueError("axes=%r and axis=%r exclude each other: leave axis at its default" % (axes, axis))
        axes, axis_weights = check_axes(axes, axis_weights)
    B, H, W = int(batch_size), int(out_size[0]), int(out_size[1])
    if B < 1:
        raise ValueError("batch_size must be at least 1")
    mm = check_sample_mm(sample_mm)
    pre = check_prefilter(prefilter)
    if mm is not None:
        if spacing is None:
            raise ValueError("sample_mm needs spacing: the voxel size in mm per array axis of the image (surface.spacing_of(affine))")
        slicing_order(spacing, axis, "spacing")
    tiles = check_tiles(tiles)
    if tiles is not None:
        if mm is None:
            raise ValueError("tiles needs sample_mm: the planes of a tiled prediction share one millimetre grid")
        if not 0.0 <= float(tile_overlap) <= 0.5:
            raise ValueError("tile overlap %r outside [0, 0.5]" % (tile_overlap,))
    ensemble = tiles is not None or n_callables is not None or tta is not None or bool(prob) or bool(entropy) or axes is not None
    limit = MAX_MEMBERS if tiles is None else MAX_TILE_MEMBERS
    n = 1 if n_callables is None else int(n_callables)
    entries = ensemble_members([None] * n, tta, limit)[1]                 # the rule counts the callables: it does not call them
    return Request(edge, B, H, W, int(num_cls), percentile, flip_correction, axis, crop, body_margin, mm, pre, tiles, tile_overlap, tuple(entries), n,
                   limit, ensemble, bool(prob), bool(entropy), post, holes, axes, axis_weights)


def _frozen(a):
    a.setflags(write=False)
    return a


def plan_view(request, image_shape, axis, box, spacing=None):
    """the host geometry of one view — `request` for the file array `image_shape` sliced along `axis`, inside `box` (resolved: _box_of's or
    body.body_box's, in the slicing order of `axis`), `spacing` per array axis — as an immutable ViewPlan.  Pure numpy: nothing here
    touches a device, and the ValueErrors that need the box (edge='skip' on fewer than 3 frames, tile counts that cannot cover it, too many
    members with the planes counted) are raised here.
      origin, strides, dims   file_layout's: where voxel (x, y, z) of the box lies in the file's array; dims = (X, Y, Z)
      vox, geom     with sample_mm the voxel size in slicing order and compose_matrix's spacing_xy / pixel_mm; None / {}
      counts, offsets, ramp   with tiles tile_plan's planes and tile_ramp's rise; None otherwise
      entries       the request's tta entries; with tiles one per (tile, view), tile-major, the tile's offset added in mm to `translate`
      maps, invs    compose_matrix of every entry: one gather each; invs = [invert_matrix(m) for m in maps] * n_callables, one per member,
                    callable-major (then tile, then view)
      kind          the paste: "labels" (pnp_paste_labels: the maximum of the interpolated logits), "ensemble" (pnp_paste_ensemble: of the
                    mean softmax) or "tiles" (pnp_paste_tiles: of the window-weighted softmax); fov: only the voxel columns
                    inside the planes' field of view are written (with sample_mm)
      coverage      with sample_mm the share of the box's voxel columns that the paste writes: inside every member's field of view, with
                    tiles inside at least one; None otherwise
      frames        (first, count, shift): centre frames first .. first + count - 1 of the gathered volume, pasted `shift` frames further.
                    edge="skip" leaves the two edge frames out (the reference's frame set); edge="replicate" predicts every frame, through
                    the gather's clamp with sample_mm and otherwise through a copy of the first and the last frame (`padded`)
      min_frames, rec_dtype, dz   what VolumeSet and the gather's records need; dz = frame_mm in voxels with sample_mm
      sigmas, taps  with prefilter prefilter_sigmas' sigmas for this box and their gaussian_weights (taps is None when no
                    axis is filtered): the normalised box is smoothed before the edge frames are copied; tta scales are ignored
      members, logits_bytes   len(invs), and the bytes of member logits alive per batch: members x 4 B H W num_cls — 21 MB per member at
                    the defaults, 1.3 GB at 64 members; where that nears the free memory, halve batch_size"""
    r = request
    H, W, mm = r.H, r.W, r.sample_mm
    box = tuple((int(a), int(b)) for a, b in box)
    origin, strides, (X, Y, Z) = file_layout(image_shape, r.flip_correction, axis, box)
    if r.edge == "skip" and Z < 3:
        raise ValueError("edge='skip' needs at least 3 frames, the box has %d" % Z)
    vox, geom = None, {}
    if mm is not None:
        vox = slicing_order(spacing, axis, "spacing")          # as prepare_pair moves `axis` last
        geom = {"spacing_xy": vox[:2], "pixel_mm": mm[:2]}
    counts = offsets = ramp = None
    entries = r.entries
    if r.tiles is not None:
        extent, plane_mm = (X * vox[0], Y * vox[1]), (H * mm[0], W * mm[1])
        offsets, counts = tile_plan(extent, plane_mm, r.tiles, r.tile_overlap)
        if r.n_callables * len(offsets) * len(entries) > MAX_TILE_MEMBERS:
            raise ValueError("%d callables x %d x %d tiles x %d tta entries = %d members, at most %d" % (
                r.n_callables, counts[0], counts[1], len(entries), r.n_callables * len(offsets) * len(entries), MAX_TILE_MEMBERS))
        ramp, offsets = tile_ramp(extent, plane_mm, counts, mm[:2]), tuple(offsets)
        at = lambda e: e.get("translate", (0.0, 0.0))
        entries = tuple(dict(e, translate=(at(e)[0] + ti, at(e)[1] + tj)) for ti, tj in offsets for e in entries)
    maps = tuple(_frozen(compose_matrix((X, Y), (H, W), **e, **geom)) for e in entries)
    invs = tuple(_frozen(invert_matrix(m)) for m in maps) * r.n_callables
    fov = mm is not None
    sigmas = taps = None
    if r.prefilter is not None:
        sigmas = prefilter_sigmas(r.prefilter, (X, Y, Z), (H, W), vox, mm)
        taps = tuple(gaussian_weights(s) for s in sigmas)
        taps = taps if any(t is not None for t in taps) else None
    # without sample_mm and with edge="replicate", centre frames 1 .. Z of the padded volume are output frames 0 .. Z - 1
    frames = (1, Z - 2, 0) if r.edge == "skip" else (0, Z, 0) if fov else (1, Z, -1)
    return ViewPlan(request=r, axis=axis, box=box, origin=origin, strides=strides, dims=(X, Y, Z), vox=vox, geom=geom, counts=counts, offsets=offsets,
                    ramp=ramp, entries=entries, maps=maps, invs=invs, kind="tiles" if ramp is not None else "ensemble" if r.ensemble else "labels",
                    fov=fov, coverage=coverage(invs, X, Y, H, W, mode="all" if ramp is None else "any") if fov else None, frames=frames,
                    padded=not fov and r.edge == "replicate", min_frames=1 if fov else 3, rec_dtype=SAMPLE_Z_DTYPE if fov else SAMPLE_DTYPE,
                    dz=np.float32(mm[2] / vox[2]) if fov else None, sigmas=sigmas, taps=taps, members=len(invs),
                    logits_bytes=len(invs) * 4 * r.B * H * W * r.num_cls)


def plan_views(request, image_shape, box, spacing=None):
    """one ViewPlan per view: for `axis` alone, or per entry of `axes`, which get the box — given in the slicing order of
    the default axis — re-expressed in their own order by view_box"""
    if request.axes is None:
        return [plan_view(request, image_shape, request.axis, box, spacing)]
    return [plan_view(request, image_shape, a, view_box(box, a), spacing) for a in request.axes]


def run_view(plan, fns, volume, out, out_p=None, out_e=None):
    """the device work of one view: `volume`, the raw float32 box [X, Y, Z] on the device, is normalised in place (pnp_volume_preprocess),
    smoothed (plan.taps) and padded (plan.padded); then per batch of ascending frames one gather per map of the plan (pnp_aug_slices[_z]),
    one forward per callable and gather, and ONE paste of all members' logits through their inverse maps into out / out_p / out_e, which lie
    in the file's array order.  The last, short batch repeats its last frame and pastes nb < B slices.  Nothing synchronises between
    batches; the fill is read once before the loop, the gather's error counter once at the end.  Geometry and options are the plan's:
    nothing is computed or checked here but the shape of what a logits_fn returns."""
    import torch
    from . import kernels as K
    r = plan.request
    B, H, W, num_cls, v, xy = r.B, r.H, r.W, r.num_cls, volume, plan.dims[:2]
    _, stats = K.volume_preprocess(v, int(r.percentile), out=v)
    fill = float(stats[3].item())                       # the one read before the loop: the fill enters the gather's descriptor table
    if plan.taps is not None:
        K.volume_smooth(v, list(plan.taps), out=v)
        K.drop_workspace("smooth")
    if plan.padded:
        v = torch.cat([v[:, :, :1], v, v[:, :, -1:]], dim=2).contiguous()          # statistics: of the unpadded volume, above
    vs = VolumeSet.from_device([v], [torch.zeros(tuple(v.shape), dtype=torch.uint8, device=v.device)], ["volume"], [fill], r.percentile,
                               min_frames=plan.min_frames)
    src = AugmentedSliceSource(vs, B, out_size=(H, W), augment=None, num_cls=num_cls, sample_mm=r.sample_mm)
    rec = np.zeros(B, dtype=plan.rec_dtype)
    if plan.dz is not None:
        rec["dz"] = plan.dz
    first, count, shift = plan.frames
    for k in range(0, count, B):
        nb = min(B, count - k)
        rec["frame"] = np.minimum(first + k + np.arange(B), first + k + nb - 1)
        xs = []
        for m in plan.maps:                                                 # one gather per distinct map, shared by the callables
            rec["m"][:] = m
            xs.append(src.gather_records(rec, num_cls, want_onehot=False)[0])
        members = []
        for fn in fns:
            for x in xs:
                logits = fn(x)
                if tuple(logits.shape) != (B, H, W, num_cls):
                    raise ValueError("logits_fn returned %s, expected %s" % (tuple(logits.shape), (B, H, W, num_cls)))
                members.append(logits.detach().contiguous())
        z = first + k + shift
        if plan.kind == "labels":
            K.paste_labels(members[0], nb, z, plan.invs[0], xy, out, plan.origin, plan.strides, fov=plan.fov)
        elif plan.kind == "tiles":
            K.paste_tiles(members, nb, z, plan.invs, plan.ramp, xy, out, plan.origin, plan.strides, prob=out_p, entropy=out_e)
        else:
            K.paste_ensemble(members, nb, z, plan.invs, xy, out, plan.origin, plan.strides, prob=out_p, entropy=out_e, fov=plan.fov)
    src.close()


def segment_volume(logits_fn, image, *, label=None, flip_correction=True, axis=2, crop=None, edge="replicate", batch_size=16, percentile=98,
                   out_size=(256, 256), num_cls=5, device="cuda", tta=None, prob=False, entropy=False, keep_largest=None, component_stats=None,
                   spacing=None, sample_mm=None, fov_stats=None, prefilter=None, tiles=None, tile_overlap=0.25, axes=None, axis_weights=None, crop_box=None,
                   fill_holes=None, hole_stats=None):
    """-> uint8 label volume of `image`'s shape and axis order, a device tensor (`.cpu().numpy()` is the caller's); with a list of
    callables, tta, prob, entropy, tiles or axes the Ensemble(label, prob, entropy) tuple (a field not asked for is None; outside the crop
    box and the field of view all three are 0).  The composition of the functions above, where each option's rule is written down:
      1. parse_request   every option but the four lists, checked before the device is looked at; logits_fn: x [B, H, W, 3] -> logits
                         [B, H, W, num_cls] (segmenter_logits / adapted_logits), or a list of them
      2. the box         crop: None, a margin around `label`'s bounding box, a box ((x0, x1), (y0, y1), (z0, z1)) in slicing order (with
                         axes: of the default axis), or "body" / ("body", margin): the prepared volume is uploaded whole and
                         body.body_box finds the box on the device (two host synchronisations; the result equals crop=<that box>).
                         crop_box: optional list, the box is appended
      3. plan_views      one plan per view; fov_stats: optional list, with sample_mm every view's coverage is appended, in axes order
      4. run_view        per view, on its box of the prepared volume
      5. with axes ONE pnp_fuse_views launch averages the views' probabilities into the first view's buffers, per voxel over the views
         that wrote it, weighted by axis_weights; peak memory is len(axes) probability volumes
      6. components.keep_largest, 7. components.fill_holes: once, in place on the finished (fused) label only;
         component_stats / hole_stats: optional lists, each pass's int64 [num_cls, 4] stats tensor is appended
    DESIGN.md §14–§26 is the long form."""
    import torch
    from . import kernels as K
    is_list = isinstance(logits_fn, (list, tuple))
    fns = list(logits_fn) if is_list else [logits_fn]
    req = parse_request(len(fns) if is_list else None, flip_correction=flip_correction, axis=axis, crop=crop, edge=edge, batch_size=batch_size,
                        percentile=percentile, out_size=out_size, num_cls=num_cls, tta=tta, prob=prob, entropy=entropy, keep_largest=keep_largest,
                        spacing=spacing, sample_mm=sample_mm, prefilter=prefilter, tiles=tiles, tile_overlap=tile_overlap, axes=axes,
                        axis_weights=axis_weights, fill_holes=fill_holes)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.PnpError("segment_volume: pnp kernels need a CUDA/HIP device (got %s) — there is no CPU fallback" % (device,))
    image = np.asarray(image)
    blank = np.zeros(image.shape, np.uint8)
    img, lab = prepare_pair(image, blank if label is None else label, flip_correction, axis, None)
    full = None
    if req.body_margin is not None:
        from . import body
        full = torch.from_numpy(img).to(device)
        box = body.body_box(full, percentile=int(percentile), margin=req.body_margin)
    else:
        box = _box_of(crop, None if label is None else lab, img.shape)
    if crop_box is not None:
        crop_box.append(box)
    plans = plan_views(req, image.shape, box, spacing)
    if fov_stats is not None:
        fov_stats.extend(p.coverage for p in plans if p.coverage is not None)
    multi, shape = req.axes is not None, tuple(image.shape)
    labels, probs = [], []
    for plan in plans:
        where = tuple(slice(a, b) for a, b in plan.box)
        labels.append(torch.zeros(shape, dtype=torch.uint8, device=device))
        # one view's body crop is taken on the device; several views take their boxes from the host, each in its own order
        view = full if full is not None and not multi else img if plan.axis == axis else prepare_pair(image, blank, flip_correction, plan.axis, None)[0]
        full = None
        v = view[where].contiguous() if torch.is_tensor(view) else torch.from_numpy(np.ascontiguousarray(view[where])).to(device)
        del view
        probs.append(torch.zeros((req.num_cls,) + shape, dtype=torch.float32, device=device) if req.prob or multi else None)
        out_e = torch.zeros(shape, dtype=torch.float32, device=device) if req.entropy and not multi else None
        run_view(plan, fns, v, labels[-1], probs[-1], out_e)
        del v, labels[1:]
    out, out_p = labels[0], probs[0]                        # the first view's buffers take the fused result
    if multi:
        _, out_p, out_e = K.fuse_views(probs, req.axis_weights, label=out, prob=out_p if req.prob else None, entropy=req.entropy)
    del probs
    from . import components
    for opts, run, stats in ((req.keep_largest, components.keep_largest, component_stats), (req.fill_holes, components.fill_holes, hole_stats)):
        if opts is not None:                                # in place, on the finished label alone: prob and entropy stay as computed
            got = run(out, num_cls=req.num_cls, out=out, **opts)[1]
            if stats is not None:
                stats.append(got)
    return Ensemble(out, out_p, out_e) if req.ensemble else out


def _body_margin(crop):
    """the margin of crop="body" / ("body", margin), None for every other crop; a malformed body crop is a ValueError"""
    if isinstance(crop, str) or (isinstance(crop, (tuple, list)) and len(crop) > 0 and isinstance(crop[0], str)):
        from . import body
        return body.parse_crop(crop)[1]
    return None


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


def trainer_predict_volumes(trainer, adapter, nii_list, output_path, label_list=None, ensemble=None, tiles=None, tile_overlap=0.25, **options):
    """Trainer.predict_volumes of both trainers: predict_volumes with the trainer's net behind `adapter` (segmenter_logits /
    adapted_logits), its num_cls and device, and batch_size defaulting to the net's.  ensemble: further nets of the same class, averaged
    with the trainer's (a checkpoint ensemble).  options: segment_volume's.  Returns the pred_* paths."""
    options.setdefault("batch_size", trainer.net.batch_size)
    if tiles is not None:              # entered only when given: without it segment_volume takes the path it took before
        options.update(tiles=tiles, tile_overlap=tile_overlap)
    fn = adapter(trainer.net) if not ensemble else [adapter(n) for n in [trainer.net] + list(ensemble)]
    return predict_volumes(fn, nii_list, output_path, label_list=label_list, num_cls=trainer.num_cls, device=trainer.net.device, **options)


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
