"""Training input straight from NIfTI volumes: the four steps the reference's README names for its data set — crop, cut
the top 2 % of each volume's intensity histogram, z-score each volume, sample 2-D slices with data augmentation — of which it ships no
code.  The volumes stay resident in HBM; preprocessing and the augmented slice gather are kernels of libpnp_hip.so (csrc/augment.hip),
the host only draws the parameters.

  VolumeSet             loads image / label pairs (nifti.load), flips and reorders them like volume_eval.test_eval, optionally crops to
                        the label bounding box, uploads, normalises on the device (pnp_volume_preprocess) and keeps the per-volume stats
                        (from_device: volumes that are on the device and normalised already — volume_predict.py's way in)
  AugmentedSliceSource  draws (volume, frame, affine map) per sample from a seeded numpy Generator and gathers the batch on the device
                        (pnp_aug_slices): next_device_batch() for feeder.DeviceFeeder, next_batch() for every consumer of the trainers'
                        [B, H, W, 4] numpy protocol

A list file holds one `image.nii[.gz] label.nii[.gz]` pair per line (paths relative to the list file's folder unless absolute).
With read_pairs(..., labels="optional") a line may name the image alone: an unlabelled target scan.  It gets an all-zero
label volume, VolumeSet.has_labels / AugmentedSliceSource.labelled say so, and VolumeSet(crop="body" | ("body", margin)) crops every volume
to the bounding box of the patient found on the device without a label (body.body_box) instead of the label bounding box.

  python -m "medical-cross-modality-domain-adaptation_amd.volume_source" --export N OUTDIR --list LIST [--augment JSON | --no-augment]
         [--sample-mm MM|PI,PJ,FRAME] [--prefilter auto|off|SX,SY,SZ] [--axes 0,1,2]
         [--foreground P [--foreground-classes C[,C..]] [--foreground-centre]] [--crop-body [N] | --crop-margin N]
writes N slices in the reference's tfrecord layout (tfrecord.write_slice) plus OUTDIR/slice_list, so that the TensorFlow reference can be
fed from the same volumes.

Output pixel (i, j) of an [H, W] slice reads the source slice [X, Y] at (sx, sy) = M (i, j, 1); `compose_matrix` folds centring, the
resize from (X, Y) to (H, W), rotation, scale, translation and flip into the six float32 entries of M.  The kernel knows nothing of angles.

Sampling on a millimetre grid (opt-in): with sample_mm = a number or (pi_mm, pj_mm, frame_mm) an output pixel is pi_mm x pj_mm
millimetres whatever the volume's voxel size (VolumeSet.spacings, from the NIfTI affine), the plane is centred on the volume and the outer
two channels lie frame_mm away from the centre frame, interpolated between frames (pnp_aug_slices_z).  Bilinear sampling aliases once a
pixel is more than about twice the voxel, as the plain resize does: that is what the prefilter below is for.

Anti-alias prefilter (opt-in): with prefilter="auto" (or sigmas in voxels) every resident volume is low-passed once, on the
device, by a separable Gaussian (pnp_volume_smooth) before anything samples it — sigma = (r - 1) / 2 per axis for r source voxels per
output sample, skimage's rule for resize(anti_aliasing=True).  Labels are never filtered.  gaussian_weights / prefilter_sigmas are the
host side; volume_predict.segment_volume applies the same rule to the scan it predicts, so train and predict with one setting.

Elastic deformation and intensity augmentation (opt-in through five more `augment` keys): a coarse lattice of random
control-point displacements per sample (a uniform cubic B-spline over the output plane, U-Net's warp) and gain / bias / Gaussian noise on
the image channels, both inside the same gather launch (pnp_aug_slices_warp).  The host draws the control points in output pixels and maps
them into source voxels with the linear part of the sample's own M.

Foreground-aware sampling (opt-in): with sampling = {"foreground": p, ...} a share p of the samples takes the frame of a
uniformly drawn voxel of a random class present in its volume instead of a uniform frame, and with "centre" the plane is centred on that
class's bounding box in the frame.  Where the classes are comes from a per-frame class table computed once per resident label volume on
the device (pnp_label_frame_stats, VolumeSet.frame_stats); the draw itself is host code (sample_params) on a third generator.
"""
import argparse
import ctypes
import json
import logging
import math
import os

import numpy as np

from . import _lib
from .parallel import rank_seed

# rotation in degrees (+-), scale (+-, log-uniform in [1 / (1 + s), 1 + s]), translation in source voxels (+-), flip probability (mirror of
# the second slice axis).  Mild by design: the hearts of MMWHS keep their orientation, so the default does not flip.
DEFAULT_AUGMENT = {"rotate": 15.0, "scale": 0.1, "translate": 10.0, "flip": 0.0}
_AUGMENT_KEYS = tuple(sorted(DEFAULT_AUGMENT))
# the opt-in keys of DESIGN.md §18 (none of them is in DEFAULT_AUGMENT): elastic = sigma of a control point's displacement in OUTPUT pixels,
# elastic_grid = cells per axis of the control lattice (1 .. 16; 4 when elastic > 0 and none is given), contrast = gain log-uniform in
# [1 / (1 + c), 1 + c], brightness = +- additive in z-score units, noise = the per-sample sigma is uniform in [0, noise]
_WARP_KEYS = ("brightness", "contrast", "elastic", "elastic_grid", "noise")
DEFAULT_ELASTIC_GRID = 4
MAX_ELASTIC_GRID = 16


def read_pairs(list_file, labels="required"):
    """list file -> [(image path, label path)]; blank lines and lines starting with # are skipped.  labels="optional": a line may name
    the image alone (an unlabelled target scan) and gives (image path, None)"""
    if labels not in ("required", "optional"):
        raise ValueError("read_pairs: labels must be \"required\" or \"optional\", got %r" % (labels,))
    if not os.path.isfile(list_file):
        raise IOError("volume list %s does not exist" % list_file)
    base = os.path.dirname(os.path.abspath(list_file))
    pairs = []
    with open(list_file) as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            parts = line.split()
            if len(parts) != 2 and not (labels == "optional" and len(parts) == 1):
                raise ValueError("%s:%d: expected `image.nii[.gz] label.nii[.gz]`, got %d fields" % (list_file, no, len(parts)))
            for p in parts:
                if not p.endswith((".nii", ".nii.gz")):
                    raise ValueError("%s:%d: %s is not a .nii / .nii.gz file name" % (list_file, no, p))
            pair = tuple(p if os.path.isabs(p) else os.path.join(base, p) for p in parts)
            for p in pair:
                if not os.path.isfile(p):
                    raise IOError("%s:%d: %s does not exist" % (list_file, no, p))
            pairs.append(pair if len(pair) == 2 else (pair[0], None))
    if not pairs:
        raise ValueError("%s: no volume pair listed" % list_file)
    return pairs


def check_augment(augment):
    """None (identity) or a dict with a subset of DEFAULT_AUGMENT's keys and of the elastic / intensity keys (_WARP_KEYS) -> None / a dict
    with all four classic keys plus those of the new keys that were given"""
    if augment is None:
        return None
    unknown = sorted(set(augment) - set(_AUGMENT_KEYS) - set(_WARP_KEYS))
    if unknown:
        raise ValueError("augment: unknown keys %s (known: %s)" % (unknown, list(_AUGMENT_KEYS + _WARP_KEYS)))
    a = {k: float(augment.get(k, 0.0)) for k in _AUGMENT_KEYS}
    if a["rotate"] < 0 or a["scale"] < 0 or a["translate"] < 0 or not 0.0 <= a["flip"] <= 1.0:
        raise ValueError("augment: rotate, scale, translate must be >= 0 and flip in [0, 1], got %r" % (a,))
    for k in _WARP_KEYS:
        if k not in augment:
            continue
        v = augment[k]
        if k == "elastic_grid":
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != int(v) or not 1 <= int(v) <= MAX_ELASTIC_GRID:
                raise ValueError("augment: elastic_grid must be an integer in [1, %d], got %r" % (MAX_ELASTIC_GRID, v))
            a[k] = int(v)
        else:
            a[k] = float(v)
            if not 0.0 <= a[k] < math.inf:
                raise ValueError("augment: %s must be a finite number >= 0, got %r" % (k, v))
    return a


def uses_warp_entry(augment):
    """whether a checked augment dict needs pnp_aug_slices_warp: one of elastic, contrast, brightness, noise is non-zero"""
    return augment is not None and any(augment.get(k, 0.0) > 0 for k in ("elastic", "contrast", "brightness", "noise"))


def elastic_grid_of(augment):
    """cells per axis of the control lattice: 0 without elastic deformation, else elastic_grid (default 4)"""
    if augment is None or augment.get("elastic", 0.0) <= 0:
        return 0
    return int(augment.get("elastic_grid", DEFAULT_ELASTIC_GRID))


def check_elastic_fold(augment, out_hw):
    """elastic <= 0.5 min(H, W) / G: neighbouring control points are min(H, W) / G pixels apart; displaced against each other by
    2 sigma each they would meet, and the plane would fold"""
    G = elastic_grid_of(augment)
    if G and augment["elastic"] > 0.5 * min(out_hw) / G:
        raise ValueError("augment: elastic = %g output pixels folds the %d x %d plane on a lattice of %d cells (at most 0.5 min(H, W) / G = %g)"
                         % (augment["elastic"], out_hw[0], out_hw[1], G, 0.5 * min(out_hw) / G))


def _cos_sin(deg):
    """exact at the multiples of 90 degrees: those rotations are integer permutations of the pixel grid"""
    q = deg / 90.0
    if q == math.floor(q):
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    r = math.radians(deg)
    return math.cos(r), math.sin(r)


def compose_matrix(src_xy, out_hw, rotate=0.0, scale=1.0, translate=(0.0, 0.0), flip=False, *, spacing_xy=None, pixel_mm=None):
    """the six float32 entries (m00, m01, m02, m10, m11, m12) of
         s = c_src + t + (1 / scale) R(rotate) F D (p - c_out),   c = (extent - 1) / 2,  D = diag(X / H, Y / W),  F = diag(1, -1) if flip
    composed in float64.  scale > 1 magnifies (the output sees a smaller part of the source).  The identity with (X, Y) = (H, W) is
    exactly (1, 0, 0, 0, 1, 0); rotations by multiples of 90 degrees and the flip of a square slice are exact integer permutations.
    With spacing_xy = (sx, sy) and pixel_mm = (pi_mm, pj_mm) (both or neither), S = diag(sx, sy), P = diag(pi_mm, pj_mm):
         s = c_src + S^-1 (t_mm + (1 / scale) R(rotate) F P (p - c_out))
    rotation and scale act in millimetres (right for anisotropic in-plane spacing), `translate` is in millimetres, and the extent of the
    source enters through its centre only.  With pi_mm / sx = X / H, pj_mm / sy = Y / W and sx = sy the entries are the ones above."""
    if (spacing_xy is None) != (pixel_mm is None):
        raise ValueError("compose_matrix: spacing_xy and pixel_mm go together")
    X, Y = float(src_xy[0]), float(src_xy[1])
    H, W = float(out_hw[0]), float(out_hw[1])
    c, s = _cos_sin(float(rotate))
    inv = 1.0 / float(scale)
    f = -1.0 if flip else 1.0
    ci, cj = (H - 1.0) / 2.0, (W - 1.0) / 2.0
    if spacing_xy is None:
        dx, dy = X / H, Y / W
        a00, a01 = inv * c * dx, inv * -s * f * dy
        a10, a11 = inv * s * dx, inv * c * f * dy
        tx, ty = float(translate[0]), float(translate[1])
    else:
        sx, sy = float(spacing_xy[0]), float(spacing_xy[1])
        pi, pj = float(pixel_mm[0]), float(pixel_mm[1])
        if not (0.0 < sx < math.inf and 0.0 < sy < math.inf and 0.0 < pi < math.inf and 0.0 < pj < math.inf):
            raise ValueError("compose_matrix: spacing_xy %r and pixel_mm %r must be positive and finite" % (spacing_xy, pixel_mm))
        a00, a01 = inv * c * (pi / sx), inv * -s * f * (pj / sx)
        a10, a11 = inv * s * (pi / sy), inv * c * f * (pj / sy)
        tx, ty = float(translate[0]) / sx, float(translate[1]) / sy
    m02 = (X - 1.0) / 2.0 + tx - (a00 * ci + a01 * cj)
    m12 = (Y - 1.0) / 2.0 + ty - (a10 * ci + a11 * cj)
    return np.array([a00, a01, m02, a10, a11, m12], dtype=np.float32)


def check_sample_mm(sample_mm):
    """None, a positive number (isotropic) or (pi_mm, pj_mm, frame_mm) -> None / a triple of floats; anything else is a ValueError"""
    if sample_mm is None:
        return None
    try:
        t = (float(sample_mm),) * 3 if np.isscalar(sample_mm) else tuple(float(v) for v in sample_mm)
    except (TypeError, ValueError):
        raise ValueError("sample_mm must be a number or (pi_mm, pj_mm, frame_mm), got %r" % (sample_mm,))
    if len(t) != 3 or not all(0.0 < v < math.inf for v in t):
        raise ValueError("sample_mm must be a positive finite number or three of them (pi_mm, pj_mm, frame_mm), got %r" % (sample_mm,))
    return t


def slicing_spacing(affine, axis=2, name="volume"):
    """(sx, sy, sz) in mm of the slicing order: surface.spacing_of's per-array-axis spacings (the affine's column norms) with `axis`
    moved last, as prepare_pair moves it (flips and crops change no spacing).  A non-finite or <= 0 spacing is a ValueError naming `name`."""
    from .surface import spacing_of
    return slicing_order(spacing_of(affine), axis, name)


def slicing_order(spacing, axis=2, name="volume"):
    """per-array-axis spacings -> slicing order (`axis` last), checked"""
    if axis not in (0, 1, 2):
        raise ValueError("%s: axis %r is not one of 0, 1, 2" % (name, axis))
    sp = list(check_spacing(spacing, name))
    return tuple(sp[:axis] + sp[axis + 1:] + [sp[axis]])


def check_spacing(spacing, name="volume"):
    try:
        sp = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError("%s: a voxel spacing is three numbers in mm, got %r" % (name, spacing))
    if len(sp) != 3 or not all(0.0 < v < math.inf for v in sp):
        raise ValueError("%s: voxel spacing %r must be three positive finite numbers (mm)" % (name, spacing))
    return sp


def check_axes(axes, weights=None):
    """the slicing axes of a multi-planar set or prediction: a non-empty sequence of distinct ints from {0, 1, 2}, and
    weights = None or as many positive finite numbers -> (tuple of ints, tuple of floats or None); anything else is a ValueError that
    quotes the offending value"""
    if isinstance(axes, (str, bytes)) or not hasattr(axes, "__iter__"):
        raise ValueError("axes must be a sequence of distinct axes from 0, 1, 2, got %r" % (axes,))
    t = tuple(axes)
    if not t:
        raise ValueError("axes: an empty sequence names no slicing axis, got %r" % (axes,))
    for a in t:
        if isinstance(a, (bool, np.bool_)) or not isinstance(a, (int, np.integer)) or a not in (0, 1, 2):
            raise ValueError("axes: %r is not one of the axes 0, 1, 2 (in %r)" % (a, axes))
    t = tuple(int(a) for a in t)
    if len(set(t)) != len(t):
        raise ValueError("axes: %r names an axis twice" % (axes,))
    if weights is None:
        return t, None
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError("axis_weights must be one positive finite number per axis, got %r" % (weights,))
    if len(w) != len(t):
        raise ValueError("axis_weights: %d weights %r for the %d axes %r" % (len(w), weights, len(t), t))
    for v in w:
        if not 0.0 < v < math.inf:
            raise ValueError("axis_weights: %r is not a positive finite number (in %r)" % (v, weights))
    return t, w


PREFILTER_TRUNCATE = 4.0
MAX_PREFILTER_RADIUS = 32            # pnp_volume_smooth's


def gaussian_weights(sigma, truncate=PREFILTER_TRUNCATE):
    """the taps of scipy.ndimage.gaussian_filter1d(sigma, truncate=truncate): R = int(truncate * sigma + 0.5), w_k = exp(-k^2 / (2 sigma^2))
    for k = -R .. R in float64, divided by their sum, rounded once to float32 -> float32 [2 R + 1], or None when R == 0 (sigma < 0.125 at
    truncate 4: the axis is not filtered).  sigma must be a finite number >= 0 with R <= 32 (sigma <= 8.1 at truncate 4): ValueError."""
    try:
        sg = float(sigma)
    except (TypeError, ValueError):
        raise ValueError("prefilter: sigma must be a number, got %r" % (sigma,))
    if not 0.0 <= sg < math.inf:
        raise ValueError("prefilter: sigma must be a finite number >= 0, got %r" % (sigma,))
    R = int(float(truncate) * sg + 0.5)
    if R > MAX_PREFILTER_RADIUS:
        raise ValueError("prefilter: sigma = %r voxels needs a radius of %d taps, at most %d (sigma <= %.1f)"
                         % (sigma, R, MAX_PREFILTER_RADIUS, (MAX_PREFILTER_RADIUS + 0.4) / float(truncate)))
    if R == 0:
        return None
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sg * sg) * k ** 2)               # scipy's own expression (_gaussian_kernel1d)
    return (w / w.sum()).astype(np.float32)


def check_prefilter(prefilter):
    """None / "off" -> None; "auto" -> "auto"; a number or a triple (sigma in voxels, slicing order) -> a triple of floats, each accepted
    by gaussian_weights; anything else is a ValueError"""
    if prefilter is None or (isinstance(prefilter, str) and prefilter == "off"):
        return None
    if isinstance(prefilter, str):
        if prefilter != "auto":
            raise ValueError("prefilter must be None, 'off', 'auto', a sigma in voxels or three of them, got %r" % (prefilter,))
        return "auto"
    try:
        t = (float(prefilter),) * 3 if np.isscalar(prefilter) else tuple(float(v) for v in prefilter)
    except (TypeError, ValueError):
        raise ValueError("prefilter must be None, 'off', 'auto', a sigma in voxels or three of them, got %r" % (prefilter,))
    if len(t) != 3:
        raise ValueError("prefilter: three sigmas (sx, sy, sz) expected, got %r" % (prefilter,))
    for v in t:
        gaussian_weights(v)
    return t


def prefilter_sigmas(prefilter, dims, out_size, spacing=None, sample_mm=None):
    """(sigma_x, sigma_y, sigma_z) in voxels, slicing order, of the Gaussian that one volume of extents `dims` gets before it is sampled
    onto an `out_size` plane:
      None / "off"   zeros: nothing runs
      "auto"         sigma_a = max(0, (r_a - 1) / 2), skimage's default for resize(anti_aliasing=True), r_a = source voxels per output
                     sample along axis a: (pi_mm / sx, pj_mm / sy, frame_mm / sz) with sample_mm (and spacing = (sx, sy, sz) in mm),
                     (X / H, Y / W, 1) without it (the plain centre-aligned resize; neighbouring array frames)
      a number or a triple   sigma in voxels, taken as given
    The augmentation's `scale` and the scales of test-time-augmentation entries are deliberately ignored: the filter belongs to the
    nominal grid, is applied once per volume, and does not follow the per-sample zoom.  A sigma below 0.125 filters nothing
    (gaussian_weights); an upsampled axis (r <= 1) gets 0."""
    p = check_prefilter(prefilter)
    if p is None:
        return (0.0, 0.0, 0.0)
    if p != "auto":
        return p
    mm = check_sample_mm(sample_mm)
    if mm is not None:
        if spacing is None:
            raise ValueError("prefilter_sigmas: sample_mm needs the volume's spacing")
        sp = check_spacing(spacing)
        r = tuple(m / s for m, s in zip(mm, sp))
    else:
        r = (float(dims[0]) / float(out_size[0]), float(dims[1]) / float(out_size[1]), 1.0)
    sig = tuple(max(0.0, (v - 1.0) / 2.0) for v in r)
    for v in sig:
        gaussian_weights(v)                 # a reduction beyond the kernel's 32 taps is an error here, not a silent alias
    return sig


_SAMPLING_KEYS = ("centre", "classes", "foreground")


def check_sampling(sampling, num_cls):
    """foreground-aware slice sampling: None, or a dict with `foreground` (required: the probability in [0, 1] that a sample
    is centred on a class instead of a uniform frame), `classes` (None = 1 .. num_cls - 1, or a non-empty sequence of distinct ints in
    [1, num_cls)) and `centre` (bool, default False: also centre the plane on the class's bounding box in the frame) -> None (also for
    foreground == 0) / a dict with all three keys, classes a sorted tuple; anything else is a ValueError"""
    if sampling is None:
        return None
    if not isinstance(sampling, dict):
        raise ValueError("sampling must be None or a dict with the keys %s, got %r" % (list(_SAMPLING_KEYS), sampling))
    unknown = sorted(set(sampling) - set(_SAMPLING_KEYS), key=str)
    if unknown:
        raise ValueError("sampling: unknown keys %s (known: %s)" % (unknown, list(_SAMPLING_KEYS)))
    if "foreground" not in sampling:
        raise ValueError("sampling: the key foreground (a probability in [0, 1]) is required, got %r" % (sampling,))
    num_cls = int(num_cls)
    p = sampling["foreground"]
    if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("sampling: foreground must be a probability in [0, 1], got %r" % (p,))
    centre = sampling.get("centre", False)
    if not isinstance(centre, (bool, np.bool_)):
        raise ValueError("sampling: centre must be a bool, got %r" % (centre,))
    classes = sampling.get("classes")
    if classes is None:
        classes = tuple(range(1, num_cls))
        if not classes:
            raise ValueError("sampling: num_cls = %d leaves no foreground class" % num_cls)
    else:
        if isinstance(classes, (str, bytes)) or not hasattr(classes, "__iter__"):
            raise ValueError("sampling: classes must be None or a sequence of distinct classes in [1, %d), got %r" % (num_cls, classes))
        t = tuple(classes)
        if not t:
            raise ValueError("sampling: classes is empty, got %r" % (classes,))
        for c in t:
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 1 <= c < num_cls:
                raise ValueError("sampling: class %r is not an int in [1, %d) (in %r)" % (c, num_cls, classes))
        if len(set(int(c) for c in t)) != len(t):
            raise ValueError("sampling: classes %r names a class twice" % (classes,))
        classes = tuple(sorted(int(c) for c in t))
    if float(p) == 0.0:
        return None
    return {"foreground": float(p), "classes": classes, "centre": bool(centre)}


def _draw_foreground(rng3, table, classes):
    """the foreground draw of one sample from one volume entry's table [Z, ncls, 5]: (class, frame), or (0, None) when none of `classes`
    (ascending) has a voxel in the frames 1 .. Z - 2 the gather accepts.  The class is uniform among those present, the frame is the frame
    of a uniformly drawn voxel of the class."""
    Z = table.shape[0]
    counts = np.asarray(table[1:Z - 1, :, 0], dtype=np.int64)
    totals = counts.sum(axis=0)
    present = [c for c in classes if totals[c] > 0]
    if not present:
        return 0, None
    c = present[int(rng3.integers(len(present)))]
    k = int(rng3.integers(int(totals[c])))
    return c, 1 + int(np.searchsorted(np.cumsum(counts[:, c]), k, side="right"))


def sample_params(rng, dims, batch_size, out_hw, augment, sample_mm=None, spacings=None, *, rng2=None, sampling=None, frame_stats=None,
                  rng3=None):
    """B draws from `rng` (numpy Generator) -> (records [B] of _lib.AugSample layout, raw draws as a dict of arrays).
    dims: [(X, Y, Z)] per volume.  Every sample draws volume and frame; with augment, rotation, log-scale, two translations and the flip
    coin follow in that order, whatever their ranges — the stream of a seed does not depend on which ranges are zero.
    With sample_mm (and spacings: [(sx, sy, sz)] per volume) the same values are drawn in the same order; the records are of
    _lib.AugSampleZ layout with dz = frame_mm / sz, the map is compose_matrix's millimetre form and the translations are millimetres.
    With a non-zero elastic / contrast / brightness / noise the records are of _lib.AugSampleW layout (dz = 1 without
    sample_mm) and `rng2`, a second Generator, gives per sample, in this order: the control points (only when elastic > 0:
    (G + 3)^2 x 2 normals of sigma `elastic` output pixels, clipped at +-3 sigma), the log-gain, the bias, the noise sigma and the 32-bit
    noise seed.  `rng` is read exactly as without those keys.  raw gains ctrl ([B, G + 3, G + 3, 2] float32 in SOURCE voxels — the draws
    mapped through the linear part of the sample's float32 map in float64 — or None), ctrl_px (the draws, output pixels), gain, bias,
    noise, seed.
    With sampling (check_sampling's dict), frame_stats (one int32 table [Z, ncls, 5] per volume: VolumeSet.frame_stats) and
    `rng3`, a third Generator: `rng` is read exactly as without it — volume, the uniform frame, the augment draws — then u = rng3.random();
    u < foreground makes the sample a foreground sample: its frame is redrawn from rng3 (_draw_foreground; a volume without any of the
    classes in its eligible frames keeps the uniform frame: raw["fallback"]), and with `centre` the offset of the class's bounding-box
    centre in that frame from the slice centre, in voxels, is added to the translation (times the in-plane spacing with sample_mm, whose
    translation is millimetres).  raw gains fg_class (0: a uniform sample), fallback and centre ([B, 2], the offsets added, in voxels).
    sampling=None: nothing of this is read or drawn."""
    B = int(batch_size)
    mm = check_sample_mm(sample_mm)
    if mm is not None and (spacings is None or len(spacings) != len(dims)):
        raise ValueError("sample_params: sample_mm needs one spacing per volume")
    warp = uses_warp_entry(augment)
    if warp and rng2 is None:
        raise ValueError("sample_params: elastic / contrast / brightness / noise draw from a second generator: pass rng2")
    rec = np.zeros(B, dtype=SAMPLE_W_DTYPE if warp else SAMPLE_DTYPE if mm is None else SAMPLE_Z_DTYPE)
    raw = {k: np.zeros(B) for k in ("rotate", "scale", "tx", "ty")}
    raw["flip"] = np.zeros(B, dtype=bool)
    raw["scale"][:] = 1.0
    if sampling is not None:
        if frame_stats is None or len(frame_stats) != len(dims) or rng3 is None:
            raise ValueError("sample_params: foreground sampling needs one frame table per volume (frame_stats) and a third generator (rng3)")
        sampling = check_sampling(sampling, frame_stats[0].shape[1])
    if sampling is not None:
        raw["fg_class"], raw["fallback"], raw["centre"] = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool), np.zeros((B, 2))
    for b in range(B):
        v = int(rng.integers(0, len(dims)))
        X, Y, Z = dims[v]
        z = int(rng.integers(1, Z - 1))           # [1, Z - 2]
        if augment is not None:
            raw["rotate"][b] = rng.uniform(-augment["rotate"], augment["rotate"])
            ls = math.log1p(augment["scale"])
            raw["scale"][b] = math.exp(rng.uniform(-ls, ls))
            raw["tx"][b] = rng.uniform(-augment["translate"], augment["translate"])
            raw["ty"][b] = rng.uniform(-augment["translate"], augment["translate"])
            raw["flip"][b] = rng.random() < augment["flip"]
        tx, ty = raw["tx"][b], raw["ty"][b]
        if sampling is not None and rng3.random() < sampling["foreground"]:
            table = frame_stats[v]
            if tuple(table.shape[::2]) != (Z, 5):
                raise ValueError("sample_params: the frame table of volume %d is %s, the volume has %d frames" % (v, table.shape, Z))
            c, zf = _draw_foreground(rng3, table, sampling["classes"])
            if zf is None:
                raw["fallback"][b] = True
            else:
                raw["fg_class"][b], z = c, zf
                if sampling["centre"]:
                    _, xmin, xmax, ymin, ymax = (float(t) for t in table[z, c])
                    raw["centre"][b] = ((xmin + xmax) / 2.0 - (X - 1) / 2.0, (ymin + ymax) / 2.0 - (Y - 1) / 2.0)
                    unit = (1.0, 1.0) if mm is None else spacings[v][:2]
                    tx, ty = tx + raw["centre"][b, 0] * unit[0], ty + raw["centre"][b, 1] * unit[1]
        rec["volume"][b], rec["frame"][b] = v, z
        geom = {}
        if mm is not None:
            sx, sy, sz = spacings[v]
            geom = {"spacing_xy": (sx, sy), "pixel_mm": mm[:2]}
            rec["dz"][b] = np.float32(mm[2] / sz)
        elif warp:
            rec["dz"][b] = 1.0
        rec["m"][b] = compose_matrix((X, Y), out_hw, raw["rotate"][b], raw["scale"][b], (tx, ty), bool(raw["flip"][b]), **geom)
    if warp:
        _sample_warp(rng2, rec, raw, out_hw, augment)
    return rec, raw


def _sample_warp(rng2, rec, raw, out_hw, augment):
    """the draws of DESIGN.md §18 from the second generator, into the records' gain / bias / noise / seed / warp and raw"""
    B = len(rec)
    check_elastic_fold(augment, out_hw)
    G = elastic_grid_of(augment)
    sigma = float(augment.get("elastic", 0.0))
    lc = math.log1p(augment.get("contrast", 0.0))
    br, nz = float(augment.get("brightness", 0.0)), float(augment.get("noise", 0.0))
    raw["ctrl_px"] = np.zeros((B, G + 3, G + 3, 2)) if G else None
    raw["gain"], raw["bias"], raw["noise"] = np.zeros(B), np.zeros(B), np.zeros(B)
    raw["seed"] = np.zeros(B, dtype=np.uint32)
    for b in range(B):
        if G:
            raw["ctrl_px"][b] = np.clip(rng2.standard_normal((G + 3, G + 3, 2)) * sigma, -3.0 * sigma, 3.0 * sigma)
        raw["gain"][b] = math.exp(rng2.uniform(-lc, lc))
        raw["bias"][b] = rng2.uniform(-br, br)
        raw["noise"][b] = rng2.uniform(0.0, nz)
        raw["seed"][b] = rng2.integers(0, 1 << 32, dtype=np.uint64)
    rec["gain"], rec["bias"], rec["noise"], rec["seed"], rec["warp"] = raw["gain"], raw["bias"], raw["noise"], raw["seed"], 1 if G else 0
    raw["ctrl"] = control_to_source(raw["ctrl_px"], rec["m"]) if G else None


def control_to_source(ctrl_px, ms):
    """control-point displacements (di, dj) in output pixels [B, n, n, 2] -> (dx, dy) in source voxels, float32: the linear part
    (m00, m01; m10, m11) of each sample's float32 map, applied in float64"""
    m = np.asarray(ms, dtype=np.float32).astype(np.float64).reshape(-1, 6)
    lin = m[:, [0, 1, 3, 4]].reshape(-1, 1, 1, 2, 2)
    return np.einsum("bnmxy,bnmy->bnmx", np.broadcast_to(lin, ctrl_px.shape[:3] + (2, 2)), np.asarray(ctrl_px, dtype=np.float64)).astype(np.float32)


VOLUME_DTYPE = np.dtype([("image", "<u8"), ("label", "<u8"), ("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("fill", "<f4")])
SAMPLE_DTYPE = np.dtype([("volume", "<i4"), ("frame", "<i4"), ("m", "<f4", (6,))])
SAMPLE_Z_DTYPE = np.dtype([("volume", "<i4"), ("frame", "<i4"), ("dz", "<f4"), ("m", "<f4", (6,))])
assert VOLUME_DTYPE.itemsize == ctypes.sizeof(_lib.AugVolume) and SAMPLE_DTYPE.itemsize == ctypes.sizeof(_lib.AugSample)
assert SAMPLE_Z_DTYPE.itemsize == ctypes.sizeof(_lib.AugSampleZ) == 36
SAMPLE_W_DTYPE = np.dtype([("volume", "<i4"), ("frame", "<i4"), ("dz", "<f4"), ("m", "<f4", (6,)), ("gain", "<f4"), ("bias", "<f4"), ("noise", "<f4"),
                           ("seed", "<u4"), ("warp", "<i4")])
assert SAMPLE_W_DTYPE.itemsize == ctypes.sizeof(_lib.AugSampleW) == 56
assert all(SAMPLE_W_DTYPE.fields[n][1] == getattr(_lib.AugSampleW, n).offset for n in SAMPLE_W_DTYPE.names)


def label_bounding_box(label, margin):
    """(slices per axis) of the non-zero labels grown by `margin` voxels and clamped to the volume; the whole volume when it has no label"""
    nz = np.nonzero(label)
    if len(nz[0]) == 0:
        return tuple(slice(0, n) for n in label.shape)
    return tuple(slice(max(int(a.min()) - margin, 0), min(int(a.max()) + 1 + margin, n)) for a, n in zip(nz, label.shape))


def prepare_pair(image, label, flip_correction=True, axis=2, crop=None, box_out=None):
    """host numpy, once per volume: the double flip of volume_eval.test_eval, `axis` moved last, the optional crop to the label bounding
    box plus `crop` voxels -> (float32 image [X, Y, Z], uint8 label [X, Y, Z]), both C-contiguous.  box_out: a list that receives the
    box of a crop, ((x0, x1), (y0, y1), (z0, z1)) half-open"""
    image, label = np.asarray(image), np.asarray(label)
    if image.ndim != 3 or image.shape != label.shape:
        raise ValueError("image %s / label %s: a 3-D pair of equal shape expected" % (image.shape, label.shape))
    if flip_correction:
        image = np.flip(np.flip(image, axis=0), axis=1)
        label = np.flip(np.flip(label, axis=0), axis=1)
    image, label = np.moveaxis(image, axis, -1), np.moveaxis(label, axis, -1)
    if label.dtype.kind == "f" and not np.all(label == np.floor(label)):
        raise ValueError("labels must be integer-valued")
    if label.size and (label.min() < 0 or label.max() > 255):
        raise ValueError("labels outside [0, 255] (%s .. %s)" % (label.min(), label.max()))
    if crop is not None:
        box = label_bounding_box(label, int(crop))
        image, label = image[box], label[box]
        if box_out is not None:
            box_out.append(tuple((sl.start, sl.stop) for sl in box))
    if not np.all(np.isfinite(image)):
        raise ValueError("the image holds non-finite voxels")
    return np.ascontiguousarray(image, dtype=np.float32), np.ascontiguousarray(label, dtype=np.uint8)


def _device_body_box(img, device, percentile, margin):
    """body.body_box of a prepared host volume: uploaded whole, released when the box is known"""
    import torch
    from . import body
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PnpError("VolumeSet: pnp kernels need a CUDA/HIP device (got %s) — there is no CPU fallback" % (dev,))
    return body.body_box(torch.from_numpy(img).to(dev), percentile=percentile, margin=margin)


class VolumeSet(object):
    """Normalised volumes resident on `device`.  pairs: [(image path, label path)] (read_pairs).  Per volume, in this order: the double
    flip volume_eval.test_eval applies (flip_correction), `axis` moved last (the slicing axis), crop=None or a margin in voxels around
    the label bounding box, upload, pnp_volume_preprocess (clip at the `percentile` order statistic, z-score).
    Unlabelled volumes and the body crop: a pair's label path may be None — the entry then gets an all-zero uint8 label
    volume (the gather kernels and their descriptor table do not change) and .has_labels, one bool per entry, says so.  crop="body" or
    ("body", margin): the prepared full volume is uploaded, body.body_box finds the patient on the device without a label, image and label
    are cropped to that box and pnp_volume_preprocess runs on the crop (the stats are the crop's).  .boxes: per entry the box used,
    ((x0, x1), (y0, y1), (z0, z1)) half-open in the entry's order, for either crop; None without a crop.  With several axes the box of a
    pair is found once, on its first axis, and permuted for the others.  An int crop needs a label: ValueError for an entry without one.
    .images / .labels: device tensors [X, Y, Z] float32 / uint8;  .stats: [{clip, mean, std, fill}];  .names: image basenames;
    .spacings: [(sx, sy, sz)] in mm, slicing order (from the image's affine; from_arrays / from_device: spacings=, default 1 mm).
    Multi-planar training: `axis` may be a sequence of distinct axes (check_axes).  The set then holds one resident entry
    per (pair, axis), pair-major and axis-minor, each prepared exactly as above with its own axis and its own slicing_spacing; with more
    than one axis an entry's name is <basename>@<axis>, with an int or a one-element sequence names are the basenames.  sample_params
    draws the ENTRY uniformly, so every orientation gets an equal share of every volume's samples.  Residency grows by the number of
    axes: 20 scans of 256 x 256 x 200 on three axes are about 3 GB of image plus 0.8 GB of label.  .axes: the axes, in order."""

    def __init__(self, pairs, device, flip_correction=True, axis=2, crop=None, percentile=98):
        from . import nifti
        from . import body
        axes = (axis,) if isinstance(axis, (int, np.integer)) and not isinstance(axis, bool) else check_axes(axis)[0]
        kind = body.parse_crop(crop)
        arrays, names, spacings, has_labels, boxes = [], [], [], [], []
        for image_fid, label_fid in pairs:
            image = nifti.load(image_fid)
            data = image.get_data()
            if label_fid is None and kind is not None and kind[0] == "label":
                raise ValueError("%s has no label: crop=%r is a margin around the label bounding box (crop=\"body\" needs none)" % (image_fid, crop))
            label = np.zeros(np.shape(data), dtype=np.uint8) if label_fid is None else nifti.load(label_fid).get_data()
            file_box = None          # the pair's body box in file order (after the flips), found on its first axis
            for ax in axes:
                if kind is None:
                    img, lab = prepare_pair(data, label, flip_correction, ax, None)
                    boxes.append(None)
                elif kind[0] == "label":
                    img, lab = prepare_pair(data, label, flip_correction, ax, crop, box_out=boxes)
                else:
                    img, lab = prepare_pair(data, label, flip_correction, ax, None)
                    if file_box is None:
                        file_box = body.unpermute_box(_device_body_box(img, device, percentile, kind[1]), ax)
                    box = body.permute_box(file_box, ax)
                    img, lab = np.ascontiguousarray(img[body.box_slices(box)]), np.ascontiguousarray(lab[body.box_slices(box)])
                    boxes.append(box)
                arrays.append((img, lab))
                has_labels.append(label_fid is not None)
                names.append(os.path.basename(str(image_fid)) + ("@%d" % ax if len(axes) > 1 else ""))
                spacings.append(slicing_spacing(image.affine, ax, str(image_fid)))
        self.axes = tuple(int(a) for a in axes)
        self._build(arrays, names, device, percentile)
        self.spacings = spacings
        self.has_labels = has_labels
        self.boxes = boxes if kind is not None else None

    @classmethod
    def from_arrays(cls, images, labels, names, device, percentile=98, spacings=None):
        """volumes already in slicing order [X, Y, Z] (no flip, no crop): float32-convertible images, integer labels in [0, 255];
        spacings: one (sx, sy, sz) in mm per volume (default: 1 mm).  A label may be None: an unlabelled volume (all-zero labels,
        has_labels False)"""
        self = cls.__new__(cls)
        arrays = [prepare_pair(i, np.zeros(np.shape(i), dtype=np.uint8) if l is None else l, flip_correction=False, axis=2, crop=None)
                  for i, l in zip(images, labels)]
        self._build(arrays, [str(n) for n in names], device, percentile)
        self.has_labels = [l is not None for l in labels]
        self.boxes = None
        self._set_spacings(spacings)
        return self

    def _set_spacings(self, spacings):
        if spacings is None:
            self.spacings = [(1.0, 1.0, 1.0)] * len(self.names)
            return
        if len(spacings) != len(self.names):
            raise ValueError("VolumeSet: %d spacings for %d volumes" % (len(spacings), len(self.names)))
        self.spacings = [check_spacing(sp, name) for sp, name in zip(spacings, self.names)]

    @classmethod
    def from_device(cls, images, labels, names, fills, percentile=98, spacings=None, min_frames=3):
        """volumes that are on the device and normalised already (volume_predict.py pads a normalised volume with copies of its edge
        frames): contiguous float32 / uint8 tensors [X, Y, Z] in slicing order, one fill value per volume.  Nothing is copied or computed.
        spacings: one (sx, sy, sz) in mm per volume (default: 1 mm); min_frames=1: a set only pnp_aug_slices_z will read."""
        import torch
        self = cls.__new__(cls)
        if not images or not (len(images) == len(labels) == len(names) == len(fills)):
            raise ValueError("VolumeSet.from_device: images, labels, names and fills must be equally long and not empty")
        self.device = images[0].device
        for v, l, name in zip(images, labels, names):
            if not (v.is_cuda and l.is_cuda):
                raise _lib.PnpError("VolumeSet: pnp kernels need a CUDA/HIP device (got %s) — there is no CPU fallback" % (v.device,))
            if v.dtype != torch.float32 or l.dtype != torch.uint8 or v.shape != l.shape or v.dim() != 3 or not (v.is_contiguous() and l.is_contiguous()):
                raise ValueError("%s: a contiguous float32 image and uint8 label of one 3-D shape expected" % name)
            if v.shape[2] < int(min_frames) or v.shape[0] > 4096 or v.shape[1] > 4096:
                raise ValueError("%s: volume %s needs at least %d frames and slice extents <= 4096" % (name, tuple(v.shape), int(min_frames)))
        self.names, self.percentile = [str(n) for n in names], int(percentile)
        self._set_spacings(spacings)
        self.images, self.labels = list(images), list(labels)
        self.dims = [tuple(int(d) for d in v.shape) for v in self.images]
        self.stats = [{"clip": None, "mean": None, "std": None, "fill": float(f)} for f in fills]
        self.has_labels = [True] * len(self.images)
        self.boxes = None
        self.set_fill(None)
        return self

    def _build(self, arrays, names, device, percentile):
        import torch
        from . import kernels as K
        if not arrays:
            raise ValueError("VolumeSet: no volume")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PnpError("VolumeSet: pnp kernels need a CUDA/HIP device (got %s) — there is no CPU fallback" % (self.device,))
        self.names, self.percentile = list(names), int(percentile)
        self.images, self.labels, stats = [], [], []
        for (img, lab), name in zip(arrays, names):
            X, Y, Z = img.shape
            if Z < 3 or X > 4096 or Y > 4096:
                raise ValueError("%s: volume %s needs at least 3 frames and slice extents <= 4096" % (name, img.shape))
            v = torch.from_numpy(img).to(self.device)
            _, st = K.volume_preprocess(v, self.percentile, out=v)
            self.images.append(v)
            self.labels.append(torch.from_numpy(lab).to(self.device))
            stats.append(st)
        self.dims = [tuple(int(d) for d in v.shape) for v in self.images]
        host = torch.stack(stats).cpu().numpy()          # one read for the whole set: the fill values enter the descriptor table
        self.stats = [{"clip": float(r[0]), "mean": float(r[1]), "std": float(r[2]), "fill": float(r[3])} for r in host]
        self.set_fill(None)

    def set_fill(self, fill):
        """fill value of image corners outside the slice: None = each volume's normalised minimum (its background), or one number"""
        import torch
        self._fill = fill
        tab = np.zeros(len(self.images), dtype=VOLUME_DTYPE)
        for n, (v, l) in enumerate(zip(self.images, self.labels)):
            tab[n] = (v.data_ptr(), l.data_ptr()) + self.dims[n] + (self.stats[n]["fill"] if fill is None else float(fill),)
        self._table_host_np = tab
        self.table_host = (_lib.AugVolume * len(tab)).from_buffer(tab)          # shares tab's memory
        self.table_dev = torch.from_numpy(tab.view(np.uint8).copy()).to(self.device)

    @property
    def sigmas(self):
        """per volume: None before apply_prefilter, the (sigma_x, sigma_y, sigma_z) it was smoothed with after"""
        return getattr(self, "_sigmas", None) or [None] * len(self.images)

    def apply_prefilter(self, sigmas):
        """the anti-alias prefilter of DESIGN.md §19: sigmas = one (sigma_x, sigma_y, sigma_z) in voxels per volume (prefilter_sigmas);
        every image is replaced by its Gaussian-smoothed version (pnp_volume_smooth, in place: one volume-sized scratch buffer is alive
        while this runs and is released at the end), the descriptor table is rebuilt with the fill that is set.  Labels, stats and the
        fill values stay those of the unsmoothed volume (a convex combination cannot go below the minimum: the fill is still a lower
        bound).  A second call with the same values does nothing; other values raise — a set must not be filtered twice."""
        from . import kernels as K
        if len(sigmas) != len(self.images):
            raise ValueError("VolumeSet.apply_prefilter: %d sigma triples for %d volumes" % (len(sigmas), len(self.images)))
        new = [check_prefilter(tuple(s)) or (0.0, 0.0, 0.0) for s in sigmas]
        if getattr(self, "_sigmas", None) is not None:
            if self._sigmas == new:
                return
            raise ValueError("VolumeSet.apply_prefilter: the set is already filtered with %r; %r would filter it twice" % (self._sigmas, new))
        for v, sg in zip(self.images, new):
            w = [gaussian_weights(s) for s in sg]
            if any(t is not None for t in w):
                K.volume_smooth(v, w, out=v)
        K.drop_workspace("smooth")
        self._sigmas = new
        fill = getattr(self, "_fill", None)
        self.set_fill(fill)

    def frame_stats(self, num_cls):
        """per resident entry the class table of its label volume: numpy int32 [Z, num_cls, 5], per frame and class the
        voxel count and the bounding box (xmin, xmax, ymin, ymax), (0, X, -1, Y, -1) for an absent class.  pnp_label_frame_stats on every
        label volume in one pass, ONE copy to the host for the whole set, cached per num_cls (labels never change: the prefilter leaves
        them alone).  Only foreground sampling asks for it."""
        import torch
        from . import kernels as K
        num_cls = int(num_cls)
        cache = self.__dict__.setdefault("_frame_stats", {})
        if num_cls not in cache:
            tables = [K.label_frame_stats(l, num_cls) for l in self.labels]
            host = torch.cat([t.reshape(-1) for t in tables]).cpu().numpy()
            ends = np.cumsum([t.numel() for t in tables])
            cache[num_cls] = [host[e - t.numel():e].reshape(tuple(t.shape)) for t, e in zip(tables, ends)]
        return cache[num_cls]

    def __len__(self):
        return len(self.images)


class AugmentedSliceSource(object):
    """Endless stream of augmented slices of a VolumeSet.
      augment   None = identity: a centre-aligned resize, the raw normalised frames bit for bit when (X, Y) = out_size;
                a dict with any of DEFAULT_AUGMENT's keys otherwise (the default: DEFAULT_AUGMENT)
      seed      the parameter stream is numpy.random.default_rng(seed + rank_seed(rank)): reproducible, and ranks differ
      shard     (rank, world) under data parallelism, as the trainers pass it; every rank holds all volumes and draws its own samples
    next_device_batch() -> (x [B,H,W,3], one-hot [B,H,W,num_cls], fids) on the device, on the current stream (what feeder.DeviceFeeder drives);
    next_batch(B) -> ([B,H,W,4] numpy: image channels 0:3, label map in channel 3, fids): the trainers' source protocol.
    A fid is "<image basename>#<frame>".
      sample_mm None, or a number / (pi_mm, pj_mm, frame_mm): sample on that millimetre grid — the plane map carries the
                pixel size, the outer channels lie frame_mm from the centre frame (pnp_aug_slices_z), augment's translate is in mm.
    With a non-zero elastic, contrast, brightness or noise in `augment` the batches come from pnp_aug_slices_warp: the
    records are SAMPLE_W_DTYPE, the new parameters are drawn from a second generator, default_rng([seed + rank_seed(rank), 1]) — the
    classic fields of a seed's records do not depend on the new keys — and last_ctrl holds the batch's control table (or None).
      prefilter None / "off", "auto" or sigmas in voxels: the per-volume sigmas follow from this source's out_size /
                sample_mm and the set's dims / spacings (prefilter_sigmas) and the SET is smoothed once, here (VolumeSet.apply_prefilter):
                a set shared with another source must get the same sigmas from it.
      sampling  None, or check_sampling's dict: a share `foreground` of the samples takes the frame of a random voxel of a
                random class present in its volume (and with `centre` the plane centred on that class in the frame) instead of a uniform
                frame.  The draws come from a third generator, default_rng([seed + rank_seed(rank), 2]): the volumes and augment draws of
                a seed do not depend on the option.  The set's class tables (VolumeSet.frame_stats) are computed here, once;
                sampling_report() counts what was drawn; last_draw holds the raw draws of the last batch (sample_params' dict).
    .labelled: every entry of the set has a label (VolumeSet.has_labels); a source that is not labelled delivers label 0 / one-hot class 0
    everywhere, the trainers skip the Dice of its batches, and foreground sampling on it is a ValueError."""

    def __init__(self, volumes, batch_size, out_size=(256, 256), augment=DEFAULT_AUGMENT, seed=0, shard=None, num_cls=5, sample_mm=None,
                 prefilter=None, sampling=None):
        import torch
        self.volumes, self.batch_size = volumes, int(batch_size)
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.augment = check_augment(augment)
        self.num_cls = int(num_cls)
        self.sample_mm = check_sample_mm(sample_mm)
        self.prefilter = check_prefilter(prefilter)
        if self.prefilter is not None:
            spacings = getattr(volumes, "spacings", None) or [None] * len(volumes.dims)
            volumes.apply_prefilter([prefilter_sigmas(self.prefilter, d, self.out_size, sp, self.sample_mm) for d, sp in zip(volumes.dims, spacings)])
        self.rank = shard[0] if shard else 0
        self.rng = np.random.default_rng(int(seed) + rank_seed(self.rank))
        self.warp = uses_warp_entry(self.augment)
        self.rng2 = np.random.default_rng([int(seed) + rank_seed(self.rank), 1]) if self.warp else None
        check_elastic_fold(self.augment, self.out_size)
        self.sampling = check_sampling(sampling, self.num_cls)
        self.labelled = all(getattr(volumes, "has_labels", None) or [True])
        if self.sampling and not self.labelled:
            raise ValueError("sampling: foreground-aware sampling reads the labels, and the set holds unlabelled volumes (%s)"
                             % ", ".join(n for n, h in zip(volumes.names, volumes.has_labels) if not h))
        self.rng3 = np.random.default_rng([int(seed) + rank_seed(self.rank), 2]) if self.sampling else None
        self._frame_stats = volumes.frame_stats(self.num_cls) if self.sampling else None
        self._drawn, self._fallbacks, self._fg = 0, 0, {c: 0 for c in (self.sampling or {}).get("classes", ())}
        self._errors = torch.zeros(1, dtype=torch.int32, device=volumes.device)
        self.last_params = self.last_ctrl = self.last_draw = None

    def _gather(self, batch_size, num_cls, want_onehot):
        B = int(batch_size or self.batch_size)
        rec, raw = sample_params(self.rng, self.volumes.dims, B, self.out_size, self.augment, self.sample_mm,
                                 getattr(self.volumes, "spacings", None), rng2=self.rng2, sampling=self.sampling,
                                 frame_stats=self._frame_stats, rng3=self.rng3)
        self._drawn += B
        self.last_draw = raw
        if self.sampling:
            self._fallbacks += int(raw["fallback"].sum())
            for c in raw["fg_class"][raw["fg_class"] > 0]:
                self._fg[int(c)] += 1
        return self.gather_records(rec, num_cls, want_onehot, ctrl=raw.get("ctrl")) + (rec,)

    def gather_records(self, rec, num_cls=None, want_onehot=True, ctrl=None):
        """the batch of given sample records (SAMPLE_DTYPE; SAMPLE_Z_DTYPE with sample_mm; SAMPLE_W_DTYPE with the elastic / intensity keys,
        then with ctrl = the control table [B, G + 3, G + 3, 2] float32 in source voxels, or None) -> (x, label, one-hot or None) on the device"""
        import torch
        from . import kernels as K
        vs = self.volumes
        H, W = self.out_size
        ncls = int(num_cls or self.num_cls)
        if self.warp:
            return self._gather_warp(rec, ctrl, ncls, want_onehot)
        if ctrl is not None:
            raise ValueError("gather_records: a control table needs a source with elastic / intensity augmentation")
        frac = self.sample_mm is not None
        rec = np.ascontiguousarray(rec, dtype=SAMPLE_Z_DTYPE if frac else SAMPLE_DTYPE)
        self.last_params = rec
        staged = torch.from_numpy(rec.view(np.uint8).copy()).pin_memory()
        sd = staged.to(vs.device, non_blocking=True)
        return (K.aug_slices_z if frac else K.aug_slices)(vs.table_host, vs.table_dev, len(vs), sd, len(rec), H, W,
                                                          self._errors, ncls=ncls, want_onehot=want_onehot)

    def _gather_warp(self, rec, ctrl, ncls, want_onehot):
        """records and control table travel in ONE pinned staging buffer and one copy; the table starts 56 B bytes into it (8-byte aligned)"""
        import torch
        from . import kernels as K
        vs = self.volumes
        rec = np.ascontiguousarray(rec, dtype=SAMPLE_W_DTYPE)
        B, G = len(rec), 0
        nrec = rec.nbytes
        if ctrl is not None:
            ctrl = np.ascontiguousarray(ctrl, dtype=np.float32)
            G = ctrl.shape[1] - 3 if ctrl.ndim == 4 else -1
            if G < 1 or ctrl.shape != (B, G + 3, G + 3, 2):
                raise ValueError("gather_records: the control table must be [B, G + 3, G + 3, 2] with G >= 1, got %s for B = %d" % (ctrl.shape, B))
        self.last_params, self.last_ctrl = rec, ctrl
        staged = torch.empty(nrec + (ctrl.nbytes if G else 0), dtype=torch.uint8).pin_memory()
        host = staged.numpy()
        host[:nrec] = rec.view(np.uint8)
        if G:
            host[nrec:] = ctrl.reshape(-1).view(np.uint8)
        both = staged.to(vs.device, non_blocking=True)
        cd = both[nrec:].view(torch.float32) if G else None
        return K.aug_slices_warp(vs.table_host, vs.table_dev, len(vs), both[:nrec], cd, G, B, self.out_size[0], self.out_size[1], self._errors,
                                 ncls=ncls, want_onehot=want_onehot)

    def _fids(self, rec):
        return ["%s#%d" % (self.volumes.names[int(v)], int(z)) for v, z in zip(rec["volume"], rec["frame"])]

    def next_device_batch(self, batch_size=None, num_cls=None):
        x, _, onehot, rec = self._gather(batch_size, num_cls, True)
        return x, onehot, self._fids(rec)

    def next_batch(self, batch_size=None):
        import torch
        x, label, _, rec = self._gather(batch_size, None, False)
        return torch.cat([x, label.unsqueeze(-1)], dim=-1).cpu().numpy(), self._fids(rec)

    def sampling_report(self):
        """what the sampler drew so far (host counters, no synchronisation): {"samples", "foreground": {class: samples centred on it},
        "fallback": foreground samples whose volume had none of the classes in an eligible frame — they kept their uniform frame};
        samples - sum(foreground) - fallback were plain uniform samples"""
        return {"samples": self._drawn, "foreground": dict(self._fg), "fallback": self._fallbacks}

    def errors(self):
        """samples the kernel refused so far (volume index or frame out of range; with sample_mm also a frame step that is not a finite
        number >= 0; a warp asked for without a control table): reads the device counter, i.e. synchronises"""
        return int(self._errors.item())

    def close(self):
        n = self.errors()
        if n:
            raise _lib.PnpError("AugmentedSliceSource: the gather refused %d samples (volume index or frame out of range); they were "
                                "delivered as fill / label 0" % n)


def sources_from_lists(train_list, val_list, device, batch_size, num_cls, augment=DEFAULT_AUGMENT, seed=0, shard=None, sample_mm=None,
                       prefilter=None, axes=None, sampling=None, crop=None, labels="required"):
    """the two sources of a trainer from two list files: the training one augmented, the validation one with augment=None; sample_mm and
    prefilter (AugmentedSliceSource's) hold for both, and so does axes (None: the default slicing axis; a sequence: VolumeSet's
    multi-planar set, DESIGN.md §21 — one resident entry per volume and axis); sampling (foreground-aware frames) goes to
    the training source only: validation stays uniform; crop (VolumeSet's: None, a label margin, "body" or ("body", margin)) and labels
    (read_pairs': "optional" admits image-only lines) hold for both lists"""
    which = {} if axes is None else {"axis": check_axes(axes)[0]}
    if crop is not None:
        which["crop"] = crop
    train = AugmentedSliceSource(VolumeSet(read_pairs(train_list, labels), device, **which), batch_size, augment=augment, seed=seed, shard=shard,
                                 num_cls=num_cls, sample_mm=sample_mm, prefilter=prefilter, sampling=sampling)
    val = AugmentedSliceSource(VolumeSet(read_pairs(val_list, labels), device, **which), batch_size, augment=None, seed=seed + 1, shard=shard,
                               num_cls=num_cls, sample_mm=sample_mm, prefilter=prefilter)
    return train, val


def parse_sample_mm(text):
    """--sample-mm: 'MM' or 'PI,PJ,FRAME' -> check_sample_mm's triple (None stays None)"""
    if text is None:
        return None
    parts = str(text).split(",")
    try:
        vals = [float(p) for p in parts]
    except ValueError:
        raise ValueError("--sample-mm: %r is not a number or three numbers PI,PJ,FRAME" % (text,))
    if len(vals) not in (1, 3):
        raise ValueError("--sample-mm: one number or three numbers PI,PJ,FRAME expected, got %r" % (text,))
    try:
        return check_sample_mm(vals[0] if len(vals) == 1 else vals)
    except ValueError as e:
        raise ValueError("--sample-mm: %s" % e)


def add_sample_mm_flag(ap):
    ap.add_argument("--sample-mm", default=None, metavar="MM|PI,PJ,FRAME", help="sample NIfTI volumes on a millimetre grid: the size of an "
                    "output pixel and the distance between the three channels' frames, whatever the voxel size in the header (one number: "
                    "isotropic); default: the whole slice squeezed onto the plane, neighbouring array frames")


def sample_mm_from_args(ap, args):
    try:
        return parse_sample_mm(args.sample_mm)
    except ValueError as e:
        ap.error(str(e))


def parse_prefilter(text):
    """--prefilter: 'off' / None -> None, 'auto' -> "auto", 'SX,SY,SZ' (or one number) -> check_prefilter's triple of sigmas in voxels"""
    if text is None or str(text) == "off":
        return None
    if str(text) == "auto":
        return "auto"
    try:
        vals = [float(p) for p in str(text).split(",")]
    except ValueError:
        raise ValueError("--prefilter: %r is not auto, off or sigmas SX,SY,SZ in voxels" % (text,))
    if len(vals) not in (1, 3):
        raise ValueError("--prefilter: auto, off, one sigma or three sigmas SX,SY,SZ expected, got %r" % (text,))
    try:
        return check_prefilter(vals[0] if len(vals) == 1 else vals)
    except ValueError as e:
        raise ValueError("--prefilter: %s" % e)


def add_prefilter_flag(ap):
    ap.add_argument("--prefilter", default="off", metavar="auto|off|SX,SY,SZ", help="anti-alias prefilter of the NIfTI volumes before they are "
                    "sampled (a Gaussian on the device): auto = sigma (r - 1) / 2 voxels per axis for r voxels per output sample (from "
                    "--sample-mm and the voxel size, else from the resize), SX,SY,SZ = sigmas in voxels; train and predict with the same "
                    "setting (default: off)")


def prefilter_from_args(ap, args):
    try:
        return parse_prefilter(args.prefilter)
    except ValueError as e:
        ap.error(str(e))


def parse_axes(text):
    """--axes: 'A[,B[,C]]' -> check_axes' tuple of distinct axes from 0, 1, 2 (None stays None)"""
    if text is None:
        return None
    parts = str(text).split(",")
    if not all(p.strip().lstrip("+").isdigit() for p in parts):
        raise ValueError("--axes: %r is not a comma-separated list of axes from 0, 1, 2" % (text,))
    try:
        return check_axes([int(p) for p in parts])[0]
    except ValueError as e:
        raise ValueError("--axes: %s" % e)


def parse_axis_weights(text, axes):
    """--axis-weights: 'W[,W[,W]]', one positive finite number per axis of --axes -> a tuple of floats (None stays None)"""
    if text is None:
        return None
    if axes is None:
        raise ValueError("--axis-weights goes with --axes")
    try:
        vals = [float(p) for p in str(text).split(",")]
    except ValueError:
        raise ValueError("--axis-weights: %r is not a comma-separated list of numbers" % (text,))
    try:
        return check_axes(axes, vals)[1]
    except ValueError as e:
        raise ValueError("--axis-weights: %s" % e)


def add_axes_flag(ap, weights=False):
    ap.add_argument("--axes", default=None, metavar="A[,B[,C]]", help="multi-planar: the slicing axes of the NIfTI volumes, distinct axes from "
                    "0, 1, 2 (e.g. 0,1,2: sagittal, coronal and axial slices of an RAS file); training holds every volume once per axis, "
                    "prediction runs once per axis and fuses the probability volumes (default: the one default axis)")
    if weights:
        ap.add_argument("--axis-weights", default=None, metavar="W[,W[,W]]", help="with --axes: one positive weight per axis for the fusion "
                        "(default: all 1)")


def axes_from_args(ap, args):
    """-> the axes, or (axes, weights) for a parser that was given add_axes_flag(weights=True)"""
    try:
        axes = parse_axes(args.axes)
        if hasattr(args, "axis_weights"):
            return axes, parse_axis_weights(args.axis_weights, axes)
        return axes
    except ValueError as e:
        ap.error(str(e))


def parse_foreground_classes(text):
    """--foreground-classes: 'C[,C..]' -> a list of ints (None stays None); check_sampling judges the values"""
    if text is None:
        return None
    parts = str(text).split(",")
    if not all(p.strip().lstrip("+").isdigit() for p in parts):
        raise ValueError("--foreground-classes: %r is not a comma-separated list of class numbers" % (text,))
    return [int(p) for p in parts]


def add_sampling_flags(ap, what="the NIfTI training source"):
    ap.add_argument("--foreground", type=float, default=None, metavar="P", help="foreground-aware slice sampling of %s: this share of the "
                    "samples (a probability in [0, 1]) takes the frame of a random voxel of a random class present in its volume instead of "
                    "a uniform frame (default: every frame uniform)" % what)
    ap.add_argument("--foreground-classes", default=None, metavar="C[,C..]", help="with --foreground: the classes to centre samples on "
                    "(default: every class but 0)")
    ap.add_argument("--foreground-centre", action="store_true", help="with --foreground: also centre the plane of such a sample on the "
                    "class's bounding box in its frame (for --sample-mm planes smaller than the scan)")


def sampling_from_args(ap, args, num_cls=5):
    """-> check_sampling's dict or None; --foreground-classes / --foreground-centre without --foreground is a parser error"""
    if args.foreground is None:
        if args.foreground_classes is not None or args.foreground_centre:
            ap.error("--foreground-classes and --foreground-centre go with --foreground")
        return None
    try:
        return check_sampling({"foreground": args.foreground, "classes": parse_foreground_classes(args.foreground_classes),
                               "centre": bool(args.foreground_centre)}, num_cls)
    except ValueError as e:
        ap.error("--foreground: %s" % e)


def add_augment_flags(ap):
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--augment", default=None, metavar="JSON", help="augmentation ranges of the NIfTI training sources, e.g. "
                   "'{\"rotate\": 15, \"scale\": 0.1, \"translate\": 10, \"flip\": 0}' (the default); opt-in keys: \"elastic\" (sigma of the "
                   "control points of a B-spline warp, output pixels), \"elastic_grid\" (cells per axis, 1..16, default 4), \"contrast\" "
                   "(gain in [1/(1+c), 1+c]), \"brightness\" (+- additive, z-score units), \"noise\" (Gaussian, sigma up to this)")
    g.add_argument("--no-augment", action="store_true", help="NIfTI training sources without augmentation (centre-aligned resize only)")


def augment_from_args(args):
    if args.no_augment:
        return None
    if args.augment is None:
        return dict(DEFAULT_AUGMENT)
    try:
        a = json.loads(args.augment)
    except ValueError as e:
        raise ValueError("--augment: not JSON: %s" % e)
    if not isinstance(a, dict):
        raise ValueError("--augment: a JSON object expected")
    return check_augment(a)


def export(n, outdir, list_file, device="cuda", augment=DEFAULT_AUGMENT, seed=0, batch_size=16, out_size=(256, 256), sample_mm=None,
           prefilter=None, axes=None, sampling=None, crop=None):
    """N augmented slices as one-record tfrecords in the reference's layout plus OUTDIR/slice_list.  data_vol is the [H, W, 3] image;
    label_vol repeats the centre frame's label map in its three channels (the reference's decoder reads channel 1 only).  axes: None, or
    the slicing axes of a multi-planar set.  sampling: None, or AugmentedSliceSource's foreground sampling.
    crop: None, or VolumeSet's crop (a label margin, "body" or ("body", margin): DESIGN.md §24)."""
    from .tfrecord import write_slice
    which = {} if axes is None else {"axis": check_axes(axes)[0]}
    if crop is not None:
        which["crop"] = crop
    src = AugmentedSliceSource(VolumeSet(read_pairs(list_file), device, **which), batch_size, out_size=out_size, augment=augment, seed=seed,
                               sample_mm=sample_mm, prefilter=prefilter, sampling=sampling)
    os.makedirs(outdir, exist_ok=True)
    files = []
    while len(files) < n:
        batch, fids = src.next_batch(min(batch_size, n - len(files)))
        for sl, fid in zip(batch, fids):
            path = os.path.join(outdir, "slice_%05d.tfrecords" % len(files))
            write_slice(path, sl[:, :, 0:3], np.repeat(sl[:, :, 3:4], 3, axis=2))
            files.append(path)
            logging.info("%s <- %s" % (path, fid))
    src.close()
    if src.sampling:
        logging.info("foreground sampling: %s" % (src.sampling_report(),))
    with open(os.path.join(outdir, "slice_list"), "w") as f:
        f.write("\n".join(files) + "\n")
    return files


def main(argv=None):
    ap = argparse.ArgumentParser(description="export augmented slices of NIfTI volumes as tfrecords")
    ap.add_argument("--export", nargs=2, metavar=("N", "OUTDIR"), required=True)
    ap.add_argument("--list", required=True, help="list file: one `image.nii[.gz] label.nii[.gz]` pair per line")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    add_augment_flags(ap)
    add_sample_mm_flag(ap)
    add_prefilter_flag(ap)
    add_axes_flag(ap)
    add_sampling_flags(ap)
    from . import body
    body.add_crop_flags(ap)
    args = ap.parse_args(argv)
    crop = body.crop_from_args(ap, args)
    files = export(int(args.export[0]), args.export[1], args.list, device=args.device, augment=augment_from_args(args), seed=args.seed,
                   sample_mm=sample_mm_from_args(ap, args), prefilter=prefilter_from_args(ap, args), axes=axes_from_args(ap, args),
                   sampling=sampling_from_args(ap, args), crop=crop)
    print("wrote %d slices and %s" % (len(files), os.path.join(args.export[1], "slice_list")))
    return files


if __name__ == "__main__":
    main()
