"""Label-free body crop (csrc/body.hip): the bounding box of the patient in a raw scan, found without a label — threshold
the scan into body and air (Otsu's rule on a histogram), keep the largest connected component, take its bounding box.  The same rule
for labelled and unlabelled volumes, for MR and CT, for training (volume_source.VolumeSet(crop="body")) and prediction
(volume_predict.segment_volume(crop="body")).

  otsu_bin(hist)                 the bin k that separates the two classes {bins <= k} and {bins > k} best; exact Python integers
  body_box(volume, ...)          ((x0, x1), (y0, y1), (z0, z1)), half-open, of a float32 CUDA volume [X, Y, Z] of raw intensities
  parse_crop(crop) / cli helpers the crop= option of VolumeSet / segment_volume and the --crop-body flag of the command lines

There is no CPU fallback: a CPU tensor raises PnpError."""
import numbers

import numpy as np

from . import _lib


def otsu_bin(hist):
    """Otsu's threshold of a histogram, as a bin index: with W = sum h_i, S = sum i h_i and the prefix sums w0(k) = sum_{i <= k} h_i,
    s0(k) = sum_{i <= k} i h_i, the FIRST k in [0, nbins - 2] with 0 < w0 < W that maximises the between-class variance, up to the constant
    factor 1 / W^2:  (w0 S - W s0)^2 / (w0 (W - w0)).  Fractions are compared by cross-multiplication in Python integers: no float enters,
    counts near 2^31 in 1024 bins are exact.  0 when no k qualifies (fewer than two occupied bins)."""
    h = [int(c) for c in np.asarray(hist).reshape(-1).tolist()]
    if any(c < 0 for c in h):
        raise ValueError("otsu_bin: negative count")
    W = sum(h)
    S = sum(i * c for i, c in enumerate(h))
    best, best_num, best_den = 0, -1, 1
    w0 = s0 = 0
    for k in range(len(h) - 1):
        w0 += h[k]
        s0 += k * h[k]
        if not 0 < w0 < W:
            continue
        d = w0 * S - W * s0
        num, den = d * d, w0 * (W - w0)
        if num * best_den > best_num * den:           # strictly better: the first maximum wins
            best, best_num, best_den = k, num, den
    return best


def check_margin(margin, what="margin"):
    if isinstance(margin, bool) or not isinstance(margin, numbers.Integral) or margin < 0:
        raise ValueError("%s must be an int >= 0, got %r" % (what, margin))
    return int(margin)


def parse_crop(crop):
    """the crop= option -> None, ("label", margin) for an int, ("body", margin) for "body" / ("body", margin); ValueError otherwise"""
    if crop is None:
        return None
    if isinstance(crop, str):
        if crop != "body":
            raise ValueError("crop: %r is not \"body\"" % (crop,))
        return ("body", 0)
    if isinstance(crop, (tuple, list)):
        if len(crop) != 2 or crop[0] != "body":
            raise ValueError("crop: a pair (\"body\", margin) expected, got %r" % (crop,))
        return ("body", check_margin(crop[1], "crop: the body margin"))
    if isinstance(crop, bool) or not isinstance(crop, numbers.Integral):
        raise ValueError("crop must be None, a label margin (int), \"body\" or (\"body\", margin), got %r" % (crop,))
    return ("label", int(crop))


def grow_box(box, margin, shape):
    return tuple((max(int(a) - margin, 0), min(int(b) + margin, int(n))) for (a, b), n in zip(box, shape))


def permute_box(box, axis):
    """the box of a volume in file order -> the box after numpy.moveaxis(volume, axis, -1)"""
    order = [a for a in range(3) if a != axis] + [axis]
    return tuple(box[a] for a in order)


def unpermute_box(box, axis):
    """the inverse of permute_box: a box in the order after numpy.moveaxis(volume, axis, -1) -> the box in file order"""
    order = [a for a in range(3) if a != axis] + [axis]
    out = [None, None, None]
    for j, a in enumerate(order):
        out[a] = box[j]
    return tuple(out)


def box_slices(box):
    return tuple(slice(a, b) for a, b in box)


def body_box(volume, percentile=98, margin=0, nbins=256, connectivity=1):
    """The bounding box ((x0, x1), (y0, y1), (z0, z1)), half-open and in the tensor's own order, of the largest bright connected region of
    a contiguous float32 CUDA volume [X, Y, Z] of raw intensities (each extent <= 4096, fewer than 2^31 voxels):
      1. kernels.volume_preprocess(volume, percentile) into a scratch copy — the clip keeps bone, metal or an MR spike from stretching the
         range; the input is not modified
      2. kernels.volume_histogram of the copy, nbins bins between its minimum and maximum      (host read 1: range and counts, one copy)
      3. otsu_bin on the host
      4. kernels.volume_threshold_mask: the voxels whose bin is above Otsu's
      5. the largest component of the mask (pnp_label_components / pnp_filter_components with num_cls = 2, keep = 1, `connectivity`, in
         place: what components.keep_largest runs; ties go to the lower root)
      6. kernels.label_frame_stats of the mask, class 1                  (host read 2: the [Z, 5] table and the component kernels' error
         counters, one copy), reduced on the host to the 3-D box
      7. the box grown by `margin` voxels and clamped to the volume.
    A constant volume gives the whole volume.  Scratch: about 13 bytes per voxel (the normalised copy 4, the mask 1, the component roots 4
    and the component workspace 4), released before returning.  Two host synchronisations per volume, both needed: the threshold is
    decided on the host from the histogram, and the crop changes tensor shapes.  No CPU fallback."""
    import torch
    from . import components
    from . import kernels as K
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda:
        raise _lib.PnpError("body_box: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    if volume.dtype != torch.float32 or volume.dim() != 3 or not volume.is_contiguous() or volume.numel() < 1:
        raise ValueError("body_box: a non-empty contiguous float32 volume [X, Y, Z] expected, got %s %s" % (volume.dtype, tuple(volume.shape)))
    margin = check_margin(margin, "body_box: margin")
    _, _, connectivity, cmask = components.check_options(2, 1, 0, connectivity)
    shape = tuple(int(d) for d in volume.shape)
    whole = tuple((0, n) for n in shape)
    v, _ = K.volume_preprocess(volume, int(percentile))
    buf = K.volume_histogram_packed(v, nbins)
    host = buf.cpu().numpy()                                  # synchronisation 1
    lo, hi = host[:2].view(np.float32)
    if hi == lo:
        return whole
    k = otsu_bin(host[2:])
    mask = K.volume_threshold_mask(v, buf[:2].view(torch.float32), k, nbins)
    del v
    roots, ws = K.label_components(mask, 2, connectivity)
    K.filter_components(mask, roots, 2, cmask, 1, 0, mask)
    del roots
    table = K.label_frame_stats(mask, 2)[:, 1, :].reshape(-1)
    t = torch.cat([ws[:8].view(torch.int32), table]).cpu().numpy()         # synchronisation 2
    del mask, ws
    K.drop_workspace("components")
    if t[0] or t[1]:
        raise _lib.PnpError("body_box: the component kernels' error counters read (%d, %d)" % (int(t[0]), int(t[1])))
    rows = t[2:].reshape(shape[2], 5)
    z = np.flatnonzero(rows[:, 0] > 0)
    if len(z) == 0:
        return whole
    box = ((int(rows[z, 1].min()), int(rows[z, 2].max()) + 1), (int(rows[z, 3].min()), int(rows[z, 4].max()) + 1), (int(z[0]), int(z[-1]) + 1))
    return grow_box(box, margin, shape)


# ---- command lines -------------------------------------------------------------------------------------------------------------------
def add_crop_flags(ap, label_margin=True):
    """--crop-body [N] (and --crop-margin N where the command line has labels to crop to and does not define the flag itself)"""
    ap.add_argument("--crop-body", nargs="?", type=int, const=0, default=None, metavar="N",
                    help="crop every volume to the bounding box of its body, found on the device without a label (threshold, largest "
                         "component: DESIGN.md §24), grown by N voxels (a bare flag: 0)")
    if label_margin:
        ap.add_argument("--crop-margin", type=int, default=None, metavar="N",
                        help="crop every volume to the bounding box of its labels grown by N voxels (needs labels)")


def crop_from_args(ap, args, have_lists=True):
    """the crop= option of the parsed arguments: None, an int (label margin) or ("body", N); argument errors end in ap.error"""
    cb, cm = getattr(args, "crop_body", None), getattr(args, "crop_margin", None)
    if cb is None and cm is None:
        return None
    if cb is not None and cm is not None:
        ap.error("--crop-body and --crop-margin exclude each other")
    if not have_lists:
        ap.error("--crop-body / --crop-margin need the NIfTI lists")
    if (cb if cb is not None else cm) < 0:
        ap.error("--crop-body / --crop-margin: the margin must be >= 0")
    return ("body", int(cb)) if cb is not None else int(cm)
