"""Connected components of label volumes on the device (csrc/components.hip): the post-processing step between prediction
and evaluation — keep the largest 3-D component of every structure, drop the islands.

  label_components(vol, num_cls, connectivity)      int32 roots of vol's shape: -1 for background, else the smallest flat (C order) index of
                                                    the voxel's component
  keep_largest(vol, num_cls, keep, min_size, ...)   (filtered uint8 volume, int64 stats [num_cls, 4]: components found, voxels before,
                                                    voxels kept, size of the largest component)
  parse_option(arg, num_cls)                        the keep_largest= argument of volume_predict.segment_volume / evaluate.evaluate -> keywords
  fill_holes(vol, num_cls, max_size, classes, ...)  (filled uint8 volume, int64 stats [num_cls, 4]): every enclosed background hole takes the
                                                    class with the most face contacts to it
  parse_fill_option(arg, num_cls)                   the fill_holes= argument of the same functions -> keywords

vol is a contiguous uint8 [D0, D1, D2] CUDA tensor (what segment_volume returns); a label >= num_cls counts as background.  A component is
a maximal set of voxels of one non-zero label joined by steps of scipy's generate_binary_structure(3, connectivity).  There is no CPU
fallback: a CPU tensor raises PnpError.  Both calls read the kernels' device error counters once (a host synchronisation) and raise if
one is set."""
import numbers

import torch

from . import _lib

OPTION_KEYS = ("keep", "min_size", "connectivity", "classes")
MAX_KEEP = 8                         # pnp_filter_components'
last_errors = (0, 0)                 # the counters the most recent call read: (labelling, filter)
FILL_OPTION_KEYS = ("max_size", "classes")        # fill_holes' 
last_fill_errors = (0, 0, 0)         # the counters the most recent fill_holes read: (labelling, size count, fill)


def class_mask(num_cls, classes=None):
    """bit c set for every filtered class; None = all of 1 .. num_cls - 1"""
    num_cls = int(num_cls)
    if not 2 <= num_cls <= 8:
        raise ValueError("num_cls %d outside [2, 8]" % num_cls)
    if classes is None:
        return (1 << num_cls) - 2
    mask = 0
    for c in classes:
        if isinstance(c, bool) or int(c) != c or not 1 <= int(c) < num_cls:
            raise ValueError("classes: %r is no class in [1, %d)" % (c, num_cls))
        mask |= 1 << int(c)
    return mask


def check_options(num_cls, keep=1, min_size=0, connectivity=1, classes=None):
    """the host checks of keep_largest's keywords -> (keep, min_size, connectivity, class mask); ValueError otherwise"""
    for name, v in (("keep", keep), ("min_size", min_size), ("connectivity", connectivity)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("%s must be an int, got %r" % (name, v))
    keep, min_size, connectivity = int(keep), int(min_size), int(connectivity)
    if not 0 <= keep <= MAX_KEEP:
        raise ValueError("keep = %d outside [0, %d]" % (keep, MAX_KEEP))
    if min_size < 0:
        raise ValueError("min_size = %d is negative" % min_size)
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity = %d outside {1, 2, 3}" % connectivity)
    return keep, min_size, connectivity, class_mask(num_cls, classes)


def parse_option(arg, num_cls=5):
    """None -> None; an int K -> {"keep": K}; a dict of keep_largest's keywords -> a checked copy.  ValueError for anything else."""
    if arg is None:
        return None
    if isinstance(arg, dict):
        unknown = sorted(set(arg) - set(OPTION_KEYS))
        if unknown:
            raise ValueError("keep_largest: unknown keys %s (known: %s)" % (unknown, list(OPTION_KEYS)))
        opts = dict(arg)
    elif isinstance(arg, numbers.Integral) and not isinstance(arg, bool):
        if arg < 0:
            raise ValueError("keep_largest = %d is negative" % arg)
        opts = {"keep": int(arg)}
    else:
        raise ValueError("keep_largest must be None, an int or a dict of %s, got %r" % (list(OPTION_KEYS), arg))
    try:
        check_options(num_cls, **opts)
    except ValueError as e:
        raise ValueError("keep_largest: %s" % e)
    return opts


def _volume(vol, what):
    if not isinstance(vol, torch.Tensor):
        raise ValueError("%s: a torch tensor expected, got %s" % (what, type(vol).__name__))
    if not vol.is_cuda:
        raise _lib.PnpError("%s: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback" % what)
    if vol.dtype != torch.uint8:
        raise ValueError("%s: a uint8 label volume expected, got %s" % (what, vol.dtype))
    if vol.dim() != 3:
        raise ValueError("%s: a [D0, D1, D2] volume expected, got shape %s" % (what, tuple(vol.shape)))
    if not vol.is_contiguous():
        raise ValueError("%s: the volume must be contiguous (C order), got strides %s" % (what, tuple(vol.stride())))
    return vol


def _raise_on(ws, what):
    global last_errors
    from . import kernels as K
    last_errors = K.components_errors(ws)
    if last_errors[0]:
        raise _lib.PnpError("%s: %d union-find loops reached their cap (pnp_label_components' error counter)" % (what, last_errors[0]))
    if last_errors[1]:
        raise _lib.PnpError("%s: roots entries outside the volume (pnp_filter_components' error counter: %d)" % (what, last_errors[1]))


def label_components(vol, num_cls=5, connectivity=1):
    from . import kernels as K
    _volume(vol, "label_components")
    _, _, connectivity, _ = check_options(num_cls, connectivity=connectivity)
    roots, ws = K.label_components(vol, int(num_cls), connectivity)
    _raise_on(ws, "label_components")
    return roots


def keep_largest(vol, num_cls=5, keep=1, min_size=0, connectivity=1, classes=None, out=None):
    """-> (filtered, stats).  keep = 0: no rank rule (min_size alone); classes: the filtered classes (None = all), the others pass through;
    out: a uint8 tensor like vol to write into — vol itself filters in place."""
    from . import kernels as K
    _volume(vol, "keep_largest")
    keep, min_size, connectivity, mask = check_options(num_cls, keep, min_size, connectivity, classes)
    if out is None:
        out = torch.empty_like(vol)
    elif _volume(out, "keep_largest: out").shape != vol.shape or out.device != vol.device:
        raise ValueError("keep_largest: out %s on %s does not match the volume %s on %s" % (tuple(out.shape), out.device, tuple(vol.shape), vol.device))
    roots, _ = K.label_components(vol, int(num_cls), connectivity)
    _, stats, ws = K.filter_components(vol, roots, int(num_cls), mask, keep, min_size, out)
    _raise_on(ws, "keep_largest")
    return out, stats


def check_fill_options(num_cls, max_size=0, classes=None):
    """the host checks of fill_holes' keywords -> (max_size, class mask); ValueError otherwise"""
    if isinstance(max_size, bool) or not isinstance(max_size, numbers.Integral):
        raise ValueError("max_size must be an int, got %r" % (max_size,))
    if int(max_size) < 0:
        raise ValueError("max_size = %d is negative" % max_size)
    return int(max_size), class_mask(num_cls, classes)


def parse_fill_option(arg, num_cls=5):
    """None / False -> None; True -> {}; a positive int N -> {"max_size": N}; a dict of fill_holes' keywords -> a checked copy.  ValueError
    for anything else."""
    if arg is None or arg is False:
        return None
    if arg is True:
        opts = {}
    elif isinstance(arg, dict):
        unknown = sorted(set(arg) - set(FILL_OPTION_KEYS))
        if unknown:
            raise ValueError("fill_holes: unknown keys %s (known: %s)" % (unknown, list(FILL_OPTION_KEYS)))
        opts = dict(arg)
    elif isinstance(arg, numbers.Integral):
        if arg < 1:
            raise ValueError("fill_holes = %d is no positive size limit (True fills cavities of any size)" % arg)
        opts = {"max_size": int(arg)}
    else:
        raise ValueError("fill_holes must be None, a bool, a positive int or a dict of %s, got %r" % (list(FILL_OPTION_KEYS), arg))
    try:
        check_fill_options(num_cls, **opts)
    except ValueError as e:
        raise ValueError("fill_holes: %s" % e)
    return opts


def fill_holes(vol, num_cls=5, max_size=0, classes=None, out=None):
    """-> (filled, stats).  Every cavity — a 6-connected set of background voxels (label 0 or >= num_cls) that touches no face of the volume:
    what scipy.ndimage.binary_fill_holes fills — takes the class with the most face contacts to it (ties: the lower class) when that class
    is in `classes` (None = all) and max_size == 0 or the cavity has at most max_size voxels; all other background becomes 0, everything
    else stays.  stats int64 [num_cls, 4]: row c = cavities filled with c, voxels filled, largest cavity filled, cavities
    won by c and left; row 0 = cavities found, their voxels, cavities left, voxels left.  out: a uint8 tensor like vol — vol itself fills
    in place."""
    global last_fill_errors
    from . import kernels as K
    _volume(vol, "fill_holes")
    max_size, mask = check_fill_options(num_cls, max_size, classes)
    if out is None:
        out = torch.empty_like(vol)
    elif _volume(out, "fill_holes: out").shape != vol.shape or out.device != vol.device:
        raise ValueError("fill_holes: out %s on %s does not match the volume %s on %s" % (tuple(out.shape), out.device, tuple(vol.shape), vol.device))
    _, stats, ws = K.fill_holes(vol, int(num_cls), mask, max_size, out)
    last_fill_errors = K.fill_holes_errors(ws)
    if last_fill_errors[0]:
        raise _lib.PnpError("fill_holes: %d union-find loops reached their cap (the labelling's error counter)" % last_fill_errors[0])
    if last_fill_errors[1] or last_fill_errors[2]:
        raise _lib.PnpError("fill_holes: inconsistent roots or cavities (pnp_fill_holes' error counters: %d, %d)" % last_fill_errors[1:])
    return out, stats


def fill_stats_line(stats):
    """one printable line of fill_holes' stats tensor / array / nested list"""
    rows = stats.cpu().tolist() if isinstance(stats, torch.Tensor) else [list(r) for r in stats]
    head = "%d cavities, %d voxels, left %d / %d" % tuple(rows[0])
    return head + "".join("   class %d: %d filled, %d voxels, largest %d, left %d" % (c, r[0], r[1], r[2], r[3])
                          for c, r in enumerate(rows) if c > 0 and (r[0] or r[3]))


def stats_line(stats, num_cls=None):
    """one printable line of a stats tensor / array / nested list: per class found, before -> kept, largest"""
    rows = stats.cpu().tolist() if isinstance(stats, torch.Tensor) else [list(r) for r in stats]
    return "   ".join("class %d: %d components, %d -> %d voxels, largest %d" % (c, r[0], r[1], r[2], r[3]) for c, r in enumerate(rows) if c > 0)


def add_cli_arguments(ap):
    """--keep-largest [K] / --min-size N / --connectivity C of the predict and evaluate command lines"""
    ap.add_argument("--keep-largest", nargs="?", type=int, const=1, default=None, metavar="K",
                    help="keep the K largest 3-D connected components of every class (a bare flag: 1), on the device")
    ap.add_argument("--min-size", type=int, default=None, metavar="N", help="drop components of fewer than N voxels (alone: no rank rule)")
    ap.add_argument("--connectivity", type=int, default=None, choices=(1, 2, 3), help="6, 18 or 26 neighbours (default 1)")
    ap.add_argument("--fill-holes", nargs="?", type=int, const=0, default=None, metavar="MAX",
                    help="fill the enclosed background holes of the label volume with the class around them, on the device, after "
                         "--keep-largest (a bare flag: holes of any size; MAX: holes of at most MAX voxels)")
    ap.add_argument("--fill-classes", default=None, metavar="C,C", help="the classes that may grow into holes (default: all)")


def cli_option(ap, a, num_cls=5):
    """the keep_largest= option of the parsed arguments, or None when none of the three was given; argument errors end in ap.error"""
    if a.keep_largest is None and a.min_size is None:
        if a.connectivity is not None:
            ap.error("--connectivity goes with --keep-largest or --min-size")
        return None
    opts = {"keep": 0 if a.keep_largest is None else a.keep_largest, "min_size": 0 if a.min_size is None else a.min_size,
            "connectivity": 1 if a.connectivity is None else a.connectivity}
    try:
        return parse_option(opts, num_cls)
    except ValueError as e:
        ap.error("--keep-largest / --min-size: %s" % e)


def cli_fill_option(ap, a, num_cls=5):
    """the fill_holes= option of the parsed arguments, or None without --fill-holes; argument errors end in ap.error"""
    if a.fill_holes is None:
        if a.fill_classes is not None:
            ap.error("--fill-classes goes with --fill-holes")
        return None
    opts = {}
    try:
        if a.fill_holes < 0:
            raise ValueError("max_size = %d is negative" % a.fill_holes)
        if a.fill_holes > 0:
            opts["max_size"] = a.fill_holes
        if a.fill_classes is not None:
            try:
                opts["classes"] = [int(c) for c in a.fill_classes.split(",")]
            except ValueError:
                raise ValueError("classes: %r is no comma-separated list of ints" % a.fill_classes)
        return parse_fill_option(opts, num_cls)
    except ValueError as e:
        ap.error("--fill-holes / --fill-classes: %s" % e)
