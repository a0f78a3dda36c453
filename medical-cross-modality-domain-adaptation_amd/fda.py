"""Fourier domain adaptation of the source segmenter's batches (Yang & Soatto, CVPR 2020; not in the reference).

Every stylised source slice keeps the phase of each channel's 2-D spectrum and takes the amplitude of a target slice on the square of low
frequencies |u|, |v| <= b, b = floor(beta * min(H, W)) (kernels.fda_amplitude_swap, csrc/fda.hip).  No network and no loss: the
segmenter sees source anatomy with target appearance.  FdaStylizer draws its target slices from a feeder of its own and its bands and
pairs from a numpy generator of its own, so a run without it is the reference's run, launch for launch.
  stylizer = FdaStylizer(target_list, beta=(0.01, 0.09), prob=0.5);  x = stylizer(x)
The paper's multi-band ensemble (mean softmax of models trained at beta = 0.01, 0.05, 0.09) is `predict --ensemble` over their checkpoints.
"""
import numpy as np

from . import kernels as K
from .parallel import rank_seed

TARGET_SEED = 2      # the NIfTI target source's parameter stream (the training source uses seed 0, validation 1)


def check_beta(beta):
    """a number or (lo, hi) in [0, 0.5) -> (lo, hi); ValueError otherwise"""
    try:
        lo, hi = (float(beta), float(beta)) if np.ndim(beta) == 0 else (float(beta[0]), float(beta[1]))
        if np.ndim(beta) and len(beta) != 2:
            raise TypeError
    except (TypeError, ValueError, IndexError):
        raise ValueError("beta: a number or (lo, hi), got %r" % (beta,))
    if not (0.0 <= lo < 0.5 and 0.0 <= hi < 0.5):
        raise ValueError("beta must lie in [0, 0.5), got %r" % (beta,))
    if lo > hi:
        raise ValueError("beta (lo, hi) needs lo <= hi, got %r" % (beta,))
    return lo, hi


def check_prob(prob):
    p = float(prob)
    if not 0.0 <= p <= 1.0:
        raise ValueError("prob must lie in [0, 1], got %r" % (prob,))
    return p


def beta_to_band(beta, H, W):
    """FDA's band of a beta: floor(beta * min(H, W)), capped at (min(H, W) - 1) // 2 (beta < 0.5 keeps it there; the cap only guards
    rounding at the edge)"""
    n = min(int(H), int(W))
    return min(int(np.floor(float(beta) * n)), (n - 1) // 2)


class FdaStylizer(object):
    """Stylises source batches with the amplitude spectra of target slices.
      target_source  a list of .tfrecords slices (read through tfrecord.SliceQueue, sharded like the trainers' lists) or any source a
                     feeder.DeviceFeeder drives (next_batch / next_device_batch); only its image channels are used
      beta           a number, or (lo, hi): beta drawn per sample uniformly from [lo, hi]; in [0, 0.5)
      prob           the share of the samples stylised; the others get band -1 (unchanged)
      seed, shard    the draws come from numpy.random.default_rng(seed + rank_seed(rank)), rank = shard[0] (0 without a shard)
    __call__(x [B, H, W, C] on the device) -> a new stylised tensor; x is never written.  The target feeder starts at the first call, with
    that call's batch size and device.  last_band / last_pair: the int32 bands and pairs of the last call."""

    def __init__(self, target_source, beta=0.01, prob=1.0, seed=0, shard=None):
        self.lo, self.hi = check_beta(beta)
        self.prob = check_prob(prob)
        self.source, self.shard = target_source, shard
        self.rank = shard[0] if shard else 0
        self.rng = np.random.default_rng(int(seed) + rank_seed(self.rank))
        self.feeder = None
        self.last_band = self.last_pair = None

    def _feed(self, batch_size, device):
        if self.feeder is None:
            from .feeder import DeviceFeeder
            src = self.source
            if not hasattr(src, "next_batch"):
                from .tfrecord import SliceQueue
                src = SliceQueue(list(src), batch_size, shard=self.shard)
            self.feeder = DeviceFeeder(src, batch_size, 1, device)      # one class: the labels are not used
        return self.feeder

    def draw(self, B, Bt, H, W):
        """(band, pair) int32 [B] of one batch: u, beta and pair per sample, in that order, from the generator"""
        u = self.rng.random(B)
        beta = self.rng.uniform(self.lo, self.hi, B)
        pair = self.rng.integers(0, Bt, B)
        band = np.array([beta_to_band(b, H, W) for b in beta], dtype=np.int32)
        band[u >= self.prob] = -1
        return band, pair.astype(np.int32)

    def __call__(self, x):
        B, H, W, _ = x.shape
        t, _, _ = self._feed(B, x.device).next()
        if tuple(t.shape[1:]) != tuple(x.shape[1:]):
            raise ValueError("FdaStylizer: target slices %s, source slices %s" % (tuple(t.shape[1:]), tuple(x.shape[1:])))
        band, pair = self.draw(B, t.shape[0], H, W)
        self.last_band, self.last_pair = band, pair
        return K.fda_amplitude_swap(x.contiguous(), t, band, pair)

    def close(self):
        if self.feeder is not None:
            self.feeder.close()
            self.feeder = None


def parse_beta(text):
    """--fda-beta: 'B' or 'LO,HI' -> a number or (lo, hi), checked by check_beta"""
    parts = str(text).split(",")
    if len(parts) not in (1, 2):
        raise ValueError("--fda-beta takes B or LO,HI, got %r" % (text,))
    vals = [float(p) for p in parts]
    check_beta(vals[0] if len(vals) == 1 else vals)
    return vals[0] if len(vals) == 1 else tuple(vals)


def add_fda_flags(ap):
    ap.add_argument("--fda-target", default=None, metavar="LIST", help="stylise every training batch with the low-frequency amplitude "
                    "spectra of these target slices (Fourier domain adaptation, DESIGN.md §30): with --nii-train a NIfTI list whose lines "
                    "may name an image alone, otherwise a list of .tfrecords slices")
    ap.add_argument("--fda-beta", default=None, metavar="B|LO,HI", help="band of the amplitude swap, floor(B * min(H, W)) frequencies; "
                    "LO,HI draws B per sample; in [0, 0.5) (default 0.01)")
    ap.add_argument("--fda-prob", default=None, type=float, metavar="P", help="share of the samples stylised, in [0, 1] (default 1)")


def fda_from_args(ap, args):
    """checks the FDA flags and fills in their defaults: args.fda_beta -> a number or (lo, hi), args.fda_prob -> a float"""
    if args.fda_target is None:
        if args.fda_beta is not None or args.fda_prob is not None:
            ap.error("--fda-beta and --fda-prob go with --fda-target")
        return
    try:
        args.fda_beta = 0.01 if args.fda_beta is None else parse_beta(args.fda_beta)
        args.fda_prob = check_prob(1.0 if args.fda_prob is None else args.fda_prob)
    except ValueError as e:
        ap.error(str(e))


def nifti_target_source(list_file, device, batch_size, sample_mm=None, prefilter=None, axes=None, crop=None, shard=None):
    """the target slices of a NIfTI list (read_pairs(labels="optional")) on the training list's grid, prefilter and axes, never
    augmented; crop only as a body crop (the list need not hold labels)"""
    from .volume_source import AugmentedSliceSource, VolumeSet, check_axes, read_pairs
    which = {} if axes is None else {"axis": check_axes(axes)[0]}
    if isinstance(crop, tuple) and crop[0] == "body":
        which["crop"] = crop
    return AugmentedSliceSource(VolumeSet(read_pairs(list_file, "optional"), device, **which), batch_size, augment=None, seed=TARGET_SEED,
                                shard=shard, num_cls=1, sample_mm=sample_mm, prefilter=prefilter)
