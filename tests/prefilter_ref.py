"""float64 numpy restatement of the anti-alias prefilter — the reference of tests/test_gpu_prefilter.py, pinned to
scipy.ndimage.gaussian_filter1d in tests/test_prefilter_host.py.

  radius / weights(sigma)          scipy's taps: R = int(4 sigma + 0.5), exp(-k^2 / (2 sigma^2)) normalised in float64, rounded ONCE to float32
                                   (what the kernel gets); None when R == 0
  pass_1d(v, w, axis)              one clamped pass (index clamped into [0, n - 1]: mode="nearest"), float32-rounded weights, float64 sums
  smooth(v, sigmas)                the passes over the filtered axes (in exact arithmetic they commute; here X, Y, Z)
  auto_sigmas(...)                 the sigma rule: max(0, (r - 1) / 2) for r source voxels per output sample
  bound(sigmas, top)               (n_x + n_y + n_z + 6) 2^-24 max|v|, n_a = 2 R_a + 1 over the filtered axes
  smooth_taps(v, (wx, wy, wz))     the same passes for ANY 2 r + 1 taps per axis (None: the axis is not filtered), symmetric or not:
                                   out[a] = sum_k w[k] v[clamp(a - r + k)], pinned to scipy.ndimage.correlate1d(mode="nearest")
  bound_taps(taps, top)            bound()'s derivation by tap count, for non-negative taps that sum to 1 in float64, rounded once to float32
  stripes() / stripe_map()         the aliasing case: cos(2 pi x 0.35 / 1.0) on 120 x 40 x 6 voxels of 0.35 mm under a 32 x 12 plane of 1 mm pixels
"""
import numpy as np

U = 2.0 ** -24
TRUNCATE = 4.0


def radius(sigma):
    return int(TRUNCATE * float(sigma) + 0.5)


def weights(sigma):
    R = radius(sigma)
    if R == 0:
        return None
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * k ** 2)          # scipy's own expression (_gaussian_kernel1d)
    return (w / w.sum()).astype(np.float32)


def pass_1d(v, w, axis):
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    R = len(w) // 2
    n = v.shape[axis]
    out = np.zeros_like(v)
    for k in range(-R, R + 1):
        out += w[k + R] * np.take(v, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)
    return out


def smooth(v, sigmas):
    out = np.asarray(v, dtype=np.float64)
    for axis, s in enumerate(sigmas):
        w = weights(s)
        if w is not None:
            out = pass_1d(out, w, axis)
    return out


def auto_sigmas(dims, out_size, spacing=None, sample_mm=None):
    if sample_mm is not None:
        r = [m / s for m, s in zip(sample_mm, spacing)]
    else:
        r = [dims[0] / out_size[0], dims[1] / out_size[1], 1.0]
    return tuple(max(0.0, (v - 1.0) / 2.0) for v in r)


def bound(sigmas, top):
    """first-order fp32 bound of up to three chains of non-negative weights that sum to 1: n_a roundings of at most u max|v| per filtered
    axis (one fmaf per tap), plus 6 u max|v| of slack (the weights' sums are 1 only up to 2R + 1 float32 ulps)"""
    n = sum(2 * radius(s) + 1 for s in sigmas if radius(s) > 0)
    return (n + 6) * U * float(top)


def smooth_taps(v, taps):
    """taps = (wx, wy, wz), each None or 2 r + 1 float32-convertible weights; the passes run in the order X, Y, Z like smooth()"""
    out = np.asarray(v, dtype=np.float64)
    assert len(taps) == 3
    for axis, w in enumerate(taps):
        if w is not None:
            assert len(w) % 2 == 1 and len(w) >= 3
            out = pass_1d(out, w, axis)
    return out


def bound_taps(taps, top):
    """bound() by tap count: every filtered axis is one fmaf chain of n_a = len(taps_a) non-negative weights that sum to 1 — one rounding
    of at most u max|v| per tap, every partial sum being a sub-convex combination of values within max|v| — plus the same 6 u max|v| of
    slack (the float32 weights sum to 1 only up to n_a ulps).  For Gaussian taps this is bound(sigmas, top) itself."""
    n = 0
    for w in taps:
        if w is not None:
            w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
            assert np.all(w64 >= 0) and abs(float(w64.sum()) - 1.0) <= len(w64) * U
            n += len(w64)
    return (n + 6) * U * float(top)


STRIPE_SHAPE, STRIPE_MM, STRIPE_SAMPLE_MM, STRIPE_OUT = (120, 40, 6), 0.35, (1.0, 1.0, 0.35), (32, 12)
# The stripes alias onto frequency 0: every pixel of the 1 mm grid reads the same phase of the 1.0 mm cosine, so what comes out is a
# constant whose size depends on where the grid lies against the stripes.  Crests that are voxel centres sit at x = 0, 20, 40, ...
# (0.35 x a whole number of mm).  The plane is translated by STRIPE_TRANSLATE_MM so that pixel row 5 reads voxel 20 (and row 12 voxel 40,
# ...): rows 0 and 31 then read x = 5.71 and 94.29, more than the filter's radius of 4 inside the volume.  With the plane centred on
# the volume instead (no translation) the rows read the phase 0.325 of the cosine and the two figures of the tests are 0.474 and 0.059.
STRIPE_TRANSLATE_MM = ((20.0 - 5.0 / STRIPE_MM) - ((STRIPE_SHAPE[0] - 1) / 2.0 - (STRIPE_OUT[0] - 1) / 2.0 / STRIPE_MM)) * STRIPE_MM, 0.0


def stripe_map(compose_matrix):
    """the six entries of the stripe case's plane map, from volume_source.compose_matrix"""
    return compose_matrix(STRIPE_SHAPE[:2], STRIPE_OUT, translate=STRIPE_TRANSLATE_MM, spacing_xy=(STRIPE_MM, STRIPE_MM), pixel_mm=STRIPE_SAMPLE_MM[:2])


def stripes():
    """[120, 40, 6] float32: a cosine of period 1.0 mm along x on voxels of 0.35 mm, constant along y and z"""
    x = np.arange(STRIPE_SHAPE[0], dtype=np.float64)
    return np.broadcast_to(np.cos(2 * np.pi * x * STRIPE_MM / 1.0)[:, None, None], STRIPE_SHAPE).astype(np.float32)
