"""the bars that the kernel tests of the per-pixel loss terms share (test_gpu_entropy.py, test_gpu_boundary.py, test_gpu_pseudo_label.py,
test_gpu_pixel_loss_domain.py): a plain helper module, no fixtures.  Each prints its figures before it asserts."""
import torch


def _bar(got, ref, what, tol=1e-5):
    """the bar of the project's kernel tests: within tol of max|ref|"""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).double()
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    print("%s: max err %.3e of max|ref| %.3e (%.2e)" % (what, err, scale, err / (scale + 1e-300)))
    assert err <= tol * scale + 1e-30, what


def _value_bar(got, ref, what):
    print("%s: value %.9g, float64 %.9g (rel %.2e)" % (what, float(got), ref, abs(float(got) - ref) / (abs(ref) + 1e-300)))
    assert abs(float(got) - ref) <= 1e-5 * abs(ref), what


def _element_bar(got, ref, scale, factor, what):
    """the per-element bar of the per-pixel loss terms (tests/pixel_loss_cases.py): every entry within
    factor * 2^-24 * scale of the float64 reference, scale = (1 + |z - max z|) * S of that entry; an entry whose scale is 0 is exact.
    numpy arrays in, the largest ratio out"""
    import numpy as np
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == scale.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref)
    unit = 2.0 ** -24 * scale
    live = unit > 0
    worst = float((err[live] / unit[live]).max()) if live.any() else 0.0
    print("%s: largest |err| / (u scale) %.3f (bar %.1f), %d entries with scale 0" % (what, worst, factor, int((~live).sum())))
    assert not err[~live].any(), what + ": an entry whose scale is 0 is not exactly 0"
    bad = err > factor * unit
    assert not bad.any(), "%s: %d entries beyond the per-element bar, the first at %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    return worst
