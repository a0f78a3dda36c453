"""the bars that the kernel tests of the per-pixel loss terms share (test_gpu_entropy.py, test_gpu_boundary.py): a plain helper module,
no fixtures.  Each prints its figures before it asserts."""
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
