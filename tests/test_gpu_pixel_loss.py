"""-m gpu: a guard on the skeleton that the per-pixel loss terms share (csrc/pixel_loss.h).  For five classes the same
logits go through the vector path (16-byte aligned bases: four pixels per five float4) and through the generic path (bases one pixel into
an allocation: one pixel of up to eight classes at a time); the per-pixel arithmetic is the term's one `pixel` function either way, and
the three lanes the generic path carries beyond the five classes add exact zeros, so the GRADIENT is the same bit for bit.  (The values
are not: the two paths deal the pixels to the threads differently, so the float32 partial sums differ in the last bits; the tests of
each term hold them to 1e-6 of each other.)  The inputs are those of the entropy and boundary terms' misaligned-base tests; the
pseudo-label term takes the entropy term's logits."""
import pytest
import torch

from conftest import pkg
from test_gpu_boundary import _loss_inputs
from test_gpu_entropy import _logits

pytestmark = pytest.mark.gpu


def _one_pixel_in(a, dev):
    base = torch.zeros((a.shape[0] + 1, a.shape[1]), device=dev)
    base[1:] = torch.from_numpy(a).to(dev)
    return base[1:]


@pytest.mark.parametrize("P", [4, 7, 1021])
@pytest.mark.parametrize("term", ["entropy", "boundary", "pseudo_label"])
def test_generic_and_vector_path_write_the_same_gradient_bits(dev, term, P):
    """pseudo_label: thresholds 0.5, every class; the term's side outputs — class / selected bytes, confidence words, counts — are held
    to the same bits as the gradient (measured on the library before the term became one of the skeleton's: 0 words differ)"""
    K = pkg("kernels")
    side = []
    if term == "entropy":
        z, _ = _logits(P, 5, 7 + P)
        inputs = (z,)
        run = lambda zd: K.softmax_entropy(zd, want_grad=True)
    elif term == "pseudo_label":
        z, _ = _logits(P, 5, 7 + P)
        inputs = (z,)
        tau = torch.full((5,), 0.5, device=dev)

        def run(zd):
            v, _, counts, labels, conf, g = K.pseudo_label_loss(zd, tau, want_grad=True)
            side.append((labels, conf.view(torch.int32), counts))
            return v, g
    else:
        inputs = _loss_inputs(P, 5, 7 + P, None)
        run = lambda zd, qd: K.boundary_loss(zd, qd, 4, want_grad=True)
    generic = [_one_pixel_in(a, dev) for a in inputs]
    vector = [t.clone() for t in generic]
    assert all(t.is_contiguous() and t.data_ptr() % 16 != 0 for t in generic) and all(t.data_ptr() % 16 == 0 for t in vector)
    vg, gg = run(*generic)
    vv, gv = run(*vector)
    differ = int((gg.view(torch.int32) != gv.view(torch.int32)).sum())
    print("%s P=%d: %d of %d gradient words differ between the generic and the vector path; values %.9g / %.9g" % (
        term, P, differ, gg.numel(), float(vg), float(vv)))
    assert float(gg.abs().max()) > 0
    assert differ == 0
    if side:
        unequal = [name for name, a, b in zip(("labels", "conf", "counts"), *side) if not torch.equal(a, b)]
        print("pseudo_label P=%d: side outputs that differ between the two paths: %s; selected %d of %d" % (P, unequal, int(side[0][2][1].sum()), P))
        assert not unequal
