"""-m gpu: pnp_paste_labels (csrc/paste.hip) against the float64 restatement of tests/paste_ref.py.

Every case pre-fills the destination with 0xAB and compares the WHOLE allocation: a store outside the frame range or the box fails.  The
shapes (paste_ref.CASES) are the smallest that reach the tails and alignments the layout can get wrong: odd extents, more than one
workgroup (37 x 23 columns), 16 frames at an odd z0 and a 7-frame batch (head bytes, packed dwords, tail bytes of the z-fastest store),
the slicing axis first with both in-plane axes flipped (negative strides, the byte-per-frame store), a box inside a larger allocation.

Bound (derived, not tuned): with the float64 interpolated logits r[v, c], the device label lies in {c : r[v, c] >= max_c r[v, c] - 2 delta},
delta = eps (Gi + Gj) + 4 * 2^-24 max|logit| (eps = 4 float32 ulps at the largest coordinate term; Gi, Gj = the largest gap between adjacent
logits of one class along each axis): the form of the image bound of the gather.  No voxel is excluded.  That the set is a single class at
all but <= 1e-3 of the voxels is checked on the CPU (tests/test_paste_host.py).  The exact cases carry no bound.
"""
import numpy as np
import pytest
import torch

import paste_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

FILL = 0xAB


def _inv(XY, HW, **kw):
    return pkg("volume_predict").invert_matrix(pkg("volume_source").compose_matrix(XY, HW, **kw))


def _run(dev, logits, nb, z0, inv, XY, elems, origin, strides):
    K = pkg("kernels")
    vol = torch.full((elems,), FILL, dtype=torch.uint8, device=dev)
    K.paste_labels(torch.from_numpy(logits).to(dev), nb, z0, inv, XY, vol, origin, strides)
    torch.cuda.synchronize()
    return vol.cpu().numpy()


def _check(got, logits, nb, z0, inv, XY, origin, strides, what):
    """the whole allocation: 0xAB wherever the launch must not write, an admissible label everywhere else"""
    X, Y = XY
    ncls = logits.shape[-1]
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    untouched = np.ones(got.size, bool)
    untouched[idx.ravel()] = False
    assert np.all(got[untouched] == FILL), "%s: %d stores outside the box / frame range" % (what, int((got[untouched] != FILL).sum()))
    lab, r = R.labels(logits, inv, X, Y, nb)
    dev_lab = got[idx]
    assert dev_lab.max() < ncls, "%s: a label >= ncls (or an unwritten voxel inside the box)" % what
    ok = np.take_along_axis(R.admissible(r, R.delta(logits[:nb], inv, X, Y)), dev_lab[..., None].astype(np.int64), axis=-1)[..., 0]
    print("%s: %d of %d labels differ from the float64 argmax, %d outside the bound" % (what, int((dev_lab != lab).sum()), lab.size, int((~ok).sum())))
    assert ok.all(), "%s: %d labels outside the bound" % (what, int((~ok).sum()))


@pytest.mark.parametrize("which", sorted(R.MAPS))
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_paste_against_the_restatement(dev, case, which):
    (H, W), (X, Y), B, nb, z0, Z, kind = R.CASES[case]
    elems, origin, strides = R.layout(kind, X, Y, Z)
    logits = R.case_logits(case, 5)
    inv = _inv((X, Y), (H, W), **R.MAPS[which])
    got = _run(dev, logits, nb, z0, inv, (X, Y), elems, origin, strides)
    _check(got, logits, nb, z0, inv, (X, Y), origin, strides, "%s/%s" % (case, which))


@pytest.mark.parametrize("which", sorted(R.MAPS))
@pytest.mark.parametrize("ncls", [1, 2, 8])
def test_paste_class_counts(dev, ncls, which):
    (H, W), (X, Y), B, nb, z0, Z, kind = R.CASES["upsample"]
    elems, origin, strides = R.layout(kind, X, Y, Z)
    logits = R.case_logits("upsample", ncls)
    inv = _inv((X, Y), (H, W), **R.MAPS[which])
    got = _run(dev, logits, nb, z0, inv, (X, Y), elems, origin, strides)
    _check(got, logits, nb, z0, inv, (X, Y), origin, strides, "upsample/%s/ncls=%d" % (which, ncls))


@pytest.mark.parametrize("kind", ["c", "zfirst_flipped"])
@pytest.mark.parametrize("rotate", [0.0, 90.0, 180.0, 270.0, -90.0])
def test_identity_and_quarter_turns_are_argmax_permuted(dev, rotate, kind):
    """bit for bit: integer coordinates return the corner's logits themselves"""
    n, B, z0, Z = 16, 3, 1, 5
    logits = np.random.default_rng(int(rotate) + 400).standard_normal((B, n, n, 5)).astype(np.float32)
    inv = _inv((n, n), (n, n), rotate=rotate)
    pi, pj = R.coords(inv, n, n)
    assert np.array_equal(pi, np.round(pi)) and pi.min() == 0 and pi.max() == n - 1 and np.array_equal(pj, np.round(pj))
    elems, origin, strides = R.layout(kind, n, n, Z)
    got = _run(dev, logits, B, z0, inv, (n, n), elems, origin, strides)
    want = np.full(elems, FILL, np.uint8)
    am = np.argmax(logits, -1).astype(np.uint8)
    R.paste(want, am[:, pi.astype(np.int64), pj.astype(np.int64)], z0, origin, strides)
    assert np.array_equal(got, want)
    if rotate == 0.0:
        assert np.array_equal(inv, np.array([1, 0, 0, 0, 1, 0], np.float32))


def test_ties_and_constant_planes(dev):
    """all-equal logits give label 0; two equal maxima give the lower index; a plane of one constant class stays that class under any map"""
    (H, W), (X, Y) = (16, 24), (37, 23)
    elems, origin, strides = R.layout("c", X, Y, 4)
    inv = _inv((X, Y), (H, W), **R.MAPS["rotated"])
    idx = R.written_index(X, Y, 4, 0, origin, strides)
    flat = np.full((4, H, W, 5), 0.375, np.float32)
    assert np.all(_run(dev, flat, 4, 0, inv, (X, Y), elems, origin, strides)[idx] == 0)
    two = np.zeros((4, H, W, 5), np.float32)
    two[..., 1] = two[..., 3] = 1.7
    two[..., 4] = -2.0
    assert np.all(_run(dev, two, 4, 0, inv, (X, Y), elems, origin, strides)[idx] == 1)
    const = np.random.default_rng(1).standard_normal((4, 1, 1, 5)).astype(np.float32) * np.ones((1, H, W, 1), np.float32)
    for b, k in enumerate((4, 0, 2, 3)):
        const[b, :, :, k] = 5.0 + b
    got = _run(dev, const, 4, 0, inv, (X, Y), elems, origin, strides)[idx]
    for b, k in enumerate((4, 0, 2, 3)):
        assert np.all(got[b] == k), (b, k)


def test_kernels_wrapper_refuses_cpu_tensors_and_reports_the_library_s_text(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lg = torch.zeros((2, 8, 8, 5), device=dev)
    vol = torch.zeros(4 * 5 * 6, dtype=torch.uint8, device=dev)
    with pytest.raises(L.PnpError, match="no CPU fallback"):
        K.paste_labels(lg, 2, 0, [1, 0, 0, 0, 1, 0], (4, 5), vol.cpu(), 0, (30, 6, 1))
    with pytest.raises(L.PnpError, match="no CPU fallback"):
        K.paste_labels(lg.cpu(), 2, 0, [1, 0, 0, 0, 1, 0], (4, 5), vol, 0, (30, 6, 1))
    with pytest.raises(L.PnpError, match="outside \\[0, 120\\)"):
        K.paste_labels(lg, 2, 5, [1, 0, 0, 0, 1, 0], (4, 5), vol, 0, (30, 6, 1))
    with pytest.raises(L.PnpError, match="collide"):
        K.paste_labels(lg, 2, 0, [1, 0, 0, 0, 1, 0], (4, 5), vol, 0, (30, 1, 1))
    assert not vol.any()
