"""-m gpu: pnp_fuse_views (csrc/paste.hip) against the float64 restatement of tests/fuse_ref.py.

Every output lies inside a larger allocation with guard elements on both sides, everything pre-filled with 0xAB / -7.0: the guards must
stay untouched and every interior element must be written (the kernel writes all of its outputs, so callers may pass torch.empty).
The bounds are fuse_ref's: |P - P_ref| <= delta_p(M) against float64 on the same float32 inputs, the label inside admissible(P_ref,
delta_p) with at most 2 elements per case that admit more than one class (tests/test_fuse_host.py checks that on the reference alone),
the entropy within entropy_bound(delta_p, ncls), and an element no view covers exactly 0 in all three outputs.

693 elements are odd, so for ncls > 1 the class planes lie on different phases of the 16-byte grid and the kernel takes its scalar path
(ncls = 1 takes the wide path with a tail); the cases at 696 elements take the wide path for ncls > 1 too, with and without a peeled
head, with the label word-aligned and not."""
import functools

import numpy as np
import pytest
import torch

import fuse_ref as F
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 64              # elements: 256 bytes of float32, 64 bytes of uint8 — the interior of an aligned run starts on a 16-byte boundary
N = int(np.prod(F.SHAPE))


@functools.lru_cache(maxsize=None)
def _case(M, ncls, n, seed=0):
    probs, w = F.make_case(M, ncls, n, seed)
    return probs, w, F.fuse(probs, w), F.fuse(probs, None)


def _guarded(dev, n, dtype, fill, off):
    whole = torch.full((GUARD + off + n + GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD + off:GUARD + off + n]


def _run(dev, probs, weights, off=0, label_off=None, alias=False, want_prob=True, want_entropy=True):
    """one launch; inputs and outputs start `off` elements into their allocations (label: label_off, default off) -> numpy (label, prob
    [ncls, n], entropy), after the guard and written-everywhere checks"""
    K = pkg("kernels")
    ncls, n = probs[0].shape
    ins = []
    for p in probs:
        t = torch.zeros(off + ncls * n, dtype=torch.float32, device=dev)
        t[off:] = torch.from_numpy(p.reshape(-1)).to(dev)
        ins.append(t[off:].view(ncls, n))
    lw, lab = _guarded(dev, n, torch.uint8, 0xAB, off if label_off is None else label_off)
    pw, prob = _guarded(dev, ncls * n, torch.float32, -7.0, off)
    hw, ent = _guarded(dev, n, torch.float32, -7.0, off)
    out_p = (ins[0] if alias else prob.view(ncls, n)) if want_prob else None
    got = K.fuse_views(ins, None if weights is None else [float(v) for v in weights], label=lab, prob=out_p, entropy=ent if want_entropy else None)
    assert got[0] is lab and got[1] is out_p and got[2] is (ent if want_entropy else None)
    torch.cuda.synchronize()
    for whole, inner, fill, used in ((lw, lab, 0xAB, True), (pw, prob, -7.0, want_prob and not alias), (hw, ent, -7.0, want_entropy)):
        w = whole.cpu().numpy()
        lo = inner.data_ptr() - whole.data_ptr()
        lo //= whole.element_size()
        assert np.all(w[:lo] == fill) and np.all(w[lo + inner.numel():] == fill), "a guard element was written"
        assert np.all(w[lo:lo + inner.numel()] != fill) if used else np.all(w[lo:lo + inner.numel()] == fill)
    P = (ins[0] if alias else prob.view(ncls, n)).cpu().numpy() if want_prob else None
    return lab.cpu().numpy(), P, ent.cpu().numpy() if want_entropy else None


def _check(got, ref, M, ncls, what):
    lab, P, H = got
    dp = F.delta_p(M)
    assert np.array_equal(ref.covered, P.sum(0) > 0.5), what
    unc = ~ref.covered
    assert not lab[unc].any() and not P[:, unc].any() and not H[unc].any(), "%s: an uncovered element is not 0" % what
    e1 = float(np.abs(P.astype(np.float64) - ref.prob).max())
    adm = F.admissible(np.moveaxis(ref.prob, 0, -1), dp)
    ok = np.take_along_axis(adm, lab[:, None].astype(np.int64), axis=-1)[:, 0]
    multi = int(((adm.sum(-1) > 1) & ref.covered).sum())
    hb = F.entropy_bound(dp, ncls)
    e2 = float(np.abs(H.astype(np.float64) - ref.entropy).max())
    print("%s: max|dP| %.3g (bound %.3g), max|dH| %.3g (bound %.3g), %d labels differ from the float64 argmax, %d elements admit more than "
          "one class, %d of %d covered" % (what, e1, dp, e2, hb, int((lab != ref.label).sum()), multi, int(ref.covered.sum()), lab.size))
    assert e1 <= dp, what
    assert bool(ok[ref.covered].all()) and multi <= 2, what
    assert e2 <= hb, what


@pytest.mark.parametrize("M,ncls", F.SWEEP)
def test_sweep_against_the_restatement(dev, M, ncls):
    probs, w, ref_w, ref_1 = _case(M, ncls, N)
    _check(_run(dev, probs, w), ref_w, M, ncls, "M = %d, ncls = %d, weights" % (M, ncls))
    _check(_run(dev, probs, None), ref_1, M, ncls, "M = %d, ncls = %d, no weights" % (M, ncls))
    if M <= 3:
        assert (~ref_w.covered).any(), "25 % zeroed per view: some element has no view"


def test_more_than_one_pass_of_the_grid(dev):
    M, ncls, n = F.BIG
    probs, w, ref_w, _ = _case(M, ncls, n, F.BIG_SEED)
    assert n > 2048 * 256
    _check(_run(dev, probs, w), ref_w, M, ncls, "2^20 + 3 elements")


def _scalar_path(dev, probs, w):
    """the same fusion with view v starting v % 2 floats into its allocation: no common phase, so every element takes the scalar path"""
    K = pkg("kernels")
    ncls, n = probs[0].shape
    ins = []
    for v, p in enumerate(probs):
        t = torch.zeros(1 + p.size, dtype=torch.float32, device=dev)
        t[v % 2:v % 2 + p.size] = torch.from_numpy(p.reshape(-1)).to(dev)
        ins.append(t[v % 2:v % 2 + p.size].view(ncls, n))
    lab, P, H = K.fuse_views(ins, [float(v) for v in w], prob=True, entropy=True)
    return lab.cpu().numpy().ravel(), P.cpu().numpy(), H.cpu().numpy().ravel()


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("label", "prob", "entropy")):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, name)


@pytest.mark.parametrize("M,ncls,n", [(3, 5, 696), (2, 8, 696), (8, 1, N)])
@pytest.mark.parametrize("off,label_off", [(0, 0), (1, 1), (1, 2), (3, 0)])
def test_the_wide_path(dev, M, ncls, n, off, label_off):
    """vol_elems % 4 == 0 (or one plane): 16-byte accesses, with a peeled head when the bases start `off` floats past a 16-byte boundary
    and with single label bytes when label + head is not word-aligned; the restatement's bounds, and the same bits as the scalar path
    gives for the same elements"""
    probs, w, ref_w, _ = _case(M, ncls, n, 1)
    got = _run(dev, probs, w, off=off, label_off=label_off)
    _check(got, ref_w, M, ncls, "wide path, %d elements, M = %d, ncls = %d, offset %d / %d" % (n, M, ncls, off, label_off))
    _same_bits(got, _scalar_path(dev, probs, w), (M, ncls, n, off, label_off))


def test_more_than_one_pass_of_the_wide_groups(dev):
    """2^21 + 8 elements are 2^19 + 2 groups of four, more than the 2^19 lanes of a pass: bit for bit the scalar path's result, which
    test_more_than_one_pass_of_the_grid holds to the restatement"""
    probs, w = F.make_case(3, 5, 2 ** 21 + 8, 0)
    _same_bits(_run(dev, probs, w, off=1, label_off=2), _scalar_path(dev, probs, w), "2^21 + 8 elements")


def test_misaligned_bases_give_the_aligned_run_bit_for_bit(dev):
    """every input and output starts one element into its allocation: aligned to 4 bytes only (1 byte for the label)"""
    for M, ncls in ((3, 5), (8, 8), (2, 1)):
        probs, w, ref_w, _ = _case(M, ncls, N)
        a = _run(dev, probs, w, off=0)
        b = _run(dev, probs, w, off=1)
        _same_bits(a, b, (M, ncls))


def test_equal_classes_give_the_lower_one(dev):
    """classes 1 and 3 bit-identical in every view (and the largest): label 1 wherever a view covers, and bit-identical fused planes"""
    M, ncls = 3, 5
    probs, w, _, _ = _case(M, ncls, N)
    twin = []
    for p in probs:
        q = p.copy()
        q[3] = q[1] = np.maximum(q[1], q[3]) + np.float32(1.0) * (q.sum(0) > 0.5)          # not a distribution any more: still covered, sums > 0.5
        twin.append(q)
    for weights in (w, None):
        lab, P, _ = _run(dev, twin, weights)
        cov = np.stack([q.sum(0) > 0.5 for q in twin]).any(0)
        assert np.array_equal(P[1].view(np.uint32), P[3].view(np.uint32))
        assert np.all(lab[cov] == 1) and not lab[~cov].any() and cov.any() and (~cov).any()


def test_one_view_without_weights_is_the_identity(dev):
    for ncls in (1, 2, 5, 8):
        probs, _, _, ref_1 = _case(1, ncls, N)
        lab, P, H = _run(dev, probs, None)
        assert np.array_equal(P.view(np.uint32), probs[0].view(np.uint32)), "ncls = %d: P is not the input bit for bit" % ncls
        first = np.argmax(probs[0], axis=0)                                # numpy's argmax is the first maximum; float32 compares exactly
        assert np.array_equal(lab, np.where(ref_1.covered, first, 0))


def test_prob_may_alias_the_first_view(dev):
    for M, ncls, n in ((3, 5, N), (8, 8, N), (3, 5, 696), (2, 1, N)):
        probs, w, _, _ = _case(M, ncls, n, 0 if n == N else 1)
        apart = _run(dev, probs, w)
        alias = _run(dev, probs, w, alias=True)
        _same_bits(apart, alias, (M, ncls, n))


def test_two_runs_give_identical_bits_and_null_outputs_are_skipped(dev):
    probs, w, ref_w, _ = _case(3, 5, N)
    a, b = _run(dev, probs, w), _run(dev, probs, w)
    _same_bits(a, b, "two runs")
    lab, P, H = _run(dev, probs, w, want_prob=False, want_entropy=False)
    assert P is None and H is None and np.array_equal(lab, a[0])
    lab, P, H = _run(dev, probs, w, want_prob=False)
    assert P is None and np.array_equal(H.view(np.uint32), a[2].view(np.uint32)) and np.array_equal(lab, a[0])
    # new tensors of the views' shape when none are passed
    K = pkg("kernels")
    ins = [torch.from_numpy(p.reshape((5,) + F.SHAPE)).to(dev) for p in probs]
    lab, P, H = K.fuse_views(ins, [float(v) for v in w], prob=True, entropy=True)
    assert tuple(lab.shape) == F.SHAPE and tuple(P.shape) == (5,) + F.SHAPE and tuple(H.shape) == F.SHAPE
    assert np.array_equal(lab.cpu().numpy().ravel(), a[0]) and np.array_equal(P.cpu().numpy().reshape(5, -1), a[1])
    lab2, P2, H2 = K.fuse_views(ins, [float(v) for v in w])
    assert P2 is None and H2 is None and torch.equal(lab2, lab)


def test_refusals_launch_nothing(dev):
    K, L = pkg("kernels"), pkg("_lib")
    n = 24
    views = [torch.full((5, n), 0.2, dtype=torch.float32, device=dev) for _ in range(9)]
    lab = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
    prob = torch.full((5, n), -7.0, dtype=torch.float32, device=dev)
    ent = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    big = torch.full((5 * n + 8,), 0.2, dtype=torch.float32, device=dev)
    for kw, text in ((dict(probs=[]), "n_views = 0 outside \\[1, 8\\]"),
                     (dict(probs=views), "n_views = 9 outside \\[1, 8\\]"),
                     (dict(probs=[torch.zeros((9, n), dtype=torch.float32, device=dev)], prob=None), "ncls 9 outside \\[1, 8\\]"),
                     (dict(probs=[views[0], views[1].cpu()]), "no CPU fallback"),
                     (dict(probs=views[:2], label=lab.cpu()), "no CPU fallback"),
                     (dict(probs=views[:2], weights=[1.0, 0.0]), "weight 1 = 0 must be positive and finite"),
                     (dict(probs=views[:2], weights=[-1.0, 1.0]), "weight 0 = -1 must be positive and finite"),
                     (dict(probs=views[:2], weights=[1.0]), "1 weights for 2 views"),
                     (dict(probs=[big[:5 * n].view(5, n), big[4:4 + 5 * n].view(5, n)]), "a view overlaps a view"),
                     (dict(probs=[big[:5 * n].view(5, n), views[1]], prob=big[8:8 + 5 * n].view(5, n)), "a view overlaps prob"),
                     (dict(probs=views[:2], prob=views[1]), "a view overlaps prob"),
                     (dict(probs=views[:2], entropy=views[0].view(-1)[:n]), "a view overlaps entropy"),
                     (dict(probs=views[:2], prob=prob[:4]), "prob must be a contiguous float32 CUDA tensor of 120 elements"),
                     (dict(probs=views[:2], entropy=ent.double()), "entropy must be a contiguous float32 CUDA tensor"),
                     (dict(probs=[views[0], views[1][:, :n - 1]]), "one shape")):
        args = dict(weights=None, label=lab, prob=prob, entropy=ent)
        args.update(kw)
        with pytest.raises(L.PnpError, match=text):
            K.fuse_views(**args)
    torch.cuda.synchronize()
    assert bool((lab == 0xAB).all()) and bool((prob == -7.0).all()) and bool((ent == -7.0).all()) and bool((big == 0.2).all())
    K.fuse_views(views[:2], label=lab, prob=prob, entropy=ent)                   # and the same buffers are served once the arguments are right
    assert not bool((lab == 0xAB).any()) and not bool((prob == -7.0).any()) and not bool((ent == -7.0).any())
