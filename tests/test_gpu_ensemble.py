"""-m gpu: pnp_paste_ensemble (csrc/paste.hip) against the float64 restatement of tests/ensemble_ref.py.

Every case pre-fills vol with 0xAB and prob / entropy with a finite sentinel and compares the WHOLE of all three allocations: a store
outside the box or the frame range fails the case.  The shapes are paste_ref.CASES / paste_ref.layout (odd extents, more than one
workgroup, head / dword / tail bytes at an odd z0, a 7-frame batch, negative strides with the slicing axis first, a box inside a larger
allocation); M in {1, 3, 8} and ncls in {1, 2, 5, 8} are swept on the `upsample` case (ensemble_ref.SWEEP), prob and entropy each null
and non-null.  The logits are smooth (ensemble_ref.smooth_logits), member m uses ensemble_ref.MAPS[m].

Bounds (derived in DESIGN.md §15 and at ensemble_ref.delta_p / entropy_bound, not tuned on the device):
  |P_c - P_c^ref| <= delta_p = delta_r / 2 + 20 * 2^-24 (delta_r = paste_ref.delta maximised over the members);
  the label lies in {c : P_c^ref >= max P^ref - 2 delta_p}, no voxel excluded (that this set is a single class at all but <= 1e-3 of the
  voxels per class count: tests/test_ensemble_host.py);
  |H - H^ref| <= ncls (-delta_p ln delta_p) / ln(ncls) + (4 ncls + 4) 2^-24;
  |sum_c P_c - 1| <= ncls 2^-23.
The exact cases carry no bound.
"""
import numpy as np
import pytest
import torch

import ensemble_ref as E
import paste_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

FILL = 0xAB
SENTINEL = -7.0


def _inv(XY, HW, **kw):
    return pkg("volume_predict").invert_matrix(pkg("volume_source").compose_matrix(XY, HW, **kw))


def _run(dev, logits, nb, z0, invs, XY, elems, origin, strides, prob=True, entropy=True):
    """logits: a list of numpy arrays; an array listed twice (the same object) is uploaded once and its pointer given twice"""
    K = pkg("kernels")
    ncls = logits[0].shape[-1]
    up = {}
    members = [up.setdefault(id(a), torch.from_numpy(a).to(dev)) for a in logits]
    vol = torch.full((elems,), FILL, dtype=torch.uint8, device=dev)
    p = torch.full((ncls * elems,), SENTINEL, dtype=torch.float32, device=dev) if prob else None
    h = torch.full((elems,), SENTINEL, dtype=torch.float32, device=dev) if entropy else None
    K.paste_ensemble(members, nb, z0, invs, XY, vol, origin, strides, prob=p, entropy=h)
    torch.cuda.synchronize()
    return vol.cpu().numpy(), None if p is None else p.cpu().numpy(), None if h is None else h.cpu().numpy()


def _check(got, logits, nb, z0, invs, XY, origin, strides, what):
    """the whole of the three allocations: the fill wherever the launch must not write, values inside the bounds everywhere else"""
    vol, prob, ent = got
    X, Y = XY
    ncls = logits[0].shape[-1]
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    untouched = np.ones(vol.size, bool)
    untouched[idx.ravel()] = False
    assert np.all(vol[untouched] == FILL), "%s: %d label stores outside the box / frame range" % (what, int((vol[untouched] != FILL).sum()))
    res = E.ensemble(logits, invs, X, Y, nb)
    dp = E.delta_p(logits, invs, X, Y, nb)
    lab = vol[idx]
    assert lab.max() < ncls, "%s: a label >= ncls (or an unwritten voxel inside the box)" % what
    ok = np.take_along_axis(E.admissible(res.prob, dp), lab[..., None].astype(np.int64), axis=-1)[..., 0]
    line = "%s: %d of %d labels differ from the float64 argmax, %d outside the bound" % (what, int((lab != res.label).sum()), lab.size, int((~ok).sum()))
    if prob is not None:
        prob = prob.reshape(ncls, vol.size)
        assert np.all(prob[:, untouched] == SENTINEL), "%s: probability stores outside the box / frame range" % what
        P = np.moveaxis(prob[:, idx.ravel()].reshape((ncls,) + idx.shape), 0, -1).astype(np.float64)
        err, serr = float(np.abs(P - res.prob).max()), float(np.abs(P.sum(-1) - 1.0).max())
        line += "; max|dP| %.3g (bound %.3g), max|sum P - 1| %.3g (bound %.3g)" % (err, dp, serr, ncls * 2.0 ** -23)
    if ent is not None:
        assert np.all(ent[untouched] == SENTINEL), "%s: entropy stores outside the box / frame range" % what
        hb = E.entropy_bound(dp, ncls)
        herr = float(np.abs(ent[idx].astype(np.float64) - res.entropy).max())
        line += "; max|dH| %.3g (bound %.3g)" % (herr, hb)
    print(line)
    assert ok.all(), line
    if prob is not None:
        assert err <= dp and serr <= ncls * 2.0 ** -23, line
    if ent is not None:
        assert herr <= hb, line
        if ncls == 1:
            assert np.all(ent[idx] == 0.0)


def _case(case, M, ncls):
    (H, W), (X, Y), B, nb, z0, Z, kind = R.CASES[case]
    elems, origin, strides = R.layout(kind, X, Y, Z)
    logits = [E.smooth_logits(case, ncls, m) for m in range(M)]
    invs = [_inv((X, Y), (H, W), **E.MAPS[m]) for m in range(M)]
    return logits, nb, z0, invs, (X, Y), elems, origin, strides


@pytest.mark.parametrize("case,M,ncls", E.SWEEP, ids=["%s-M%d-ncls%d" % c for c in E.SWEEP])
def test_ensemble_against_the_restatement(dev, case, M, ncls):
    logits, nb, z0, invs, XY, elems, origin, strides = _case(case, M, ncls)
    got = _run(dev, logits, nb, z0, invs, XY, elems, origin, strides)
    _check(got, logits, nb, z0, invs, XY, origin, strides, "%s/M=%d/ncls=%d" % (case, M, ncls))


@pytest.mark.parametrize("prob,entropy", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("case", ["sixteen_at_odd", "axis_first_flip"])
def test_null_outputs(dev, case, prob, entropy):
    """prob and entropy each null: the outputs that are asked for do not change, bit for bit"""
    logits, nb, z0, invs, XY, elems, origin, strides = _case(case, 3, 5)
    got = _run(dev, logits, nb, z0, invs, XY, elems, origin, strides, prob=prob, entropy=entropy)
    assert (got[1] is None) == (not prob) and (got[2] is None) == (not entropy)
    _check(got, logits, nb, z0, invs, XY, origin, strides, "%s/prob=%s/entropy=%s" % (case, prob, entropy))
    both = _run(dev, logits, nb, z0, invs, XY, elems, origin, strides)
    for a, b in zip(got, both):
        assert a is None or np.array_equal(a, b)


@pytest.mark.parametrize("kind", ["c", "zfirst_flipped"])
def test_a_member_given_2_4_8_times_is_that_member(dev, kind):
    """the same pointer and inv M = 2, 4, 8 times: labels, probabilities and entropy bit-identical to M = 1 (the member sum runs in two
    runs of four, p + p + p + p is exact, and acc * (1.0f / M) is exact for a power of two)"""
    (H, W), (X, Y), B, nb, z0, Z = (16, 24), (37, 23), 4, 3, 1, 6
    elems, origin, strides = R.layout(kind, X, Y, Z)
    lg = E.smooth_logits("upsample", 5, 0)
    inv = _inv((X, Y), (H, W), **E.MAPS[1])
    one = _run(dev, [lg], nb, z0, [inv], (X, Y), elems, origin, strides)
    assert len(np.unique(one[0])) > 2
    for M in (2, 4, 8):
        many = _run(dev, [lg] * M, nb, z0, [inv] * M, (X, Y), elems, origin, strides)
        for a, b, name in zip(one, many, ("label", "prob", "entropy")):
            assert np.array_equal(a, b), "M = %d: %s differs from M = 1 at %d elements" % (M, name, int((a != b).sum()))


def test_equal_logits_ties_and_one_class(dev):
    """all-equal logits: label 0 and every P_c the float32 value of 1 / ncls (entropy 1 within its rounding term); two equal maxima: the
    lower index; ncls = 1: P = 1 and entropy 0 — under a map that reaches the clamp, for M = 1, 2, 4, 8"""
    (H, W), (X, Y) = (16, 24), (37, 23)
    elems, origin, strides = R.layout("c", X, Y, 4)
    inv = _inv((X, Y), (H, W), **E.MAPS[1])
    idx = R.written_index(X, Y, 4, 0, origin, strides)
    for M in (1, 2, 4, 8):
        for ncls in (2, 3, 5, 8):
            flat = np.full((4, H, W, ncls), 0.375, np.float32)
            vol, prob, ent = _run(dev, [flat] * M, 4, 0, [inv] * M, (X, Y), elems, origin, strides)
            assert np.all(vol[idx] == 0)
            assert np.all(prob.reshape(ncls, elems)[:, idx.ravel()] == np.float32(1.0) / np.float32(ncls)), (M, ncls)
            # the reference entropy of 1 / ncls is 1; the float32 value of 1 / ncls is within 2^-25 of it
            assert np.abs(ent[idx].astype(np.float64) - 1.0).max() <= E.entropy_bound(2.0 ** -25, ncls), (M, ncls)
        two = np.zeros((4, H, W, 5), np.float32)
        two[..., 1] = two[..., 3] = 1.7
        two[..., 4] = -2.0
        vol, prob, _ = _run(dev, [two] * M, 4, 0, [inv] * M, (X, Y), elems, origin, strides)
        p = prob.reshape(5, elems)[:, idx.ravel()]
        assert np.all(vol[idx] == 1) and np.array_equal(p[1], p[3]) and np.all(p[1] > p[0])
        single = np.random.default_rng(M).standard_normal((4, H, W, 1)).astype(np.float32)
        vol, prob, ent = _run(dev, [single] * M, 4, 0, [inv] * M, (X, Y), elems, origin, strides)
        assert np.all(vol[idx] == 0) and np.all(prob[idx.ravel()] == 1.0) and np.all(ent[idx] == 0.0)
    # M = 3 is not a power of two: 3 * fl(1 / 3) still rounds to 1 for one class
    vol, prob, ent = _run(dev, [single] * 3, 4, 0, [inv] * 3, (X, Y), elems, origin, strides)
    assert np.all(prob[idx.ravel()] == 1.0) and np.all(ent[idx] == 0.0)


@pytest.mark.parametrize("kind", ["c", "zfirst_flipped"])
@pytest.mark.parametrize("rotate", [0.0, 90.0, 180.0, 270.0, -90.0])
def test_identity_and_quarter_turns_are_the_corners_softmax_permuted(dev, rotate, kind):
    """M = 1, integer coordinates: the interpolation returns the corner's logits bit for bit, so prob is the identity map's prob permuted,
    bit for bit, the label is the argmax of the logits permuted, and the identity map's prob is the float64 softmax of the logits within
    the rounding term of the bound alone (20 * 2^-24)"""
    n, B, z0, Z, ncls = 16, 3, 1, 5, 5
    logits = (3.0 * np.random.default_rng(int(rotate) + 400).standard_normal((B, n, n, ncls))).astype(np.float32)
    inv = _inv((n, n), (n, n), rotate=rotate)
    pi, pj = R.coords(inv, n, n)
    assert np.array_equal(pi, np.round(pi)) and pi.min() == 0 and pi.max() == n - 1 and np.array_equal(pj, np.round(pj))
    elems, origin, strides = R.layout(kind, n, n, Z)
    idx = R.written_index(n, n, B, z0, origin, strides)
    vol, prob, ent = _run(dev, [logits], B, z0, [inv], (n, n), elems, origin, strides)
    ident = _run(dev, [logits], B, z0, [[1, 0, 0, 0, 1, 0]], (n, n), elems, origin, strides)
    P_id = np.moveaxis(ident[1].reshape(ncls, elems)[:, idx.ravel()].reshape(ncls, B, n, n), 0, -1)          # [B, n, n, ncls] of the identity map
    assert np.abs(P_id.astype(np.float64) - E.softmax(logits.astype(np.float64))).max() <= E.K_ROUND * E.U
    ii, jj = pi.astype(np.int64), pj.astype(np.int64)
    want_v, want_p, want_h = np.full(elems, FILL, np.uint8), np.full(ncls * elems, SENTINEL, np.float32), np.full(elems, SENTINEL, np.float32)
    want_v[idx.ravel()] = ident[0][idx][:, ii, jj].ravel()
    want_p.reshape(ncls, elems)[:, idx.ravel()] = P_id[:, ii, jj].reshape(-1, ncls).T
    want_h[idx.ravel()] = ident[2][idx][:, ii, jj].ravel()
    assert np.array_equal(vol, want_v) and np.array_equal(prob, want_p) and np.array_equal(ent, want_h)
    # the labels are the argmax of the logits wherever float32 softmax keeps the two largest logits apart
    am = np.argmax(logits, -1)[:, ii, jj]
    top = np.sort(logits.astype(np.float64), -1)
    clear = ((top[..., -1] - top[..., -2]) > 1e-5)[:, ii, jj]
    assert clear.mean() > 0.99 and np.array_equal(vol[idx][clear], am[clear].astype(np.uint8))


def test_kernels_wrapper_refuses_cpu_tensors_and_reports_the_library_s_text(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lg = torch.zeros((2, 8, 8, 5), device=dev)
    ident = [1, 0, 0, 0, 1, 0]
    vol = torch.zeros(4 * 5 * 6, dtype=torch.uint8, device=dev)
    prob = torch.zeros(5 * 4 * 5 * 6, device=dev)
    ent = torch.zeros(4 * 5 * 6, device=dev)
    args = lambda **kw: dict(dict(logits=[lg, lg], nb=2, z0=0, invs=[ident, ident], src_xy=(4, 5), vol=vol, origin=0, strides=(30, 6, 1), prob=prob, entropy=ent), **kw)
    for bad in (dict(vol=vol.cpu()), dict(logits=[lg, lg.cpu()]), dict(prob=prob.cpu()), dict(entropy=ent.cpu())):
        with pytest.raises(L.PnpError, match="no CPU fallback"):
            K.paste_ensemble(**args(**bad))
    for bad, text in ((dict(logits=[lg, lg.double()]), "float32"), (dict(logits=[lg, lg.permute(0, 2, 1, 3)]), "contiguous"),
                      (dict(logits=[lg, lg[:1]]), "one shape"), (dict(prob=prob[:-1]), "600 elements"), (dict(entropy=ent.double()), "float32"),
                      (dict(vol=vol.float()), "uint8"), (dict(invs=[ident]), "2 members with 1 maps"), (dict(logits=[], invs=[]), "0 members"),
                      (dict(logits=[lg] * 9, invs=[ident] * 9), "M = 9 members outside \\[1, 8\\]"),
                      (dict(z0=5), "pnp_paste_ensemble: the box addresses elements outside \\[0, 120\\)"),
                      (dict(strides=(30, 1, 1)), "pnp_paste_ensemble: strides 30 1 1 let two voxels")):
        with pytest.raises(L.PnpError, match=text):
            K.paste_ensemble(**args(**bad))
    torch.cuda.synchronize()
    assert not vol.any() and not prob.any() and not ent.any()          # untouched after every refusal
    K.paste_ensemble(**args())
    torch.cuda.synchronize()
    idx = R.written_index(4, 5, 2, 0, 0, (30, 6, 1)).ravel()
    assert np.all(prob.cpu().numpy().reshape(5, 120)[:, idx] == np.float32(1.0) / np.float32(5.0)) and (prob != 0).sum().item() == 5 * idx.size
