"""-m gpu: pnp_paste_tiles (csrc/paste.hip) against the float64 restatement of tests/tiles_ref.py.

Every case pre-fills vol with 0xAB and prob / entropy with a finite sentinel and compares the WHOLE of all three allocations: a store
outside the box, outside the frame range or on a column that no member covers fails the case.  The cases are tiles_ref.CASES: member
counts 1, 2, 4, 9, 64 and class counts 1, 2, 5, 8, the three store layouts (sz = +1 and sz = -1 at an odd offset and an unaligned z0, the
slicing axis first with negative in-plane strides), a short last batch, columns covered by 0, 1, 2, 4 and (M = 64) more than 8 members,
rotated, scaled and flipped tiles.  The logits are smooth (tiles_ref.case_logits).

Bounds (derived in DESIGN.md §20 and at tiles_ref.k_tiles / delta_p_tiles, not tuned on the device):
  |P_c - P_c^ref| <= delta_p_tiles = delta_r / 2 + (2 M + 18) 2^-24 (+ 2 coord_eps where a member's coordinates are not exact in float32);
  the label lies in {c : P_c^ref >= max P^ref - 2 delta_p_tiles} (a single class at all but <= 5 % of the voxels: tests/test_tiles_host.py);
  |H - H^ref| <= ensemble_ref.entropy_bound(delta_p_tiles, ncls);   |sum_c P_c - 1| <= ncls 2^-23.
Coverage is decided in float32 on the device: the columns of tiles_ref.edge_columns (within paste_ref.coord_eps of a member's border; at
most 2 % of a box, none on these cases: tests/test_tiles_host.py) may be written or not and carry no bound.  The exact cases carry no bound.
"""
import numpy as np
import pytest
import torch

import ensemble_ref as E
import paste_ref as R
import tiles_ref as T
from conftest import pkg

pytestmark = pytest.mark.gpu

FILL = 0xAB
SENTINEL = -7.0


def _inv(XY, HW, **kw):
    return pkg("volume_predict").invert_matrix(pkg("volume_source").compose_matrix(XY, HW, **kw, spacing_xy=T.SPACING, pixel_mm=T.PIXEL))


def _run(dev, logits, nb, z0, invs, ramp, XY, elems, origin, strides, prob=True, entropy=True):
    """logits: a list of numpy arrays; an array listed twice (the same object) is uploaded once and its pointer given twice"""
    K = pkg("kernels")
    ncls = logits[0].shape[-1]
    up = {}
    members = [up.setdefault(id(a), torch.from_numpy(a).to(dev)) for a in logits]
    vol = torch.full((elems,), FILL, dtype=torch.uint8, device=dev)
    p = torch.full((ncls * elems,), SENTINEL, dtype=torch.float32, device=dev) if prob else None
    h = torch.full((elems,), SENTINEL, dtype=torch.float32, device=dev) if entropy else None
    K.paste_tiles(members, nb, z0, invs, ramp, XY, vol, origin, strides, prob=p, entropy=h)
    torch.cuda.synchronize()
    return vol.cpu().numpy(), None if p is None else p.cpu().numpy(), None if h is None else h.cpu().numpy()


def _check(got, logits, nb, z0, invs, ramp, XY, origin, strides, what):
    """the whole of the three allocations: the fill wherever the launch must not write, values inside the bounds everywhere else"""
    vol, prob, ent = got
    X, Y = XY
    (H, W), ncls = logits[0].shape[1:3], logits[0].shape[-1]
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    res = T.tiles(logits, invs, X, Y, ramp, nb)
    edge = T.edge_columns(invs, X, Y, H, W)
    assert edge.mean() <= 0.02, what
    cmp_ = np.broadcast_to((res.covered & ~edge)[None], idx.shape)          # written for certain, compared with the bounds
    bare = np.broadcast_to((~res.covered & ~edge)[None], idx.shape)         # not written for certain
    untouched = np.ones(vol.size, bool)
    untouched[idx.ravel()] = False
    untouched[idx[bare]] = True
    assert cmp_.any() and np.all(vol[untouched] == FILL), "%s: %d label stores outside the box / the frame range / the covered columns" % (
        what, int((vol[untouched] != FILL).sum()))
    dp = T.delta_p_tiles(logits, invs, X, Y, nb)
    lab = vol[idx[cmp_]]
    assert lab.max() < ncls, "%s: a label >= ncls (or an unwritten voxel on a covered column)" % what
    ok = np.take_along_axis(E.admissible(res.prob[cmp_], dp), lab[:, None].astype(np.int64), axis=-1)[:, 0]
    line = "%s: %d of %d labels differ from the float64 argmax, %d outside the bound" % (what, int((lab != res.label[cmp_]).sum()), lab.size, int((~ok).sum()))
    if prob is not None:
        prob = prob.reshape(ncls, vol.size)
        assert np.all(prob[:, untouched] == SENTINEL), "%s: probability stores outside the box / the frame range / the covered columns" % what
        P = prob[:, idx[cmp_]].T.astype(np.float64)
        err, serr = float(np.abs(P - res.prob[cmp_]).max()), float(np.abs(P.sum(-1) - 1.0).max())
        line += "; max|dP| %.3g (bound %.3g, of which the coordinate term %.3g), max|sum P - 1| %.3g (bound %.3g)" % (
            err, dp, T.coord_shift(invs, X, Y), serr, ncls * 2.0 ** -23)
    if ent is not None:
        assert np.all(ent[untouched] == SENTINEL), "%s: entropy stores outside the box / the frame range / the covered columns" % what
        hb = E.entropy_bound(dp, ncls)
        herr = float(np.abs(ent[idx[cmp_]].astype(np.float64) - res.entropy[cmp_]).max())
        line += "; max|dH| %.3g (bound %.3g)" % (herr, hb)
    print(line)
    assert ok.all(), line
    if prob is not None:
        assert err <= dp and serr <= ncls * 2.0 ** -23, line
    if ent is not None:
        assert herr <= hb, line
        if ncls == 1:
            assert np.all(ent[idx[cmp_]] == 0.0)


def _case(name):
    (H, W), (X, Y), B, nb, z0, Z, kind, ncls, ramp, members = T.CASES[name]
    elems, origin, strides = T.layout(kind, X, Y, Z)
    logits = [T.case_logits(name, m) for m in range(len(members))]
    invs = [_inv((X, Y), (H, W), **m) for m in members]
    return logits, nb, z0, invs, ramp, (X, Y), elems, origin, strides


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_tiles_against_the_restatement(dev, name):
    logits, nb, z0, invs, ramp, XY, elems, origin, strides = _case(name)
    got = _run(dev, logits, nb, z0, invs, ramp, XY, elems, origin, strides)
    _check(got, logits, nb, z0, invs, ramp, XY, origin, strides, "%s/M=%d/ncls=%d" % (name, len(logits), logits[0].shape[-1]))


@pytest.mark.parametrize("name", ["quad", "nine"])
def test_null_outputs_and_determinism(dev, name):
    """prob and entropy each null: the outputs that remain do not change, bit for bit; the same call twice is bit-identical"""
    logits, nb, z0, invs, ramp, XY, elems, origin, strides = _case(name)
    both = _run(dev, logits, nb, z0, invs, ramp, XY, elems, origin, strides)
    again = _run(dev, logits, nb, z0, invs, ramp, XY, elems, origin, strides)
    for a, b in zip(both, again):
        assert np.array_equal(a, b)
    for prob, entropy in ((True, False), (False, True), (False, False)):
        got = _run(dev, logits, nb, z0, invs, ramp, XY, elems, origin, strides, prob=prob, entropy=entropy)
        assert (got[1] is None) == (not prob) and (got[2] is None) == (not entropy)
        for a, b in zip(got, both):
            assert a is None or np.array_equal(a, b)


@pytest.mark.parametrize("name", ["pair", "quad", "nine_flip"])
def test_a_member_given_twice_is_that_member_given_once(dev, name):
    """a member listed twice (same tensor, same map): w p + w p and w + w are exact doublings, so all three outputs are bit-identical to
    the launch with that member once — for every member of the case (up to four), each with its own partial coverage"""
    logits, nb, z0, invs, ramp, XY, elems, origin, strides = _case(name)
    for m in range(min(len(logits), 4)):
        one = _run(dev, [logits[m]], nb, z0, [invs[m]], ramp, XY, elems, origin, strides)
        two = _run(dev, [logits[m]] * 2, nb, z0, [invs[m]] * 2, ramp, XY, elems, origin, strides)
        assert len(np.unique(one[0])) > 2 and (one[0] == FILL).any()
        for a, b, what in zip(one, two, ("label", "prob", "entropy")):
            assert np.array_equal(a, b), "member %d: %s differs at %d elements" % (m, what, int((a != b).sum()))


@pytest.mark.parametrize("name", ["quad", "many"])
def test_equal_logits_in_every_member(dev, name):
    """label 0, P = 1 / ncls and entropy 1 within the bounds (delta_r = 0 on constant logits: the rounding term alone), on every covered
    column, whatever the weights"""
    (H, W), (X, Y), B, nb, z0, Z, kind, _, ramp, members = T.CASES[name]
    elems, origin, strides = T.layout(kind, X, Y, Z)
    invs = [_inv((X, Y), (H, W), **m) for m in members]
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    covered = T.member_covers(invs, X, Y, H, W).any(axis=0) & ~T.edge_columns(invs, X, Y, H, W)
    at = idx[np.broadcast_to(covered[None], idx.shape)]
    for ncls in (2, 5, 8):
        flat = np.full((B, H, W, ncls), 0.375, np.float32)
        vol, prob, ent = _run(dev, [flat] * len(members), nb, z0, invs, ramp, (X, Y), elems, origin, strides)
        dp = T.k_tiles(len(members)) * T.U
        assert np.all(vol[at] == 0), (name, ncls, np.unique(vol[at], return_counts=True), prob.reshape(ncls, elems)[:, at[vol[at] != 0][:3]])
        assert np.abs(prob.reshape(ncls, elems)[:, at].astype(np.float64) - 1.0 / ncls).max() <= dp, (name, ncls)
        assert np.abs(ent[at].astype(np.float64) - 1.0).max() <= E.entropy_bound(dp, ncls), (name, ncls)


def test_seam_between_two_tiles(dev):
    """two axis-aligned tiles that overlap by ramp = 4 pixels; A's logits say class 1 everywhere, B's class 2 (a gap of 20).  Across the
    overlap P_1 is the float64 w_A / (w_A + w_B) within the bound, and the label switches exactly where the float64 weights cross; the
    columns at which the two classes are within the bound of each other are left out: at most one per row"""
    (H, W), (X, Y), B, nb, z0, Z, ncls, ramp = (12, 16), (40, 24), 3, 3, 1, 5, 3, 4.0
    elems, origin, strides = T.layout("zup", X, Y, Z)
    invs = [_inv((X, Y), (H, W), translate=(t, 0.0)) for t in (-4.0, 4.0)]
    logits = [np.zeros((B, H, W, ncls), np.float32) for _ in (0, 1)]
    logits[0][..., 1] = 20.0
    logits[1][..., 2] = 20.0
    vol, prob, ent = _run(dev, logits, nb, z0, invs, ramp, (X, Y), elems, origin, strides)
    _check((vol, prob, ent), logits, nb, z0, invs, ramp, (X, Y), origin, strides, "seam")
    res = T.tiles(logits, invs, X, Y, ramp, nb)
    w = res.weights
    both = (w > 0).all(axis=0)
    assert both.any(axis=1).sum() == 8 and res.covered.all()
    dp = T.delta_p_tiles(logits, invs, X, Y, nb)
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    P1 = prob.reshape(ncls, elems)[1][idx].astype(np.float64)                # [nb, X, Y]
    share = w[0] / w.sum(axis=0)
    assert np.abs(res.prob[..., 1] - share[None]).max() < 1e-8              # the softmax of a gap of 20 is 1 - 4e-9
    assert np.abs(P1 - share[None])[:, both].max() <= dp + 1e-8 and len(np.unique(share[both])) >= 6
    near = np.abs(res.prob[0, :, :, 1] - res.prob[0, :, :, 2]) <= 2.0 * dp  # the crossing itself
    assert near.sum(axis=0).max() <= 1
    lab = vol[idx]
    want = np.where(w[0] > w[1], 1, 2).astype(np.uint8)
    assert np.array_equal(lab[:, ~near], np.broadcast_to(want[None], lab.shape)[:, ~near])
    assert set(np.unique(lab[:, both]).tolist()) == {1, 2} and not (lab == 0).any()


def test_one_tile_against_the_ensemble_path(dev):
    """M = 1: the label is pnp_paste_ensemble_fov's wherever the top-2 gap of P exceeds the bound, P is within the bound, and the columns
    written are the same (the interpolation code is shared)"""
    K = pkg("kernels")
    logits, nb, z0, invs, ramp, XY, elems, origin, strides = _case("one")
    ncls = logits[0].shape[-1]
    vol, prob, ent = _run(dev, logits, nb, z0, invs, ramp, XY, elems, origin, strides)
    lg = torch.from_numpy(logits[0]).to(dev)
    v2 = torch.full((elems,), FILL, dtype=torch.uint8, device=dev)
    p2 = torch.full((ncls * elems,), SENTINEL, dtype=torch.float32, device=dev)
    h2 = torch.full((elems,), SENTINEL, dtype=torch.float32, device=dev)
    K.paste_ensemble([lg], nb, z0, invs, XY, v2, origin, strides, prob=p2, entropy=h2, fov=True)
    torch.cuda.synchronize()
    v2, p2 = v2.cpu().numpy(), p2.cpu().numpy()
    assert np.array_equal(vol == FILL, v2 == FILL) and np.array_equal(prob == SENTINEL, p2 == SENTINEL) and 0.3 < (vol != FILL).mean() < 0.9
    dp = T.delta_p_tiles(logits, invs, XY[0], XY[1], nb)
    wr = vol != FILL
    Pa, Pb = prob.reshape(ncls, elems)[:, wr].astype(np.float64), p2.reshape(ncls, elems)[:, wr].astype(np.float64)
    assert np.abs(Pa - Pb).max() <= dp
    top = np.sort(Pb, axis=0)
    clear = top[-1] - top[-2] > 2.0 * dp
    print("one tile: %d of %d voxels with a top-2 gap under the bound, max|dP| %.3g (bound %.3g)" % (int((~clear).sum()), clear.size, np.abs(Pa - Pb).max(), dp))
    assert clear.mean() >= 0.95 and np.array_equal(vol[wr][clear], v2[wr][clear])


def test_refusals_leave_the_outputs_untouched(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lg = torch.zeros((2, 8, 8, 5), device=dev)
    ident = [1, 0, 0, 0, 1, 0]
    vol = torch.zeros(4 * 5 * 6, dtype=torch.uint8, device=dev)
    prob = torch.zeros(5 * 4 * 5 * 6, device=dev)
    ent = torch.zeros(4 * 5 * 6, device=dev)
    args = lambda **kw: dict(dict(logits=[lg, lg], nb=2, z0=0, invs=[ident, ident], ramp=1.0, src_xy=(4, 5), vol=vol, origin=0, strides=(30, 6, 1),
                                  prob=prob, entropy=ent), **kw)
    for bad in (dict(vol=vol.cpu()), dict(logits=[lg, lg.cpu()]), dict(prob=prob.cpu()), dict(entropy=ent.cpu())):
        with pytest.raises(L.PnpError, match="no CPU fallback"):
            K.paste_tiles(**args(**bad))
    for bad, text in ((dict(logits=[], invs=[]), "pnp_paste_tiles: M = 0 members outside \\[1, 64\\]"),
                      (dict(logits=[lg] * 65, invs=[ident] * 65), "pnp_paste_tiles: M = 65 members outside \\[1, 64\\]"),
                      (dict(ramp=0.5), "pnp_paste_tiles: ramp = 0.5 must be finite and at least 1"),
                      (dict(ramp=float("nan")), "pnp_paste_tiles: ramp = nan must be finite and at least 1"),
                      (dict(prob=prob[:-1]), "600 elements"), (dict(entropy=ent.double()), "float32"), (dict(invs=[ident]), "2 members with 1 maps"),
                      (dict(logits=[lg, lg[:1]]), "one shape"), (dict(vol=vol.float()), "uint8"),
                      (dict(z0=5), "pnp_paste_tiles: the box addresses elements outside \\[0, 120\\)"),
                      (dict(strides=(30, 1, 1)), "pnp_paste_tiles: strides 30 1 1 let two voxels")):
        with pytest.raises(L.PnpError, match=text):
            K.paste_tiles(**args(**bad))
    torch.cuda.synchronize()
    assert not vol.any() and not prob.any() and not ent.any()          # untouched after every refusal
    K.paste_tiles(**args())
    torch.cuda.synchronize()
    idx = R.written_index(4, 5, 2, 0, 0, (30, 6, 1)).ravel()
    assert np.all(prob.cpu().numpy().reshape(5, 120)[:, idx] == np.float32(1.0) / np.float32(5.0)) and (prob != 0).sum().item() == 5 * idx.size
