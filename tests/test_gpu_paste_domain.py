"""-m gpu: csrc/paste.hip over the store paths, instantiations, borders and extents that the feature tests leave out.
The cases are tests/volume_store_cases.py's; tests/test_volume_store_host.py shows without a GPU which branch each exists for.

Every launch pre-fills vol with 0xAB and prob / entropy with -7.0 and the WHOLE of every allocation is compared.

  a  the z-fastest store paths, exact: the identity map on a 5 x 7 plane, logits 4.0 at class (b + 3 x + 5 y) mod 8 — integer coordinates
     return the corner's logits bit for bit, so the labels carry no bound; prob and entropy of a launch are, bit for bit, what the
     reference launch (sz = +1, no offset) wrote for the same (b, x, y), and that launch is held to the float64 softmax within
     ensemble_ref.K_ROUND 2^-24 and ensemble_ref.entropy_bound of that.  Both signs of sz, every phase of the 4-byte grid, 1 .. 12
     frames, through the five entry points; then the slicing axis first with sy = +1 and sy = -1.
  b  every template instantiation that no other sweep launches, under the bounds of the files whose cases they are.
  c  the closed field of view, exact: dyadic maps put columns ON -0.5 and on H - 0.5; the written set is the closed-interval rule.
  d  NaN, +-1e30 and inf * 0 coordinates: the plain entry points write the clamped corner (NaN -> pixel 0), the others nothing.
  e  extents 1 .. 4096 on planes down to 1 x 1, under paste_ref's and ensemble_ref's bounds.
"""
import numpy as np
import pytest
import torch

import ensemble_ref as E
import fuse_ref as F
import paste_ref as R
import tiles_ref as T
import test_gpu_ensemble as GE
import test_gpu_fuse as GF
import test_gpu_paste as GP
import test_gpu_tiles as GT
import volume_store_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

FILL, SENTINEL = 0xAB, -7.0
IDENT = [1, 0, 0, 0, 1, 0]
ENTRIES = ("labels", "labels_fov", "ensemble", "ensemble_fov", "tiles")


def _launch(dev, entry, members, nb, z0, invs, XY, elems, origin, strides, ramp=1.0):
    """one launch of an entry point on fresh, pre-filled allocations -> numpy (vol, prob [ncls, elems] or None, entropy or None)"""
    K = pkg("kernels")
    ncls = int(members[0].shape[-1])
    vol = torch.full((elems,), FILL, dtype=torch.uint8, device=dev)
    assert vol.data_ptr() % 16 == 0
    if entry.startswith("labels"):
        assert len(members) == 1
        K.paste_labels(members[0], nb, z0, invs[0], XY, vol, origin, strides, fov=entry.endswith("fov"))
        return vol.cpu().numpy(), None, None
    p = torch.full((ncls * elems,), SENTINEL, dtype=torch.float32, device=dev)
    h = torch.full((elems,), SENTINEL, dtype=torch.float32, device=dev)
    if entry == "tiles":
        K.paste_tiles(members, nb, z0, invs, ramp, XY, vol, origin, strides, prob=p, entropy=h)
    else:
        K.paste_ensemble(members, nb, z0, invs, XY, vol, origin, strides, prob=p, entropy=h, fov=entry.endswith("fov"))
    return vol.cpu().numpy(), p.cpu().numpy().reshape(ncls, elems), h.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- a. the store paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_store_paths_of_a_z_fastest_column(dev, entry):
    X, Y = C.SWEEP_XY
    ncls = C.SWEEP_NCLS
    lg = C.sweep_logits(C.SWEEP_B_MAX)
    lab = C.sweep_label(*np.meshgrid(np.arange(C.SWEEP_B_MAX), np.arange(X), np.arange(Y), indexing="ij")).astype(np.uint8)
    on_dev = {}
    member = lambda B: on_dev.setdefault(B, torch.from_numpy(np.ascontiguousarray(lg[:B])).to(dev))
    soft = not entry.startswith("labels")
    if soft:
        ref = C.Setting(1, 0, 13, C.SWEEP_B_MAX, 0, C.SWEEP_B_MAX)
        elems, origin, strides = C.sweep_layout(ref)
        vol, p, h = _launch(dev, entry, [member(ref.B)], ref.nb, ref.z0, [IDENT], (X, Y), elems, origin, strides)
        idx = R.written_index(X, Y, ref.nb, ref.z0, origin, strides)
        P_ref, H_ref = p[:, idx], h[idx]                                                     # [ncls, B, X, Y], [B, X, Y]
        assert np.array_equal(vol[idx], lab)
        want = E.softmax(lg.astype(np.float64))
        dp = E.K_ROUND * E.U
        e1 = float(np.abs(np.moveaxis(P_ref, 0, -1) - want).max())
        e2 = float(np.abs(H_ref - E.entropy(want)).max())
        print("%s, the reference launch: max|dP| / bound %.3f, max|dH| / bound %.3f" % (entry, e1 / dp, e2 / E.entropy_bound(dp, ncls)))
        assert e1 <= dp and e2 <= E.entropy_bound(dp, ncls)
    launches = [(s.B, s.nb, s.z0, C.sweep_layout(s), s) for s in C.SWEEP]
    for sy, nb, z0 in C.AXIS_FIRST:                                                          # the byte-per-frame path: one label per lane and frame
        launches.append((nb, nb, z0, C.axis_first_layout(sy, X, Y, z0 + nb), "slicing axis first, sy = %d" % sy))
    for B, nb, z0, (elems, origin, strides), what in launches:
        vol, p, h = _launch(dev, entry, [member(B)], nb, z0, [IDENT], (X, Y), elems, origin, strides)
        idx = R.written_index(X, Y, nb, z0, origin, strides)
        want = np.full(elems, FILL, np.uint8)
        want[idx] = lab[:nb]
        assert np.array_equal(vol, want), (entry, what, np.flatnonzero(vol != want)[:8])
        if soft:
            wp, wh = np.full((ncls, elems), SENTINEL, np.float32), np.full(elems, SENTINEL, np.float32)
            wp[:, idx] = P_ref[:, :nb]
            wh[idx] = H_ref[:nb]
            assert _same_bits(p, wp) and _same_bits(h, wh), (entry, what)


# ---- b. every instantiation --------------------------------------------------------------------------------------------------------------
def _ensemble_case(M, ncls):
    (H, W), (X, Y), B, nb, z0, Z, kind = R.CASES[C.ENSEMBLE_CASE]
    elems, origin, strides = R.layout(kind, X, Y, Z)
    logits = [E.smooth_logits(C.ENSEMBLE_CASE, ncls, m, C.ENSEMBLE_SEED) for m in range(M)]
    invs = [GE._inv((X, Y), (H, W), **E.MAPS[m]) for m in range(M)]
    return logits, nb, z0, invs, (X, Y), (H, W), elems, origin, strides


@pytest.mark.parametrize("M,ncls", C.ENSEMBLE_INSTANCES, ids=["M%d-ncls%d" % c for c in C.ENSEMBLE_INSTANCES])
def test_ensemble_instances(dev, M, ncls):
    logits, nb, z0, invs, XY, _, elems, origin, strides = _ensemble_case(M, ncls)
    got = GE._run(dev, logits, nb, z0, invs, XY, elems, origin, strides)
    GE._check(got, logits, nb, z0, invs, XY, origin, strides, "%s/M=%d/ncls=%d" % (C.ENSEMBLE_CASE, M, ncls))


@pytest.mark.parametrize("M,ncls", C.ENSEMBLE_FOV_INSTANCES, ids=["M%d-ncls%d" % c for c in C.ENSEMBLE_FOV_INSTANCES])
def test_ensemble_fov_instances(dev, M, ncls):
    """the columns inside every member's field of view carry pnp_paste_ensemble's bits (held to §15's bounds), the others nothing; the
    columns whose coverage float32 may decide otherwise (tiles_ref.edge_columns) may be either"""
    logits, nb, z0, invs, (X, Y), (H, W), elems, origin, strides = _ensemble_case(M, ncls)
    members = [torch.from_numpy(a).to(dev) for a in logits]
    full = _launch(dev, "ensemble", members, nb, z0, invs, (X, Y), elems, origin, strides)
    GE._check((full[0], full[1].reshape(-1), full[2]), logits, nb, z0, invs, (X, Y), origin, strides, "%s/M=%d/ncls=%d (fov's values)" % (C.ENSEMBLE_CASE, M, ncls))
    vol, p, h = _launch(dev, "ensemble_fov", members, nb, z0, invs, (X, Y), elems, origin, strides)
    cov, edge = T.member_covers(invs, X, Y, H, W).all(axis=0), T.edge_columns(invs, X, Y, H, W)
    assert 0.2 < cov.mean() < 1.0 and edge.mean() <= 0.02
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    sure_in, sure_out = np.zeros(elems, bool), np.ones(elems, bool)
    sure_in[idx[:, cov & ~edge].ravel()] = True
    sure_out[idx[:, cov | edge].ravel()] = False
    written = vol != FILL
    assert written[sure_in].all() and not written[sure_out].any()
    assert np.array_equal(written, h != SENTINEL) and np.array_equal(written, (p != SENTINEL).all(axis=0)) and np.array_equal(written, (p != SENTINEL).any(axis=0))
    assert _same_bits(vol[written], full[0][written]) and _same_bits(p[:, written], full[1][:, written]) and _same_bits(h[written], full[2][written])


@pytest.mark.parametrize("ncls", C.TILES_NCLS)
def test_tiles_instances(dev, ncls):
    (H, W), (X, Y), B, nb, z0, Z, kind, _, ramp, members = T.CASES[C.TILES_CASE]
    elems, origin, strides = T.layout(kind, X, Y, Z)
    logits = [C.pair_logits(ncls, m) for m in range(len(members))]
    invs = [GT._inv((X, Y), (H, W), **m) for m in members]
    got = GT._run(dev, logits, nb, z0, invs, ramp, (X, Y), elems, origin, strides)
    GT._check(got, logits, nb, z0, invs, ramp, (X, Y), origin, strides, "%s/M=%d/ncls=%d" % (C.TILES_CASE, len(members), ncls))


@pytest.mark.parametrize("M,ncls,n", C.FUSE_INSTANCES)
def test_fuse_instances(dev, M, ncls, n):
    probs, w = F.make_case(M, ncls, n, C.FUSE_SEED)
    GF._check(GF._run(dev, probs, w), F.fuse(probs, w), M, ncls, "%d elements, M = %d, ncls = %d, weights" % (n, M, ncls))
    GF._check(GF._run(dev, probs, None), F.fuse(probs, None), M, ncls, "%d elements, M = %d, ncls = %d, no weights" % (n, M, ncls))


# ---- c. the closed field of view ---------------------------------------------------------------------------------------------------------
def _fov_setup(dev):
    (H, W), (X, Y) = C.FOV_HW, C.FOV_XY
    elems, origin, strides = R.layout("c", X, Y, C.FOV_Z)
    logits = [C.fov_logits(m) for m in range(2)]
    members = [torch.from_numpy(a).to(dev) for a in logits]
    idx = R.written_index(X, Y, C.FOV_NB, C.FOV_Z0, origin, strides)
    cover = [C.closed_cover(inv, X, Y, H, W) for inv in (C.FOV_MAP_A, C.FOV_MAP_B)]
    return logits, members, idx, cover, (elems, origin, strides)


def _written_exactly(arrays, idx, cols, elems):
    """every output is written on the columns `cols` of the box and nowhere else"""
    want = np.zeros(elems, bool)
    want[idx[:, cols].ravel()] = True
    vol, p, h = arrays
    assert np.array_equal(vol != FILL, want), "labels: written %d, the closed rule %d" % (int((vol != FILL).sum()), int(want.sum()))
    if p is not None:
        assert np.array_equal((p != SENTINEL).all(axis=0), want) and np.array_equal((p != SENTINEL).any(axis=0), want)
        assert np.array_equal(h != SENTINEL, want)
    return want


def test_closed_field_of_view_labels(dev):
    logits, members, idx, cover, (elems, origin, strides) = _fov_setup(dev)
    X, Y = C.FOV_XY
    full = GP._run(dev, logits[0], C.FOV_NB, C.FOV_Z0, C.FOV_MAP_A, (X, Y), elems, origin, strides)
    GP._check(full, logits[0], C.FOV_NB, C.FOV_Z0, C.FOV_MAP_A, (X, Y), origin, strides, "closed fov, map A")
    got = _launch(dev, "labels_fov", members[:1], C.FOV_NB, C.FOV_Z0, [C.FOV_MAP_A], (X, Y), elems, origin, strides)
    want = _written_exactly(got, idx, cover[0], elems)
    assert cover[0][1, 1] and cover[0][9, 9] and not cover[0][0, 5] and not cover[0][10, 5]
    assert np.array_equal(got[0][want], full[want])


def test_closed_field_of_view_ensemble_is_the_intersection(dev):
    logits, members, idx, cover, (elems, origin, strides) = _fov_setup(dev)
    X, Y = C.FOV_XY
    invs = [C.FOV_MAP_A, C.FOV_MAP_B]
    full = _launch(dev, "ensemble", members, C.FOV_NB, C.FOV_Z0, invs, (X, Y), elems, origin, strides)
    GE._check((full[0], full[1].reshape(-1), full[2]), logits, C.FOV_NB, C.FOV_Z0, invs, (X, Y), origin, strides, "closed fov, maps A and B")
    got = _launch(dev, "ensemble_fov", members, C.FOV_NB, C.FOV_Z0, invs, (X, Y), elems, origin, strides)
    want = _written_exactly(got, idx, cover[0] & cover[1], elems)
    assert int((cover[0] & cover[1]).sum()) == 64
    assert _same_bits(got[0][want], full[0][want]) and _same_bits(got[1][:, want], full[1][:, want]) and _same_bits(got[2][want], full[2][want])


def test_closed_field_of_view_tiles_is_the_union(dev):
    """no column is exempt: the coordinates are exact (tiles_ref.coords_exact), so the bound is delta_r / 2 + K(2) 2^-24 alone"""
    logits, members, idx, cover, (elems, origin, strides) = _fov_setup(dev)
    (H, W), (X, Y), nb, ncls = C.FOV_HW, C.FOV_XY, C.FOV_NB, C.FOV_NCLS
    invs = [C.FOV_MAP_A, C.FOV_MAP_B]
    vol, p, h = _launch(dev, "tiles", members, nb, C.FOV_Z0, invs, (X, Y), elems, origin, strides, ramp=C.FOV_RAMP)
    union = cover[0] | cover[1]
    _written_exactly((vol, p, h), idx, union, elems)
    assert int(union.sum()) == 98 and T.coord_shift(invs, X, Y) == 0.0
    res = T.tiles(logits, invs, X, Y, C.FOV_RAMP, nb)
    assert np.array_equal(res.covered, union)
    dp = T.delta_p_tiles(logits, invs, X, Y, nb)
    at = idx[:, union]                                                                       # [nb, columns]
    lab = vol[at]
    ok = np.take_along_axis(E.admissible(res.prob[:, union], dp), lab[..., None].astype(np.int64), axis=-1)[..., 0]
    P = np.moveaxis(p[:, at], 0, -1).astype(np.float64)
    err, serr = float(np.abs(P - res.prob[:, union]).max()), float(np.abs(P.sum(-1) - 1.0).max())
    herr, hb = float(np.abs(h[at] - res.entropy[:, union]).max()), E.entropy_bound(dp, ncls)
    print("closed fov, tiles A | B: %d labels differ from the float64 argmax, max|dP| / bound %.3f, max|dH| / bound %.3f" % (
        int((lab != res.label[:, union]).sum()), err / dp, herr / hb))
    assert lab.max() < ncls and ok.all() and err <= dp and serr <= ncls * 2.0 ** -23 and herr <= hb


# ---- d. maps that leave the plane --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sub_box", "zfirst_flipped"])
@pytest.mark.parametrize("name", list(C.WILD_MAPS))
def test_maps_that_leave_the_plane(dev, name, kind):
    """csrc/paste.hip clamps with fminf(fmaxf(p, 0), n - 1) before floorf and the integer conversion, in paste_labels_kernel and in
    softmax_at alike, and in_fov's comparisons are false for NaN: a coordinate that is NaN takes pixel 0, one beyond the plane its border"""
    (H, W), (X, Y), nb, z0, ncls = C.WILD_HW, C.WILD_XY, C.WILD_NB, C.WILD_Z0, C.WILD_NCLS
    inv = C.WILD_MAPS[name]
    elems, origin, strides = R.layout(kind, X, Y, C.WILD_Z)
    lg = C.wild_logits()
    member = torch.from_numpy(lg).to(dev)
    i, j = C.wild_pixel(inv, X, Y, H, W)
    idx = R.written_index(X, Y, nb, z0, origin, strides)
    want = np.full(elems, FILL, np.uint8)
    want[idx] = np.argmax(lg, -1)[:, i, j].astype(np.uint8)
    ref = E.softmax(lg.astype(np.float64))[:, i, j]                                          # [nb, X, Y, ncls]
    dp = E.K_ROUND * E.U
    for entry, members, invs in (("labels", [member], [inv]), ("ensemble", [member], [inv]), ("ensemble", [member] * 2, [inv, C.WILD_MAPS["nan"]])):
        vol, p, h = _launch(dev, entry, members, nb, z0, invs, (X, Y), elems, origin, strides)
        if len(invs) == 1:
            assert np.array_equal(vol, want), (entry, name)
        if p is not None and len(invs) == 1:
            untouched = np.ones(elems, bool)
            untouched[idx.ravel()] = False
            assert np.all(p[:, untouched] == SENTINEL) and np.all(h[untouched] == SENTINEL)
            assert np.abs(np.moveaxis(p[:, idx], 0, -1) - ref).max() <= dp and np.abs(h[idx] - E.entropy(ref)).max() <= E.entropy_bound(dp, ncls)
        if len(invs) == 2:                                                                   # a second member on pixel (0, 0): finite, in the box
            assert np.array_equal(vol != FILL, want != FILL) and vol[idx].max() < ncls and np.isfinite(p).all() and np.isfinite(h).all()
    for entry, members, invs in (("labels_fov", [member], [inv]), ("ensemble_fov", [member], [inv]), ("tiles", [member], [inv]),
                                 ("tiles", [member] * 2, [inv, C.WILD_MAPS["nan"]])):
        vol, p, h = _launch(dev, entry, members, nb, z0, invs, (X, Y), elems, origin, strides)
        assert np.all(vol == FILL) and (p is None or (np.all(p == SENTINEL) and np.all(h == SENTINEL))), (entry, name)


# ---- e. extents --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", C.EXTENT_HW, ids=["plane%dx%d" % hw for hw in C.EXTENT_HW])
def test_extents(dev, HW):
    nb, z0 = C.EXTENT_NB, C.EXTENT_Z0
    for XY in C.EXTENT_XY:
        logits, invs = [C.extent_logits(XY, HW, m) for m in range(2)], C.extent_maps(XY, HW)
        for kind in C.EXTENT_LAYOUTS:
            elems, origin, strides = R.layout(kind, XY[0], XY[1], C.EXTENT_Z)
            what = "%d x %d columns, plane %d x %d, %s" % (XY + HW + (kind,))
            for m in range(2):
                got = GP._run(dev, logits[m], nb, z0, invs[m], XY, elems, origin, strides)
                GP._check(got, logits[m], nb, z0, invs[m], XY, origin, strides, "%s, map %d" % (what, m))
            got = GE._run(dev, logits, nb, z0, invs, XY, elems, origin, strides)
            GE._check(got, logits, nb, z0, invs, XY, origin, strides, what)
