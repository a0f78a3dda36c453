"""not gpu: the host side of tiled inference — volume_predict.tile_plan / tile_ramp / coverage(mode=), the restatement of
tests/tiles_ref.py pinned to scipy.ndimage.map_coordinates(order=1, mode="nearest") + an explicit weighted mean, the window's shape,
the host refusals of pnp_paste_tiles by their text (decided before any HIP call: the buffers are small host buffers, never read), the
CLI's --tiles / --tile-overlap, and that the bounds of tests/test_gpu_tiles.py are not vacuous on its cases."""
import ctypes
import math

import numpy as np
import pytest

import ensemble_ref as E
import paste_ref as R
import tiles_ref as T
from conftest import pkg


def case_maps(name):
    """the inverse maps (float32, what the kernel gets) of a tiles_ref case"""
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (H, W), (X, Y) = T.CASES[name][:2]
    return [vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), **m, spacing_xy=T.SPACING, pixel_mm=T.PIXEL)) for m in T.CASES[name][9]]


# ---- tile_plan ---------------------------------------------------------------------------------------------------------------------------
GRID = [(L, F, o) for L in (100.0, 256.0, 257.0, 300.5, 400.0, 512.0, 1000.0) for F in (64.0, 200.0, 256.0) for o in (0.0, 0.1, 0.25, 0.5)]


def test_plan_counts_follow_the_formula():
    vp = pkg("volume_predict")
    for L, F, o in GRID:
        n = 1 if L <= F else int(math.ceil((L - o * F) / (F - o * F)))
        offs, counts = vp.tile_plan((L, 90.0), (F, 128.0), "auto", o)
        assert counts == (n, 1) and len(offs) == n, (L, F, o, counts)
        assert vp.tile_plan((90.0, L), (128.0, F), "auto", o)[1] == (1, n)
        if n > 1:                                             # n planes with overlaps of o F reach the box, n - 1 would not
            assert n * F - (n - 1) * o * F >= L > (n - 1) * F - (n - 2) * o * F, (L, F, o, n)


def test_plan_is_flush_evenly_spaced_and_tile_major():
    vp = pkg("volume_predict")
    for L, F, o in GRID:
        offs, (ni, nj) = vp.tile_plan((L, 1.5 * L), (F, F), "auto", o)
        ti = sorted({t[0] for t in offs})
        tj = sorted({t[1] for t in offs})
        assert offs == [(a, b) for a in ti for b in tj] and (len(ti), len(tj)) == (ni, nj)
        for t, ext, n in ((ti, L, ni), (tj, 1.5 * L, nj)):
            if n == 1:
                assert t == [0.0]                             # a single plane is centred
                continue
            assert abs((t[0] - F / 2) - (-ext / 2)) < 1e-9 and abs((t[-1] + F / 2) - ext / 2) < 1e-9       # flush with the box's edges
            assert np.allclose(np.diff(t), (ext - F) / (n - 1), rtol=0, atol=1e-9)
            assert F - (ext - F) / (n - 1) >= o * F - 1e-9    # the achieved overlap is at least the one asked for
    offs, counts = vp.tile_plan((300.0, 100.0), (128.0, 128.0), (4, 2), 0.25)
    assert counts == (4, 2) and len(offs) == 8 and offs[0] == (-86.0, 14.0) and offs[-1] == (86.0, -14.0)


def test_plan_errors():
    vp = pkg("volume_predict")
    for bad in (-0.01, 0.51, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            vp.tile_plan((300.0, 300.0), (128.0, 128.0), "auto", bad)
    with pytest.raises(ValueError, match="cannot cover"):
        vp.tile_plan((300.0, 100.0), (128.0, 128.0), (2, 1))
    for bad in ("grid", (2,), (0, 1), (1.5, 2), (True, 1), 3):
        with pytest.raises(ValueError, match="tiles"):
            vp.tile_plan((300.0, 100.0), (128.0, 128.0), bad)
    with pytest.raises(ValueError, match="positive"):
        vp.tile_plan((300.0, 0.0), (128.0, 128.0))
    # segment_volume decides these before any device work (device="cpu" would be refused later)
    img = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(ValueError, match="tiles needs sample_mm"):
        vp.segment_volume(None, img, tiles="auto", device="cpu")
    with pytest.raises(ValueError, match="tile overlap"):
        vp.segment_volume(None, img, tiles="auto", tile_overlap=0.7, sample_mm=1.0, spacing=(1, 1, 1), device="cpu")
    with pytest.raises(ValueError, match="at most 64"):
        vp.segment_volume([None] * 13, img, tiles="auto", tta="default", sample_mm=1.0, spacing=(1, 1, 1), device="cpu")
    with pytest.raises(ValueError, match="at most 8"):        # without tiles the ensemble's limit stands
        vp.segment_volume([None] * 2, img, tta="default", sample_mm=1.0, spacing=(1, 1, 1), device="cpu")


def test_ramp_is_the_smallest_achieved_overlap_in_pixels():
    vp = pkg("volume_predict")
    assert vp.tile_ramp((100.0, 90.0), (128.0, 128.0), (1, 1), (1.0, 1.0)) == 1.0
    # 300 mm by 3 planes of 128 mm: neighbours share 128 - 86 = 42 mm = 42 px of 1 mm, 52.5 px of 0.8 mm
    assert vp.tile_ramp((300.0, 90.0), (128.0, 128.0), (3, 1), (1.0, 1.0)) == pytest.approx(42.0)
    assert vp.tile_ramp((300.0, 200.0), (128.0, 128.0), (3, 2), (0.8, 1.0)) == pytest.approx(52.5)
    assert vp.tile_ramp((300.0, 200.0), (128.0, 128.0), (3, 2), (1.0, 0.5)) == pytest.approx(42.0)
    assert vp.tile_ramp((256.0, 90.0), (128.0, 128.0), (2, 1), (1.0, 1.0)) == 1.0           # planes that only abut


PLANNED = [((41, 37), (0.5, 0.5), (16, 16), 1.0, "auto", 0.25), ((40, 36), (0.5, 0.5), (16, 16), 1.0, (2, 2), 0.25),
           ((37, 29), (0.7, 1.3), (16, 12), 1.0, "auto", 0.1), ((64, 23), (0.35, 0.8), (12, 20), 0.8, "auto", 0.5),
           ((50, 50), (1.0, 1.0), (16, 16), 1.0, "auto", 0.0), ((33, 90), (1.0, 0.5), (20, 16), 1.25, (2, 4), 0.3)]


@pytest.mark.parametrize("XY,sp,HW,px,tiles,overlap", PLANNED)
def test_planned_tiles_cover_the_whole_box(XY, sp, HW, px, tiles, overlap):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (X, Y), (H, W) = XY, HW
    offs, counts = vp.tile_plan((X * sp[0], Y * sp[1]), (H * px, W * px), tiles, overlap)
    invs = [vp.invert_matrix(vs.compose_matrix(XY, HW, translate=t, spacing_xy=sp, pixel_mm=(px, px))) for t in offs]
    assert vp.coverage(invs, X, Y, H, W, mode="any") == 1.0
    assert T.member_covers(invs, X, Y, H, W).any(axis=0).all()
    if len(offs) > 1:
        assert vp.coverage(invs, X, Y, H, W) < 1.0 and vp.coverage(invs, X, Y, H, W, mode="all") == vp.coverage(invs, X, Y, H, W)
    # against a brute-force loop
    cov = T.member_covers(invs, X, Y, H, W)
    assert vp.coverage(invs, X, Y, H, W, mode="all") == cov.all(axis=0).mean() and vp.coverage(invs[:1], X, Y, H, W, mode="any") == cov[0].mean()
    with pytest.raises(ValueError, match="mode"):
        vp.coverage(invs, X, Y, H, W, mode="some")


def test_one_tile_is_the_plane_of_today():
    """a box inside the field of view: the plan is one centred tile, and its map has the six float32 entries segment_volume uses untiled"""
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    for XY, sp, HW, px in (((23, 19), (0.5, 0.7), (16, 16), 1.0), ((9, 11), (2.0, 1.5), (24, 24), 1.0)):
        offs, counts = vp.tile_plan((XY[0] * sp[0], XY[1] * sp[1]), (HW[0] * px, HW[1] * px))
        assert counts == (1, 1) and offs == [(0.0, 0.0)]
        geom = {"spacing_xy": sp, "pixel_mm": (px, px)}
        for e in ({}, {"rotate": 7.5, "translate": (1.5, -2.0)}):
            t = e.get("translate", (0.0, 0.0))
            tiled = vs.compose_matrix(XY, HW, **dict(e, translate=(t[0] + offs[0][0], t[1] + offs[0][1])), **geom)
            assert tiled.dtype == np.float32 and np.array_equal(tiled, vs.compose_matrix(XY, HW, **e, **geom))


# ---- the window --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ramp", [(12, 1.0), (16, 4.0), (20, 6.5), (256, 64.0)])
def test_window_shape(n, ramp):
    p = np.linspace(-0.5, n - 0.5, 4 * n + 1)
    g = T.window(p, n, ramp)
    assert np.allclose(g, g[::-1], rtol=0, atol=1e-15)                                    # symmetric about the plane's centre
    assert g[0] == g[-1] == 0.5 / ramp and g.min() == 0.5 / ramp and g.max() == 1.0
    assert np.all(g[(p + 0.5 >= ramp) & (n - 0.5 - p >= ramp)] == 1.0)                    # 1 from ramp pixels inward
    assert np.all(g[(p + 0.5 < ramp) & (p + 0.5 > 0.5)] < 1.0) and np.all(np.diff(g[p <= (n - 1) / 2.0]) >= 0)
    assert np.all(T.window(np.array([-0.5, -0.25, 0.0]), n, ramp) == 0.5 / ramp)          # the first half pixel is flat: d below 0.5


def test_weights_sum_to_a_constant_across_a_seam():
    """two axis-aligned tiles that overlap by exactly `ramp` pixels: d_A + d_B = ramp, so w_A + w_B = 1 times the other axis' factor wherever both d >= 0.5"""
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (H, W), (X, Y), ramp = (12, 16), (40, 24), 4.0
    invs = [vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), translate=(t, 0.0), spacing_xy=(0.5, 0.5), pixel_mm=(1.0, 1.0))) for t in (-4.0, 4.0)]
    w = T.weights(invs, X, Y, H, W, ramp)
    both = (w > 0).all(axis=0)
    pi_a = R.coords(invs[0], X, Y)[0]
    d_a, d_b = (H - 0.5) - pi_a, R.coords(invs[1], X, Y)[0] + 0.5
    assert both.any(axis=1).sum() == 8 and np.allclose((d_a + d_b)[both], ramp, rtol=0, atol=1e-12)
    inner = both & (d_a >= 0.5) & (d_b >= 0.5)
    g_j = T.window(R.coords(invs[0], X, Y)[1], W, ramp)      # the other axis' factor is the same for both tiles: constant along the seam's normal
    assert inner.any(axis=1).sum() >= 6 and np.allclose(w.sum(axis=0)[inner], g_j[inner], rtol=0, atol=1e-12) and (g_j[inner] == 1.0).any()
    assert np.all(np.diff(w[0][:, 0][both[:, 0]]) < 0) and np.all(np.diff(w[1][:, 0][both[:, 0]]) > 0)      # A fades out as B fades in


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quad", "nine_flip"])
def test_restatement_is_scipy_nearest_plus_a_weighted_mean(name):
    nd, sp = pytest.importorskip("scipy.ndimage"), pytest.importorskip("scipy.special")
    (H, W), (X, Y), B, nb = T.CASES[name][:4]
    ncls, ramp, members = T.CASES[name][7], T.CASES[name][8], T.CASES[name][9]
    invs = case_maps(name)
    logits = [T.case_logits(name, m) for m in range(len(members))]
    res = T.tiles(logits, invs, X, Y, ramp, nb)
    acc, wsum = np.zeros((nb, X, Y, ncls)), np.zeros((X, Y))
    for lg, inv in zip(logits, invs):
        pi, pj = R.coords(inv, X, Y)
        r = np.stack([np.stack([nd.map_coordinates(lg[b, :, :, c].astype(np.float64), [pi, pj], order=1, mode="nearest") for c in range(ncls)], -1)
                      for b in range(nb)])
        w = np.zeros((X, Y))
        for x in range(X):                                   # the rule and the window written out per column
            for y in range(Y):
                if -0.5 <= pi[x, y] <= H - 0.5 and -0.5 <= pj[x, y] <= W - 0.5:
                    di, dj = min(pi[x, y] + 0.5, H - 0.5 - pi[x, y]), min(pj[x, y] + 0.5, W - 0.5 - pj[x, y])
                    w[x, y] = min(1.0, max(di, 0.5) / ramp) * min(1.0, max(dj, 0.5) / ramp)
        acc += w[None, :, :, None] * sp.softmax(r, axis=-1)
        wsum += w
    cov = wsum > 0
    assert np.array_equal(cov, res.covered) and 0 < cov.mean() and len(np.unique((res.weights > 0).sum(0))) >= 3
    P = acc[:, cov] / wsum[cov][None, :, None]
    np.testing.assert_allclose(res.prob[:, cov], P, rtol=0, atol=1e-12)
    assert np.array_equal(res.label[:, cov], np.argmax(P, -1))
    np.testing.assert_allclose(res.entropy[:, cov], -(P * np.log(P)).sum(-1) / np.log(ncls), rtol=0, atol=1e-12)
    np.testing.assert_allclose(P.sum(-1), 1.0, rtol=0, atol=1e-12)


def test_restatement_paste_and_bound():
    name = "quad"
    (H, W), (X, Y), B, nb, z0, Z, kind, ncls, ramp, members = T.CASES[name]
    invs = case_maps(name)
    logits = [T.case_logits(name, m) for m in range(len(members))]
    res = T.tiles(logits, invs, X, Y, ramp, nb)
    elems, origin, strides = T.layout(kind, X, Y, Z)
    vol, prob, ent = np.full(elems, 0xAB, np.uint8), np.full(ncls * elems, -7.0, np.float32), np.full(elems, -7.0, np.float32)
    idx, wr = T.paste(vol, prob, ent, res, z0, origin, strides)
    n = nb * int(res.covered.sum())
    assert 0 < n < nb * X * Y and (vol != 0xAB).sum() == n and (ent != -7.0).sum() == n and (prob != -7.0).sum() == ncls * n
    assert np.all(vol[idx[~wr]] == 0xAB) and np.allclose(prob.reshape(ncls, elems)[:, idx[wr]].sum(0), 1.0, atol=1e-6)
    assert [T.k_tiles(M) for M in (1, 2, 64)] == [E.K_ROUND, 22, 146]
    dp = T.delta_p_tiles(logits, invs, X, Y, nb)
    assert all(T.coords_exact(i, X, Y) for i in invs) and T.coord_shift(invs, X, Y) == 0.0          # axis-aligned planes on a half-voxel grid
    assert dp == 0.5 * E.delta_r(logits, invs, X, Y, nb) + 26 * 2.0 ** -24
    rot = case_maps("nine")
    assert not T.coords_exact(rot[1], 40, 34) and T.coord_shift(rot, 40, 34) == 2 * max(R.coord_eps(i, 40, 34) for i in rot if not T.coords_exact(i, 40, 34))


# ---- the bounds of the GPU sweep are not vacuous -----------------------------------------------------------------------------------------
def test_sweep_covers_what_it_should():
    """member and class counts, the three layouts, columns covered by 0, 1, 2 and 4 members, more than 8 in the M = 64 cases, a short batch"""
    Ms, ns, kinds, counts = set(), set(), set(), set()
    for name, ((H, W), (X, Y), B, nb, z0, Z, kind, ncls, ramp, members) in T.CASES.items():
        assert 12 <= H <= 20 and 12 <= W <= 16 and X <= 40 and Y <= 40 and nb <= 5 and nb <= B and z0 + nb <= Z and ramp >= 1
        Ms.add(len(members)); ns.add(ncls); kinds.add(kind)
        n = T.member_covers(case_maps(name), X, Y, H, W).sum(axis=0)
        counts |= set(np.unique(n).tolist())
        if len(members) == 64:
            assert n.max() > 8, (name, n.max())
    assert Ms == {1, 2, 4, 9, 64} and ns == {1, 2, 5, 8} and kinds == {"zup", "zdown", "zfirst"} and {0, 1, 2, 4} <= counts
    assert any(c[3] < c[2] for c in T.CASES.values()) and any(c[4] % 4 for c in T.CASES.values())


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_bounds_are_not_vacuous_on_the_sweep(name):
    """on the reference alone: the columns left out for their coverage are at most 2 % of the box, and at most 5 % of the compared voxels
    have more than one class within 2 delta_p_tiles of the largest probability"""
    (H, W), (X, Y), B, nb = T.CASES[name][:4]
    ncls, ramp, members = T.CASES[name][7], T.CASES[name][8], T.CASES[name][9]
    invs = case_maps(name)
    edge = T.edge_columns(invs, X, Y, H, W)
    assert edge.mean() <= 0.02, (name, edge.mean())
    logits = [T.case_logits(name, m) for m in range(len(members))]
    res = T.tiles(logits, invs, X, Y, ramp, nb)
    dp = T.delta_p_tiles(logits, invs, X, Y, nb)
    assert T.k_tiles(len(members)) * T.U < dp < 2e-4, (name, dp)
    cmp_ = res.covered & ~edge
    assert cmp_.sum() >= 0.4 * X * Y, (name, cmp_.mean())
    multi = (E.admissible(res.prob, dp).sum(-1) > 1)[:, cmp_]
    print("%s: %d edge columns of %d, %d of %d compared voxels with more than one admissible class, delta_p %.3g, coordinate term %.3g"
          % (name, int(edge.sum()), X * Y, int(multi.sum()), multi.size, dp, T.coord_shift(invs, X, Y)))
    assert (multi.mean() if ncls > 1 else 0.0) <= 0.05, (name, multi.mean())


# ---- argument refusals of pnp_paste_tiles --------------------------------------------------------------------------------------------------
def test_refusals_before_any_hip_call(built):
    lib = built._lib.load()
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    members = (ctypes.c_void_p * 65)(*([ptr.value] * 65))
    maps = (ctypes.c_float * (6 * 65))(*([1, 0, 0, 0, 1, 0] * 65))

    def call(msg, M=2, logits=members, inv=maps, ramp=2.0, ncls=5, z0=1, s=(30, 6, 1), elems=120, vol=ptr):
        rc = lib.pnp_paste_tiles(M, logits, inv, ramp, 2, 8, 8, ncls, 2, z0, 4, 5, vol, elems, 0, s[0], s[1], s[2], None, None, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())
    call(b"pnp_paste_tiles: M = 0 members outside [1, 64]", M=0)
    call(b"pnp_paste_tiles: M = 65 members outside [1, 64]", M=65)
    call(b"pnp_paste_tiles: null pointer", vol=None)
    call(b"pnp_paste_tiles: null inv", inv=None)
    call(b"pnp_paste_tiles: member 1 of 2 is a null pointer", logits=(ctypes.c_void_p * 2)(ptr.value, None))
    call(b"pnp_paste_tiles: ramp = 0.5 must be finite and at least 1", ramp=0.5)
    call(b"pnp_paste_tiles: ramp = nan must be finite", ramp=float("nan"))
    call(b"pnp_paste_tiles: ramp = inf must be finite", ramp=float("inf"))
    call(b"pnp_paste_tiles: ncls 9 outside [1, 8]", ncls=9)
    call(b"pnp_paste_tiles: the box addresses elements outside [0, 120)", z0=5)
    call(b"pnp_paste_tiles: strides 30 1 1 let two voxels", s=(30, 1, 1))
    call(b"pnp_paste_tiles: ncls * vol_elems = 5 * ", elems=2 ** 62, s=(2 ** 40, 2 ** 20, 1))


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path):
    pr, nifti = pkg("predict"), pkg("nifti")
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16), np.diag([0.5, 0.7, 2.0, 1.0])), a)
    model = tmp_path / "m.npz"
    np.savez(str(model), x=np.zeros(1))
    base = ["--model", str(model), "--net", "segmenter", "--out", str(tmp_path / "o"), "--images", a]
    mm = ["--sample-mm", "1.0"]
    plain = pr.parse_args(base + mm)[3]
    assert "tiles" not in plain and "tile_overlap" not in plain                          # without the options nothing enters
    assert pr.parse_args(base + mm + ["--tiles", "auto"])[3]["tiles"] == "auto"
    assert "tile_overlap" not in pr.parse_args(base + mm + ["--tiles", "auto"])[3]
    o = pr.parse_args(base + mm + ["--tiles", "3x2", "--tile-overlap", "0.4"])[3]
    assert o["tiles"] == (3, 2) and o["tile_overlap"] == 0.4
    assert pr.parse_tiles("2X5") == (2, 5)
    for bad in (["--tiles", "auto"],                                                      # refused without --sample-mm
                mm + ["--tiles", "3"], mm + ["--tiles", "0x2"], mm + ["--tiles", "2x2x2"], mm + ["--tiles", "axb"],
                mm + ["--tile-overlap", "0.25"],                                          # goes with --tiles
                mm + ["--tiles", "auto", "--tile-overlap", "0.6"], mm + ["--tiles", "auto", "--tile-overlap", "-0.1"],
                mm + ["--tiles", "4x4", "--tta", "default"]):                             # 16 tiles x 5 views = 80 members
        with pytest.raises(SystemExit):
            pr.parse_args(base + bad)
    # with tiles the limit is pnp_paste_tiles': 2 x 2 tiles x 5 views = 20 members pass, without tiles 2 checkpoints x 5 views do not
    assert pr.parse_args(base + mm + ["--tiles", "2x2", "--tta", "default"])[3]["tiles"] == (2, 2)
    with pytest.raises(SystemExit):
        pr.parse_args(base + mm + ["--tta", "default", "--ensemble", str(model)])
    import io
    import contextlib
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
        pr.parse_args(["--help"])
    text = " ".join(out.getvalue().split("--tiles auto|NIxNJ")[-1].split())      # the option's own help text
    assert "--tiles" in out.getvalue() and "--sample-mm" in text[:120], text[:200]
