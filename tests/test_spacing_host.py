"""not gpu: the host side of the millimetre-grid sampling — compose_matrix's millimetre form, slicing_spacing, the
restatement of tests/spacing_ref.py pinned to scipy.ndimage.map_coordinates, the parameter stream, coverage, the flags and keyword
errors, and the argument refusals of the three new entry points (decided on the host before any HIP call)."""
import ctypes
import math
import os

import numpy as np
import pytest

import augment_ref as A
import spacing_ref as S
from conftest import ROOT, pkg


# ---- the plane map ---------------------------------------------------------------------------------------------------------------------
def test_reduction_to_the_resize_map():
    vs = pkg("volume_source")
    m = vs.compose_matrix((32, 24), (16, 16), spacing_xy=(1.0, 1.0), pixel_mm=(2.0, 1.5))
    assert m.dtype == np.float32 and np.array_equal(m, np.array([2, 0, 0.5, 0, 1.5, 0.25], np.float32))
    assert np.array_equal(m, vs.compose_matrix((32, 24), (16, 16)))
    # any isotropic spacing, rotated and scaled (translate = 0: it changes unit)
    for sp in (1.0, 0.5, 0.35):
        kw = {"rotate": 17.0, "scale": 1.2, "flip": True}
        got = vs.compose_matrix((32, 24), (16, 16), spacing_xy=(sp, sp), pixel_mm=(2.0 * sp, 1.5 * sp), **kw)
        np.testing.assert_allclose(got, vs.compose_matrix((32, 24), (16, 16), **kw), rtol=2e-7, atol=1e-6)
    # without the two keywords nothing changed: the formula of §13, entry by entry
    X, Y, H, W = 37.0, 29.0, 16.0, 24.0
    c, s = math.cos(math.radians(11.0)), math.sin(math.radians(11.0))
    a = np.array([c * X / H / 1.1, s * Y / W / 1.1, 0, s * X / H / 1.1, -c * Y / W / 1.1, 0])
    a[2] = (X - 1) / 2 + 2.0 - (a[0] * (H - 1) / 2 + a[1] * (W - 1) / 2)
    a[5] = (Y - 1) / 2 - 3.0 - (a[3] * (H - 1) / 2 + a[4] * (W - 1) / 2)
    np.testing.assert_allclose(vs.compose_matrix((37, 29), (16, 24), 11.0, 1.1, (2.0, -3.0), True), a.astype(np.float32), rtol=1e-6, atol=1e-6)
    for kw in ({"spacing_xy": (1, 1)}, {"pixel_mm": (1, 1)}, {"spacing_xy": (0, 1), "pixel_mm": (1, 1)}, {"spacing_xy": (1, 1), "pixel_mm": (1, np.nan)}):
        with pytest.raises(ValueError):
            vs.compose_matrix((8, 8), (8, 8), **kw)


@pytest.mark.parametrize("rotate", [0.0, 7.5, 33.0, 90.0, -141.0])
def test_rotation_and_scale_act_in_millimetres(rotate):
    """|S A (p1 - p2)| = |P (p1 - p2)| / scale: a step on the plane is the same length in the scan, in mm, whatever the angle"""
    sp, px, scale = (0.7, 1.3), (1.25, 0.8), 1.1
    m = S.compose_mm((23, 19), (16, 20), sp, px, rotate=rotate, scale=scale, flip=True, translate=(1.5, -2.0))
    A2 = np.array([[m[0], m[1]], [m[3], m[4]]])
    rng = np.random.default_rng(0)
    for _ in range(20):
        d = rng.standard_normal(2) * 5
        lhs = np.linalg.norm(np.diag(sp) @ A2 @ d)
        rhs = np.linalg.norm(np.diag(px) @ d) / scale
        assert abs(lhs - rhs) <= 1e-13 * rhs
    # the package's entries are these, rounded once to float32
    got = pkg("volume_source").compose_matrix((23, 19), (16, 20), rotate, scale, (1.5, -2.0), True, spacing_xy=sp, pixel_mm=px)
    assert np.abs(got - m.astype(np.float32)).max() <= 2 * np.spacing(np.float32(np.abs(m).max()))


def test_translate_is_in_millimetres():
    vs = pkg("volume_source")
    m0 = vs.compose_matrix((23, 19), (16, 16), spacing_xy=(0.5, 2.0), pixel_mm=(1, 1))
    m1 = vs.compose_matrix((23, 19), (16, 16), translate=(3.0, -4.0), spacing_xy=(0.5, 2.0), pixel_mm=(1, 1))
    assert np.array_equal(m1 - m0, np.array([0, 0, 6.0, 0, 0, -2.0], np.float32))


def test_quarter_turns_and_the_flip_stay_exact():
    vs = pkg("volume_source")
    for sp in (1.0, 0.5):
        for rot, want in ((0.0, [1, 0, 0, 1]), (90.0, [0, -1, 1, 0]), (180.0, [-1, 0, 0, -1]), (270.0, [0, 1, -1, 0])):
            m = vs.compose_matrix((16, 16), (16, 16), rotate=rot, spacing_xy=(sp, sp), pixel_mm=(sp, sp))
            assert np.array_equal(m[[0, 1, 3, 4]], np.array(want, np.float32)), (rot, m)
            sx, sy = A.coords(m, 16, 16)
            assert np.array_equal(sx, np.round(sx)) and sx.min() == 0 and sx.max() == 15 and sy.min() == 0 and sy.max() == 15
        m = vs.compose_matrix((16, 16), (16, 16), flip=True, spacing_xy=(sp, sp), pixel_mm=(sp, sp))
        assert np.array_equal(m, np.array([1, 0, 0, 0, -1, 15], np.float32))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_slicing_spacing_follows_the_axis_move(axis):
    vs, surface = pkg("volume_source"), pkg("surface")
    # unequal, obliquely oriented columns: rotations of (0.4, 1.1, 2.5) mm steps
    r = np.linalg.qr(np.random.default_rng(1).standard_normal((3, 3)))[0]
    aff = np.eye(4)
    aff[:3, :3] = r @ np.diag([0.4, 1.1, 2.5])
    aff[:3, 3] = (10, -20, 5)
    per_axis = surface.spacing_of(aff)
    np.testing.assert_allclose(per_axis, (0.4, 1.1, 2.5), rtol=1e-12)
    got = vs.slicing_spacing(aff, axis, "scan.nii.gz")
    # prepare_pair moves `axis` last: the shape of a probe array tells which array axis became which slicing axis
    probe = np.zeros((2, 3, 4))
    moved = np.moveaxis(probe, axis, -1).shape
    want = tuple(per_axis[(2, 3, 4).index(n)] for n in moved)
    assert got == want
    bad = aff.copy()
    bad[:3, 1] = 0
    with pytest.raises(ValueError, match="scan.nii.gz"):
        vs.slicing_spacing(bad, axis, "scan.nii.gz")
    bad[:3, 1] = np.nan
    with pytest.raises(ValueError, match="scan.nii.gz"):
        vs.slicing_spacing(bad, axis, "scan.nii.gz")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,dz", [(3, 0.37), (3, 1.0), (0, 2.5), (6, 0.37), (3, 7.9), (2, 0.0)])
def test_restatement_is_scipy_on_preinterpolated_frames(frame, dz):
    nd = pytest.importorskip("scipy.ndimage")
    vs = pkg("volume_source")
    rng = np.random.default_rng(5)
    vol = rng.standard_normal((13, 11, 7)).astype(np.float32)
    H, W = 12, 9
    m = vs.compose_matrix((13, 11), (H, W), rotate=31.0, scale=0.8, translate=(1.3, -0.7), flip=True, spacing_xy=(0.7, 1.3), pixel_mm=(1.0, 1.1))
    sx, sy = A.coords(m, H, W)
    fill = -1.75
    got = S.gather_image_z(vol, frame, dz, sx, sy, fill)
    v = vol.astype(np.float64)
    lo, hi = S.frame_positions(frame, dz, 7)
    assert 0 <= lo <= frame <= hi <= 6
    for c, zf in enumerate((lo, float(frame), hi)):
        # the frame at zf, interpolated by scipy along z (clamped coordinates: no edge mode is reached), then in the plane
        xx, yy = np.meshgrid(np.arange(13.0), np.arange(11.0), indexing="ij")
        fr = nd.map_coordinates(v, [xx, yy, np.full_like(xx, zf)], order=1, mode="nearest")
        ref = nd.map_coordinates(fr, [sx, sy], order=1, mode="grid-constant", cval=fill)
        np.testing.assert_allclose(got[:, :, c], ref, rtol=0, atol=1e-12)
    if dz == 1.0:
        assert np.array_equal(got, A.gather_image(vol, frame, sx, sy, fill))           # the three array frames
    if dz == 0.0:
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 2], got[..., 1])


def test_image_bound_terms():
    vol = np.zeros((4, 3, 5), np.float32)
    vol[:, :, 3] = 8.0
    assert S.frame_gap(vol) == 8.0 and S.frame_gap(vol[:, :, :1]) == 0.0
    assert S.z_eps(5) == 4 * 2.0 ** -21 and S.z_eps(1) == 4 * 2.0 ** -23
    m = np.array([[1, 0, 0, 0, 1, 0]], np.float32)
    b = S.image_bound(vol, 0.0, m, 4, 3)
    assert b == A.coord_eps(m, 4, 3) * 16.0 + 8 * S.U * 8.0 + S.z_eps(5) * 8.0


# ---- the parameter stream --------------------------------------------------------------------------------------------------------------
def test_parameter_stream_does_not_depend_on_sample_mm():
    vs = pkg("volume_source")
    dims = [(37, 29, 5), (64, 80, 9)]
    spacings = [(0.7, 1.3, 2.0), (0.35, 0.35, 0.6)]
    aug = vs.check_augment({"rotate": 20, "scale": 0.2, "translate": 8, "flip": 0.5})
    for augment in (aug, None):
        r0, raw0 = vs.sample_params(np.random.default_rng(4), dims, 64, (16, 24), augment)
        r1, raw1 = vs.sample_params(np.random.default_rng(4), dims, 64, (16, 24), augment, sample_mm=(1.0, 1.5, 2.5), spacings=spacings)
        assert r0.dtype == vs.SAMPLE_DTYPE and r1.dtype == vs.SAMPLE_Z_DTYPE and r1.dtype.itemsize == 36
        assert np.array_equal(r0["volume"], r1["volume"]) and np.array_equal(r0["frame"], r1["frame"])
        for k in raw0:
            assert np.array_equal(raw0[k], raw1[k]), k
        for b in range(64):
            v = int(r1["volume"][b])
            assert 1 <= r1["frame"][b] <= dims[v][2] - 2
            assert r1["dz"][b] == np.float32(2.5 / spacings[v][2])
            want = vs.compose_matrix(dims[v][:2], (16, 24), raw1["rotate"][b], raw1["scale"][b], (raw1["tx"][b], raw1["ty"][b]), bool(raw1["flip"][b]),
                                     spacing_xy=spacings[v][:2], pixel_mm=(1.0, 1.5))
            assert np.array_equal(r1["m"][b], want)
    # the generators are left in the same state
    g0, g1 = np.random.default_rng(9), np.random.default_rng(9)
    vs.sample_params(g0, dims, 5, (8, 8), aug)
    vs.sample_params(g1, dims, 5, (8, 8), aug, sample_mm=2.0, spacings=spacings)
    assert g0.random() == g1.random()
    with pytest.raises(ValueError, match="spacing"):
        vs.sample_params(g0, dims, 5, (8, 8), aug, sample_mm=2.0)


def test_records_mirror_the_header():
    vs, L = pkg("volume_source"), pkg("_lib")
    assert ctypes.sizeof(L.AugSampleZ) == 36 == vs.SAMPLE_Z_DTYPE.itemsize
    for name in ("volume", "frame", "dz", "m"):
        assert getattr(L.AugSampleZ, name).offset == vs.SAMPLE_Z_DTYPE.fields[name][1]
    header = open(os.path.join(ROOT, "include", "pnp_hip.h")).read()
    assert "typedef struct pnp_aug_sample_z {\n    int32_t volume, frame;\n    float dz;\n    float m[6];\n} pnp_aug_sample_z;" in header


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(S.GEOMETRIES))
def test_coverage_against_a_brute_force_loop(case):
    vs, vp = pkg("volume_source"), pkg("volume_predict")
    (X, Y), sp, px, (H, W), kw, margin, share = S.GEOMETRIES[case]
    inv = vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), spacing_xy=sp, pixel_mm=px, **kw))
    m = [float(v) for v in inv.astype(np.float64)]
    n = 0
    for x in range(X):
        for y in range(Y):
            pi = m[0] * x + m[1] * y + m[2]
            pj = m[3] * x + m[4] * y + m[5]
            n += -0.5 <= pi <= H - 0.5 and -0.5 <= pj <= W - 0.5
    got = vp.coverage(inv, X, Y, H, W)
    assert got == n / (X * Y) == S.covered(inv, X, Y, H, W).mean()
    # the figures the cases were chosen for
    assert abs(got - share) < 0.005 and abs(S.border_margin(inv, X, Y, H, W) - margin) < 0.05 * margin + 1e-6
    assert S.border_margin(inv, X, Y, H, W) >= 1e-3
    # several maps: the intersection; NaN: nothing
    both = vp.coverage([inv, vp.invert_matrix(vs.compose_matrix((X, Y), (H, W), rotate=20.0, spacing_xy=sp, pixel_mm=px))], X, Y, H, W)
    assert both <= got
    assert vp.coverage(np.full(6, np.nan, np.float32), X, Y, H, W) == 0.0


# ---- keywords and flags ----------------------------------------------------------------------------------------------------------------
def test_sample_mm_values():
    vs = pkg("volume_source")
    assert vs.check_sample_mm(None) is None and vs.check_sample_mm(1.5) == (1.5, 1.5, 1.5) and vs.check_sample_mm([1, 2, 3]) == (1.0, 2.0, 3.0)
    assert vs.parse_sample_mm(None) is None and vs.parse_sample_mm("0.8") == (0.8, 0.8, 0.8) and vs.parse_sample_mm("1,1.5,2.5") == (1.0, 1.5, 2.5)
    for bad in (0, -1.0, np.nan, np.inf, (1, 2), (1, 2, 0), (1, 2, 3, 4), "x", [None, 1, 1]):
        with pytest.raises(ValueError, match="sample_mm"):
            vs.check_sample_mm(bad)
    for bad in ("", "a", "1,2", "1,2,3,4", "0", "1,-1,1", "nan"):
        with pytest.raises(ValueError, match="--sample-mm"):
            vs.parse_sample_mm(bad)


def test_segment_volume_keyword_errors():
    """decided before any device work (device="cpu" would be refused later)"""
    vp = pkg("volume_predict")
    img = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(ValueError, match="sample_mm needs spacing"):
        vp.segment_volume(None, img, sample_mm=1.0, device="cpu")
    with pytest.raises(ValueError, match="sample_mm"):
        vp.segment_volume(None, img, sample_mm=-1.0, spacing=(1, 1, 1), device="cpu")
    with pytest.raises(ValueError, match="spacing"):
        vp.segment_volume(None, img, sample_mm=1.0, spacing=(1, 0, 1), device="cpu")
    with pytest.raises(ValueError, match="spacing"):
        vp.segment_volume(None, img, sample_mm=1.0, spacing=(1, 1), device="cpu")


def _nii(tmp_path, name, shape=(4, 4, 3), zooms=(0.5, 0.7, 2.0)):
    nifti = pkg("nifti")
    p = str(tmp_path / name)
    nifti.save(nifti.Nifti1Image(np.zeros(shape, np.int16), np.diag(list(zooms) + [1.0])), p)
    return p


def test_cli_flags(tmp_path):
    pr, ts, tg, vs = pkg("predict"), pkg("train_segmenter"), pkg("train_gan"), pkg("volume_source")
    a = _nii(tmp_path, "a.nii.gz")
    model = tmp_path / "m.npz"
    np.savez(str(model), x=np.zeros(1))
    base = ["--model", str(model), "--net", "segmenter", "--out", str(tmp_path / "o"), "--images", a]
    assert "sample_mm" not in pr.parse_args(base)[3]
    assert pr.parse_args(base + ["--sample-mm", "1.0"])[3]["sample_mm"] == (1.0, 1.0, 1.0)
    assert pr.parse_args(base + ["--sample-mm", "1,0.8,2.5"])[3]["sample_mm"] == (1.0, 0.8, 2.5)
    # --spacing keeps its meaning: the units of --score
    with pytest.raises(SystemExit):
        pr.parse_args(base + ["--spacing", "header"])
    for bad in ("0", "1,2", "x", "-1", "1,1,inf"):
        with pytest.raises(SystemExit):
            pr.parse_args(base + ["--sample-mm", bad])
        with pytest.raises(SystemExit):
            ts.main(["--nii-train", "t", "--nii-val", "v", "--sample-mm", bad])
        with pytest.raises(SystemExit):
            tg.parse_args("pre-train", ["--sample-mm", bad])
        with pytest.raises(SystemExit):
            vs.main(["--export", "1", str(tmp_path / "e"), "--list", "l", "--sample-mm", bad])
    with pytest.raises(SystemExit):
        ts.main(["--synthetic", "4", "--sample-mm", "1.0"])              # no NIfTI lists
    with pytest.raises(SystemExit):
        tg.parse_args("pre-train", ["--sample-mm", "1.0"])
    lists = ["--mr-nii-train", "a", "--mr-nii-val", "b", "--ct-nii-train", "c", "--ct-nii-val", "d"]
    assert tg.parse_args("pre-train", lists + ["--sample-mm", "1.5"]).sample_mm == (1.5, 1.5, 1.5)
    assert tg.parse_args("pre-train", lists).sample_mm is None


def test_predict_volumes_reads_the_spacing_from_the_affine(tmp_path, monkeypatch, caplog):
    import logging
    import torch
    vp = pkg("volume_predict")
    img = _nii(tmp_path, "scan.nii.gz", (7, 5, 4), (0.5, 0.7, 2.0))
    seen = []

    def fake(logits_fn, image, label=None, **kw):
        seen.append(kw)
        if "fov_stats" in kw:
            kw["fov_stats"].append(0.25)
        return torch.zeros(np.asarray(image).shape, dtype=torch.uint8)
    monkeypatch.setattr(vp, "segment_volume", fake)
    with caplog.at_level(logging.INFO):
        vp.predict_volumes(None, [img], str(tmp_path / "out"), device="cpu", sample_mm=(1.0, 1.0, 2.0))
    assert seen[0]["sample_mm"] == (1.0, 1.0, 2.0) and np.allclose(seen[0]["spacing"], (0.5, 0.7, 2.0))
    assert any(r.levelno == logging.WARNING and "25.0 %" in r.getMessage() for r in caplog.records)
    vp.predict_volumes(None, [img], str(tmp_path / "out"), device="cpu")
    assert "spacing" not in seen[1] and "fov_stats" not in seen[1] and "sample_mm" not in seen[1]


# ---- argument refusals of the new entry points -----------------------------------------------------------------------------------------
def test_refusals_before_any_hip_call(built):
    L = built._lib
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    ident = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)

    def vols(Z):
        t = (L.AugVolume * 1)()
        t[0].image, t[0].label, t[0].X, t[0].Y, t[0].Z, t[0].fill = ptr.value, ptr.value, 4, 4, Z, 0.0
        return t

    def gather(msg, table, B=1, H=4, W=4, x=ptr, ncls=5):
        rc = lib.pnp_aug_slices_z(ctypes.cast(table, ctypes.c_void_p), ptr, 1, ptr, B, H, W, x, ptr, ptr, ncls, ptr, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())
    gather(b"pnp_aug_slices_z: volume 0: Z = 0, at least 1 frames", vols(0))
    gather(b"pnp_aug_slices_z: B = 0", vols(1), B=0)
    gather(b"pnp_aug_slices_z: output size 0 x 4", vols(1), H=0)
    gather(b"pnp_aug_slices_z: null output pointer", vols(1), x=None)
    gather(b"pnp_aug_slices_z: ncls 33 outside [1, 32]", vols(1), ncls=33)
    # the three-frame entry keeps its own limit and its own name
    rc = lib.pnp_aug_slices(ctypes.cast(vols(2), ctypes.c_void_p), ptr, 1, ptr, 1, 4, 4, ptr, ptr, ptr, 5, ptr, None)
    assert rc == -1 and b"pnp_aug_slices: volume 0: Z = 2, at least 3 frames are needed" in lib.pnp_last_error()

    def labels(msg, **kw):
        a = dict(logits=ptr, B=2, H=8, W=8, ncls=5, nb=2, z0=1, inv=ident, X=4, Y=5, vol=ptr, elems=120, origin=0, s=(30, 6, 1))
        a.update(kw)
        rc = lib.pnp_paste_labels_fov(a["logits"], a["B"], a["H"], a["W"], a["ncls"], a["nb"], a["z0"], a["inv"], a["X"], a["Y"], a["vol"], a["elems"],
                                      a["origin"], a["s"][0], a["s"][1], a["s"][2], None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())
    labels(b"pnp_paste_labels_fov: null pointer", vol=None)
    labels(b"pnp_paste_labels_fov: ncls 9 outside [1, 8]", ncls=9)
    labels(b"pnp_paste_labels_fov: the box addresses elements outside [0, 120)", z0=5)
    labels(b"pnp_paste_labels_fov: strides 30 1 1 let two voxels", s=(30, 1, 1))
    members = (ctypes.c_void_p * 2)(ptr.value, ptr.value)
    two = (ctypes.c_float * 12)(*([1, 0, 0, 0, 1, 0] * 2))

    def ens(msg, M=2, logits=members, inv=two, z0=1):
        rc = lib.pnp_paste_ensemble_fov(M, logits, inv, 2, 8, 8, 5, 2, z0, 4, 5, ptr, 120, 0, 30, 6, 1, None, None, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())
    ens(b"pnp_paste_ensemble_fov: M = 9 members outside [1, 8]", M=9)
    ens(b"pnp_paste_ensemble_fov: null inv", inv=None)
    ens(b"pnp_paste_ensemble_fov: member 1 of 2 is a null pointer", logits=(ctypes.c_void_p * 2)(ptr.value, None))
    ens(b"pnp_paste_ensemble_fov: the box addresses elements outside [0, 120)", z0=5)
