"""not gpu: the host side of the anti-alias prefilter — the restatement of tests/prefilter_ref.py pinned to
scipy.ndimage.gaussian_filter1d, the weights, the sigma rule, the flag, the aliasing claim itself (in the restatement) and the argument
refusals of pnp_volume_smooth (decided on the host before any HIP call)."""
import ctypes

import numpy as np
import pytest

import augment_ref as A
import prefilter_ref as R
import spacing_ref as S
from conftest import pkg

SHAPES = [(13, 11, 7), (9, 17, 5), (6, 5, 1), (70, 3, 33)]
SIGMAS = [(0.3, 1.0, 2.2), (8, 0, 0.93), (2.2, 2.2, 8)]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigmas", SIGMAS)
def test_restatement_against_scipy(shape, sigmas):
    """bound: the restatement uses the float32-rounded weights, scipy the float64 ones — at most 2^-24 max|v| per pass — plus one unit of
    slack: 4 * 2^-24 max|v|"""
    nd = pytest.importorskip("scipy.ndimage")
    v = (np.random.default_rng(sum(shape)).standard_normal(shape) * 3).astype(np.float32)
    ref = v.astype(np.float64)
    for axis, s in enumerate(sigmas):
        if R.radius(s) > 0:
            ref = nd.gaussian_filter1d(ref, s, axis=axis, mode="nearest", truncate=4.0)
    got = R.smooth(v, sigmas)
    top = float(np.abs(v).max())
    err = float(np.abs(got - ref).max())
    print("restatement vs scipy %s %s: %.3f of 2^-24 max|v|" % (shape, sigmas, err / (R.U * top)))
    assert err <= 4 * R.U * top


# ---- the weights -----------------------------------------------------------------------------------------------------------------------
def test_weights():
    vs = pkg("volume_source")
    assert vs.gaussian_weights(0.0) is None and vs.gaussian_weights(0.1249) is None and len(vs.gaussian_weights(0.125)) == 3
    for sigma in (0.125, 0.3, 0.5, 0.9286, 1.0, 1.583, 2.2, 8.0, 8.1):
        w = vs.gaussian_weights(sigma)
        Rr = int(4.0 * sigma + 0.5)
        assert w.dtype == np.float32 and w.shape == (2 * Rr + 1,) and Rr <= 32
        assert np.array_equal(w, R.weights(sigma))                                   # the package's taps are the restatement's, bit for bit
        assert np.array_equal(w, w[::-1]) and np.all(w > 0) and w[Rr] == w.max()
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * Rr + 1) * 2.0 ** -24
        k = np.arange(-Rr, Rr + 1, dtype=np.float64)
        e = np.exp(-k * k / (2 * sigma * sigma))
        assert np.abs(w - (e / e.sum()).astype(np.float32)).max() <= 2.0 ** -24              # the formula, however its exponent is rounded
    assert len(vs.gaussian_weights(8.1)) == 65
    for bad in (-0.1, np.nan, np.inf, -np.inf, 8.2, "x", None):
        with pytest.raises(ValueError, match="sigma"):
            vs.gaussian_weights(bad)
    with pytest.raises(ValueError, match="8.2"):
        vs.gaussian_weights(8.2)


# ---- the sigma rule --------------------------------------------------------------------------------------------------------------------
def test_sigma_rule():
    vs = pkg("volume_source")
    ct = vs.prefilter_sigmas("auto", (512, 512, 300), (256, 256), (0.35, 0.35, 0.6), (1.0, 1.0, 2.5))
    np.testing.assert_allclose(ct, (0.9286, 0.9286, 1.583), atol=5e-4)
    np.testing.assert_allclose(ct, R.auto_sigmas((512, 512, 300), (256, 256), (0.35, 0.35, 0.6), (1.0, 1.0, 2.5)), rtol=1e-15)
    mr = vs.prefilter_sigmas("auto", (256, 256, 120), (256, 256), (1.0, 1.0, 1.6), (1.0, 1.0, 2.5))
    assert mr[:2] == (0.0, 0.0) and abs(mr[2] - 0.28125) < 1e-12
    assert vs.prefilter_sigmas("auto", (512, 512, 200), (256, 256)) == (0.5, 0.5, 0.0)
    assert vs.prefilter_sigmas("auto", (512, 384, 200), (256, 256), (0.35, 0.35, 0.6)) == (0.5, 0.25, 0.0)       # no sample_mm: the resize
    assert vs.prefilter_sigmas("auto", (100, 128, 50), (256, 256)) == (0.0, 0.0, 0.0)                            # upsampling
    assert vs.prefilter_sigmas("auto", (100, 100, 50), (256, 256), (2.0, 1.5, 3.0), 1.0) == (0.0, 0.0, 0.0)
    for off in (None, "off"):
        assert vs.prefilter_sigmas(off, (512, 512, 200), (256, 256), (0.35, 0.35, 0.6), 1.0) == (0.0, 0.0, 0.0)
    assert vs.prefilter_sigmas(1.5, (8, 8, 8), (256, 256)) == (1.5, 1.5, 1.5)
    assert vs.prefilter_sigmas((1, 0, 2.5), (8, 8, 8), (4, 4), (0.1, 0.1, 0.1), 5.0) == (1.0, 0.0, 2.5)          # taken as given
    with pytest.raises(ValueError, match="spacing"):
        vs.prefilter_sigmas("auto", (8, 8, 8), (4, 4), None, 1.0)
    with pytest.raises(ValueError, match="sigma"):
        vs.prefilter_sigmas("auto", (8, 8, 8), (4, 4), (0.01, 1, 1), 1.0)                                        # 100 voxels per pixel: 65 taps do not hold it
    for bad in ("on", (1, 2), (1, 2, 3, 4), (1, -1, 1), (1, np.nan, 1), 9.0, [None, 1, 1]):
        with pytest.raises(ValueError, match="prefilter|sigma"):
            vs.prefilter_sigmas(bad, (8, 8, 8), (4, 4))


# ---- the flag --------------------------------------------------------------------------------------------------------------------------
def test_flag_parsing(tmp_path):
    pr, ts, tg, vs, nifti = pkg("predict"), pkg("train_segmenter"), pkg("train_gan"), pkg("volume_source"), pkg("nifti")
    assert vs.parse_prefilter(None) is None and vs.parse_prefilter("off") is None and vs.parse_prefilter("auto") == "auto"
    assert vs.parse_prefilter("1,1,0") == (1.0, 1.0, 0.0) and vs.parse_prefilter("0.93,0.93,1.58") == (0.93, 0.93, 1.58)
    for bad in ("", "on", "1,2", "1,2,3,4", "1,-1,1", "nan,1,1", "9,1,1", "a,b,c"):
        with pytest.raises(ValueError, match="--prefilter"):
            vs.parse_prefilter(bad)
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16), np.diag([0.5, 0.7, 2.0, 1.0])), a)
    model = tmp_path / "m.npz"
    np.savez(str(model), x=np.zeros(1))
    base = ["--model", str(model), "--net", "segmenter", "--out", str(tmp_path / "o"), "--images", a]
    assert "prefilter" not in pr.parse_args(base)[3] and "prefilter" not in pr.parse_args(base + ["--prefilter", "off"])[3]
    assert pr.parse_args(base + ["--prefilter", "auto"])[3]["prefilter"] == "auto"
    assert pr.parse_args(base + ["--prefilter", "1,1,0", "--sample-mm", "1.0"])[3]["prefilter"] == (1.0, 1.0, 0.0)
    lists = ["--mr-nii-train", "a", "--mr-nii-val", "b", "--ct-nii-train", "c", "--ct-nii-val", "d"]
    assert tg.parse_args("pre-train", lists + ["--prefilter", "auto"]).prefilter == "auto"
    assert tg.parse_args("pre-train", lists).prefilter is None
    for bad in ("on", "1,2", "x", "1,1,-1", "1,1,inf"):
        with pytest.raises(SystemExit):
            pr.parse_args(base + ["--prefilter", bad])
        with pytest.raises(SystemExit):
            ts.main(["--nii-train", "t", "--nii-val", "v", "--prefilter", bad])
        with pytest.raises(SystemExit):
            tg.parse_args("pre-train", lists + ["--prefilter", bad])
        with pytest.raises(SystemExit):
            vs.main(["--export", "1", str(tmp_path / "e"), "--list", "l", "--prefilter", bad])
    with pytest.raises(SystemExit):
        ts.main(["--synthetic", "4", "--prefilter", "auto"])             # no NIfTI lists
    with pytest.raises(SystemExit):
        tg.parse_args("pre-train", ["--prefilter", "auto"])


def test_segment_volume_keyword_errors():
    """decided before any device work (device="cpu" would be refused later)"""
    vp = pkg("volume_predict")
    img = np.zeros((8, 8, 4), np.float32)
    for bad in ("on", (1, 2), -1.0, 9.0):
        with pytest.raises(ValueError, match="prefilter|sigma"):
            vp.segment_volume(None, img, prefilter=bad, device="cpu")


# ---- the aliasing claim itself, in the restatement ------------------------------------------------------------------------------------------
def test_stripes_alias_without_the_filter_and_vanish_with_it():
    """a cosine of period 1.0 mm on voxels of 0.35 mm, sampled bilinearly on pixels of 1 mm: one sample per period, so the stripes come out
    as a constant (an alias at frequency 0) — of full amplitude where the grid meets the crests (prefilter_ref.STRIPE_TRANSLATE_MM puts
    it there; centred on the volume it reads another phase: 0.474).  After the "auto" filter (sigma 0.93 voxels along x) exp(-2 pi^2
    sigma^2 0.35^2) = 0.125 of it is left.  Measured: 1.000 and 0.124."""
    vs = pkg("volume_source")
    vol = R.stripes()
    sp = (R.STRIPE_MM,) * 3
    m = R.stripe_map(vs.compose_matrix)
    sx, sy = A.coords(m, *R.STRIPE_OUT)
    assert sx.min() >= 5 and sx.max() <= R.STRIPE_SHAPE[0] - 6 and sy.min() >= 0 and sy.max() <= R.STRIPE_SHAPE[1] - 1     # inside, beyond the radius of 4 from the x borders
    assert abs(sx[5, 0] - 20.0) < 1e-5                                              # a pixel row on a crest that is a voxel centre
    dz = np.float32(R.STRIPE_SAMPLE_MM[2] / sp[2])
    raw = S.gather_image_z(vol, 3, dz, sx, sy, 0.0)
    sig = vs.prefilter_sigmas("auto", R.STRIPE_SHAPE, R.STRIPE_OUT, sp, R.STRIPE_SAMPLE_MM)
    np.testing.assert_allclose(sig, (0.92857, 0.92857, 0.0), atol=1e-5)
    filt = S.gather_image_z(R.smooth(vol, sig), 3, dz, sx, sy, 0.0)
    a_raw, a_filt = float(np.abs(raw[..., 1]).max()), float(np.abs(filt[..., 1]).max())
    print("stripes of period 1.0 mm on a 1 mm grid: max|x| %.3f unfiltered, %.3f with prefilter='auto'" % (a_raw, a_filt))
    assert a_raw >= 0.9 and a_filt <= 0.2


# ---- argument refusals of pnp_volume_smooth ------------------------------------------------------------------------------------------------
def test_refusals_before_any_hip_call(built):
    lib = built._lib.load()
    buf = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(buf)
    ptr = ctypes.c_void_p(base)
    w3 = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    w67 = (ctypes.c_float * 67)(*([1.0 / 67] * 67))
    wp = lambda w: ctypes.cast(w, ctypes.c_void_p)

    def smooth(msg, src=ptr, dst=ptr, dims=(4, 4, 4), wx=wp(w3), rx=1, wy=wp(w3), ry=1, wz=None, rz=0, ws=ctypes.c_void_p(base + 4096), ws_bytes=4096):
        rc = lib.pnp_volume_smooth(src, dst, dims[0], dims[1], dims[2], wx, rx, wy, ry, wz, rz, ws, ws_bytes, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())
    assert lib.pnp_volume_smooth_workspace_bytes(4, 4, 4, 1, 1, 0) == 256               # one volume of 64 floats
    assert lib.pnp_volume_smooth_workspace_bytes(4, 4, 4, 0, 0, 1) == 0                 # the z pass of a short row runs in place
    assert lib.pnp_volume_smooth_workspace_bytes(4, 4, 4, 0, 0, 0) == 0
    assert lib.pnp_volume_smooth_workspace_bytes(2, 2, 4096, 1, 1, 1) == 2 * 65536      # long rows: the z pass runs out of place
    assert lib.pnp_volume_smooth_workspace_bytes(4, 4, 4, 33, 0, 0) == 0 and lib.pnp_volume_smooth_workspace_bytes(0, 4, 4, 1, 0, 0) == 0
    smooth(b"pnp_volume_smooth: radii 33, 1, 0 outside [0, 32]", wx=wp(w67), rx=33)
    smooth(b"pnp_volume_smooth: radii 1, -1, 0 outside [0, 32]", ry=-1)
    smooth(b"pnp_volume_smooth: axis 0: null weights with radius 1", wx=None)
    smooth(b"pnp_volume_smooth: axis 2: null weights with radius 1", rz=1)
    smooth(b"pnp_volume_smooth: extents 4 x 0 x 4 must be at least 1", dims=(4, 0, 4))
    smooth(b"pnp_volume_smooth: X = 4097", dims=(4097, 1, 1))
    smooth(b"pnp_volume_smooth: X * Y * Z = 2147483648 is not below 2^31", dims=(1024, 1024, 2048))
    smooth(b"pnp_volume_smooth: workspace too small: 255 bytes < 256", ws_bytes=255)
    smooth(b"pnp_volume_smooth: workspace too small: 0 bytes < 256", ws=None)
    smooth(b"pnp_volume_smooth: src and dst overlap partially", dst=ctypes.c_void_p(base + 16))
    smooth(b"pnp_volume_smooth: src and dst overlap partially", src=ctypes.c_void_p(base + 252), dst=ptr)
    smooth(b"pnp_volume_smooth: null pointer", dst=None)
    bad = (ctypes.c_float * 3)(0.25, float("nan"), 0.25)
    smooth(b"pnp_volume_smooth: axis 1: weight 1 is not finite", wy=wp(bad))
    bad[1] = float("inf")
    smooth(b"pnp_volume_smooth: axis 0: weight 1 is not finite", wx=wp(bad))
