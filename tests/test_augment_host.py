"""not gpu: the host side of the NIfTI training input (volume_source.py) — the restatement of tests/augment_ref.py pinned to
scipy.ndimage.map_coordinates, the composed matrices, the parameter sampler, list files, the preparation of a volume pair, the entry
points' flags, and every argument refusal of pnp_volume_preprocess / pnp_aug_slices (decided on the host before any HIP call: the buffers
are small host buffers, never read)."""
import ctypes
import os

import numpy as np
import pytest

import augment_ref as R
from conftest import pkg


def _volume(rng, shape):
    return rng.standard_normal(shape).astype(np.float32), rng.integers(0, 5, shape).astype(np.uint8)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rotated", "mostly_outside", "identity", "shifted_half"])
def test_restatement_is_scipy_grid_constant(case):
    nd = pytest.importorskip("scipy.ndimage")
    vs = pkg("volume_source")
    rng = np.random.default_rng(3)
    vol, lab = _volume(rng, (13, 9, 4))
    H, W = 11, 14
    m = {"rotated": vs.compose_matrix((13, 9), (H, W), rotate=31.0, scale=0.9, translate=(1.3, -0.7), flip=True),
         "mostly_outside": vs.compose_matrix((13, 9), (H, W), rotate=-70.0, scale=0.2, translate=(6.0, 5.0)),
         "identity": vs.compose_matrix((13, 9), (13, 9)),
         "shifted_half": np.array([1, 0, 0.5, 0, 1, -0.5], dtype=np.float32)}[case]
    if case == "identity":
        H, W = 13, 9
    sx, sy = R.coords(m, H, W)
    fill = -1.75
    got = R.gather_image(vol, 2, sx, sy, fill)
    for c in range(3):
        ref = nd.map_coordinates(vol[:, :, 1 + c].astype(np.float64), [sx, sy], order=1, mode="grid-constant", cval=fill)
        np.testing.assert_allclose(got[:, :, c], ref, rtol=0, atol=1e-12)
    ref = nd.map_coordinates(lab[:, :, 2].astype(np.float64), [sx, sy], order=0, mode="grid-constant", cval=0.0)
    gl = R.gather_label(lab, 2, sx, sy)
    if case == "shifted_half":
        # exact half-way coordinates: the contract is floor(s + 0.5); scipy agrees wherever it rounds a half up
        assert np.mean(gl == ref) > 0.5
    else:
        np.testing.assert_array_equal(gl, ref)
    if case == "identity":
        assert np.array_equal(got, vol[:, :, 1:4].astype(np.float64)) and np.array_equal(gl, lab[:, :, 2])
    if case == "mostly_outside":
        assert np.mean(got == fill) > 0.5


def test_clip_index_is_numpy_higher():
    for n in (1, 2, 3, 51, 101, 1000, 4099):
        v = np.random.default_rng(n).permutation(n).astype(np.float32)
        k = R.clip_index(n)
        assert 0 <= k <= n - 1 and k == -((-98 * (n - 1)) // 100)          # ceil(0.98 (n - 1)) in integers
        assert np.partition(v, k)[k] == np.percentile(v.astype(np.float64), 98, method="higher")
        out, st = R.preprocess(v)
        assert st["clip"] == float(k)                                     # v is a permutation of 0 .. n-1
    assert R.clip_index(1 << 30) == (98 * ((1 << 30) - 1) + 99) // 100
    out, st = R.preprocess(np.full(7, 3.5, np.float32))
    assert st["std"] == 0 and not out.any()


# ---- composed matrices -----------------------------------------------------------------------------------------------------------------
def test_identity_matrix_is_exact():
    vs = pkg("volume_source")
    for n in (3, 256, 255, 4096):
        m = vs.compose_matrix((n, n + 1), (n, n + 1))
        assert m.dtype == np.float32 and np.array_equal(m, np.array([1, 0, 0, 0, 1, 0], dtype=np.float32))


def test_quarter_turns_and_flip_are_integer_permutations():
    vs = pkg("volume_source")
    rng = np.random.default_rng(0)
    for n in (8, 9):
        vol, lab = _volume(rng, (n, n, 3))
        for kwargs, expect in (({"rotate": 90.0}, lambda a: np.rot90(a, -1)), ({"rotate": 180.0}, lambda a: a[::-1, ::-1]),
                               ({"rotate": -90.0}, lambda a: np.rot90(a, 1)), ({"rotate": 360.0}, lambda a: a),
                               ({"flip": True}, lambda a: a[:, ::-1]), ({"rotate": 90.0, "flip": True}, lambda a: np.rot90(a, -1)[:, ::-1])):      # the flip mirrors the OUTPUT's second axis
            m = vs.compose_matrix((n, n), (n, n), **kwargs)
            assert np.array_equal(m, np.round(m)), (kwargs, m)
            sx, sy = R.coords(m, n, n)
            assert np.array_equal(sx, np.round(sx)) and sx.min() == 0 and sx.max() == n - 1 and sy.min() == 0 and sy.max() == n - 1
            img = R.gather_image(vol, 1, sx, sy, fill=99.0)
            assert np.array_equal(img, expect(vol.astype(np.float64))), kwargs
            assert np.array_equal(R.gather_label(lab, 1, sx, sy), expect(lab[:, :, 1])), kwargs


def test_resize_is_centre_aligned():
    vs = pkg("volume_source")
    m = vs.compose_matrix((100, 60), (256, 128))
    sx, sy = R.coords(m, 256, 128)
    np.testing.assert_allclose(sx[:, 0], (np.arange(256) + 0.5) * 100 / 256 - 0.5, atol=1e-5)
    np.testing.assert_allclose(sy[0, :], (np.arange(128) + 0.5) * 60 / 128 - 0.5, atol=1e-5)
    # scale > 1 magnifies about the centre; the translation is in source voxels
    m2 = vs.compose_matrix((100, 60), (256, 128), scale=2.0, translate=(3.0, -2.0))
    sx2, sy2 = R.coords(m2, 256, 128)
    np.testing.assert_allclose(sx2 - 3.0 - 49.5, (sx - 49.5) / 2, atol=1e-4)
    np.testing.assert_allclose(sy2 + 2.0 - 29.5, (sy - 29.5) / 2, atol=1e-4)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def test_sampler_is_reproducible_in_range_and_differs_by_rank():
    vs, par = pkg("volume_source"), pkg("parallel")
    dims = [(20, 30, 3), (64, 64, 9), (7, 5, 4)]
    aug = {"rotate": 20.0, "scale": 0.25, "translate": 4.0, "flip": 0.5}
    draw = lambda seed, rank, a=aug: vs.sample_params(np.random.default_rng(seed + par.rank_seed(rank)), dims, 64, (32, 32), vs.check_augment(a))
    r0, raw0 = draw(5, 0)
    r0b, _ = draw(5, 0)
    assert r0.tobytes() == r0b.tobytes()
    r1, _ = draw(5, 1)
    assert r1.tobytes() != r0.tobytes() and draw(6, 0)[0].tobytes() != r0.tobytes()
    assert r0["volume"].min() >= 0 and r0["volume"].max() < len(dims) and len(set(r0["volume"])) == len(dims)
    Z = np.array([dims[v][2] for v in r0["volume"]])
    assert np.all(r0["frame"] >= 1) and np.all(r0["frame"] <= Z - 2)
    assert np.all(r0["frame"][Z == 3] == 1)
    assert np.all(np.abs(raw0["rotate"]) <= 20.0) and np.all(np.abs(raw0["tx"]) <= 4.0) and np.all(np.abs(raw0["ty"]) <= 4.0)
    assert np.all(raw0["scale"] <= 1.25 + 1e-12) and np.all(raw0["scale"] >= 1 / 1.25 - 1e-12)
    assert 0 < raw0["flip"].sum() < 64
    assert np.all(np.isfinite(r0["m"]))
    # augment=None: identity maps (a centre-aligned resize), frames still in range
    rn, rawn = draw(5, 0, None)
    assert not rawn["rotate"].any() and not rawn["flip"].any() and np.all(rawn["scale"] == 1.0)
    for rec in rn:
        X, Y, Zv = dims[rec["volume"]]
        assert np.array_equal(rec["m"], vs.compose_matrix((X, Y), (32, 32))) and 1 <= rec["frame"] <= Zv - 2


def test_augment_dict_is_checked():
    vs = pkg("volume_source")
    assert vs.check_augment(None) is None
    assert vs.check_augment({"rotate": 5}) == {"rotate": 5.0, "scale": 0.0, "translate": 0.0, "flip": 0.0}
    assert set(vs.DEFAULT_AUGMENT) == {"rotate", "scale", "translate", "flip"} and vs.check_augment(vs.DEFAULT_AUGMENT) == vs.DEFAULT_AUGMENT
    for bad in ({"shear": 1}, {"rotate": -1}, {"flip": 1.5}, {"scale": -0.1}):
        with pytest.raises(ValueError):
            vs.check_augment(bad)


# ---- list files and volume preparation -------------------------------------------------------------------------------------------------
def test_list_file_parsing_and_its_errors(tmp_path):
    vs, nifti = pkg("volume_source"), pkg("nifti")
    for name in ("a_image.nii.gz", "a_label.nii.gz", "b_image.nii", "b_label.nii"):
        nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16)), str(tmp_path / name))
    good = tmp_path / "list"
    good.write_text("# comment\na_image.nii.gz a_label.nii.gz\n\n%s   b_label.nii\n" % (tmp_path / "b_image.nii"))
    pairs = vs.read_pairs(str(good))
    assert pairs == [(str(tmp_path / "a_image.nii.gz"), str(tmp_path / "a_label.nii.gz")), (str(tmp_path / "b_image.nii"), str(tmp_path / "b_label.nii"))]
    with pytest.raises(IOError, match="does not exist"):
        vs.read_pairs(str(tmp_path / "nothing"))
    for text, exc, what in (("a_image.nii.gz\n", ValueError, "got 1 fields"), ("a_image.nii.gz a_label.nii.gz x.nii\n", ValueError, "got 3 fields"),
                            ("a_image.nii.gz a_label.txt\n", ValueError, "not a .nii"), ("a_image.nii.gz missing.nii\n", IOError, ":1: .*missing.nii does not exist"),
                            ("\n# only a comment\n", ValueError, "no volume pair")):
        bad = tmp_path / "bad"
        bad.write_text(text)
        with pytest.raises(exc, match=what):
            vs.read_pairs(str(bad))


def test_prepare_pair_flips_reorders_and_crops():
    vs = pkg("volume_source")
    rng = np.random.default_rng(1)
    img = rng.standard_normal((6, 7, 8))
    lab = np.zeros((6, 7, 8), np.int16)
    lab[2:4, 3:6, 1:3] = 2
    a, l = vs.prepare_pair(img, lab)
    assert a.dtype == np.float32 and l.dtype == np.uint8 and a.flags.c_contiguous and l.flags.c_contiguous
    assert np.array_equal(a, img[::-1, ::-1, :].astype(np.float32)) and np.array_equal(l, lab[::-1, ::-1, :])
    a, l = vs.prepare_pair(img, lab, flip_correction=False, axis=0)
    assert a.shape == (7, 8, 6) and np.array_equal(a, np.moveaxis(img, 0, -1).astype(np.float32))
    a, l = vs.prepare_pair(img, lab, flip_correction=False, crop=1)
    assert a.shape == (4, 5, 4) and np.array_equal(a, img[1:5, 2:7, 0:4].astype(np.float32)) and np.array_equal(l, lab[1:5, 2:7, 0:4])
    a, l = vs.prepare_pair(img, np.zeros_like(lab), flip_correction=False, crop=0)
    assert a.shape == img.shape                                           # no label: nothing to crop to
    for bad_img, bad_lab in ((img, lab[:5]), (img, lab + 0.5), (img, lab - 1), (img, lab + 300), (np.where(img > 2, np.nan, img), lab)):
        with pytest.raises(ValueError):
            vs.prepare_pair(bad_img, bad_lab)


def test_volume_set_needs_a_gpu_device(tmp_path):
    vs, L = pkg("volume_source"), pkg("_lib")
    with pytest.raises(L.PnpError, match="no CPU fallback"):
        vs.VolumeSet.from_arrays([np.zeros((4, 4, 3))], [np.zeros((4, 4, 3), np.uint8)], ["v"], "cpu")


def test_entry_point_flags():
    tg, vs = pkg("train_gan"), pkg("volume_source")
    a = tg.parse_args("pre-train", [])
    assert all(getattr(a, f) is None for f in tg.NII_FLAGS) and a.augment is None and a.no_augment is False
    assert vs.augment_from_args(a) == vs.DEFAULT_AUGMENT
    a = tg.parse_args("pre-train", ["--mr-nii-train", "a", "--mr-nii-val", "b", "--ct-nii-train", "c", "--ct-nii-val", "d", "--augment", '{"rotate": 3}'])
    assert (a.mr_nii_train, a.ct_nii_val) == ("a", "d") and vs.augment_from_args(a)["rotate"] == 3.0
    assert vs.augment_from_args(tg.parse_args("pre-train", ["--no-augment"])) is None
    for argv in (["--mr-nii-train", "a"], ["--no-augment", "--augment", "{}"],
                 ["--mr-nii-train", "a", "--mr-nii-val", "b", "--ct-nii-train", "c", "--ct-nii-val", "d", "--synthetic", "4"]):
        with pytest.raises(SystemExit):
            tg.parse_args("pre-train", argv)
    ts = pkg("train_segmenter")
    for argv in (["--nii-train", "a"], ["--nii-val", "a"], ["--nii-train", "a", "--nii-val", "b", "--synthetic", "2"]):
        with pytest.raises(SystemExit):
            ts.main(argv)
    with pytest.raises(ValueError):
        vs.augment_from_args(tg.parse_args("pre-train", ["--augment", "not json"]))


# ---- argument refusals of the entry points ---------------------------------------------------------------------------------------------
def test_preprocess_refusals_before_any_hip_call(built):
    L = built._lib
    lib = L.load()
    buf = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    need = int(lib.pnp_volume_preprocess_workspace_bytes(1000))
    assert 0 < need <= len(buf) and need == int(lib.pnp_volume_preprocess_workspace_bytes(1)) == int(lib.pnp_volume_preprocess_workspace_bytes((1 << 31) - 1))
    assert lib.pnp_volume_preprocess_workspace_bytes(0) == 0 and lib.pnp_volume_preprocess_workspace_bytes(1 << 31) == 0

    def refused(msg, v=ptr, out=ptr, n=1000, pct=98, stats=ptr, ws=ptr, nbytes=need):
        rc = lib.pnp_volume_preprocess(v, out, n, pct, stats, ws, nbytes, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())

    refused(b"at least one voxel", n=0)
    refused(b"at least one voxel", n=-5)
    refused(b"not below 2^31", n=1 << 31)
    refused(b"percentile 101 outside", pct=101)
    refused(b"percentile -1 outside", pct=-1)
    refused(b"null pointer", v=None)
    refused(b"null pointer", out=None)
    refused(b"null pointer", stats=None)
    refused(b"null pointer", ws=None)
    refused(b"workspace too small", nbytes=need - 1)


def test_aug_slices_refusals_before_any_hip_call(built):
    L = built._lib
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 15) & ~15
    ptr = ctypes.c_void_p(base)

    def table(**over):
        t = (L.AugVolume * 2)()
        for i in range(2):
            t[i].image, t[i].label, t[i].X, t[i].Y, t[i].Z, t[i].fill = base, base, 16, 4096, 3, 0.0
        for k, v in over.items():
            setattr(t[1], k, v)
        return t

    def refused(msg, vols=None, dev=ptr, nvol=2, samples=ptr, B=2, H=8, W=8, x=ptr, label=ptr, onehot=ptr, ncls=5, err=ptr):
        vols = table() if vols is None else vols
        rc = lib.pnp_aug_slices(ctypes.cast(vols, ctypes.c_void_p) if vols != 0 else None, dev, nvol, samples, B, H, W, x, label, onehot, ncls, err, None)
        assert rc == -1 and msg in lib.pnp_last_error(), (rc, lib.pnp_last_error())

    refused(b"B = 0", B=0)
    refused(b"output size 0 x 8", H=0)
    refused(b"output size 8 x -1", W=-1)
    refused(b"null table", vols=0)
    refused(b"null table", dev=None)
    refused(b"null table", samples=None)
    refused(b"nvol = 0", nvol=0)
    refused(b"null output pointer", x=None)
    refused(b"null output pointer", label=None)
    refused(b"null output pointer", err=None)
    refused(b"ncls 0 outside [1, 32]", ncls=0)
    refused(b"ncls 33 outside [1, 32]", ncls=33)
    refused(b"16-byte aligned", x=ctypes.c_void_p(base + 4))
    refused(b"16-byte aligned", onehot=ctypes.c_void_p(base + 8))
    refused(b"not below 2^31", B=1 << 11, H=1 << 10, W=1 << 10)
    refused(b"volume 1: extents 4097 x 4096", vols=table(X=4097))
    refused(b"volume 1: extents 16 x 0", vols=table(Y=0))
    refused(b"volume 1: Z = 2", vols=table(Z=2))
    refused(b"volume 1: null pointer", vols=table(image=None))
    refused(b"volume 1: null pointer", vols=table(label=None))


def test_struct_mirrors_match_the_header(built):
    L, vs = built._lib, pkg("volume_source")
    assert ctypes.sizeof(L.AugVolume) == 32 and ctypes.sizeof(L.AugSample) == 32
    assert vs.VOLUME_DTYPE.itemsize == 32 and vs.SAMPLE_DTYPE.itemsize == 32
    assert [vs.VOLUME_DTYPE.fields[n][1] for n in ("image", "label", "X", "Y", "Z", "fill")] == [getattr(L.AugVolume, n).offset for n in ("image", "label", "X", "Y", "Z", "fill")]
    assert [vs.SAMPLE_DTYPE.fields[n][1] for n in ("volume", "frame", "m")] == [getattr(L.AugSample, n).offset for n in ("volume", "frame", "m")]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnp_hip.h")).read()
    assert "typedef struct pnp_aug_volume" in hdr and "typedef struct pnp_aug_sample" in hdr
