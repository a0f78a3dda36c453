"""Host side of the label-free body crop, no GPU: body.otsu_bin against a brute force over exact fractions, the numpy
restatement of the chain (tests/body_ref.py) on the torso phantoms, the image-only list lines, and every argument refusal that is decided
before any device work — VolumeSet / AugmentedSliceSource / segment_volume, the four command lines' flags and the two entry points' host
checks."""
import ctypes

import numpy as np
import pytest

import body_ref as R
from conftest import pkg


# ---- otsu_bin ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_otsu_bin_equals_the_brute_force_on_random_histograms(seed):
    body = pkg("body")
    rng = np.random.default_rng(seed)
    nbins = int(rng.integers(2, 40))
    h = rng.integers(0, 50, nbins)
    h[rng.random(nbins) < 0.4] = 0                         # empty bins, empty ends
    assert body.otsu_bin(h) == R.otsu_bin(h), h
    big = rng.integers(0, 2 ** 20, 256)
    assert body.otsu_bin(big) == R.otsu_bin(big)


def test_otsu_bin_ties_one_bin_and_large_counts():
    body = pkg("body")
    two = np.zeros(64, dtype=np.int64)
    two[9], two[40] = 700, 300
    # every k in [9, 39] separates the two spikes equally well: the first of the run wins, the lower spike's bin
    assert body.otsu_bin(two) == R.otsu_bin(two) == 9
    assert body.otsu_bin([5]) == 0 and body.otsu_bin([0, 0, 7, 0]) == 0 == R.otsu_bin([0, 0, 7, 0])          # one occupied bin: no k qualifies
    assert body.otsu_bin([3, 4]) == 0
    near = np.zeros(1024, dtype=np.int64)
    near[3], near[4], near[700], near[1023] = 2 ** 31 - 5, 2 ** 30 + 1, 2 ** 31 - 1, 17          # products far beyond int64: exact all the same
    assert body.otsu_bin(near) == R.otsu_bin(near)
    assert body.otsu_bin(near.astype(np.uint32)) == R.otsu_bin(near)                               # what a device histogram arrives as
    with pytest.raises(ValueError):
        body.otsu_bin([1, -1])


# ---- the chain's restatement on the phantoms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ct", "mr"])
@pytest.mark.parametrize("seed", range(3))
def test_the_reference_chain_finds_the_phantoms_body(kind, seed):
    v, box = R.phantom((48, 40, 12), kind, seed)
    assert box == ((8, 37), (7, 30), (2, 11))
    info = {}
    vn = R.normalise_host(v)
    assert R.box_of_normalised(vn, info=info) == box
    found, before, kept, largest = (int(x) for x in info["stats"][1])
    if kind == "ct":
        assert found == 2 and before - kept == 768           # the detached table plate (2 x 32 x 12) goes with the largest-component step
    assert int(info["hist"].sum()) == v.size
    # the margin grows the box and clamps at the borders: z has 2 frames below and 1 above, y 7 and 10 voxels
    assert R.box_of_normalised(vn, margin=3) == ((5, 40), (4, 33), (0, 12))
    assert R.box_of_normalised(vn, margin=9) == ((0, 46), (0, 39), (0, 12))
    assert pkg("body").grow_box(box, 9, v.shape) == ((0, 46), (0, 39), (0, 12))
    assert R.box_of_normalised(np.full((4, 5, 6), 2.5, np.float32)) == ((0, 4), (0, 5), (0, 6))       # a constant volume: the whole volume


def test_reference_bins_on_edges_and_constant():
    lo, hi, nbins = np.float32(-1.0), np.float32(3.0), 8
    v = lo + np.arange(nbins + 1, dtype=np.float32) * np.float32(0.5)              # exactly on every edge, and hi
    assert R.bins(v, lo, hi, nbins).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7]
    (a, b), h = R.histogram(np.full(10, 4.0, np.float32), 4)
    assert a == b == 4.0 and h.tolist() == [10, 0, 0, 0] and not R.mask(np.full(10, 4.0, np.float32), a, b, 0, 4).any()


def test_box_permutations_round_trip():
    body = pkg("body")
    box = ((1, 2), (3, 4), (5, 6))
    shape = (7, 8, 9)
    for ax in (0, 1, 2):
        moved = np.moveaxis(np.zeros(shape), ax, -1).shape
        p = body.permute_box(tuple((0, n) for n in shape), ax)
        assert tuple(b for _, b in p) == moved
        assert body.unpermute_box(body.permute_box(box, ax), ax) == box
        assert body.permute_box(box, ax) == pkg("volume_predict").view_box(box, ax)


# ---- lists with and without labels -------------------------------------------------------------------------------------------------------
def test_read_pairs_with_optional_labels(tmp_path):
    vs = pkg("volume_source")
    for name in ("a.nii.gz", "a_lab.nii.gz", "b.nii"):
        (tmp_path / name).write_bytes(b"")
    lst = tmp_path / "list"
    lst.write_text("# target scans\na.nii.gz a_lab.nii.gz\n\nb.nii\n")
    got = vs.read_pairs(str(lst), labels="optional")
    assert got == [(str(tmp_path / "a.nii.gz"), str(tmp_path / "a_lab.nii.gz")), (str(tmp_path / "b.nii"), None)]
    with pytest.raises(ValueError, match="got 1 fields"):
        vs.read_pairs(str(lst))                                                    # the default is what it was
    with pytest.raises(ValueError, match="got 1 fields"):
        vs.read_pairs(str(lst), labels="required")
    with pytest.raises(ValueError, match="required"):
        vs.read_pairs(str(lst), labels="maybe")
    lst.write_text("a.nii.gz a_lab.nii.gz b.nii\n")
    with pytest.raises(ValueError, match="got 3 fields"):
        vs.read_pairs(str(lst), labels="optional")
    lst.write_text("missing.nii\n")
    with pytest.raises(IOError):
        vs.read_pairs(str(lst), labels="optional")


# ---- argument errors, all before any device work ---------------------------------------------------------------------------------------
def test_crop_option_parsing():
    body = pkg("body")
    assert body.parse_crop(None) is None and body.parse_crop(4) == ("label", 4) and body.parse_crop("body") == ("body", 0)
    assert body.parse_crop(("body", 3)) == ("body", 3) and body.parse_crop(["body", np.int64(2)]) == ("body", 2)
    for bad in ("torso", ("body", -1), ("body", 1.5), ("body",), ("label", 2), 2.5, True):
        with pytest.raises(ValueError):
            body.parse_crop(bad)


def test_volume_set_and_segment_volume_argument_errors(tmp_path):
    vs, vp, nifti = pkg("volume_source"), pkg("volume_predict"), pkg("nifti")
    v, _ = R.phantom((48, 40, 12), "ct", 0)
    fid = str(tmp_path / "scan.nii.gz")
    nifti.save(nifti.Nifti1Image(v, np.eye(4)), fid)
    with pytest.raises(ValueError, match="margin"):
        vs.VolumeSet([(fid, None)], "cuda", crop=("body", -2))
    with pytest.raises(ValueError, match="has no label"):
        vs.VolumeSet([(fid, None)], "cuda", crop=3)                                # an int crop is a margin around the LABEL box
    with pytest.raises(ValueError, match="margin"):
        vp.segment_volume(lambda x: x, v, crop=("body", -1))
    with pytest.raises(ValueError):
        vp.segment_volume(lambda x: x, v, crop="torso")
    with pytest.raises(ValueError, match="margin"):
        vp.segment_volume(lambda x: x, v, crop=("body", -1), axes=(0, 1, 2))
    with pytest.raises(pkg("_lib").PnpError):
        pkg("body").body_box(__import__("torch").zeros(4, 4, 4))                   # a CPU tensor: no fallback

    class Unlabelled(object):                     # what AugmentedSliceSource reads of a set before it touches the device
        names, has_labels, dims = ["a", "b"], [True, False], [(8, 8, 4)] * 2
    with pytest.raises(ValueError, match="unlabelled volumes \\(b\\)"):
        vs.AugmentedSliceSource(Unlabelled(), 2, sampling={"foreground": 0.5})


def test_flag_exclusions_on_the_four_command_lines(capsys):
    ts, tg, vs, pr = pkg("train_segmenter"), pkg("train_gan"), pkg("volume_source"), pkg("predict")
    four = ["--mr-nii-train", "a", "--mr-nii-val", "b", "--ct-nii-train", "c", "--ct-nii-val", "d"]
    assert tg.parse_args("train-gan", four + ["--crop-body", "2"]).crop == ("body", 2)
    assert tg.parse_args("train-gan", four + ["--crop-body"]).crop == ("body", 0)
    assert tg.parse_args("train-gan", four + ["--crop-margin", "5"]).crop == 5
    assert tg.parse_args("train-gan", four).crop is None and tg.parse_args("train-gan", []).crop is None

    def refused(fn, text):
        with pytest.raises(SystemExit):
            fn()
        assert text in capsys.readouterr().err, text
    refused(lambda: tg.parse_args("train-gan", four + ["--crop-body", "--crop-margin", "2"]), "exclude each other")
    refused(lambda: tg.parse_args("train-gan", ["--crop-body"]), "need the NIfTI lists")
    refused(lambda: tg.parse_args("train-gan", ["--synthetic", "4", "--crop-margin", "1"]), "need the NIfTI lists")
    refused(lambda: tg.parse_args("train-gan", four + ["--crop-body", "-1"]), ">= 0")
    refused(lambda: ts.main(["--nii-train", "a", "--nii-val", "b", "--crop-body", "1", "--crop-margin", "2"]), "exclude each other")
    refused(lambda: ts.main(["--crop-body"]), "need the NIfTI lists")
    refused(lambda: ts.main(["--synthetic", "4", "--crop-margin", "2"]), "need the NIfTI lists")
    refused(lambda: vs.main(["--export", "1", "out", "--list", "l", "--crop-body", "--crop-margin", "2"]), "exclude each other")
    base = ["--model", "m", "--net", "segmenter", "--images", "i.nii.gz", "--out", "o"]
    refused(lambda: pr.parse_args(base + ["--crop-body", "--crop", "0:1,0:1,0:1"]), "--crop-body excludes")
    refused(lambda: pr.parse_args(base + ["--crop-body", "2", "--crop-margin", "1", "--labels", "l.nii.gz"]), "--crop-body excludes")
    refused(lambda: pr.parse_args(base + ["--crop-body", "-3"]), ">= 0")


def test_predict_takes_crop_body_without_labels(tmp_path):
    pr = pkg("predict")
    for name in ("m.npz", "i.nii.gz"):
        (tmp_path / name).write_bytes(b"")
    base = ["--model", str(tmp_path / "m.npz"), "--net", "segmenter", "--images", str(tmp_path / "i.nii.gz"), "--out", str(tmp_path / "o")]
    assert pr.parse_args(base + ["--crop-body", "4"])[3]["crop"] == ("body", 4)
    assert pr.parse_args(base + ["--crop-body"])[3]["crop"] == ("body", 0)
    assert pr.parse_args(base)[3]["crop"] is None


# ---- the entry points' host refusals (before any HIP call: the pointers are never dereferenced) ------------------------------------------
def test_entry_points_refuse_on_the_host(built):
    lib = built._lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    p = lambda off=0: ctypes.c_void_p(a + off)

    def hist(v=p(), n=8, nbins=16, rng=p(128), h=p(160)):
        return lib.pnp_volume_histogram(v, n, nbins, rng, h, None)

    def mask(v=p(), n=8, rng=p(128), nbins=16, k=3, m=p(200)):
        return lib.pnp_volume_threshold_mask(v, n, rng, nbins, k, m, None)
    for call, name in ((hist, b"pnp_volume_histogram"), (mask, b"pnp_volume_threshold_mask")):
        for kw, text in (({"v": None}, b"null"), ({"rng": None}, b"null"), ({"n": 0}, b"outside [1, 2^31)"), ({"n": 1 << 31}, b"outside [1, 2^31)"),
                         ({"nbins": 1}, b"outside [2, 1024]"), ({"nbins": 1025}, b"outside [2, 1024]"), ({"v": p(2)}, b"aligned")):
            assert call(**kw) == -1 and name in lib.pnp_last_error() and text in lib.pnp_last_error(), (name, kw, lib.pnp_last_error())
    assert hist(h=None) == -1 and b"null" in lib.pnp_last_error()
    assert mask(m=None) == -1 and b"null" in lib.pnp_last_error()
    for k in (-1, 16):
        assert mask(k=k) == -1 and b"k = %d outside [0, 15]" % k in lib.pnp_last_error()
    for off in (0, 31, 4):                                   # mask [off, off + 8) against v [0, 32)
        assert mask(m=p(off)) == -1 and b"overlaps" in lib.pnp_last_error()
