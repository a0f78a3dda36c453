"""not gpu: the host side of foreground-aware slice sampling (volume_source.check_sampling / sample_params / the command-line flags;
DESIGN.md §22).  The class tables come from the numpy restatement (tests/frame_stats_ref.py), so nothing here needs the kernel.
Every comparison is exact; the one bound (the `centre` test) is the float32 rounding of the six matrix entries."""
import argparse

import numpy as np
import pytest

import frame_stats_ref as R
from conftest import pkg

ELASTIC = {"rotate": 15.0, "scale": 0.1, "translate": 10.0, "flip": 0.3, "elastic": 1.0, "noise": 0.1, "contrast": 0.2, "brightness": 0.1}
CLASSIC = ("rotate", "scale", "tx", "ty", "flip")
WARP = ("ctrl_px", "gain", "bias", "noise", "seed")


def _volumes():
    """three label volumes: no foreground at all; class 2 in the two outermost frames only (never eligible) next to an ordinary class 1;
    an ordinary one with classes 1, 2 and 3"""
    rng = np.random.default_rng(5)
    a = np.zeros((12, 10, 7), dtype=np.uint8)
    b = np.zeros((9, 14, 6), dtype=np.uint8)
    b[2:6, 3:9, 2:4] = 1
    b[1:4, 1:5, 0] = 2
    b[5:8, 8:12, 5] = 2
    c = np.zeros((16, 11, 9), dtype=np.uint8)
    c[3:9, 2:7, 1:5] = 1
    c[10:14, 6:10, 3:8] = 2
    c[1:3, 8:10, 6] = 3
    c[rng.random(c.shape) < 0.02] = 4
    return [a, b, c]


@pytest.fixture(scope="module")
def vols():
    labels = _volumes()
    return {"labels": labels, "dims": [l.shape for l in labels], "tables": [R.frame_stats(l, 5) for l in labels],
            "spacings": [(0.5, 0.8, 1.5), (1.0, 1.0, 2.0), (0.7, 0.9, 1.0)]}


def test_check_sampling_accepts_and_refuses():
    vs = pkg("volume_source")
    assert vs.check_sampling(None, 5) is None
    assert vs.check_sampling({"foreground": 0}, 5) is None and vs.check_sampling({"foreground": 0.0, "classes": [2], "centre": True}, 5) is None
    assert vs.check_sampling({"foreground": 0.5}, 5) == {"foreground": 0.5, "classes": (1, 2, 3, 4), "centre": False}
    assert vs.check_sampling({"foreground": 1, "classes": None}, 3) == {"foreground": 1.0, "classes": (1, 2), "centre": False}
    got = vs.check_sampling({"foreground": np.float32(0.25), "classes": (3, np.int64(1)), "centre": True}, 5)
    assert got == {"foreground": 0.25, "classes": (1, 3), "centre": True}
    assert vs.check_sampling(got, 5) == got                                      # a checked dict passes unchanged
    for bad in ({}, {"classes": [1]}, {"foreground": -0.1}, {"foreground": 1.5}, {"foreground": float("nan")}, {"foreground": "0.5"},
                {"foreground": True}, {"foreground": None}, {"foreground": 0.5, "frames": 3}, {"foreground": 0.5, "classes": []},
                {"foreground": 0.5, "classes": [0]}, {"foreground": 0.5, "classes": [5]}, {"foreground": 0.5, "classes": [1, 1]},
                {"foreground": 0.5, "classes": [1.0]}, {"foreground": 0.5, "classes": [True]}, {"foreground": 0.5, "classes": "12"},
                {"foreground": 0.5, "classes": 2}, {"foreground": 0.5, "centre": 1}, {"foreground": 0.5, "centre": "yes"},
                {"foreground": 0.0, "classes": [7]}, [0.5], 0.5):
        with pytest.raises(ValueError):
            vs.check_sampling(bad, 5)
    with pytest.raises(ValueError):
        vs.check_sampling({"foreground": 0.5}, 1)                                # no class but the background


def _parser(vs):
    ap = argparse.ArgumentParser()
    vs.add_sampling_flags(ap)
    return ap


def test_command_line_round_trip_and_parser_errors(capsys):
    vs = pkg("volume_source")
    ap = _parser(vs)
    assert vs.sampling_from_args(ap, ap.parse_args([])) is None
    assert vs.sampling_from_args(ap, ap.parse_args(["--foreground", "0"])) is None
    assert vs.sampling_from_args(ap, ap.parse_args(["--foreground", "0.33"])) == {"foreground": 0.33, "classes": (1, 2, 3, 4), "centre": False}
    got = vs.sampling_from_args(ap, ap.parse_args(["--foreground", "1", "--foreground-classes", "4,2", "--foreground-centre"]))
    assert got == {"foreground": 1.0, "classes": (2, 4), "centre": True}
    for argv, text in ((["--foreground-classes", "1"], "go with --foreground"), (["--foreground-centre"], "go with --foreground"),
                       (["--foreground", "1.5"], "probability"), (["--foreground", "0.5", "--foreground-classes", "0"], "[1, 5)"),
                       (["--foreground", "0.5", "--foreground-classes", "1,x"], "comma-separated")):
        with pytest.raises(SystemExit):
            vs.sampling_from_args(ap, ap.parse_args(argv))
        assert text in capsys.readouterr().err, argv


def test_trainers_and_export_take_the_flags():
    """the flags reach the three command lines, and "goes with the --nii lists" holds for them as for --axes"""
    ts, tg = pkg("train_segmenter"), pkg("train_gan")
    with pytest.raises(SystemExit):
        tg.parse_args("train-gan", ["--foreground", "0.5"])
    with pytest.raises(SystemExit):
        tg.parse_args("train-gan", ["--foreground-centre"])
    args = tg.parse_args("train-gan", ["--foreground", "0.5", "--foreground-classes", "2,3", "--mr-nii-train", "a", "--mr-nii-val", "b",
                                       "--ct-nii-train", "c", "--ct-nii-val", "d"])
    assert args.sampling == {"foreground": 0.5, "classes": (2, 3), "centre": False}
    assert tg.parse_args("train-gan", []).sampling is None
    for argv in (["--foreground", "0.5"], ["--foreground-classes", "2"], ["--nii-train", "a", "--nii-val", "b", "--foreground-centre"]):
        with pytest.raises(SystemExit):
            ts.main(argv)
    with pytest.raises(SystemExit):
        pkg("volume_source").main(["--export", "1", "out", "--list", "l", "--foreground-centre"])


@pytest.mark.parametrize("mm", [None, 1.0])
@pytest.mark.parametrize("augment", [None, "default", "elastic"])
def test_the_classic_stream_does_not_depend_on_the_option(vols, augment, mm):
    vs = pkg("volume_source")
    aug = vs.check_augment({None: None, "default": vs.DEFAULT_AUGMENT, "elastic": ELASTIC}[augment])
    warp = vs.uses_warp_entry(aug)
    B, hw = 40, (16, 12)

    def run(sampling, explicit=True):
        kw = dict(rng2=np.random.default_rng([3, 1]) if warp else None)
        if explicit:
            kw.update(sampling=sampling, frame_stats=vols["tables"] if sampling else None, rng3=np.random.default_rng([3, 2]) if sampling else None)
        return vs.sample_params(np.random.default_rng(3), vols["dims"], B, hw, aug, mm, vols["spacings"] if mm else None, **kw)

    rec0, raw0 = run(None, explicit=False)
    rec1, raw1 = run(None)
    assert rec0.tobytes() == rec1.tobytes() and sorted(raw0) == sorted(raw1) and "fg_class" not in raw1      # sampling=None: today's records
    if not warp:                            # ... and those are what the restatement's classic half gives
        ref = R.draw(vs.compose_matrix, 3, vols["dims"], B, hw, aug, vols["tables"], 0.0, (1, 2, 3, 4), False,
                     vs.check_sample_mm(mm), vols["spacings"])[0]
        assert ref.tobytes() == rec0.tobytes()
    for centre in (False, True):
        rec, raw = run({"foreground": 0.5, "centre": centre})
        assert rec.dtype == rec0.dtype and np.array_equal(rec["volume"], rec0["volume"])
        for k in CLASSIC + (WARP if warp else ()):
            assert (raw[k] is None and raw0[k] is None) or np.array_equal(raw[k], raw0[k]), k
        if warp:
            for k in ("gain", "bias", "noise", "seed", "warp", "dz"):
                assert np.array_equal(rec[k], rec0[k]), k
        if not centre:
            assert rec["m"].tobytes() == rec0["m"].tobytes() and not raw["centre"].any()
        else:
            moved = (raw["centre"] != 0).any(axis=1)
            assert moved.any() and np.array_equal(rec["m"][~moved], rec0["m"][~moved]) and not np.array_equal(rec["m"][moved], rec0["m"][moved])
        assert (rec["frame"] != rec0["frame"]).any() and np.array_equal(rec["frame"][raw["fg_class"] == 0], rec0["frame"][raw["fg_class"] == 0])


@pytest.mark.parametrize("mm", [None, (1.0, 0.8, 1.5)])
@pytest.mark.parametrize("augment", [None, "default"])
@pytest.mark.parametrize("sampling", [{"foreground": 0.6}, {"foreground": 1.0, "centre": True}, {"foreground": 0.7, "classes": (2, 3), "centre": True}])
def test_the_draw_is_the_restatement(vols, sampling, augment, mm):
    vs = pkg("volume_source")
    aug = vs.check_augment(vs.DEFAULT_AUGMENT if augment else None)
    B, hw, seed = 96, (20, 14), 11
    s = vs.check_sampling(sampling, 5)
    rec, raw = vs.sample_params(np.random.default_rng(seed), vols["dims"], B, hw, aug, mm, vols["spacings"] if mm else None, sampling=sampling,
                                frame_stats=vols["tables"], rng3=np.random.default_rng([seed, 2]))
    ref, fg, fb, cen = R.draw(vs.compose_matrix, seed, vols["dims"], B, hw, aug, vols["tables"], s["foreground"], s["classes"], s["centre"],
                              mm, vols["spacings"])
    assert rec.dtype == ref.dtype and rec.tobytes() == ref.tobytes()
    assert np.array_equal(raw["fg_class"], fg) and np.array_equal(raw["fallback"], fb) and raw["centre"].tobytes() == cen.tobytes()
    v = rec["volume"]
    # volume 0 has no foreground: every foreground sample of it falls back; volume 1's class 2 lives in frames 0 and Z - 1 only
    assert fb[v == 0].sum() > 0 and not fg[v == 0].any() and not fb[v == 2].any()
    assert (v == 1).sum() > 0 and ((fg[v == 1] == 1).any() or s["classes"] == (2, 3))
    assert not (fg[v == 1] == 2).any()
    if s["classes"] == (2, 3):
        assert fb[v == 1].sum() > 0 and set(fg[v == 2]) <= {0, 2, 3} and (fg[v == 2] == 3).any()
    if s["foreground"] == 1.0:
        assert ((fg > 0) | fb).all()


def test_foreground_one_lands_on_frames_that_hold_the_class(vols):
    vs = pkg("volume_source")
    rec, raw = vs.sample_params(np.random.default_rng(2), vols["dims"], 200, (8, 8), None, sampling={"foreground": 1.0},
                                frame_stats=vols["tables"], rng3=np.random.default_rng([2, 2]))
    n = 0
    for b in range(200):
        v, z, c = int(rec["volume"][b]), int(rec["frame"][b]), int(raw["fg_class"][b])
        Z = vols["dims"][v][2]
        assert 1 <= z <= Z - 2
        if raw["fallback"][b]:
            assert c == 0
            continue
        assert c > 0 and vols["tables"][v][z, c, 0] > 0 and (vols["labels"][v][:, :, z] == c).any()
        n += 1
    assert n > 50
    # every class that is eligible somewhere is drawn: a uniform class among those present, not a voxel-weighted one
    assert set(raw["fg_class"][rec["volume"] == 2]) == {1, 2, 3, 4}


def test_sample_params_refuses_half_an_option(vols):
    vs = pkg("volume_source")
    with pytest.raises(ValueError):
        vs.sample_params(np.random.default_rng(0), vols["dims"], 2, (8, 8), None, sampling={"foreground": 0.5})
    with pytest.raises(ValueError):
        vs.sample_params(np.random.default_rng(0), vols["dims"], 2, (8, 8), None, sampling={"foreground": 0.5}, frame_stats=vols["tables"][:1],
                         rng3=np.random.default_rng(1))
    with pytest.raises(ValueError):                              # a table of another volume
        vs.sample_params(np.random.default_rng(0), vols["dims"], 8, (8, 8), None, sampling={"foreground": 1.0}, frame_stats=vols["tables"][::-1],
                         rng3=np.random.default_rng(1))


@pytest.mark.parametrize("mm", [None, (0.6, 0.7, 1.0)])
def test_centre_puts_the_plane_centre_on_the_bounding_box(vols, mm):
    """M (c_out) = the bounding-box centre of the class in the drawn frame + the augment's jitter (voxels; with sample_mm millimetres
    over the anisotropic in-plane spacing (0.5, 0.8)), whatever the rotation, the scale and the flip: in float64 from the table and the
    raw draws.  The records hold M in float32: the bound is half an ulp of each of the three entries of a row, times what multiplies
    it."""
    vs = pkg("volume_source")
    aug = vs.check_augment(dict(vs.DEFAULT_AUGMENT, flip=0.5))
    hw = (20, 14)
    spacings = [(0.5, 0.8, 1.5)] * 3
    rec, raw = vs.sample_params(np.random.default_rng(9), vols["dims"], 120, hw, aug, mm, spacings if mm else None,
                                sampling={"foreground": 1.0, "centre": True}, frame_stats=vols["tables"], rng3=np.random.default_rng([9, 2]))
    ci, cj = (hw[0] - 1) / 2.0, (hw[1] - 1) / 2.0
    seen = 0
    for b in range(120):
        v, z, c = int(rec["volume"][b]), int(rec["frame"][b]), int(raw["fg_class"][b])
        X, Y, _ = vols["dims"][v]
        sx, sy = (spacings[v][0], spacings[v][1]) if mm else (1.0, 1.0)
        if c:
            _, xmin, xmax, ymin, ymax = (float(t) for t in vols["tables"][v][z, c])
            want = ((xmin + xmax) / 2 + raw["tx"][b] / sx, (ymin + ymax) / 2 + raw["ty"][b] / sy)
            assert tuple(raw["centre"][b]) == ((xmin + xmax) / 2 - (X - 1) / 2, (ymin + ymax) / 2 - (Y - 1) / 2)
            seen += 1
        else:
            want = ((X - 1) / 2 + raw["tx"][b] / sx, (Y - 1) / 2 + raw["ty"][b] / sy)
            assert not raw["centre"][b].any()
        m = rec["m"][b].astype(np.float64)
        for r in (0, 1):
            got = m[3 * r] * ci + m[3 * r + 1] * cj + m[3 * r + 2]
            bound = 2.0 ** -24 * (abs(m[3 * r]) * ci + abs(m[3 * r + 1]) * cj + abs(m[3 * r + 2])) + 1e-12
            assert abs(got - want[r]) <= bound, (b, r, got, want[r], bound)
    assert seen > 40
