"""not gpu: the host side of the connected-component filter — the numpy restatement against scipy, every host refusal of the
three entry points by its text, the command-line argument errors of predict / evaluate and segment_volume's keep_largest= parsing."""
import ctypes

import numpy as np
import pytest

import components_ref as R
from conftest import pkg

CASES = {"random": R.case_random, "snake": R.case_snake, "blobs": R.case_blobs, "ties": R.case_ties}


@pytest.fixture(scope="module")
def volumes():
    return {k: f() for k, f in CASES.items()}


def test_the_cases_are_what_the_documents_say(volumes):
    assert volumes["random"].shape == (37, 29, 45) and volumes["snake"].shape == (33, 33, 64) and volumes["blobs"].shape == (96, 80, 72)
    assert int(volumes["snake"].sum()) == 18784
    for c in (1, 2, 3):
        r = R.roots(volumes["snake"], 5, c)
        assert set(np.unique(r)) == {-1, 0}, "the snake is one component that starts at voxel 0"
    assert len(R.offsets(1)) == 6 and len(R.offsets(2)) == 18 and len(R.offsets(3)) == 26


@pytest.mark.parametrize("conn", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_scipy_label(volumes, name, conn):
    """roots == the minimum flat index per scipy label, per class; scipy numbers components in raster order of their first voxel (the minimum
    indices are strictly increasing), so "the first largest label" of np.argmax(np.bincount(labels)) is "the lowest root" of the tie rule;
    keep = 1 keeps exactly that component"""
    ndimage = pytest.importorskip("scipy.ndimage")
    v = volumes[name]
    st = ndimage.generate_binary_structure(3, conn)
    r = R.roots(v, 5, conn)
    out, stats, _ = R.keep_largest(v, 5, keep=1, connectivity=conn)
    idx = np.arange(v.size).reshape(v.shape)
    for c in range(1, 5):
        lab, nl = ndimage.label(v == c, st)
        assert stats[c, 0] == nl and stats[c, 1] == int((v == c).sum())
        if nl == 0:
            continue
        mins = np.asarray(ndimage.minimum(idx, lab, np.arange(1, nl + 1))).astype(np.int64)
        assert np.all(np.diff(mins) > 0)
        assert np.array_equal(r[v == c], mins[lab[v == c] - 1])
        counts = np.bincount(lab.reshape(-1))[1:]
        first_largest = int(np.argmax(counts)) + 1
        assert np.array_equal(out == c, lab == first_largest)
        assert stats[c, 2] == stats[c, 3] == counts.max()
    assert np.array_equal(r < 0, v == 0)


def test_restatement_rules_on_the_ties_case(volumes):
    v = volumes["ties"]
    out, stats, r = R.keep_largest(v, 5, keep=1)
    assert sorted(np.unique(r).tolist()) == [-1, 1, 18, 40, 60, 90, 119]
    assert stats.tolist() == [[0, 0, 0, 0], [3, 10, 4, 4], [3, 5, 3, 3], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert out[0, 0, 1:5].all() and not out[1].any() and not out[3, 0].any()         # root 1 beats root 40 at equal size
    out2, stats2, _ = R.keep_largest(v, 5, keep=2)
    assert stats2[1].tolist() == [3, 10, 8, 4] and stats2[2].tolist() == [3, 5, 4, 3]
    assert out2[1, 1, 4] == 1 and out2[2, 0, 0] == 2 and out2[3, 4, 5] == 0           # of the two single voxels the lower root stays
    out3, stats3, _ = R.keep_largest(v, 5, keep=0, min_size=3)
    assert stats3[1].tolist() == [3, 10, 8, 4] and stats3[2].tolist() == [3, 5, 3, 3] and not out3[3, 0].any()
    out4, stats4, _ = R.keep_largest(v, 5, keep=1, classes=[2])
    assert np.array_equal(out4 == 1, v == 1) and stats4[1].tolist() == [3, 10, 10, 4] and stats4[2, 2] == 3
    hi = (v + 4 * (v > 0)).astype(np.uint8)                                             # labels 5 and 6: background for ncls = 5
    out5, stats5, r5 = R.keep_largest(hi, 5)
    assert not out5.any() and not stats5.any() and (r5 == -1).all()


def _buffers():
    buf = ctypes.create_string_buffer(1 << 16)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_workspace_query(built):
    lib = built._lib.load()
    q = lib.pnp_components_workspace_bytes
    assert q(1, 1, 1) == 1024 + 256 and q(37, 29, 45) == 1024 + (4 * 37 * 29 * 45 + 255) // 256 * 256
    assert q(256, 256, 200) == 1024 + 4 * 256 * 256 * 200
    assert q(0, 4, 4) == 0 and q(4, -1, 4) == 0 and q(4, 4, 4097) == 0 and q(4096, 4096, 128) == 0          # n = 2^31
    assert q(4096, 4096, 127) == 1024 + 4 * 4096 * 4096 * 127


def test_every_host_refusal_by_its_text(built):
    """decided on the host before any HIP call: the tensors are small host buffers that are never read, and there is no GPU here"""
    lib = built._lib.load()
    buf, p = _buffers()
    need = int(lib.pnp_components_workspace_bytes(4, 5, 6))

    def label(vol=p, D=(4, 5, 6), ncls=5, conn=1, roots=p, ws=p, wsb=need):
        return lib.pnp_label_components(vol, D[0], D[1], D[2], ncls, conn, roots, ws, wsb, None)

    def filt(vol=p, roots=p, D=(4, 5, 6), ncls=5, mask=0b11110, keep=1, min_size=0, out=p, stats=p, ws=p, wsb=need):
        return lib.pnp_filter_components(vol, roots, D[0], D[1], D[2], ncls, mask, keep, min_size, out, stats, ws, wsb, None)

    def refused(rc, text):
        msg = lib.pnp_last_error()
        assert rc == -1 and text in msg, (rc, msg)

    for kw in ({"vol": None}, {"roots": None}, {"ws": None}):
        refused(label(**kw), b"pnp_label_components: null pointer")
    for kw in ({"vol": None}, {"roots": None}, {"out": None}, {"stats": None}, {"ws": None}):
        refused(filt(**kw), b"pnp_filter_components: null pointer")
    for fn, who in ((label, b"pnp_label_components"), (filt, b"pnp_filter_components")):
        for D in ((0, 5, 6), (4, 4097, 6), (4, 5, -1)):
            refused(fn(D=D, wsb=1 << 40), who + b": extents")
        refused(fn(D=(4096, 4096, 128), wsb=1 << 40), who + b": 4096 x 4096 x 128 = 2147483648 voxels, fewer than 2^31")
        for ncls in (1, 9, 0, -3):
            refused(fn(ncls=ncls), who + b": ncls")
        refused(fn(wsb=need - 1), who + b": workspace too small")
        refused(fn(wsb=0), who + b": workspace too small")
    for conn in (0, 4, -1):
        refused(label(conn=conn), b"pnp_label_components: connectivity")
    for keep in (-1, 9):
        refused(filt(keep=keep), b"pnp_filter_components: keep")
    refused(filt(min_size=-1), b"pnp_filter_components: min_size")
    for ncls, mask in ((5, 0b00001), (5, 0b100000), (5, 0b111111), (2, 0b100), (8, 1 << 8)):
        refused(filt(ncls=ncls, mask=mask), b"pnp_filter_components: class_mask")


def test_python_wrappers_refuse_on_the_host(built):
    import torch
    C = pkg("components")
    cpu = torch.zeros((3, 4, 5), dtype=torch.uint8)
    with pytest.raises(built._lib.PnpError, match="no CPU fallback"):
        C.label_components(cpu)
    with pytest.raises(built._lib.PnpError, match="no CPU fallback"):
        C.keep_largest(cpu)
    with pytest.raises(ValueError, match="torch tensor"):
        C.keep_largest(np.zeros((3, 4, 5), np.uint8))
    assert C.class_mask(5) == 0b11110 and C.class_mask(5, [2, 4]) == 0b10100 and C.class_mask(2) == 0b10
    for bad in ([0], [5], [1.5], [True]):
        with pytest.raises(ValueError, match="classes"):
            C.class_mask(5, bad)
    for kw, text in (({"keep": -1}, "keep"), ({"keep": 9}, "keep"), ({"min_size": -1}, "min_size"), ({"connectivity": 4}, "connectivity"),
                     ({"keep": 1.0}, "keep must be an int"), ({"keep": True}, "keep must be an int")):
        with pytest.raises(ValueError, match=text):
            C.check_options(5, **kw)
    with pytest.raises(ValueError, match="num_cls"):
        C.check_options(9)
    assert C.check_options(5, np.int64(2), 3, 2, (1,)) == (2, 3, 2, 0b10)
    assert C.stats_line([[0, 0, 0, 0], [3, 10, 4, 4]]) == "class 1: 3 components, 10 -> 4 voxels, largest 4"


def test_segment_volume_checks_keep_largest_before_any_gpu_work(built):
    vp, C = pkg("volume_predict"), pkg("components")
    image = np.zeros((8, 8, 4), np.int16)
    never = lambda x: pytest.fail("the network must not run")
    for bad, text in (("1", "must be None, an int or a dict"), (1.0, "must be None, an int or a dict"), (True, "must be None, an int or a dict"),
                      ([1], "must be None, an int or a dict"), (-1, "is negative"), (9, "keep = 9 outside"),
                      ({"size": 3}, "unknown keys"), ({"keep": -2}, "keep = -2 outside"), ({"connectivity": 0}, "connectivity"),
                      ({"min_size": -5}, "min_size"), ({"classes": [7]}, "classes")):
        with pytest.raises(ValueError, match=text):
            vp.segment_volume(never, image, keep_largest=bad, device="cuda")
    assert C.parse_option(None) is None and C.parse_option(2) == {"keep": 2} and C.parse_option(0) == {"keep": 0}
    assert C.parse_option({"keep": 1, "min_size": 10, "classes": [1, 2]}) == {"keep": 1, "min_size": 10, "classes": [1, 2]}
    ev = pkg("evaluate")
    with pytest.raises(ValueError, match="is negative"):
        ev.evaluate([], keep_largest=-3, device="cpu")


def test_command_line_argument_errors(built, tmp_path, capsys):
    pr, ev, nifti = pkg("predict"), pkg("evaluate"), pkg("nifti")
    img, ck = str(tmp_path / "a.nii.gz"), str(tmp_path / "ck.npz")
    nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16), np.eye(4)), img)
    np.savez(ck, a=np.zeros(1))
    base = ["--model", ck, "--net", "segmenter", "--images", img, "--out", str(tmp_path / "o")]
    for extra, text in ((["--keep-largest", "-1"], "keep = -1 outside"), (["--keep-largest", "9"], "keep = 9 outside"),
                        (["--keep-largest", "x"], "invalid int value"), (["--min-size", "-2"], "min_size = -2 is negative"),
                        (["--connectivity", "2"], "--connectivity goes with"), (["--keep-largest", "--connectivity", "4"], "invalid choice")):
        with pytest.raises(SystemExit):
            pr.parse_args(base + extra)
        assert text in capsys.readouterr().err, extra
        with pytest.raises(SystemExit):
            ev.main(["--pred", img, "--gt", img] + extra)
        assert text in capsys.readouterr().err, extra
    _, _, _, opts = pr.parse_args(base)
    assert "keep_largest" not in opts                                                  # the default path is untouched
    _, _, _, opts = pr.parse_args(base + ["--keep-largest"])
    assert opts["keep_largest"] == {"keep": 1, "min_size": 0, "connectivity": 1}
    _, _, _, opts = pr.parse_args(base + ["--keep-largest", "3", "--min-size", "20", "--connectivity", "3"])
    assert opts["keep_largest"] == {"keep": 3, "min_size": 20, "connectivity": 3}
    _, _, _, opts = pr.parse_args(base + ["--min-size", "20"])
    assert opts["keep_largest"] == {"keep": 0, "min_size": 20, "connectivity": 1}
