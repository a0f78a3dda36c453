"""not gpu: the host side of the hole filling — the numpy restatement against scipy, every host refusal of the two entry
points by its text, the workspace query, the wrappers' and parse_fill_option's errors, segment_volume's fill_holes= parsing and the
command-line argument errors of predict / evaluate."""
import ctypes

import numpy as np
import pytest

import holes_ref as R
from conftest import pkg


@pytest.fixture(scope="module")
def volumes():
    return {k: f() for k, f in R.CASES.items()}


def test_the_cases_are_what_the_documents_say(volumes):
    assert volumes["random"].shape == (37, 29, 45) and volumes["snake"].shape == (33, 33, 64) and volumes["blobs"].shape == (96, 80, 72)
    counts = {}
    for name in ("random", "blobs", "snake", "snake_leak"):
        _, stats, info = R.fill_holes(volumes[name], 5)
        counts[name] = (info["cavities"], info["ties"], info["multi"], int(stats[0, 1]))
    assert counts["random"] == (3235, 1002, 3233, 7886)
    assert counts["blobs"] == (2081, 181, 1877, 8798) and int((volumes["blobs"] == 0).sum()) - 8798 == 104524       # the open background
    assert counts["snake"] == (1, 0, 1, 16127) and counts["snake_leak"] == (0, 0, 0, 0)
    for name in ("random", "blobs"):
        assert counts[name][0] >= 100 and counts[name][1] >= 10 and counts[name][2] >= 100


@pytest.mark.parametrize("ncls", [5, 2, 8])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_equals_scipy(volumes, name, ncls):
    """with no mask and max_size = 0 the filled voxels are binary_fill_holes(vol > 0) & background, the cavities are the scipy.ndimage.label
    components of the background that touch no face, only background is rewritten, and every rewritten voxel takes a class that touches
    its cavity"""
    ndimage = pytest.importorskip("scipy.ndimage")
    v = np.where(volumes[name] < ncls, volumes[name], 0).astype(np.uint8)
    out, stats, info = R.fill_holes(volumes[name], ncls)
    bg = v == 0
    assert np.array_equal((out != 0) & bg, ndimage.binary_fill_holes(v > 0) & bg)
    assert np.array_equal(out[~bg], v[~bg])
    lab, nl = ndimage.label(bg)                          # the default structure: 6 neighbours
    face = np.ones(v.shape, dtype=bool)
    face[tuple(slice(1, -1) for _ in range(3))] = False
    closed = np.setdiff1d(np.arange(1, nl + 1), np.unique(lab[face]))
    assert info["cavities"] == len(closed) == stats[0, 0] and stats[0, 2] == 0 and stats[0, 3] == 0
    idx = np.arange(v.size).reshape(v.shape)
    if len(closed):
        mins = np.asarray(ndimage.minimum(idx, lab, closed)).astype(np.int64)
        sizes = np.bincount(lab.reshape(-1), minlength=nl + 1)[closed]
        assert np.array_equal(mins, info["root"]) and np.array_equal(sizes, info["size"])
        assert stats[0, 1] == sizes.sum() == int(((out != 0) & bg).sum()) and stats[1:, 1].sum() == sizes.sum()
        assert stats[1:, 2].max() == sizes.max()
        for k in np.linspace(0, len(closed) - 1, min(len(closed), 25)).astype(int):       # the winner by hand, on a sample
            cav = lab == closed[k]
            ring = ndimage.binary_dilation(cav) & ~cav
            assert not bg[ring].any()
            cnt = np.zeros(ncls, dtype=np.int64)
            for ax in range(3):
                for sh in (1, -1):
                    nb = np.roll(v, sh, axis=ax)         # a cavity touches no face: nothing wraps into it
                    cnt += np.bincount(nb[cav], minlength=ncls)
            assert info["winner"][k] == 1 + int(np.argmax(cnt[1:])) and (out[cav] == info["winner"][k]).all()
    else:
        assert np.array_equal(out, v) and not stats.any()


def test_restatement_options(volumes):
    v = volumes["sizes"]
    out, stats, _ = R.fill_holes(v, 5, max_size=8)
    assert stats.tolist() == [[4, 100, 2, 91], [2, 9, 8, 2], [0] * 4, [0] * 4, [0] * 4]
    assert out[2, 2, 2] == 1 and out[4, 4, 4] == 1 and out[10, 10, 10] == 0 and out[14, 14, 30] == 0
    out, stats, _ = R.fill_holes(volumes["vote"], 5, classes=[2])              # the runner-up never inherits the cavity
    assert out[8, 8, 32] == 0 and stats[0].tolist() == [1, 1, 1, 1] and stats[3].tolist() == [0, 0, 0, 1] and not stats[2].any()
    out, stats, _ = R.fill_holes(volumes["tie"], 5)
    assert out[16, 8, 31] == 2
    out, _, _ = R.fill_holes(volumes["high"], 5)
    assert out[13, 13, 23] == 1 and out[0, 0, 0] == 0 and out.max() == 1
    out, stats, _ = R.fill_holes(volumes["pocket"], 5)                         # a class inside a class is anatomy
    assert np.array_equal(out, volumes["pocket"]) and not stats.any()


def _buffers():
    buf = ctypes.create_string_buffer((1 << 16) + 16)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)       # pnp_fill_holes wants a 16-byte aligned workspace


def test_workspace_query(built):
    lib = built._lib.load()
    q = lib.pnp_fill_holes_workspace_bytes
    r = lambda b: (b + 255) // 256 * 256
    want = lambda n, ncls: 2048 + 2 * r(4 * n) + r(n) + r(4 * n * (ncls - 1))
    assert q(1, 1, 1, 2) == 2048 + 4 * 256 and q(37, 29, 45, 5) == want(37 * 29 * 45, 5) and q(37, 29, 45, 8) == want(37 * 29 * 45, 8)
    assert q(256, 256, 200, 5) == 2048 + 25 * 256 * 256 * 200
    assert q(0, 4, 4, 5) == 0 and q(4, -1, 4, 5) == 0 and q(4, 4, 4097, 5) == 0 and q(4096, 4096, 128, 5) == 0
    assert q(4, 4, 4, 1) == 0 and q(4, 4, 4, 9) == 0
    assert q(4096, 4096, 127, 8) == want(4096 * 4096 * 127, 8) > 1 << 35


def test_every_host_refusal_by_its_text(built):
    """decided on the host before any HIP call: the tensors are small host buffers that are never read, and there is no GPU here"""
    lib = built._lib.load()
    buf, p = _buffers()
    need = int(lib.pnp_fill_holes_workspace_bytes(4, 5, 6, 5))

    def fill(vol=p, D=(4, 5, 6), ncls=5, mask=0b11110, max_size=0, out=p, stats=p, ws=p, wsb=need):
        return lib.pnp_fill_holes(vol, D[0], D[1], D[2], ncls, mask, max_size, out, stats, ws, wsb, None)

    def refused(rc, text):
        msg = lib.pnp_last_error()
        assert rc == -1 and text in msg, (rc, msg)

    for kw in ({"vol": None}, {"out": None}, {"stats": None}, {"ws": None}):
        refused(fill(**kw), b"pnp_fill_holes: null pointer")
    for D in ((0, 5, 6), (4, 4097, 6), (4, 5, -1)):
        refused(fill(D=D, wsb=1 << 40), b"pnp_fill_holes: extents")
    refused(fill(D=(4096, 4096, 128), wsb=1 << 40), b"pnp_fill_holes: 4096 x 4096 x 128 = 2147483648 voxels, fewer than 2^31")
    for ncls in (1, 9, 0, -3):
        refused(fill(ncls=ncls), b"pnp_fill_holes: ncls")
    for ncls, mask in ((5, 0b00001), (5, 0b100000), (5, 0b111111), (2, 0b100), (8, 1 << 8)):
        refused(fill(ncls=ncls, mask=mask), b"pnp_fill_holes: class_mask")
    refused(fill(max_size=-1), b"pnp_fill_holes: max_size")
    refused(fill(wsb=need - 1), b"pnp_fill_holes: workspace too small")
    refused(fill(wsb=0), b"pnp_fill_holes: workspace too small")
    need8 = int(lib.pnp_fill_holes_workspace_bytes(4, 5, 6, 8))
    assert need8 > need
    refused(fill(ncls=8, mask=0b10, wsb=need), b"pnp_fill_holes: workspace too small")        # the query depends on ncls


def test_python_wrappers_refuse_on_the_host(built):
    import torch
    C = pkg("components")
    cpu = torch.zeros((3, 4, 5), dtype=torch.uint8)
    with pytest.raises(built._lib.PnpError, match="no CPU fallback"):
        C.fill_holes(cpu)
    with pytest.raises(ValueError, match="torch tensor"):
        C.fill_holes(np.zeros((3, 4, 5), np.uint8))
    for kw, text in (({"max_size": -1}, "max_size = -1 is negative"), ({"max_size": 1.0}, "max_size must be an int"),
                     ({"max_size": True}, "max_size must be an int"), ({"classes": [0]}, "classes"), ({"classes": [5]}, "classes")):
        with pytest.raises(ValueError, match=text):
            C.check_fill_options(5, **kw)
    with pytest.raises(ValueError, match="num_cls"):
        C.check_fill_options(9)
    assert C.check_fill_options(5) == (0, 0b11110) and C.check_fill_options(5, np.int64(7), (1, 3)) == (7, 0b01010)
    assert C.OPTION_KEYS == ("keep", "min_size", "connectivity", "classes") and C.FILL_OPTION_KEYS == ("max_size", "classes")
    assert C.fill_stats_line([[2, 9, 1, 8], [1, 1, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]]) == \
        "2 cavities, 9 voxels, left 1 / 8   class 1: 1 filled, 1 voxels, largest 1, left 0   class 2: 0 filled, 0 voxels, largest 0, left 1"


def test_parse_fill_option(built):
    C = pkg("components")
    assert C.parse_fill_option(None) is None and C.parse_fill_option(False) is None
    assert C.parse_fill_option(True) == {} and C.parse_fill_option(12) == {"max_size": 12} and C.parse_fill_option(np.int64(3)) == {"max_size": 3}
    given = {"max_size": 10, "classes": [1, 2]}
    got = C.parse_fill_option(given)
    assert got == given and got is not given
    assert C.parse_fill_option({}) == {} and C.parse_fill_option({"classes": [1]}, 2) == {"classes": [1]}
    for bad, text in (("1", "must be None, a bool, a positive int or a dict"), (1.0, "must be None, a bool"), ([1], "must be None, a bool"),
                      (0, "no positive size limit"), (-4, "no positive size limit"), ({"size": 3}, "unknown keys"),
                      ({"max_size": -2}, "max_size = -2 is negative"), ({"max_size": 2.5}, "max_size must be an int"),
                      ({"classes": [7]}, "classes"), ({"classes": [0]}, "classes"), ({"keep": 1}, "unknown keys")):
        with pytest.raises(ValueError, match=text):
            C.parse_fill_option(bad)
    with pytest.raises(ValueError, match="classes"):
        C.parse_fill_option({"classes": [3]}, 3)
    assert C.parse_option(2) == {"keep": 2}                                              # keep_largest's parser is as it was
    with pytest.raises(ValueError, match="unknown keys"):
        C.parse_option({"max_size": 3})


def test_segment_volume_checks_fill_holes_before_any_gpu_work(built):
    vp = pkg("volume_predict")
    image = np.zeros((8, 8, 4), np.int16)
    never = lambda x: pytest.fail("the network must not run")
    for bad, text in (("1", "fill_holes must be None"), (1.5, "fill_holes must be None"), (0, "no positive size limit"), (-1, "no positive size limit"),
                      ({"size": 3}, "unknown keys"), ({"max_size": -5}, "max_size"), ({"classes": [7]}, "classes")):
        with pytest.raises(ValueError, match=text):
            vp.segment_volume(never, image, fill_holes=bad, device="cuda")
        with pytest.raises(ValueError, match=text):
            vp.segment_volume(never, image, fill_holes=bad, axes=(0, 1, 2), device="cuda")
    ev = pkg("evaluate")
    with pytest.raises(ValueError, match="no positive size limit"):
        ev.evaluate([], fill_holes=-3, device="cpu")
    import inspect
    names = list(inspect.signature(vp.segment_volume).parameters)
    assert names[-2:] == ["fill_holes", "hole_stats"], "the new keywords are appended after the existing ones"
    assert list(inspect.signature(ev.evaluate).parameters)[-1] == "fill_holes"


def test_command_line_argument_errors(built, tmp_path, capsys):
    pr, ev, nifti = pkg("predict"), pkg("evaluate"), pkg("nifti")
    img, ck = str(tmp_path / "a.nii.gz"), str(tmp_path / "ck.npz")
    nifti.save(nifti.Nifti1Image(np.zeros((4, 4, 3), np.int16), np.eye(4)), img)
    np.savez(ck, a=np.zeros(1))
    base = ["--model", ck, "--net", "segmenter", "--images", img, "--out", str(tmp_path / "o")]
    for extra, text in ((["--fill-holes", "-1"], "max_size = -1 is negative"), (["--fill-holes", "x"], "invalid int value"),
                        (["--fill-classes", "1,2"], "--fill-classes goes with --fill-holes"),
                        (["--fill-holes", "--fill-classes", "1,9"], "classes: 9 is no class"),
                        (["--fill-holes", "--fill-classes", "0"], "classes: 0 is no class"),
                        (["--fill-holes", "4", "--fill-classes", "a,b"], "no comma-separated list of ints")):
        with pytest.raises(SystemExit):
            pr.parse_args(base + extra)
        assert text in capsys.readouterr().err, extra
        with pytest.raises(SystemExit):
            ev.main(["--pred", img, "--gt", img] + extra)
        assert text in capsys.readouterr().err, extra
    _, _, _, opts = pr.parse_args(base)
    assert "fill_holes" not in opts and "hole_stats" not in opts                       # the default path is untouched
    _, _, _, opts = pr.parse_args(base + ["--fill-holes"])
    assert opts["fill_holes"] == {} and "keep_largest" not in opts
    _, _, _, opts = pr.parse_args(base + ["--fill-holes", "50", "--fill-classes", "1,3", "--keep-largest"])
    assert opts["fill_holes"] == {"max_size": 50, "classes": [1, 3]} and opts["keep_largest"] == {"keep": 1, "min_size": 0, "connectivity": 1}
    _, _, _, opts = pr.parse_args(base + ["--fill-holes", "0"])
    assert opts["fill_holes"] == {}
