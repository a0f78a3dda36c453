"""not gpu: the host plan of a volume prediction (volume_predict.parse_request / plan_view / plan_views) against independently stated
values, at the smallest shapes that reach each branch: a 40 x 36 x 5 scan of 0.5 mm voxels under 16 x 16 planes of 1 mm (20 x 18 mm against
16 mm: two planes per axis, centred +-2 mm and +-1 mm from the box's centre, overlapping by 12 and 14 pixels) for the tile branches, an
8 x 8 x 4 image for the rest."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg

XYZ, SP, HW = (40, 36, 5), (0.5, 0.5, 2.0), (16, 16)
GEOM = dict(spacing_xy=(0.5, 0.5), pixel_mm=(1.0, 1.0))
OFFSETS = ((-2.0, -1.0), (-2.0, 1.0), (2.0, -1.0), (2.0, 1.0))          # tile-major: i outer, j inner
SMALL = (8, 8, 4)


def _whole(shape, flip=True, axis=2):
    return tuple((0, n) for n in pkg("volume_predict").file_layout(shape, flip, axis)[2])


def _plan(shape=SMALL, n_callables=None, axis=2, box=None, spacing=None, **options):
    vp = pkg("volume_predict")
    req = vp.parse_request(n_callables, axis=axis, spacing=spacing, **options)
    return vp.plan_view(req, shape, axis, _whole(shape, req.flip_correction, axis) if box is None else box, spacing)


def _tiled(n_callables=2, tiles=(2, 2), **more):
    return _plan(XYZ, n_callables, spacing=SP, sample_mm=1.0, out_size=HW, tiles=tiles, tta=[{}, {"flip": True}], batch_size=3, **more)


def test_member_order_is_callable_major_then_tile_then_view():
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    p = _tiled()
    assert p.counts == (2, 2) and p.ramp == 12.0 and tuple(p.offsets) == OFFSETS
    assert len(p.maps) == 8 and len(p.invs) == 16 and p.members == 16 and p.kind == "tiles" and p.fov
    assert p.logits_bytes == 16 * 4 * 3 * 16 * 16 * 5                     # members x 4 B H W num_cls
    for c in range(2):
        for t, (ti, tj) in enumerate(OFFSETS):
            for v, flip in enumerate((False, True)):
                m = vs.compose_matrix((40, 36), HW, translate=(ti, tj), flip=flip, **GEOM)
                assert m.dtype == p.maps[t * 2 + v].dtype == np.float32 and np.array_equal(p.maps[t * 2 + v], m)
                k = c * 8 + t * 2 + v
                assert p.invs[k].dtype == np.float32 and np.array_equal(p.invs[k], vp.invert_matrix(m)), k
    # a tta translate is in millimetres and adds to the tile's offset
    q = _plan(XYZ, spacing=SP, sample_mm=1.0, out_size=HW, tiles=(2, 2), tta=[{"translate": (0.5, -0.25)}])
    assert [e["translate"] for e in q.entries] == [(ti + 0.5, tj - 0.25) for ti, tj in OFFSETS]
    assert np.array_equal(q.maps[3], vs.compose_matrix((40, 36), HW, translate=(2.5, 0.75), **GEOM))
    # "auto" counts the same planes for this scan
    a = _tiled(tiles="auto")
    assert a.counts == (2, 2) and all(np.array_equal(x, y) for x, y in zip(a.invs, p.invs))


@pytest.mark.parametrize("edge,mm,frames,padded", [("replicate", None, (1, 4, -1), True), ("skip", None, (1, 2, 0), False),
                                                   ("replicate", (1.0, 1.0, 2.0), (0, 4, 0), False), ("skip", (1.0, 1.0, 2.0), (1, 2, 0), False)])
def test_frame_schedule_and_padding(edge, mm, frames, padded):
    vs = pkg("volume_source")
    p = _plan(edge=edge, sample_mm=mm, spacing=None if mm is None else (1.0, 1.0, 0.5))
    assert p.frames == frames and p.padded is padded and p.min_frames == (3 if mm is None else 1)
    assert p.rec_dtype == (vs.SAMPLE_DTYPE if mm is None else vs.SAMPLE_Z_DTYPE)
    if mm is None:
        assert p.dz is None and p.vox is None and p.geom == {} and not p.fov and p.coverage is None
    else:
        assert p.dz == np.float32(4.0) and type(p.dz) is np.float32 and p.vox == (1.0, 1.0, 0.5)
        assert p.geom == {"spacing_xy": (1.0, 1.0), "pixel_mm": (1.0, 1.0)} and p.fov


def test_kind_follows_the_options():
    assert _plan().kind == "labels" and not _plan().request.ensemble and _plan().members == 1 and len(_plan().maps) == 1
    for options in (dict(n_callables=1), dict(n_callables=2), dict(tta=[{}]), dict(tta="default"), dict(prob=True), dict(entropy=True)):
        p = _plan(**options)
        assert p.kind == "ensemble" and p.request.ensemble, options
    assert _plan(n_callables=2, tta=[{}, {"rotate": 5.0}]).members == 4
    assert _plan(tiles="auto", sample_mm=1.0, spacing=(1, 1, 1)).kind == "tiles"
    assert _plan(axes=(0, 2), axis=2).kind == "ensemble"                   # every view of a fused prediction returns probabilities


def test_coverage_is_the_share_the_paste_writes():
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    tiled = _tiled(1)
    assert tiled.coverage == 1.0 == vp.coverage(tiled.invs, 40, 36, 16, 16, mode="any")
    single = _plan(XYZ, spacing=SP, sample_mm=1.0, out_size=HW, tta=[{}, {"rotate": 10.0}])
    assert single.coverage == vp.coverage(single.invs, 40, 36, 16, 16, mode="all") and 0.5 < single.coverage < 1.0
    assert single.coverage < vp.coverage(single.invs, 40, 36, 16, 16, mode="any")            # the two modes differ here
    one = _plan(XYZ, spacing=SP, sample_mm=1.0, out_size=HW)
    inv = vp.invert_matrix(vs.compose_matrix((40, 36), HW, **GEOM))
    x, y = np.arange(40.0)[:, None], np.arange(36.0)[None, :]
    pi, pj = inv[0] * x + inv[1] * y + inv[2], inv[3] * x + inv[4] * y + inv[5]
    inside = (pi >= -0.5) & (pi <= 15.5) & (pj >= -0.5) & (pj <= 15.5)
    assert one.coverage == inside.mean() and 0.5 < one.coverage < 1.0


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("boxed", [False, True])
def test_layout_is_file_layouts(axis, flip, boxed):
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    shape = (5, 6, 7)
    dims = vp.file_layout(shape, flip, axis)[2]
    box = tuple((1, n - 1 - k) for k, n in enumerate(dims)) if boxed else None
    p = _plan(shape, axis=axis, flip_correction=flip, box=box)
    assert (p.origin, p.strides, p.dims) == vp.file_layout(shape, flip, axis, box) and p.box == (box or _whole(shape, flip, axis)) and p.axis == axis
    # and against the array prepare_pair builds: voxel (x, y, z) of the box lies at origin + x sx + y sy + z sz
    file = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    img = vs.prepare_pair(file, np.zeros(shape, np.uint8), flip, axis, None)[0][tuple(slice(a, b) for a, b in p.box)]
    g = np.meshgrid(*[np.arange(n) for n in p.dims], indexing="ij")
    assert np.array_equal(file.ravel()[p.origin + sum(s * i for s, i in zip(p.strides, g))], img)


def test_views_get_the_box_in_their_own_order():
    vp = pkg("volume_predict")
    shape, box = (9, 10, 11), ((1, 8), (2, 9), (3, 7))
    req = vp.parse_request(axes=(0, 1, 2), axis_weights=(1, 2, 3), edge="skip")
    plans = vp.plan_views(req, shape, box, None)
    assert [p.axis for p in plans] == [0, 1, 2] and req.axis_weights == (1.0, 2.0, 3.0)
    for p, a in zip(plans, (0, 1, 2)):
        assert p.box == vp.view_box(box, a) and (p.origin, p.strides, p.dims) == vp.file_layout(shape, True, a, vp.view_box(box, a))
    assert [p.dims for p in plans] == [(7, 4, 7), (7, 4, 7), (7, 7, 4)] and [p.frames for p in plans] == [(1, 5, 0), (1, 5, 0), (1, 2, 0)]
    # one axis: the box is in that axis's own order already
    one = vp.parse_request(axis=0)
    assert [p.box for p in vp.plan_views(one, shape, ((0, 10), (0, 11), (0, 9)), None)] == [((0, 10), (0, 11), (0, 9))]


def test_errors_need_no_device():
    vp = pkg("volume_predict")
    mm = dict(spacing=SP, sample_mm=1.0, out_size=HW)
    with pytest.raises(ValueError, match="cannot cover"):
        _plan(XYZ, tiles=(1, 2), **mm)
    with pytest.raises(ValueError, match=r"4 callables x 3 x 3 tiles x 2 tta entries = 72 members, at most 64"):
        _plan(XYZ, 4, tiles=(3, 3), tta=[{}, {"flip": True}], **mm)
    with pytest.raises(ValueError, match="13 callables x 5 tta entries = 65 members, at most 64"):
        vp.parse_request(13, tiles="auto", tta="default", sample_mm=1.0, spacing=(1, 1, 1))
    with pytest.raises(ValueError, match="2 callables x 5 tta entries = 10 members, at most 8"):
        vp.parse_request(2, tta="default")
    with pytest.raises(ValueError, match="edge='skip' needs at least 3 frames, the box has 2"):
        _plan(edge="skip", box=((0, 8), (0, 8), (1, 3)))
    with pytest.raises(ValueError, match="edge='skip' needs at least 3 frames"):
        _plan((8, 8, 2), edge="skip", sample_mm=1.0, spacing=(1, 1, 1))
    with pytest.raises(ValueError, match="an empty list has no member"):
        vp.parse_request(0)
    # the order of the request's errors: edge, keep_largest, fill_holes, crop, axes, batch size, sample_mm, prefilter, spacing, tiles, members
    bad = dict(edge="wrap", keep_largest=-1, fill_holes=0, crop="torso", axis_weights=(1,), batch_size=0, sample_mm=-1.0, prefilter="on",
               tiles=(0, 1), tta=[{"shear": 1}])
    for key, text in (("edge", "edge must be"), ("keep_largest", "is negative"), ("fill_holes", "no positive size"), ("crop", "body"),
                      ("axis_weights", "goes with axes"), ("batch_size", "at least 1"), ("sample_mm", "sample_mm must"), ("prefilter", "prefilter must"),
                      ("tiles", "tiles must"), ("tta", "unknown keys")):
        with pytest.raises(ValueError, match=text):
            vp.parse_request(**bad)
        del bad[key]
    assert not bad and not vp.parse_request().ensemble


def test_the_plan_is_immutable_and_carries_the_prefilter():
    vs = pkg("volume_source")
    p = _plan(XYZ, spacing=SP, sample_mm=(1.0, 1.0, 2.0), out_size=HW, prefilter="auto")
    assert p.sigmas == vs.prefilter_sigmas("auto", XYZ, HW, SP, (1.0, 1.0, 2.0)) == (0.5, 0.5, 0.0)
    assert [None if t is None else len(t) for t in p.taps] == [5, 5, None]
    assert _plan().sigmas is None and _plan().taps is None and _plan(prefilter=(0.0, 0.0, 0.0)).taps is None
    with pytest.raises(AttributeError):
        p.ramp = 2.0
    with pytest.raises(ValueError):
        p.invs[0][0] = 0.0
    with pytest.raises(ValueError):
        p.maps[0][0] = 0.0


def test_planning_touches_no_device():
    """a fresh interpreter plans a tiled, multi-planar prediction; the package imports torch (for its import order), so the statement is
    that nothing initialised the device"""
    code = ("import importlib, sys\n"
            "sys.path.insert(0, %r)\n"
            "vp = importlib.import_module(%r + '.volume_predict')\n"
            "req = vp.parse_request(2, axes=(0, 1, 2), sample_mm=1.0, spacing=(0.5, 0.5, 0.5), tiles='auto', out_size=(16, 16), prefilter='auto')\n"
            "plans = vp.plan_views(req, (40, 36, 20), ((0, 40), (0, 36), (0, 20)), (0.5, 0.5, 0.5))\n"
            "import torch\n"
            "assert len(plans) == 3 and not torch.cuda.is_initialized()\n"
            "print('planned', [p.counts for p in plans])\n" % (ROOT, PKG))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "planned [(2, 1), (2, 1), (2, 2)]" in r.stdout, r.stdout + r.stderr
