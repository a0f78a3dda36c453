"""-m gpu: foreground-aware slice sampling on the device: pnp_label_frame_stats against the numpy restatement
(tests/frame_stats_ref.py) — integer-exact, bit-equal from call to call, inside guard zones — its host refusals, VolumeSet.frame_stats,
and AugmentedSliceSource(sampling=) end to end: the two end-to-end tests cannot pass without the feature."""
import ctypes
import time

import numpy as np
import pytest
import torch

import frame_stats_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 3), (3, 2, 5), (7, 5, 67), (5, 3, 130), (33, 17, 64), (16, 16, 257), (4096, 1, 3), (1, 4096, 4), (64, 64, 8)]
GUARD = 1024                    # int32 words on either side of the table
SENTINEL = -0x5A5A5A5B


def _labels(shape, ncls, seed, blocky):
    """labels from {0 .. ncls - 1, ncls, 200, 255}; class ncls - 1 (when there are three or more) is absent everywhere and class 1 (when
    there are two or more) lives in one voxel only; blocky: constant along stretches of y, so that a lane's walk meets runs"""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    values = np.array(list(range(ncls)) + [ncls, 200, 255], dtype=np.uint8)
    if blocky:
        lab = np.repeat(rng.choice(values, size=(X, -(-Y // 5), Z)), 5, axis=1)[:, :Y, :]
    else:
        lab = rng.choice(values, size=shape)
    lab = np.ascontiguousarray(lab)
    if ncls >= 3:
        lab[lab == ncls - 1] = 0
    if ncls >= 2:
        lab[lab == 1] = 0
        lab[tuple(int(rng.integers(n)) for n in shape)] = 1
    return lab


def _on_device(dev, lab, offset):
    """the label volume as buf[o:o + n].view(X, Y, Z): a base `offset` bytes past the allocation's (aligned) start"""
    buf = torch.empty(lab.size + offset + 16, dtype=torch.uint8, device=dev)
    t = buf[offset:offset + lab.size].view(lab.shape)
    t.copy_(torch.from_numpy(lab))
    assert t.data_ptr() % 16 == offset % 16 and t.is_contiguous()
    return t


def _kernel(dev, t, ncls):
    """the C entry point on a table inside a sentinel-filled buffer, twice -> the table (numpy); both guard zones intact, the second call
    bit-equal to the first"""
    K, L = pkg("kernels"), pkg("_lib")
    X, Y, Z = t.shape
    n = Z * ncls * 5
    outs = []
    for _ in range(2):
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        rc = L.load().pnp_label_frame_stats(ctypes.c_void_p(t.data_ptr()), X, Y, Z, ncls, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD), K._stream())
        assert rc == 0, L.load().pnp_last_error()
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "the kernel wrote outside its table"
        outs.append(host[GUARD:GUARD + n].reshape(Z, ncls, 5))
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_restatement(dev, shape):
    for i, ncls in enumerate((1, 2, 5, 8)):
        for blocky in (False, True):
            lab = _labels(shape, ncls, 10 * i + blocky, blocky)
            offset = (2 * i + blocky) % 4
            got = _kernel(dev, _on_device(dev, lab, offset), ncls)
            want = R.frame_stats(lab, ncls)
            assert got.dtype == want.dtype and np.array_equal(got, want), (shape, ncls, blocky, offset)
            if ncls >= 3:
                assert (got[:, ncls - 1] == (0, shape[0], -1, shape[1], -1)).all() and got[:, 1, 0].sum() == 1


@pytest.mark.parametrize("shape", [(7, 5, 67), (5, 3, 130), (33, 17, 64), (16, 16, 257), (1, 4096, 4), (64, 64, 8)], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_bases(dev, shape):
    """every base offset of the issue (0 .. 3: the widest load the extents allow, then byte loads) and the ones that select the 4- and
    8-byte loads of a Z that allows 16"""
    lab = _labels(shape, 5, 3, True)
    want = R.frame_stats(lab, 5)
    for offset in (0, 1, 2, 3, 4, 8):
        assert np.array_equal(_kernel(dev, _on_device(dev, lab, offset), 5), want), (shape, offset)


def test_one_class_everywhere(dev):
    """the contention case: every voxel adds to the same ncls entries of its frame"""
    for c, ncls in ((0, 1), (3, 5), (7, 8)):
        lab = np.full((64, 64, 8), c, dtype=np.uint8)
        got = _kernel(dev, _on_device(dev, lab, 0), ncls)
        assert np.array_equal(got, R.frame_stats(lab, ncls)) and (got[:, c] == (4096, 0, 63, 0, 63)).all()


def test_binding(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lab = _labels((7, 5, 67), 5, 1, False)
    got = K.label_frame_stats(_on_device(dev, lab, 3), 5)
    assert got.dtype == torch.int32 and tuple(got.shape) == (67, 5, 5) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), R.frame_stats(lab, 5))
    with pytest.raises(L.PnpError):
        K.label_frame_stats(torch.from_numpy(lab), 5)                       # a CPU tensor: no fallback
    with pytest.raises(L.PnpError):
        K.label_frame_stats(_on_device(dev, lab, 0).permute(1, 0, 2), 5)    # not contiguous
    with pytest.raises(L.PnpError):
        K.label_frame_stats(_on_device(dev, lab, 0), 9)


def test_host_refusals(built):
    """every argument class is refused with its message before any HIP call: the pointers are host dummies, a launch would fault"""
    lib = built._lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)
    odd = ctypes.c_void_p(p.value + 2)
    for args, text in (((None, 4, 4, 4, 5, p), b"null pointer"), ((p, 4, 4, 4, 5, None), b"null pointer"),
                       ((p, 0, 4, 4, 5, p), b"outside [1, 4096]"), ((p, 4097, 4, 4, 5, p), b"outside [1, 4096]"),
                       ((p, 4, 0, 4, 5, p), b"outside [1, 4096]"), ((p, 4, 4097, 4, 5, p), b"outside [1, 4096]"),
                       ((p, 4, 4, 0, 5, p), b"Z = 0 must be at least 1"), ((p, 4, 4, -3, 5, p), b"must be at least 1"),
                       ((p, 4096, 4096, 128, 5, p), b"not below 2^31"), ((p, 1, 1, 2 ** 31 - 1, 0, p), b"ncls = 0 outside [1, 8]"),
                       ((p, 4, 4, 4, 9, p), b"ncls = 9 outside [1, 8]"), ((p, 4, 4, 4, 5, odd), b"4-byte aligned")):
        rc = lib.pnp_label_frame_stats(*(args + (None,)))
        assert rc == -1 and b"pnp_label_frame_stats" in lib.pnp_last_error() and text in lib.pnp_last_error(), (args[1:5], lib.pnp_last_error())


def _image(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_end_to_end_frames(dev):
    vs = pkg("volume_source")
    lab = np.zeros((24, 20, 9), dtype=np.uint8)
    lab[6:14, 5:12, 4:6] = 1
    lab[15:20, 2:6, 2] = 2
    vol = vs.VolumeSet.from_arrays([_image(lab.shape, 0)], [lab], ["box"], dev)
    kw = dict(out_size=(24, 20), augment=None, num_cls=3, seed=4)
    src = vs.AugmentedSliceSource(vol, 16, sampling={"foreground": 1.0}, **kw)
    frames, classes = [], []
    for _ in range(4):
        batch, fids = src.next_batch()
        assert batch.shape == (16, 24, 20, 4)
        for sl, fid, c in zip(batch, fids, src.last_draw["fg_class"]):
            z = int(fid.split("#")[1])
            assert fid.startswith("box#") and z in (2, 4, 5) and c in (1, 2) and (sl[:, :, 3] == c).any(), (fid, c)
            assert np.array_equal(sl[:, :, 3], lab[:, :, z])                 # augment=None at the volume's own extents: the frame itself
            frames.append(z)
            classes.append(int(c))
    assert src.errors() == 0 and set(frames) == {2, 4, 5}
    rep = src.sampling_report()
    assert rep == {"samples": 64, "foreground": {1: classes.count(1), 2: classes.count(2)}, "fallback": 0}
    assert rep["foreground"][1] + rep["foreground"][2] == 64 and min(rep["foreground"].values()) > 0
    plain = vs.AugmentedSliceSource(vol, 16, **kw)
    other = [int(f.split("#")[1]) for _ in range(4) for f in plain.next_batch()[1]]
    assert any(z not in (2, 4, 5) for z in other) and plain.errors() == 0
    assert plain.sampling_report() == {"samples": 64, "foreground": {}, "fallback": 0}


def test_end_to_end_centre(dev):
    """a 16 mm plane in the middle of a 64 mm slice misses a box near its edge; centred on the class it holds all of it"""
    vs = pkg("volume_source")
    lab = np.zeros((64, 64, 5), dtype=np.uint8)
    lab[4:10, 50:56, 1:4] = 1
    vol = vs.VolumeSet.from_arrays([_image(lab.shape, 1)], [lab], ["edge"], dev, spacings=[(1.0, 1.0, 1.0)])
    kw = dict(out_size=(16, 16), augment=None, sample_mm=1.0, seed=0)
    plain = vs.AugmentedSliceSource(vol, 8, **kw)
    assert not plain.next_batch()[0][..., 3].any() and "_frame_stats" not in vol.__dict__       # without the option no table is ever built
    src = vs.AugmentedSliceSource(vol, 8, sampling={"foreground": 1.0, "centre": True}, **kw)
    for _ in range(3):
        assert not plain.next_batch()[0][..., 3].any()
        batch, _ = src.next_batch()
        assert ((batch[..., 3] == 1).sum(axis=(1, 2)) == 36).all() and (batch[..., 3] <= 1).all()
        assert np.array_equal(src.last_draw["centre"], np.tile([[6.5 - 31.5, 52.5 - 31.5]], (8, 1)))
    assert src.errors() == 0 and plain.errors() == 0 and src.sampling_report()["foreground"] == {1: 24, 2: 0, 3: 0, 4: 0}


def test_frame_stats_of_a_multi_planar_set(dev):
    """one scan held on two slicing axes (from_arrays with the transposed copy, as VolumeSet(axis=(2, 1)) holds it): every entry's table
    is the restatement of that entry's own array; one host copy for the set, cached per num_cls; from_device sets are served too"""
    vs = pkg("volume_source")
    lab = _labels((12, 10, 16), 5, 7, True)
    arrays = [lab, np.ascontiguousarray(np.moveaxis(lab, 1, -1))]
    vol = vs.VolumeSet.from_arrays([_image(a.shape, 2) for a in arrays], arrays, ["scan@2", "scan@1"], dev)
    tabs = vol.frame_stats(5)
    assert len(tabs) == 2 and [t.shape for t in tabs] == [(16, 5, 5), (10, 5, 5)] and all(t.dtype == np.int32 for t in tabs)
    for t, a in zip(tabs, arrays):
        assert np.array_equal(t, R.frame_stats(a, 5))
    assert vol.frame_stats(5) is tabs and vol.frame_stats(3) is not tabs
    assert all(np.array_equal(t, R.frame_stats(a, 3)) for t, a in zip(vol.frame_stats(3), arrays))
    again = vs.VolumeSet.from_device(vol.images, vol.labels, vol.names, [0.0, 0.0])
    assert all(np.array_equal(t, u) for t, u in zip(again.frame_stats(5), tabs))


def _torch_table(label, ncls):
    """the same table from torch ops on the device: a one-hot mask per class plus reductions"""
    X, Y, Z = label.shape
    xs = torch.arange(X, device=label.device, dtype=torch.int32).view(X, 1)
    ys = torch.arange(Y, device=label.device, dtype=torch.int32).view(Y, 1)
    rows = []
    for c in range(ncls):
        m = label == c
        ax, ay = m.any(dim=1), m.any(dim=0)
        rows.append(torch.stack([m.sum(dim=(0, 1)).to(torch.int32), torch.where(ax, xs, X).amin(dim=0), torch.where(ax, xs, -1).amax(dim=0),
                                 torch.where(ay, ys, Y).amin(dim=0), torch.where(ay, ys, -1).amax(dim=0)], dim=-1))
    return torch.stack(rows, dim=1).to(torch.int32)


def test_a_realistic_volume_and_its_time(dev):
    """256 x 256 x 200, five classes in blobs (a coarse random field, upsampled) plus a sprinkle of labels outside the classes.  The two
    times are printed, not asserted."""
    K = pkg("kernels")
    rng = np.random.default_rng(0)
    coarse = rng.choice(np.arange(5, dtype=np.uint8), size=(16, 16, 10), p=[0.6, 0.1, 0.1, 0.1, 0.1])
    lab = np.ascontiguousarray(np.repeat(np.repeat(np.repeat(coarse, 16, axis=0), 16, axis=1), 20, axis=2))
    lab[rng.random(lab.shape) < 0.001] = 9
    t = torch.from_numpy(lab).to(dev)
    got = K.label_frame_stats(t, 5)
    assert np.array_equal(got.cpu().numpy(), R.frame_stats(lab, 5))
    assert torch.equal(_torch_table(t, 5), got)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 20 * 1e6
    print("pnp_label_frame_stats 256x256x200, 5 classes: %.1f us per call; the same table from torch ops: %.1f us"
          % (timed(lambda: K.label_frame_stats(t, 5)), timed(lambda: _torch_table(t, 5))))
