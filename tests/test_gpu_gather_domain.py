"""-m gpu: csrc/augment.hip where its stores and its grid change shape.  The cases are tests/volume_store_cases.py's.

  a  the one-hot interleave of store_group — 4 ncls floats of a group of four pixels across float4 stores — for EVERY ncls in 1 .. 32,
     on batches whose pixel count leaves a tail of 1, 2, 3 and 0 (groups cross row and sample borders), with labels up to and beyond
     ncls, through pnp_aug_slices and, for ncls in {2, 4, 7, 31}, pnp_aug_slices_z and pnp_aug_slices_warp (G = 0 and G = 2).  Exact: the
     one-hot output is augment_ref.onehot of the label output (and label_decomp's), image and label are bit for bit those of the call
     without a one-hot output, and every output lies between guards of 64 floats, all pre-filled with -7.0, that must stay untouched.
  b  pnp_volume_preprocess at the sizes where its grid changes — one block to two at 256 voxels, the cap of 1024 blocks at 262144 — and
     two voxels beyond twice the cap, at percentiles 0, 1, 50, 99, 100 (every percentile at 2, 3, 100 and 101 voxels), and on inputs
     whose radix keys differ in the lowest or in the highest byte only; under the checks of tests/test_gpu_augment.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import augment_ref as R
import volume_store_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = C.GUARD
U = 2.0 ** -24


def _guarded(dev, n, off=0):
    whole = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole, whole[GUARD + off:GUARD + off + n]


def _guards_intact(whole, inner):
    lo = (inner.data_ptr() - whole.data_ptr()) // 4
    return bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + inner.numel():] == SENTINEL).all())


# ---- a. the one-hot stores ---------------------------------------------------------------------------------------------------------------
ENTRIES = ("plain", "z", "warp_G0", "warp_G2")


def _volume_set(dev, ncls):
    vs = pkg("volume_source")
    img = (np.random.default_rng(ncls).standard_normal(C.ONEHOT_VOLUME) * 40 + 100).astype(np.float32)
    lab = C.onehot_label_volume(ncls)
    vset = vs.VolumeSet.from_device([torch.from_numpy(img).to(dev)], [torch.from_numpy(lab).to(dev)], ["v"], [float(img.min()) - 1.0], min_frames=1)
    return vset, lab


def _records(entry, B):
    """sample b: the identity, the map flipped along x, flipped along y, ... — integer coordinates, so the label is the voxel's"""
    vs = pkg("volume_source")
    X, Y, Z = C.ONEHOT_VOLUME
    maps = ([1, 0, 0, 0, 1, 0], [-1, 0, X - 1, 0, 1, 0], [1, 0, 0, 0, -1, Y - 1])
    rec = np.zeros(B, dtype={"plain": vs.SAMPLE_DTYPE, "z": vs.SAMPLE_Z_DTYPE}.get(entry, vs.SAMPLE_W_DTYPE))
    for b in range(B):
        rec["m"][b] = maps[b % 3]
        rec["frame"][b] = 1 if entry == "plain" else b % Z
        if entry != "plain":
            rec["dz"][b] = 0.5
        if entry.startswith("warp"):
            rec["gain"][b], rec["bias"][b], rec["noise"][b], rec["seed"][b] = 1.25, -0.5, 0.1, 17 + b
            rec["warp"][b] = int(entry == "warp_G2")
    return rec


def _gather(dev, entry, vset, rec, ctrl, B, H, W, ncls, want_onehot):
    """the library call itself, on guarded outputs -> (x, label, one-hot or None) after the guard checks"""
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    P = B * H * W
    xw, x = _guarded(dev, 3 * P)
    lw, label = _guarded(dev, P)
    ow, onehot = _guarded(dev, ncls * P) if want_onehot else (None, None)
    errors = torch.zeros(1, dtype=torch.int32, device=dev)
    sd = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    head = (ctypes.cast(vset.table_host, ctypes.c_void_p), vp(vset.table_dev), len(vset), vp(sd))
    tail = (B, H, W, vp(x), vp(label), vp(onehot), ncls, vp(errors), K._stream())
    if entry.startswith("warp"):
        G = 2 if entry == "warp_G2" else 0
        L.check(lib.pnp_aug_slices_warp(*head, vp(ctrl), G, *tail), "pnp_aug_slices_warp")
    else:
        name = "pnp_aug_slices" if entry == "plain" else "pnp_aug_slices_z"
        L.check(getattr(lib, name)(*head, *tail), name)
    torch.cuda.synchronize()
    assert int(errors.item()) == 0
    assert _guards_intact(xw, x) and _guards_intact(lw, label) and (onehot is None or _guards_intact(ow, onehot)), "a guard element was written"
    return x.view(B, H, W, 3), label.view(B, H, W), None if onehot is None else onehot.view(B, H, W, ncls)


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_hot_stores_for_every_class_count(dev, entry):
    K = pkg("kernels")
    for ncls in (C.ONEHOT_NCLS if entry == "plain" else C.ONEHOT_ENTRIES_NCLS):
        vset, lab = _volume_set(dev, ncls)
        for B, H, W in C.ONEHOT_SIZES:
            rec = _records(entry, B)
            ctrl = None
            if entry == "warp_G2":
                ctrl = torch.from_numpy(np.random.default_rng(B).uniform(-0.8, 0.8, (B, 5, 5, 2)).astype(np.float32)).to(dev)
            x, label, onehot = _gather(dev, entry, vset, rec, ctrl, B, H, W, ncls, True)
            x2, label2, none = _gather(dev, entry, vset, rec, ctrl, B, H, W, ncls, False)
            what = (entry, ncls, B, H, W)
            assert none is None and torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(label.view(torch.int32), label2.view(torch.int32)), what
            lg = label.cpu().numpy()
            assert np.array_equal(onehot.cpu().numpy(), R.onehot(lg, ncls)), what
            assert torch.equal(onehot, K.label_decomp(label.clone(), ncls)), what
            assert bool((x != SENTINEL).all()) and np.array_equal(lg, np.floor(lg)) and lg.min() >= 0 and lg.max() <= ncls + 1
            if entry != "warp_G2":                                           # integer coordinates: the label of the voxel itself
                for b in range(B):
                    sx, sy = R.coords(rec["m"][b], H, W)
                    assert np.array_equal(lg[b], R.gather_label(lab, int(rec["frame"][b]), sx, sy)), what
                if B * H * W >= 35:
                    assert lg.max() >= ncls and bool((onehot.sum(-1) == 0).any()), what          # labels beyond ncls: all-zero rows


# ---- b. pnp_volume_preprocess ------------------------------------------------------------------------------------------------------------
def _check_preprocess(dev, v, percentiles, what):
    """the checks of test_gpu_augment.py::test_preprocess_against_the_restatement, per percentile, on a guarded output"""
    K = pkg("kernels")
    vd = torch.from_numpy(v).to(dev)
    for pct in percentiles:
        ref, st = R.preprocess(v, pct)
        whole, out = _guarded(dev, v.size)
        o, stats = K.volume_preprocess(vd, pct, out=out)
        assert o is out
        out2, stats2 = K.volume_preprocess(vd, pct)
        got, s = out.cpu().numpy(), stats.cpu().numpy()
        assert _guards_intact(whole, out), (what, pct)
        assert torch.equal(vd.cpu(), torch.from_numpy(v))
        assert np.array_equal(got.view(np.uint32), out2.cpu().numpy().view(np.uint32)) and np.array_equal(s.view(np.uint64), stats2.cpu().numpy().view(np.uint64))
        k = R.clip_index(v.size, pct)
        assert s[0] == st["clip"] == np.partition(v, k)[k], (what, pct, s[0], st["clip"])
        scale = np.abs(np.minimum(v.astype(np.float64), st["clip"])).mean()
        assert abs(s[1] - st["mean"]) <= 1e-9 * scale and abs(s[1] - st["mean"]) <= 1e-9 * abs(st["mean"]), (what, pct, s[1], st["mean"])
        assert abs(s[2] - st["std"]) <= 1e-9 * st["std"], (what, pct, s[2], st["std"])
        if st["std"] == 0:
            assert s[2] == 0 and not got.any() and s[3] == 0
        assert np.abs(got - ref).max() <= 4 * U * max(1.0, np.abs(ref).max()), (what, pct)
        assert s[3] == got.min()


@pytest.mark.parametrize("n", C.PRE_SIZES)
def test_preprocess_where_the_grid_changes(dev, n):
    _check_preprocess(dev, C.pre_values(n), C.PRE_PERCENTILES, "n = %d" % n)


@pytest.mark.parametrize("n", C.PRE_SMALL)
def test_preprocess_every_percentile(dev, n):
    _check_preprocess(dev, C.pre_values(n), range(101), "n = %d" % n)


@pytest.mark.parametrize("kind", ["low_byte", "high_byte"])
def test_preprocess_keys_that_differ_in_one_byte(dev, kind):
    """the selection takes one byte of the key per round, the highest first: three rounds see a single bin, one sees them all"""
    for n in (4099, 262145):
        _check_preprocess(dev, C.pre_values(n, kind), C.PRE_PERCENTILES, "%s, n = %d" % (kind, n))
