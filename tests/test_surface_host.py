"""not gpu: the float64 surface-distance reference (tests/surface_ref.py) on known answers, and the binding of the surface-distance
entry points (csrc/surface.hip) without a GPU: symbols, workspace query, argument checks before any HIP call, input checks of surface.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import surface_ref as R
from conftest import pkg


# ---- reference known answers -----------------------------------------------------------------------------------------------------
def test_reference_single_voxels():
    a = np.zeros((8, 8, 4), np.int32)
    b = np.zeros_like(a)
    a[1, 1, 2] = 1
    b[4, 5, 2] = 1                                       # offset (3, 4, 0)
    m = R.metrics(a, b, 2)
    for k in ("asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95"):
        assert m[k][1] == 5.0, k
    m = R.metrics(a, b, 2, spacing=(2.0, 0.5, 1.0))
    for k in ("asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95"):
        assert math.isclose(m[k][1], math.sqrt(40.0), rel_tol=1e-15), k
    assert np.isnan(m["assd"][0]) and np.isnan(m["n_border_pred"][0])


def test_reference_nested_cubes():
    big = np.zeros((9, 9, 9), np.int32)
    small = np.zeros_like(big)
    big[2:7, 2:7, 2:7] = 1
    small[3:6, 3:6, 3:6] = 1
    m = R.metrics(small, big, 2)                       # prediction = the 3^3 cube
    assert (m["n_border_pred"][1], m["n_border_gt"][1]) == (26, 98)
    assert m["asd_pred_gt"][1] == 1.0
    assert math.isclose(m["asd_gt_pred"][1], (8 * math.sqrt(3) + 36 * math.sqrt(2) + 54) / 98, rel_tol=1e-14)
    assert math.isclose(m["hd"][1], math.sqrt(3), rel_tol=1e-15) and math.isclose(m["hd95"][1], math.sqrt(3), rel_tol=1e-15)


def test_reference_full_volume_border():
    assert R.border(np.ones((4, 4, 4), bool)).sum() == 56


def test_reference_matches_the_scipy_recipe():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    for trial in range(3):
        shape = (14, 11, 9)
        a = R.ellipsoids(shape, 2, 10 + trial) == 1
        b = R.ellipsoids(shape, 2, 20 + trial) == 1
        if not a.any() or not b.any():
            continue
        sp = tuple(rng.uniform(0.5, 2.0, 3))
        fp = nd.generate_binary_structure(3, 1)

        def recipe(x, y):
            bx = x ^ nd.binary_erosion(x, structure=fp, iterations=1)
            by = y ^ nd.binary_erosion(y, structure=fp, iterations=1)
            return nd.distance_transform_edt(~by, sampling=sp)[bx]
        assert np.array_equal(R.border(a), a ^ nd.binary_erosion(a, structure=fp, iterations=1))
        np.testing.assert_allclose(np.sort(R.sds(a, b, sp)), np.sort(recipe(a, b)), rtol=1e-12)
        mask = rng.random(shape) < 0.02
        np.testing.assert_allclose(R.edt_sq(mask, sp), nd.distance_transform_edt(~mask, sampling=sp) ** 2, rtol=1e-12)


# ---- binding without a GPU ---------------------------------------------------------------------------------------------------------
SYMS = ("pnp_edt3d_sq", "pnp_surface_workspace_bytes", "pnp_surface_distances")


def test_symbols_and_prototypes(built):
    lib = built._lib.load()
    for s in SYMS:
        assert hasattr(lib, s) and s in built._lib.PROTOTYPES, s
    assert built._lib.PROTOTYPES["pnp_surface_workspace_bytes"][0] is ctypes.c_size_t
    assert lib.pnp_abi_version() == 4


def test_workspace_query(built):
    lib = built._lib.load()
    ws = lib.pnp_surface_workspace_bytes
    base = ws(16, 16, 16, 5)
    assert base > 0
    assert ws(17, 16, 16, 5) > base and ws(16, 17, 16, 5) > base and ws(16, 16, 17, 5) > base
    assert ws(16, 16, 16, 2) < ws(16, 16, 16, 3) < base < ws(16, 16, 16, 32)
    assert ws(1025, 4, 4, 5) == 0 and ws(4, 4, 4, 1) == 0 and ws(4, 4, 4, 33) == 0


def _call(lib, X=8, Y=8, Z=8, ncls=5, sp=(1.0, 1.0, 1.0), ws_short=0):
    fake = ctypes.c_void_p(0x1000)              # never dereferenced: every check comes before the first HIP call
    need = lib.pnp_surface_workspace_bytes(8, 8, 8, 5)
    return lib.pnp_surface_distances(fake, fake, X, Y, Z, ncls, sp[0], sp[1], sp[2], fake, fake, need - ws_short, None)


def test_argument_checks_before_any_launch(built):
    lib = built._lib.load()
    cases = [(dict(X=1025), b"extents"), (dict(Z=0), b"extents"), (dict(ncls=1), b"ncls"), (dict(ncls=33), b"ncls"),
             (dict(sp=(1.0, 0.0, 1.0)), b"spacing"), (dict(sp=(1.0, 1.0, -2.0)), b"spacing"), (dict(sp=(float("nan"), 1.0, 1.0)), b"spacing"),
             (dict(ws_short=1), b"workspace")]
    for kw, word in cases:
        assert _call(lib, **kw) == -1, kw
        assert word in lib.pnp_last_error(), (kw, lib.pnp_last_error())
    fake = ctypes.c_void_p(0x1000)
    assert lib.pnp_surface_distances(None, fake, 8, 8, 8, 5, 1.0, 1.0, 1.0, fake, fake, 1 << 30, None) == -1
    assert b"null" in lib.pnp_last_error()
    assert lib.pnp_edt3d_sq(fake, fake, 2000, 2, 2, 1.0, 1.0, 1.0, None) == -1 and b"extents" in lib.pnp_last_error()
    assert lib.pnp_edt3d_sq(fake, fake, 2, 2, 2, 1.0, float("inf"), 1.0, None) == -1 and b"spacing" in lib.pnp_last_error()
    assert lib.pnp_edt3d_sq(None, fake, 2, 2, 2, 1.0, 1.0, 1.0, None) == -1 and b"null" in lib.pnp_last_error()


def test_cpu_tensors_raise(built):
    S, K = pkg("surface"), pkg("kernels")
    t = torch.zeros((4, 4, 4), dtype=torch.int32)
    with pytest.raises(built._lib.PnpError):
        S.surface_metrics(t, t, 5)
    with pytest.raises(built._lib.PnpError):
        K.surface_distances(t, t, 5)
    with pytest.raises(built._lib.PnpError):
        K.edt_sq(torch.zeros((4, 4, 4), dtype=torch.uint8))


def test_non_integer_labels_raise(built):
    S = pkg("surface")
    a = np.zeros((4, 4, 4))
    b = a.copy()
    b[1, 1, 1] = 0.5
    with pytest.raises(ValueError):
        S.surface_metrics(a, b, 5)
    with pytest.raises(ValueError):
        S.surface_metrics(np.full((4, 4, 4), np.nan), a, 5)
    with pytest.raises(ValueError):
        S.asd(a, a, connectivity=2)


def test_spacing_of():
    S = pkg("surface")
    assert S.spacing_of(np.diag([1.25, 1.25, 2.0, 1.0])) == (1.25, 1.25, 2.0)
    rot = np.array([[0.0, -2.0, 0.0, 5.0], [1.5, 0.0, 0.0, 1.0], [0.0, 0.0, 3.0, 0.0], [0, 0, 0, 1.0]])
    assert S.spacing_of(rot) == (1.5, 2.0, 3.0)


def test_rows_to_metrics_bookkeeping():
    S = pkg("surface")
    nan = float("nan")
    rows = np.array([[nan] * 7, [4, 2, 6.0, 3.0, 2.5, 1.75, 2.0], [3, 0, nan, nan, nan, nan, nan]])
    m = S.rows_to_metrics(rows)
    assert m["asd_pred_gt"][1] == 1.5 and m["asd_gt_pred"][1] == 1.5 and m["assd"][1] == 1.5
    assert m["hd"][1] == 2.5 and m["hd95"][1] == 2.0
    assert m["n_border_pred"][2] == 3 and m["n_border_gt"][2] == 0 and np.isnan(m["assd"][2]) and np.isnan(m["hd"][2])
    assert all(np.isnan(m[k][0]) for k in S.FIELDS)
