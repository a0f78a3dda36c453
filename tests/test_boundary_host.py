"""CPU side of the boundary term: the exact restatement of tests/boundary_ref.py against scipy's Euclidean distance
transform and against torch autograd, the --bnd-weight / --bnd-ramp / --bnd-classes flags, the cost keys of Full_DRN, the epoch ramp of
the Trainer, and the four entry points of the C-ABI."""
import os
import re

import numpy as np
import pytest
import torch

from boundary_ref import boundary_ref, patterns, phi_ref
from conftest import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pnp_signed_distance_2d_workspace_bytes", "pnp_signed_distance_2d", "pnp_boundary_loss_workspace_bytes", "pnp_boundary_loss")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _scipy_phi(m):
    """one_hot2dist of the boundary-loss paper's code on one bool mask"""
    edt = pytest.importorskip("scipy.ndimage").distance_transform_edt
    return edt(~m) * ~m - (edt(m) - 1) * m


def test_restatement_equals_scipy_on_random_masks():
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    worst = 0.0
    for i in range(200):
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        dens = float(rng.uniform(0.02, 0.99))
        m = rng.random((H, W)) < dens
        phi, d2 = phi_ref(m[None, :, :, None].astype(np.float32), classes=[0])
        if not m.any() or m.all():
            assert not phi.any() and not d2.any()          # (scipy measures to an imaginary corner here; the term's rule is 0)
            continue
        ref = _scipy_phi(m)
        worst = max(worst, float(np.abs(phi[0, :, :, 0] - ref).max()))
        inside = np.where(m, (1.0 - ref) ** 2, ref ** 2)
        assert np.array_equal(np.rint(inside).astype(np.int64), d2[0, :, :, 0]), (i, H, W)
    assert worst == 0.0, worst


def test_restatement_full_empty_and_unselected_are_zero():
    rng = np.random.default_rng(1)
    oh = np.zeros((3, 9, 11, 4), np.float32)
    oh[0, :, :, 1] = 1                                     # class 1 fills slice 0, is absent from slice 1
    oh[1, :, :, 2] = 1
    oh[2, :, :, 1] = rng.random((9, 11)) < 0.4
    phi, d2 = phi_ref(oh)
    assert not phi[0, :, :, 1].any() and not phi[1, :, :, 1].any() and phi[2, :, :, 1].any()
    assert not phi[..., 0].any() and not d2[..., 0].any()   # the background is not selected by default
    assert not phi[..., 3].any()                            # absent everywhere
    phi_s, _ = phi_ref(oh, classes=[2])
    assert not phi_s[..., 1].any() and not phi_s[..., 2].any()      # class 2 is absent or full on every slice
    phi_e, _ = phi_ref(oh, classes=[])
    assert not phi_e.any()


def test_restatement_patterns_against_scipy():
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    for H, W in ((7, 9), (33, 65), (1, 7), (7, 1)):
        for name, m in patterns(H, W, rng).items():
            phi, _ = phi_ref(m[None, :, :, None].astype(np.float32), classes=[0])
            if not m.any() or m.all():
                assert not phi.any(), name
            else:
                assert np.array_equal(phi[0, :, :, 0], _scipy_phi(m)), (name, H, W)


def test_float32_sqrt_is_the_rounded_float64_root():
    """the kernel takes one sqrtf of an exact integer: every integer up to 2 * 1023^2"""
    n = np.arange(0, 2 * 1023 * 1023 + 1, dtype=np.int64)
    assert np.array_equal(np.sqrt(n.astype(np.float32)), np.sqrt(n.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("P,C,nsel", [(1, 5, 4), (7, 5, 4), (257, 2, 1), (257, 3, 2), (257, 8, 8), (64, 1, 1)])
def test_gradient_against_torch_float64_autograd(P, C, nsel):
    rng = np.random.default_rng(P * 10 + C)
    z = rng.standard_normal((P, C)) * 3.0
    if P > 4:
        z[0, 0] += 300.0
        z[3, C - 1] -= 400.0
    q = rng.uniform(-360.0, 360.0, (P, C))
    val, grad = boundary_ref(z, q, nsel)
    t = torch.from_numpy(z).requires_grad_(True)
    L = (torch.softmax(t, -1) * torch.from_numpy(q)).sum() / (P * nsel)
    L.backward()
    assert np.isfinite(val) and np.isfinite(grad).all()
    assert abs(val - float(L.detach())) <= 1e-13 * abs(float(L.detach())) + 1e-300
    assert float(np.abs(grad - t.grad.numpy()).max()) <= 1e-13 * float(np.abs(t.grad.numpy()).max()) + 1e-300
    v3, g3 = boundary_ref(z, q, nsel, coef=-0.375)
    assert v3 == val and np.array_equal(g3, -0.375 * grad)
    v0, g0 = boundary_ref(z, q, 0)
    assert v0 == 0.0 and not g0.any()


# ---- flags and keys ------------------------------------------------------------------------------------------------------------------------
REFERENCE_COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}


def test_bnd_flags_parsing():
    ts = pkg("train_segmenter")
    _, a = ts.parse_args([])
    assert a.bnd_weight == 0.0 and a.bnd_ramp is None and a.bnd_classes is None
    assert ts.cost_kwargs_from_args(a) == REFERENCE_COST                 # the default is the configuration of today
    _, a = ts.parse_args(["--bnd-weight", "0.01"])
    assert ts.cost_kwargs_from_args(a) == dict(REFERENCE_COST, bnd_weight=0.01)
    _, a = ts.parse_args(["--bnd-weight", "0.01", "--bnd-ramp", "3", "--bnd-classes", "1,3"])
    assert a.bnd_ramp == 3 and ts.cost_kwargs_from_args(a) == dict(REFERENCE_COST, bnd_weight=0.01, bnd_classes=(1, 3))
    assert all(f in ts.__doc__ for f in ("--bnd-weight", "--bnd-ramp", "--bnd-classes"))


@pytest.mark.parametrize("argv,word", [(["--bnd-weight", "-0.1"], "bnd-weight"), (["--bnd-weight", "1", "--bnd-ramp", "0"], "bnd-ramp"),
                                       (["--bnd-weight", "1", "--bnd-classes", "1,5"], "bnd-classes"),
                                       (["--bnd-weight", "1", "--bnd-classes", "a"], "bnd-classes"), (["--bnd-ramp", "2"], "bnd-weight"),
                                       (["--bnd-classes", "1"], "bnd-weight")])
def test_bad_bnd_flags_are_refused_on_the_command_line(capsys, argv, word):
    ts = pkg("train_segmenter")
    with pytest.raises(SystemExit):
        ts.parse_args(argv)
    assert word in capsys.readouterr().err


def test_bnd_keys_of_the_network():
    ss = pkg("source_segmenter")
    mk = lambda ck: ss.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs=ck, device="cpu")
    with pytest.raises(ValueError, match="bnd_weight"):
        mk({"bnd_weight": -1.0})
    for bad in ([5], [-1], [1, 7], [1.5], "x"):
        with pytest.raises(ValueError, match="bnd_classes"):
            mk({"bnd_weight": 1.0, "bnd_classes": bad})
    ck = dict(REFERENCE_COST, bnd_weight=0.5, bnd_classes=[2, 4])
    before = dict(ck)
    net = mk(ck)
    assert ck == before and ck["bnd_classes"] == [2, 4]                   # the caller's dict is not mutated
    assert net.bnd_weight == 0.5 and net.bnd_classes == (2, 4) and net.bnd_value is None
    net0 = mk(dict(REFERENCE_COST))
    assert net0.bnd_weight == 0.0 and net0.bnd_classes is None and net0.bnd_value is None
    assert list(net.store.vars) == list(net0.store.vars)                  # the term has no variable of its own


def test_trainer_ramp_and_capture_refusal():
    ss = pkg("source_segmenter")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs=dict(REFERENCE_COST, bnd_weight=0.2), device="cpu")
    tr = ss.Trainer(net, None, None, num_cls=5, batch_size=1, optimizer="adam", opt_kwargs={"learning_rate": 1e-3}, bnd_ramp=4)
    assert [tr.bnd_epoch_weight(e) for e in range(6)] == [0.2 * 0.25, 0.2 * 0.5, 0.2 * 0.75, 0.2, 0.2, 0.2]
    with pytest.raises(RuntimeError, match="bnd_ramp"):
        tr.capture_step(torch.zeros(1, 256, 256, 3), torch.zeros(1, 256, 256, 5), 0.75)
    tr0 = ss.Trainer(net, None, None, num_cls=5, batch_size=1, optimizer="adam", opt_kwargs={"learning_rate": 1e-3})
    assert tr0.bnd_ramp is None and [tr0.bnd_epoch_weight(e) for e in (0, 9)] == [0.2, 0.2]
    with pytest.raises(ValueError, match="bnd_ramp"):
        ss.Trainer(net, None, None, num_cls=5, batch_size=1, bnd_ramp=-2)


def test_class_mask():
    K = pkg("kernels")
    assert K.class_mask(None, 5) == 0b11110 and K.class_mask(None, 1) == 0 and K.class_mask([], 5) == 0
    assert K.class_mask([0], 5) == 1 and K.class_mask((2, 4, 2), 5) == 0b10100
    for bad in ([5], [-1], [0.5]):
        with pytest.raises(ValueError):
            K.class_mask(bad, 5)


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_four_entry_points(built):
    L = pkg("_lib")
    with open(os.path.join(ROOT, "include", "pnp_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in L.PROTOTYPES, name
        assert re.search(r"\b%s\(" % name, header), name
    lib = L.load()
    assert lib.pnp_abi_version() == 4
    # one int16 per pixel and selected class
    assert lib.pnp_signed_distance_2d_workspace_bytes(2, 256, 256, 5, 0b11110) == 2 * 4 * 256 * 256 * 2
    assert lib.pnp_signed_distance_2d_workspace_bytes(1, 7, 3, 5, 0) == 0
    assert lib.pnp_signed_distance_2d_workspace_bytes(1, 1024, 1024, 8, 0xFF) == 8 * 1024 * 1024 * 2
    # one float per block of 256 threads x 8 pixels, at most 2048 blocks
    assert lib.pnp_boundary_loss_workspace_bytes(1, 5) == 4 and lib.pnp_boundary_loss_workspace_bytes(2049, 5) == 8
    assert lib.pnp_boundary_loss_workspace_bytes(1 << 33, 5) == 2048 * 4


def test_cpu_tensors_are_refused(built):
    K, L = pkg("kernels"), pkg("_lib")
    with pytest.raises(L.PnpError, match="CPU"):
        K.signed_distance_2d(torch.zeros(1, 4, 4, 5))
    with pytest.raises(L.PnpError, match="CPU"):
        K.boundary_loss(torch.zeros(4, 5), torch.zeros(4, 5), 4)


def test_bad_calls_are_refused_before_any_launch(built):
    """(no device is needed to be refused: the pointers below are never dereferenced)"""
    import ctypes
    L = pkg("_lib")
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    need = lib.pnp_signed_distance_2d_workspace_bytes(2, 9, 7, 5, 0b11110)
    base = dict(B=2, H=9, W=7, C=5, mask=0b11110, y=fake, phi=fake, ws=fake, n=need)
    for change, msg in ((dict(C=9), "at most 8 classes"), (dict(H=1025), "at most 1024"), (dict(W=1025), "at most 1024"),
                        (dict(B=0), "bad argument"), (dict(H=0), "bad argument"), (dict(C=0, mask=0), "bad argument"),
                        (dict(mask=0b100000), "beyond ncls"), (dict(y=None), "null pointer"), (dict(phi=None), "null pointer"),
                        (dict(ws=None), "null pointer"), (dict(n=need - 1), "workspace too small")):
        a = dict(base, **change)
        code = lib.pnp_signed_distance_2d(a["y"], a["B"], a["H"], a["W"], a["C"], a["mask"], a["phi"], a["ws"], a["n"], None)
        assert code == -1, change           # PNP_EINVAL
        with pytest.raises(L.PnpError, match=msg):
            L.check(code, "pnp_signed_distance_2d")
    P, needl = 1021, lib.pnp_boundary_loss_workspace_bytes(1021, 5)
    bl = lambda z, q, P_, C, nsel, out, ws, n: lib.pnp_boundary_loss(z, q, P_, C, nsel, 1.0, None, out, ws, n, None)
    for args, msg in (((fake, fake, P, 9, 4, fake, fake, needl), "at most 8 classes"), ((fake, fake, P, 5, 4, fake, fake, needl - 1), "workspace too small"),
                      ((None, fake, P, 5, 4, fake, fake, needl), "bad argument"), ((fake, None, P, 5, 4, fake, fake, needl), "bad argument"),
                      ((fake, fake, 0, 5, 4, fake, fake, needl), "bad argument"), ((fake, fake, P, 5, 6, fake, fake, needl), "selected classes"),
                      ((fake, fake, P, 5, -1, fake, fake, needl), "selected classes"), ((fake, fake, P, 5, 4, None, fake, needl), "bad argument"),
                      ((fake, fake, P, 5, 4, fake, None, needl), "bad argument")):
        code = bl(*args)
        assert code == -1
        with pytest.raises(L.PnpError, match=msg):
            L.check(code, "pnp_boundary_loss")
