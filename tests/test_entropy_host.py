"""CPU side of the entropy term: the float64 reference of the kernel tests against torch autograd, the --ent-weight /
--monitor-entropy flags, the cost key of Full_DRN, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from conftest import pkg
from entropy_ref import entropy_ref, special_rows


@pytest.mark.parametrize("P,C", [(1, 5), (7, 5), (257, 2), (257, 3), (257, 8), (64, 1)])
def test_reference_against_torch_float64_autograd(P, C):
    rng = np.random.default_rng(P * 10 + C)
    z = rng.standard_normal((P, C)) * 3.0
    special_rows(z, rng)
    val, grad = entropy_ref(z)
    t = torch.from_numpy(z).requires_grad_(True)
    H = -(torch.softmax(t, -1) * torch.log_softmax(t, -1)).sum(-1)
    if C == 1:
        assert val == 0.0 and not grad.any()         # the convention of soft_entropy: one class has entropy 0 and no normaliser
        return
    L = H.mean() / np.log(float(C))
    L.backward()
    assert np.isfinite(val) and np.isfinite(grad).all()
    assert abs(val - float(L.detach())) <= 1e-13 * abs(float(L.detach())) + 1e-300
    assert float(np.abs(grad - t.grad.numpy()).max()) <= 1e-13 * float(np.abs(t.grad.numpy()).max()) + 1e-300
    assert 0.0 <= val <= 1.0 + 1e-12
    v3, g3 = entropy_ref(z, coef=-0.375)
    assert v3 == val and np.array_equal(g3, -0.375 * grad)


def test_reference_special_rows():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((64, 5))
    idx = special_rows(z, rng)
    assert all(len(v) == 2 for v in idx.values())
    _, g = entropy_ref(z)
    for r in idx["equal"]:
        v, _ = entropy_ref(z[r:r + 1])
        assert abs(v - 1.0) < 1e-14 and float(np.abs(g[r]).max()) < 1e-16
    for r in idx["ahead"]:
        v, _ = entropy_ref(z[r:r + 1])
        assert 0.0 <= v < 1e-80 and float(np.abs(g[r]).max()) < 1e-80
    for r in idx["huge"]:                           # several classes may tie at +1e4: any entropy in [0, 1], but finite
        v, _ = entropy_ref(z[r:r + 1])
        assert 0.0 <= v <= 1.0 and np.isfinite(g[r]).all()


def test_ent_weight_flag_parsing():
    tg = pkg("train_gan")
    for phase in ("pre-train", "train-gan", "fine-tune"):
        a = tg.parse_args(phase, [])
        assert a.ent_weight == 0.0 and a.monitor_entropy is False
        assert tg.configure_args(a) == tg.configure(phase)          # the default is the configuration of today
        a = tg.parse_args(phase, ["--ent-weight", "0.01"])
        ck, nc, tc = tg.configure_args(a)
        ck0, nc0, tc0 = tg.configure(phase)
        assert ck["ent_weight"] == 0.01
        assert {k: v for k, v in ck.items() if k != "ent_weight"} == ck0 and nc == nc0 and tc == tc0
        a = tg.parse_args(phase, ["--monitor-entropy"])
        ck, nc, tc = tg.configure_args(a)
        assert ck == ck0 and nc == nc0 and tc.pop("monitor_entropy") is True and tc == tc0
    assert "--ent-weight" in tg.__doc__ and "--monitor-entropy" in tg.__doc__


def test_negative_ent_weight_is_refused_on_the_command_line(capsys):
    tg = pkg("train_gan")
    with pytest.raises(SystemExit):
        tg.parse_args("train-gan", ["--ent-weight", "-0.1"])
    assert "ent-weight" in capsys.readouterr().err


def test_ent_weight_of_the_network():
    adv = pkg("adversarial")
    with pytest.raises(ValueError, match="ent_weight"):
        adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs={"ent_weight": -1.0}, device="cpu")
    ck = {"ent_weight": 0.5, "lambda_mask_loss": 0.3}
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs=ck, device="cpu")
    assert net.ent_weight == 0.5 and net.ent_value is None and ck == {"ent_weight": 0.5, "lambda_mask_loss": 0.3}
    net0 = adv.Full_DRN(channels=3, n_class=5, batch_size=1, device="cpu")
    assert net0.ent_weight == 0.0 and net0.ent_value is None and not hasattr(net0, "ct_entropy_eval")
    assert list(net.store.vars) == list(net0.store.vars)            # the term has no variable of its own


def test_cpu_tensors_are_refused(built):
    K, L = pkg("kernels"), pkg("_lib")
    with pytest.raises(L.PnpError, match="CPU"):
        K.softmax_entropy(torch.zeros(4, 5))
    with pytest.raises(L.PnpError, match="CPU"):
        K.softmax_entropy(torch.zeros(4, 5), coef=2.0, want_grad=True)


def test_abi_has_the_two_entry_points(built):
    L = pkg("_lib")
    assert "pnp_softmax_entropy" in L.PROTOTYPES and "pnp_softmax_entropy_workspace_bytes" in L.PROTOTYPES
    lib = L.load()
    assert lib.pnp_abi_version() == 4
    # one float per block of 256 threads x 8 pixels, at most 2048 blocks
    assert lib.pnp_softmax_entropy_workspace_bytes(1, 5) == 4
    assert lib.pnp_softmax_entropy_workspace_bytes(2048, 5) == 4 and lib.pnp_softmax_entropy_workspace_bytes(2049, 5) == 8
    assert lib.pnp_softmax_entropy_workspace_bytes(16 * 256 * 256, 5) == 512 * 4
    assert lib.pnp_softmax_entropy_workspace_bytes(1 << 33, 5) == 2048 * 4


def test_bad_calls_are_refused_before_any_launch(built):
    """(no device is needed to be refused: the pointers below are never dereferenced)"""
    import ctypes
    L = pkg("_lib")
    lib = L.load()
    fake = ctypes.c_void_p(4096)
    P, need = 1021, lib.pnp_softmax_entropy_workspace_bytes(1021, 5)
    call = lambda logits, P_, C, out, ws, n: lib.pnp_softmax_entropy(logits, P_, C, 1.0, None, out, ws, n, None)
    for args, msg in (((fake, P, 9, fake, fake, need), "at most 8 classes"), ((fake, P, 5, fake, fake, need - 1), "workspace too small"),
                      ((None, P, 5, fake, fake, need), "bad argument"), ((fake, 0, 5, fake, fake, need), "bad argument"),
                      ((fake, P, 0, fake, fake, need), "bad argument"), ((fake, P, 5, None, fake, need), "bad argument"),
                      ((fake, P, 5, fake, None, need), "bad argument")):
        code = call(*args)
        assert code == -1           # PNP_EINVAL
        with pytest.raises(L.PnpError, match=msg):
            L.check(code, "pnp_softmax_entropy")
