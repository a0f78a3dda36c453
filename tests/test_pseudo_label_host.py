"""CPU side of the pseudo-label term: the --pl-* flags, the cost keys of Full_DRN, the four entry points' prototypes,
workspace queries and refusals, and the float64 restatement of the kernel tests against torch's cross_entropy and np.sort."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from pseudo_label_ref import build_logits, order_statistic, pseudo_label_ref, rank_of, update_ref


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C,classes", [(1, 5, None), (7, 5, None), (1021, 5, (1, 2, 3, 4)), (257, 2, None), (257, 3, (0, 2)), (257, 8, None),
                                          (64, 1, None)])
def test_reference_against_torch_cross_entropy(P, C, classes):
    """value and gradient = cross_entropy(ignore_index) against the arg-max on the selected pixels, summed and divided by P"""
    tau = np.linspace(0.35, 0.8, C) if C > 1 else np.array([0.5])
    z = build_logits(P, C, 10 * P + C, tau)
    r = pseudo_label_ref(z, tau, classes, coef=1.0)
    t = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    target = torch.from_numpy(np.where(r["sel"], (r["labels"] & 0x7f).astype(np.int64), -100))
    L = torch.nn.functional.cross_entropy(t, target, ignore_index=-100, reduction="sum") / P
    L.backward()
    assert r["labels"].dtype == np.uint8 and np.array_equal(r["labels"] & 0x7f, z.argmax(1)) and np.array_equal(r["labels"] >> 7, r["sel"])
    assert abs(r["value"] - float(L.detach())) <= 1e-13 * abs(float(L.detach())) + 1e-300
    assert float(np.abs(r["grad"] - t.grad.numpy()).max()) <= 1e-13 * float(np.abs(t.grad.numpy()).max()) + 1e-300
    assert r["counts"][0].sum() == P and r["counts"][1].sum() == r["sel"].sum() and (r["counts"][1] <= r["counts"][0]).all()
    assert r["share"] == r["sel"].sum() / P
    if classes is not None:
        assert not r["counts"][1][[c for c in range(C) if c not in classes]].any()
    r3 = pseudo_label_ref(z, tau, classes, coef=-0.375)
    assert r3["value"] == r["value"] and np.allclose(r3["grad"], -0.375 * r["grad"], rtol=1e-14, atol=0.0)


def test_reference_thresholds_at_the_ends():
    z = build_logits(257, 5, 3, np.full(5, 0.5))
    r0 = pseudo_label_ref(z, np.zeros(5))
    assert r0["sel"].all() and r0["share"] == 1.0
    r2 = pseudo_label_ref(z, np.full(5, 1.5))
    assert not r2["sel"].any() and r2["value"] == 0.0 and not r2["grad"].any()
    tie = np.array([[1.0, 2.5, 2.5, 0.0, 2.5]])
    assert pseudo_label_ref(tie, np.zeros(5))["labels"][0] == (1 | 0x80)          # the lowest index wins


@pytest.mark.parametrize("portion", [1e-4, 0.2, 0.5, 1.0])
def test_reference_order_statistic_against_sort(portion):
    rng = np.random.default_rng(5)
    P, C = 4099, 5
    conf = rng.random(P).astype(np.float32) * 0.8 + 0.2
    labels = (rng.integers(0, 4, P) | (rng.integers(0, 2, P) << 7)).astype(np.uint8)        # class 4 is absent; bit 7 is ignored
    labels[7] = 3
    conf[labels & 0x7f == 2] = np.float32(0.625)                                            # one class: all equal
    q = order_statistic(conf, labels, C, portion)
    assert q.dtype == np.float32 and np.isnan(q[4])
    for k in range(4):
        v = np.sort(conf[(labels & 0x7f) == k])[::-1]
        r = rank_of(portion, v.size)
        assert 1 <= r <= v.size and r == int(np.ceil(portion * v.size)) and q[k] == v[r - 1]
    assert q[2] == np.float32(0.625)
    assert rank_of(1.0, 9) == 9 and rank_of(0.5, 9) == 5 and rank_of(1e-9, 9) == 1 and rank_of(0.5, 1) == 1
    tau = np.array([0.9, 0.8, 0.7, 0.6, 0.5])
    assert np.array_equal(update_ref(tau, q, 1.0)[4:], tau[4:]) and np.allclose(update_ref(tau, q, 1.0), tau, rtol=1e-15)
    assert np.array_equal(update_ref(tau, q, 0.0)[:4], q[:4].astype(np.float64)) and update_ref(tau, q, 0.0)[4] == 0.5
    assert np.allclose(update_ref(tau, q, 0.9)[:4], 0.1 * q[:4] + 0.9 * tau[:4], rtol=1e-14)


def test_builder_leaves_no_pixel_near_a_threshold():
    from pseudo_label_ref import CONF_MARGIN, GAP_MARGIN
    tau = np.array([0.9, 0.5, 0.7, 0.6, 0.8])
    z = build_logits(2 * 64 * 64, 5, 11, tau)
    assert z.dtype == np.float32
    r = pseudo_label_ref(z, tau)
    top = np.sort(z.astype(np.float64), 1)
    assert float(np.abs(r["conf"] - tau[r["labels"] & 0x7f]).min()) > CONF_MARGIN and float((top[:, -1] - top[:, -2]).min()) >= GAP_MARGIN
    assert 0 < r["sel"].sum() < z.shape[0]


# ---- flags and cost keys -----------------------------------------------------------------------------------------------------------------
PL_KEYS = ("pl_weight", "pl_portion", "pl_momentum", "pl_init", "pl_classes")


def test_pl_flag_parsing():
    tg = pkg("train_gan")
    for phase in ("pre-train", "train-gan", "fine-tune"):
        a = tg.parse_args(phase, [])
        assert (a.pl_weight, a.pl_portion, a.pl_momentum, a.pl_init, a.pl_classes) == (0.0, 0.5, 0.9, 0.9, None)
        assert tg.configure_args(a) == tg.configure(phase)                # the default is the configuration of today
        a = tg.parse_args(phase, ["--pl-portion", "0.3", "--pl-classes", "1,2"])
        assert tg.configure_args(a) == tg.configure(phase)                # the other flags alone change nothing
        ck0, nc0, tc0 = tg.configure(phase)
        ck, nc, tc = tg.configure_args(tg.parse_args(phase, ["--pl-weight", "0.01"]))
        assert {k: ck[k] for k in PL_KEYS if k in ck} == {"pl_weight": 0.01, "pl_portion": 0.5, "pl_momentum": 0.9, "pl_init": 0.9}
        assert {k: v for k, v in ck.items() if k not in PL_KEYS} == ck0 and nc == nc0 and tc == tc0
        ck, _, _ = tg.configure_args(tg.parse_args(phase, ["--pl-weight", "2", "--pl-portion", "0.25", "--pl-momentum", "0", "--pl-init", "0.5",
                                                           "--pl-classes", "1,2,4", "--ent-weight", "0.1"]))
        assert {k: ck[k] for k in PL_KEYS} == {"pl_weight": 2.0, "pl_portion": 0.25, "pl_momentum": 0.0, "pl_init": 0.5, "pl_classes": (1, 2, 4)}
        assert ck["ent_weight"] == 0.1
    for flag in ("--pl-weight", "--pl-portion", "--pl-momentum", "--pl-init", "--pl-classes"):
        assert flag in tg.__doc__


@pytest.mark.parametrize("argv,word", [(["--pl-weight", "-0.1"], "pl-weight"), (["--pl-portion", "0"], "pl-portion"),
                                       (["--pl-portion", "1.5"], "pl-portion"), (["--pl-momentum", "1.1"], "pl-momentum"),
                                       (["--pl-momentum", "-0.1"], "pl-momentum"), (["--pl-init", "-1"], "pl-init"),
                                       (["--pl-init", "nan"], "pl-init"), (["--pl-classes", "1,x"], "pl-classes")])
def test_bad_pl_flags_are_refused_on_the_command_line(capsys, argv, word):
    tg = pkg("train_gan")
    with pytest.raises(SystemExit):
        tg.parse_args("train-gan", argv)
    assert word in capsys.readouterr().err


def test_pl_keys_of_the_network():
    adv = pkg("adversarial")
    new = lambda ck: adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs=ck, device="cpu")
    for bad, word in (({"pl_weight": -1.0}, "pl_weight"), ({"pl_weight": 1.0, "pl_portion": 0.0}, "pl_portion"),
                      ({"pl_weight": 1.0, "pl_portion": 1.5}, "pl_portion"), ({"pl_weight": 1.0, "pl_momentum": 1.5}, "pl_momentum"),
                      ({"pl_weight": 1.0, "pl_momentum": -0.5}, "pl_momentum"), ({"pl_weight": 1.0, "pl_init": -0.5}, "pl_init"),
                      ({"pl_weight": 1.0, "pl_init": float("nan")}, "pl_init"), ({"pl_weight": 1.0, "pl_classes": (1, 5)}, "class index")):
        with pytest.raises(ValueError, match=word):
            new(bad)
    ck = {"pl_weight": 0.5, "pl_init": 0.75, "pl_classes": [1, 2], "lambda_mask_loss": 0.3}
    net = new(ck)
    assert ck == {"pl_weight": 0.5, "pl_init": 0.75, "pl_classes": [1, 2], "lambda_mask_loss": 0.3}
    assert (net.pl_weight, net.pl_portion, net.pl_momentum, net.pl_init, net.pl_classes) == (0.5, 0.5, 0.9, 0.75, (1, 2))
    assert net.pl_threshold.dtype == torch.float32 and net.pl_threshold.tolist() == [0.75] * 5
    assert net.pl_value is None and net.pl_share is None and net.pl_counts is None
    for ck0 in ({}, {"pl_weight": 0.0}, {"pl_weight": 0.0, "pl_init": 0.5}):
        net0 = new(ck0)
        assert net0.pl_weight == 0.0 and not hasattr(net0, "pl_threshold") and net0.pl_value is None
        assert list(net.store.vars) == list(net0.store.vars)            # the term has no variable in the store


def test_checkpoint_carries_the_thresholds(tmp_path):
    """save_checkpoint writes them into optimizer.npz, restore_optimizer brings them back in place; a checkpoint without them (or a net
    without the term) leaves everything as it is"""
    adv = pkg("adversarial")

    def make(ck):
        net = adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs=ck, device="cpu")
        tr = adv.Trainer(net, None, None, None, None, num_cls=5, batch_size=1, opt_kwargs={"learning_rate": 1e-3}, train_config={})
        tr._get_optimizer()
        return net, tr
    net, tr = make({"pl_weight": 0.5})
    net.pl_threshold.copy_(torch.tensor([0.91, 0.52, 0.63, 0.74, 0.85]))
    tr.global_step = 12
    d1, d0 = str(tmp_path / "with"), str(tmp_path / "without")
    os.makedirs(d1), os.makedirs(d0)
    tr.save_checkpoint(d1)
    with np.load(d1 + "/optimizer.npz") as z:
        assert z["pl_threshold"].dtype == np.float32 and np.array_equal(z["pl_threshold"], net.pl_threshold.numpy())
    net2, tr2 = make({"pl_weight": 0.5, "pl_init": 0.3})
    ptr = net2.pl_threshold.data_ptr()
    assert tr2.restore_optimizer(d1, clear_rms=False, lr_update=False) and tr2.global_step == 12
    assert torch.equal(net2.pl_threshold, net.pl_threshold) and net2.pl_threshold.data_ptr() == ptr
    net0, tr0 = make({})
    tr0.save_checkpoint(d0)
    with np.load(d0 + "/optimizer.npz") as z:
        assert "pl_threshold" not in z.files
    assert tr2.restore_optimizer(d0, clear_rms=False, lr_update=False) and torch.equal(net2.pl_threshold, net.pl_threshold)      # untouched
    net3, tr3 = make({"pl_weight": 0.5, "pl_init": 0.3})
    assert tr3.restore_optimizer(d0, clear_rms=False, lr_update=False) and net3.pl_threshold.tolist() == [np.float32(0.3)] * 5   # from pl_init
    assert tr0.restore_optimizer(d1, clear_rms=False, lr_update=False) and not hasattr(net0, "pl_threshold")


# ---- the entry points ----------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused(built):
    K, L = pkg("kernels"), pkg("_lib")
    with pytest.raises(L.PnpError, match="CPU"):
        K.pseudo_label_loss(torch.zeros(4, 5), torch.zeros(5))
    with pytest.raises(L.PnpError, match="CPU"):
        K.pseudo_label_update(torch.zeros(4, dtype=torch.uint8), torch.zeros(4), torch.zeros(5), 0.5, 0.9)


def test_abi_has_the_four_entry_points(built):
    L = pkg("_lib")
    names = ("pnp_pseudo_label_loss", "pnp_pseudo_label_loss_workspace_bytes", "pnp_pseudo_label_update", "pnp_pseudo_label_update_workspace_bytes")
    assert all(n in L.PROTOTYPES for n in names)
    lib = L.load()
    assert lib.pnp_abi_version() == 4
    # the loss: per block of 256 threads x 8 pixels (at most 2048 blocks) one float and 2 ncls int32 counts
    for P, nblk in ((1, 1), (2048, 1), (2049, 2), (16 * 256 * 256, 512), (1 << 30, 2048)):
        for C in (1, 5, 8):
            assert lib.pnp_pseudo_label_loss_workspace_bytes(P, C) == nblk * 4 * (1 + 2 * C), (P, C)
        # the update: four rounds of [8][256] uint32 histograms and 8 selection states of 12 bytes, whatever P and ncls
        assert lib.pnp_pseudo_label_update_workspace_bytes(P, 5) == 4 * 8 * 256 * 4 + 8 * 12, P
    assert lib.pnp_pseudo_label_update_workspace_bytes(1, 1) == lib.pnp_pseudo_label_update_workspace_bytes(1 << 30, 8)


def test_bad_calls_are_refused_before_any_launch(built):
    """(no device is needed to be refused: the host buffers below are never touched — they keep their fill)"""
    L = pkg("_lib")
    lib = L.load()
    P = 1021
    bufs = {k: np.full(n, 0x5A, dtype=np.uint8) for k, n in (("z", P * 5 * 4), ("tau", 32), ("dl", P * 5 * 4), ("lab", P), ("conf", P * 4),
                                                               ("out", 8), ("cnt", 64), ("q", 32), ("ws", 1 << 16))}
    p = {k: ctypes.c_void_p(v.ctypes.data) for k, v in bufs.items()}
    need = lib.pnp_pseudo_label_loss_workspace_bytes(P, 5)

    def loss(z="z", tau="tau", P_=P, C=5, lab="lab", conf="conf", out="out", cnt="cnt", ws="ws", n=need):
        g = lambda k: p[k] if k else None
        return lib.pnp_pseudo_label_loss(g(z), g(tau), P_, C, 31, 1.0, p["dl"], g(lab), g(conf), g(out), g(cnt), g(ws), n, None)
    cases = [(dict(C=9), "at most 8 classes"), (dict(n=need - 1), "workspace too small"), (dict(P_=0), "bad argument"), (dict(C=0), "bad argument"),
             (dict(P_=1 << 31, n=1 << 16), "not below 2\\^31")]
    cases += [({k: None}, "bad argument") for k in ("z", "tau", "lab", "conf", "out", "cnt", "ws")]
    for kw, msg in cases:
        code = loss(**kw)
        assert code == -1, kw           # PNP_EINVAL
        with pytest.raises(L.PnpError, match=msg):
            L.check(code, "pnp_pseudo_label_loss")
    need_u = lib.pnp_pseudo_label_update_workspace_bytes(P, 5)

    def update(lab="lab", conf="conf", P_=P, C=5, portion=0.5, beta=0.9, tau="tau", ws="ws", n=need_u):
        g = lambda k: p[k] if k else None
        return lib.pnp_pseudo_label_update(g(lab), g(conf), P_, C, portion, beta, g(tau), p["q"], g(ws), n, None)
    cases = [(dict(C=9), "at most 8 classes"), (dict(n=need_u - 1), "workspace too small"), (dict(P_=0), "bad argument"), (dict(C=0), "bad argument"),
             (dict(P_=1 << 31), "not below 2\\^31"), (dict(portion=0.0), "portion"), (dict(portion=1.0000001), "portion"),
             (dict(portion=float("nan")), "portion"), (dict(beta=-0.01), "momentum"), (dict(beta=1.01), "momentum"),
             (dict(beta=float("nan")), "momentum")]
    cases += [({k: None}, "bad argument") for k in ("lab", "conf", "tau", "ws")]
    for kw, msg in cases:
        code = update(**kw)
        assert code == -1, kw
        with pytest.raises(L.PnpError, match=msg):
            L.check(code, "pnp_pseudo_label_update")
    assert all(int(v.min()) == 0x5A and int(v.max()) == 0x5A for v in bufs.values())
