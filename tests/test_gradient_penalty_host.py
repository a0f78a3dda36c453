"""not gpu: the WGAN-GP gradient penalty's host side — its C-ABI symbols, the walker's unit plan of both critics against the units the
CPU oracle records, the --gp-weight flag and the refusals of unsupported combinations."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg
from oracle import nets_adv

NEW_SYMBOLS = ("pnp_gp_interpolate", "pnp_gp_workspace_bytes", "pnp_gp_penalty", "pnp_bn_dbl_bwd_workspace_bytes", "pnp_bn_dbl_bwd")


def test_new_symbols_in_header_library_and_prototypes():
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "pnp_hip.h")).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in lib.PROTOTYPES, name
        assert hasattr(so, name), name
    assert lib.ABI_VERSION == 4


@pytest.fixture(scope="module")
def oracle_units():
    """the conv units the oracle records for one CT + MR dis-step forward at B = 1 (float32), with a product net's variables"""
    adv = pkg("adversarial")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=1, device="cpu")
    V = {k: torch.from_numpy(v.copy()) for k, v in net.store.state_dict().items()}
    rng = np.random.default_rng(0)
    x = [torch.from_numpy(rng.standard_normal((1, 256, 256, 3)).astype(np.float32)) for _ in range(2)]
    units = []
    with torch.no_grad():
        nets_adv.adv_forward(V, x[0], x[1], 0.75, seed=3, segmenter_no_grad=True, units=units)
    return net, V, units


@pytest.mark.parametrize("critic,scope", [("cls", "cls_scope/"), ("mask", "mask_cls_scope/")])
def test_unit_plan_matches_oracle_records(oracle_units, critic, scope):
    net, V, units = oracle_units
    gp = pkg("gradient_penalty")
    plan, fc = gp.unit_plan(critic, net.feature_base, net.n_class)
    for br in ("ct", "mr"):
        rec = [r for r in units if r["kind"] == "conv" and r["branch"] == br and r["w"].startswith(scope)]
        want = [(r["w"], int(V[r["w"]].shape[0]), r["stride"], r["padding"], r["bn"], r["shortcut"] is not None,
                 r["shortcut"] is not None and r["shortcut"].shape[-1] != r["out"].shape[-1], r["keep"]) for r in rec]
        got = [(u["w"], u["k"], u["stride"], u["padding"], u["bn"], u["shortcut"] is not None, u["inc_dim"], gp_keep()) for u in plan]
        assert got == want
        fcs = [r["w"] for r in units if r["kind"] == "fc" and r["branch"] == br and r["w"].startswith(scope)]
        assert fcs == [fc]
    # every filter of the plan has the shape the plan convolves with, and the shortcut of a tail is its head's input
    for i, u in enumerate(plan):
        assert tuple(net.store.vars[u["w"]].shape) == (u["k"], u["k"], u["cin"], u["cout"])
        if u["shortcut"] is not None:
            assert u["shortcut"] == i - 1 and plan[i - 1]["cin"] * (2 if u["inc_dim"] else 1) == u["cout"]


def gp_keep():
    return pkg("adversarial").CRITIC_KEEP_PROB


def test_critic_builders_read_the_one_table():
    """every critic variable the builders create is named by the table (filters, BN scopes, fc), in creation order"""
    adv, gp = pkg("adversarial"), pkg("gradient_penalty")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=2, device="cpu")
    for critic, scope in (("cls", "cls_scope/"), ("mask", "mask_cls_scope/")):
        plan, fc = gp.unit_plan(critic, net.feature_base, net.n_class)
        made = [n for n in net.store.vars if n.startswith(scope) and "Variable" in n]
        assert made == [u["w"] for u in plan] + [fc]
        bns = sorted({n.rsplit("/", 1)[0] for n in net.store.vars if n.startswith(scope) and "Variable" not in n})
        assert bns == sorted(u["bn"] for u in plan)


def test_gp_weight_flag_parsing():
    tg = pkg("train_gan")
    for phase in ("pre-train", "train-gan", "fine-tune"):
        a = tg.parse_args(phase, [])
        assert a.gp_weight == 0.0
        assert tg.configure_args(a) == tg.configure(phase)          # lambda = 0: the configuration of today
        a = tg.parse_args(phase, ["--gp-weight", "10"])
        ck, nc, tc = tg.configure_args(a)
        assert ck["gp_weight"] == 10.0
        ck0, nc0, tc0 = tg.configure(phase)
        assert {k: v for k, v in ck.items() if k != "gp_weight"} == ck0 and nc == nc0 and tc == tc0


@pytest.mark.parametrize("argv", [["--gp-weight", "-1"], ["--gp-weight", "10", "--dtype", "bf16"], ["--gp-weight", "10", "--sync-stats"]])
def test_unsupported_gp_combinations_are_refused(argv, capsys):
    tg = pkg("train_gan")
    with pytest.raises(SystemExit):
        tg.parse_args("pre-train", argv)
    assert "gp-weight" in capsys.readouterr().err


def test_negative_gp_weight_is_refused_by_the_network():
    adv = pkg("adversarial")
    with pytest.raises(ValueError, match="gp_weight"):
        adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs={"gp_weight": -1.0}, device="cpu")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs={"gp_weight": 10.0}, device="cpu")
    assert net.gp_weight == 10.0
    assert adv.Full_DRN(channels=3, n_class=5, batch_size=1, device="cpu").gp_weight == 0.0


def test_bf16_convolutions_are_refused_by_the_walker():
    adv, gp, F = pkg("adversarial"), pkg("gradient_penalty"), pkg("functional")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=1, cost_kwargs={"gp_weight": 10.0}, device="cpu")
    F.set_conv_dtype("bf16")
    try:
        with pytest.raises(RuntimeError, match="bf16"):
            gp.critic_gradient_penalty(net, "mask", torch.zeros(1, 256, 256, 5), torch.zeros(1, 256, 256, 5), 10.0, 1, 0)
    finally:
        F.set_conv_dtype("f32")
