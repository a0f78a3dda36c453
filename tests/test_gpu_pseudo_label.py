"""-m gpu: class-balanced pseudo-label self-training on the CT predictions (csrc/pseudo_label.hip): the loss kernel against
the float64 restatement of tests/pseudo_label_ref.py, the threshold update against a host sort of the device's own maps, the generator
step with the term against the CPU oracle (oracle/nets_adv.py) with the term added in torch, pl_weight = 0 being today's step,
determinism, the term next to the entropy term, bf16 arithmetic, step capture and the entry point."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from kernel_bars import _bar, _value_bar
from oracle import nets_adv
from oracle import tf_ops as T
from pseudo_label_ref import build_logits, order_statistic, pseudo_label_ref, rank_of, update_ref
from test_gpu_adversarial import COST, NETCFG, grad_report, he_state, make_vars

pytestmark = pytest.mark.gpu

KEEP = 0.75
LR = 3e-4


def _bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def _tau(C):
    """mixed thresholds per class, exact in float32 (the kernel reads float32, the restatement gets the same numbers)"""
    return np.array([0.9, 0.35, 0.6, 0.5, 0.75, 0.4, 0.8, 0.55][:C], dtype=np.float32).astype(np.float64)


# ---- 1. the loss kernel against float64 ----------------------------------------------------------------------------------------------
# C = 5: below one four-pixel group, one group, a group and a tail, many blocks with a tail, whole groups only; the other class counts on
# the generic path; 2 * 256 * 256 pixels: 64 blocks of 256 threads, every thread walks the grid-stride loop twice
SHAPES = [(P, 5) for P in (1, 3, 4, 7, 1021, 2 * 64 * 64, 2 * 256 * 256)] + [(257, C) for C in (1, 2, 3, 8)]


def _check_against_reference(K, zd, z, tau, classes, coef, what):
    C = z.shape[-1]
    P = z.shape[0]
    taud = torch.from_numpy(tau.astype(np.float32)).to(zd.device)
    ref = pseudo_label_ref(z, tau, classes, coef)
    v, share, counts, labels, conf, g = K.pseudo_label_loss(zd, taud, classes, coef=coef, want_grad=True)
    v0, share0, counts0, labels0, conf0, g0 = K.pseudo_label_loss(zd, taud, classes)
    v2, share2, counts2, labels2, conf2, g2 = K.pseudo_label_loss(zd, taud, classes, coef=coef, want_grad=True)
    assert g0 is None and tuple(v.shape) == (1,) and tuple(share.shape) == (1,) and g.shape == zd.shape
    assert tuple(counts.shape) == (2, C) and counts.dtype == torch.int32 and labels.dtype == torch.uint8 and tuple(labels.shape) == (P,)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(conf).all()), what
    _value_bar(v, ref["value"], what)
    _bar(g, torch.from_numpy(ref["grad"]), what + " gradient")
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]), what + ": class / selected bytes"
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref["counts"]), what + ": counts"
    rel = np.abs(conf.cpu().numpy().astype(np.float64) - ref["conf"]) / ref["conf"]
    print("%s: confidence max relative error %.3e, selected %d of %d" % (what, rel.max(), ref["counts"][1].sum(), P))
    assert float(rel.max()) <= 1e-6, what
    assert abs(float(share) - ref["share"]) <= 1e-6
    assert torch.equal(v0, v) and torch.equal(share0, share) and torch.equal(counts0, counts) and torch.equal(labels0, labels) \
        and torch.equal(_bits(conf0), _bits(conf)), "dlogits = NULL changes an output"      # bit for bit
    assert torch.equal(v2, v) and torch.equal(_bits(g2), _bits(g)) and torch.equal(labels2, labels) and torch.equal(counts2, counts) \
        and torch.equal(_bits(conf2), _bits(conf)) and torch.equal(share2, share), "two runs differ"
    return v, labels, conf, g


@pytest.mark.parametrize("classes", [None, "no0"])
@pytest.mark.parametrize("P,C", SHAPES)
def test_kernel_against_float64(dev, P, C, classes):
    K = pkg("kernels")
    if classes == "no0":
        classes = tuple(range(1, C))             # a class mask that drops class 0 (C = 1: the empty mask)
    tau = _tau(C)
    z = build_logits(P, C, 100 * C + P % 97, tau)
    zd = torch.from_numpy(z).to(dev)
    assert zd.data_ptr() % 16 == 0
    _, labels, _, g = _check_against_reference(K, zd, z, tau, classes, 0.375 * 0.25, "P=%d C=%d classes=%s" % (P, C, classes))
    if classes is not None:                      # class 0 is predicted, never selected, and pulls nothing
        lab = labels.cpu().numpy()
        assert not (lab == 0x80).any() and float(g[torch.from_numpy((lab & 0x7f) == 0).to(dev)].abs().sum()) == 0.0


@pytest.mark.parametrize("P", [7, 1021])
def test_kernel_misaligned_base_takes_the_generic_path(dev, P):
    """logits that start one pixel (20 bytes) into an allocation: no float4 load is aligned, the launch takes the generic path"""
    K = pkg("kernels")
    tau = _tau(5)
    z = build_logits(P, 5, 7 + P, tau)
    base = torch.zeros((P + 1, 5), device=dev)
    base[1:] = torch.from_numpy(z).to(dev)
    zd = base[1:]
    assert zd.is_contiguous() and zd.data_ptr() % 16 != 0
    v, labels, conf, g = _check_against_reference(K, zd, z, tau, None, 1.0, "misaligned P=%d" % P)
    taud = torch.from_numpy(tau.astype(np.float32)).to(dev)
    va, _, _, la, ca, ga = K.pseudo_label_loss(zd.clone(), taud, want_grad=True)      # the aligned copy on the vector path
    _bar(g, ga.detach().cpu(), "misaligned against aligned")
    assert abs(float(v) - float(va)) <= 1e-5 * abs(float(va)) and torch.equal(labels, la)
    assert float(((conf - ca).abs() / ca).max()) <= 1e-6


def _one_row(K, dev, row, tau):
    zd = torch.tensor([row], dtype=torch.float32, device=dev)
    taud = torch.full((len(row),), tau, dtype=torch.float32, device=dev)
    v, share, counts, labels, conf, g = K.pseudo_label_loss(zd, taud, want_grad=True)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(conf).all())
    return float(v), float(share), counts.cpu().numpy(), int(labels[0]), float(conf[0]), g[0].cpu().numpy()


def test_special_rows(dev):
    K = pkg("kernels")
    # two (three) equal top logits: the lower index wins
    v, share, counts, lab, conf, g = _one_row(K, dev, [1.0, 2.5, 2.5, 0.0, 2.5], 0.0)
    assert lab == (1 | 0x80) and counts.tolist() == [[0, 1, 0, 0, 0], [0, 1, 0, 0, 0]] and share == 1.0
    assert _one_row(K, dev, [-3.0, -3.0], 0.0)[3] == (0 | 0x80) and _one_row(K, dev, [0.5] * 8, 0.0)[3] == (0 | 0x80)
    # a class 200 logits ahead: s = 1 and the confidence exactly 1 — selected at tau = 1, loss 0, gradient 0
    for row, k in (([0.3, -1.0, 200.2, 0.5, 1.0], 2), ([200.0, 0.0, 0.0, 0.0, 0.0], 0), ([1e4, -1e4, 1e4 - 200.0], 0)):
        v, share, counts, lab, conf, g = _one_row(K, dev, row, 1.0)
        assert conf == 1.0 and lab == (k | 0x80) and v == 0.0 and share == 1.0 and not g.any(), row
    # tau above 1: nothing is selected — value 0, gradient exactly 0
    v, share, counts, lab, conf, g = _one_row(K, dev, [0.3, -1.0, 200.2, 0.5, 1.0], 1.5)
    assert lab == 2 and v == 0.0 and share == 0.0 and not g.any() and counts.tolist() == [[0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]


def test_thresholds_at_the_ends(dev):
    """tau = 0: every pixel is selected, value and gradient are the cross-entropy against the arg-max; tau > 1: nothing is selected"""
    K = pkg("kernels")
    P = 1021
    z = build_logits(P, 5, 1, np.full(5, 0.5))
    zd = torch.from_numpy(z).to(dev)
    v, share, counts, labels, conf, g = K.pseudo_label_loss(zd, torch.zeros(5, device=dev), want_grad=True)
    t = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    L = torch.nn.functional.cross_entropy(t, t.detach().argmax(1))
    L.backward()
    _value_bar(v, float(L.detach()), "tau = 0 against cross_entropy")
    _bar(g, t.grad, "tau = 0 gradient against cross_entropy")
    assert float(share) == 1.0 and bool((labels >= 0x80).all()) and torch.equal(counts[0], counts[1]) and int(counts[0].sum()) == P
    v, share, counts, labels, conf, g = K.pseudo_label_loss(zd, torch.full((5,), 1.0 + 2.0 ** -20, device=dev), want_grad=True)
    assert float(v) == 0.0 and float(share) == 0.0 and float(g.abs().max()) == 0.0 and bool((labels < 0x80).all())
    assert int(counts[0].sum()) == P and int(counts[1].abs().sum()) == 0


def test_autograd_function_scales_by_coef_and_gscale(dev):
    F = pkg("functional")
    tau = _tau(5)
    z = build_logits(1021, 5, 3, tau)
    taud = torch.from_numpy(tau.astype(np.float32)).to(dev)
    for coef, gscale, classes in ((1.0, 1.0, None), (0.01, 0.125, None), (2.5, 0.5, (1, 2, 3, 4))):
        zd = torch.from_numpy(z).to(dev).requires_grad_(True)
        val, share, counts, labels, conf = F.PseudoLabelLossFn.apply(zd, taud, classes, coef, gscale)
        assert val.requires_grad and not share.requires_grad and not conf.requires_grad
        val.backward(torch.ones(1, device=dev))
        ref = pseudo_label_ref(z, tau, classes, coef * gscale)
        _value_bar(val.detach(), ref["value"], "PseudoLabelLossFn coef %g gscale %g" % (coef, gscale))      # the value is not scaled
        _bar(zd.grad, torch.from_numpy(ref["grad"]), "PseudoLabelLossFn gradient coef %g gscale %g" % (coef, gscale))
        assert np.array_equal(labels.cpu().numpy(), ref["labels"])


def test_wrappers_refuse_before_any_launch(dev):
    K, L = pkg("kernels"), pkg("_lib")
    with pytest.raises(L.PnpError, match="at most 8 classes"):
        K.pseudo_label_loss(torch.zeros((4, 9), device=dev), torch.zeros(9, device=dev))
    with pytest.raises(L.PnpError, match="thresholds"):
        K.pseudo_label_loss(torch.zeros((4, 5), device=dev), torch.zeros(4, device=dev))
    with pytest.raises(ValueError, match="class index"):
        K.pseudo_label_loss(torch.zeros((4, 5), device=dev), torch.zeros(5, device=dev), classes=(5,))
    lab, conf, tau = torch.zeros(4, dtype=torch.uint8, device=dev), torch.full((4,), 0.5, device=dev), torch.full((5,), 0.25, device=dev)
    for portion, beta, word in ((0.0, 0.5, "portion"), (1.5, 0.5, "portion"), (0.5, -0.1, "momentum"), (0.5, 1.5, "momentum")):
        with pytest.raises(L.PnpError, match=word):
            K.pseudo_label_update(lab, conf, tau, portion, beta)
    with pytest.raises(L.PnpError, match="uint8"):
        K.pseudo_label_update(lab.float(), conf, tau, 0.5, 0.5)
    assert tau.tolist() == [0.25] * 5


# ---- 2. the threshold update against a host sort of the device's own maps --------------------------------------------------------------
def _update_case(K, dev, z, tau0, portion, beta, what):
    """-> (q, thresholds after) as numpy float32; asserts everything the issue asks of one update"""
    C = z.shape[-1]
    zd = torch.from_numpy(z).to(dev)
    tau0 = np.asarray(tau0, dtype=np.float32)
    taud = torch.from_numpy(tau0).to(dev)
    _, _, counts, labels, conf, _ = K.pseudo_label_loss(zd, taud)
    t1 = taud.clone()
    q = K.pseudo_label_update(labels, conf, t1, portion, beta)
    t2 = taud.clone()
    q2 = K.pseudo_label_update(labels, conf, t2, portion, beta)
    assert torch.equal(_bits(q), _bits(q2)) and torch.equal(_bits(t1), _bits(t2)), what + ": two updates from the same state differ"
    assert torch.equal(_bits(taud), torch.from_numpy(tau0).view(torch.int32)), what + ": the loss wrote the thresholds"
    conf_h, lab_h, n = conf.cpu().numpy(), labels.cpu().numpy(), counts[0].cpu().numpy()
    qh, th = q.cpu().numpy(), t1.cpu().numpy()
    for k in range(C):
        v = np.sort(conf_h[(lab_h & 0x7f) == k])[::-1]           # the device's own map, sorted on the host
        assert v.size == n[k]
        if v.size == 0:
            assert np.isnan(qh[k]) and th[k].view(np.uint32) == tau0[k].view(np.uint32), (what, k)      # absent: tau bit for bit
            continue
        r = rank_of(portion, v.size)
        assert qh[k].view(np.uint32) == v[r - 1].view(np.uint32), (what, k, r, v.size, float(qh[k]), float(v[r - 1]))
        if beta == 0.0:
            assert th[k].view(np.uint32) == qh[k].view(np.uint32), (what, k)
        elif beta == 1.0:
            assert th[k].view(np.uint32) == tau0[k].view(np.uint32), (what, k)
    assert np.array_equal(order_statistic(conf_h, lab_h, C, portion).view(np.uint32), qh.view(np.uint32)), what      # (NaN bits included)
    want = update_ref(tau0, qh, beta)
    assert float((np.abs(th.astype(np.float64) - want) / np.abs(want)).max()) <= 1e-6, what
    print("%s: n_k %s q %s tau %s -> %s" % (what, n.tolist(), qh.tolist(), tau0.tolist(), th.tolist()))
    return qh, th


def _crafted(P, seed):
    """(P, 5): classes 0 and 1 random; every pixel predicted as 2 carries the SAME logits (one confidence float: ties through all four
    rounds); class 3 has one pixel; class 4 is absent"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((P, 5)) * 3.0).astype(np.float32)
    z[:, 2:] = -50.0
    z[rng.choice(P, size=P // 5, replace=False)] = np.array([0.0, 0.5, 3.0, -1.0, -50.0], dtype=np.float32)
    z[7] = np.array([0.25, -0.5, 1.0, 2.0, -50.0], dtype=np.float32)
    return z


@pytest.mark.parametrize("portion", [1e-3, 0.5, 1.0])
@pytest.mark.parametrize("beta", [0.0, 0.9, 1.0])
def test_update_on_crafted_classes(dev, portion, beta):
    K = pkg("kernels")
    P = 4099
    z = _crafted(P, 11)
    tau0 = [0.9, 0.8, 0.7, 0.6, 0.3]
    q, t = _update_case(K, dev, z, tau0, portion, beta, "crafted portion %g beta %g" % (portion, beta))
    k = z.astype(np.float64).argmax(1)
    assert (k == 4).sum() == 0 and (k == 3).sum() == 1 and (k == 2).sum() >= P // 5 - 1 and np.isnan(q[4]) and not np.isnan(q[:4]).any()
    s2 = np.exp(np.array([0.0, 0.5, 3.0, -1.0, -50.0]) - 3.0).sum()
    assert abs(q[2] * s2 - 1.0) <= 1e-6                         # the one confidence of class 2, whatever the rank
    if portion == 1e-3:
        assert q[0] > 0.99 and q[1] > 0.99                     # r = ceil(1e-3 n): among the largest few
    assert t[4] == np.float32(0.3)


@pytest.mark.parametrize("P,C,portion,beta", [(1, 5, 0.5, 0.0), (3, 5, 1.0, 0.5), (257, 1, 0.5, 0.9), (257, 3, 1.0, 0.0), (257, 8, 0.3, 0.9),
                                                (2 * 64 * 64, 5, 0.2, 0.9), (2 * 256 * 256, 5, 0.5, 0.9)])
def test_update_on_random_logits(dev, P, C, portion, beta):
    """random logits through the loss, every class count and both paths of the loss kernel; 2 * 256 * 256 pixels: every thread of the 256
    histogram blocks walks the grid-stride loop twice"""
    K = pkg("kernels")
    z = build_logits(P, C, 5 * P + C, _tau(C))
    _update_case(K, dev, z, _tau(C), portion, beta, "random P=%d C=%d portion %g beta %g" % (P, C, portion, beta))


def test_update_walks_the_grid_stride_loop(dev):
    """P = 5 * 256 * 256 + 3 on maps made directly: five sweeps of the 256-block histogram grid and a ragged sixth; bit 7 of the class byte
    is ignored"""
    K = pkg("kernels")
    P, C = 5 * 256 * 256 + 3, 5
    rng = np.random.default_rng(2)
    conf = (rng.random(P) * 0.8 + 0.2).astype(np.float32)
    lab = (rng.integers(0, C, P) | (rng.integers(0, 2, P) << 7)).astype(np.uint8)
    tau0 = np.array([0.9, 0.8, 0.7, 0.6, 0.5], dtype=np.float32)
    t = torch.from_numpy(tau0).to(dev)
    q = K.pseudo_label_update(torch.from_numpy(lab).to(dev), torch.from_numpy(conf).to(dev), t, 0.37, 0.0).cpu().numpy()
    assert np.array_equal(q.view(np.uint32), order_statistic(conf, lab, C, 0.37).view(np.uint32))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), q.view(np.uint32))


# ---- 3. the generator step with the term against the oracle, B = 2 ----------------------------------------------------------------
B = 2
LAM = COST["lambda_mask_loss"]
GEN_SEED = 23
# The He-initialised net of this fixture is confident: of its 131 072 CT pixels a quarter lie below a confidence of 0.99, a tenth below
# 0.85, half above 0.9999.  Thresholds far below 1 sit where the confidences are sparse (about 0.1 to 0.6 pixels within 2e-6 of them),
# thresholds near 1 would sit where thousands of pixels crowd.  Measured with the oracle on the CPU (float32 logits taken to float64):
# PL_NEAR below.
PL_TAU = (0.99, 0.9, 0.97, 0.8, 0.95)
# PL_NEAR: at these thresholds 2 of the 131 072 pixels of the oracle's float32 logits lie within 2e-6 of their threshold (cap 13), the
# float32 and the float64 oracle agree on every byte of the map, 83.3 % of the pixels are selected and the float64 term is 4.689e-3.
# PL_NORMS: the float64 oracle's two gradient norms (the term teacher-forced with its own map) are 0.1386 * (miu_gen / 0.002) for the
# critics and 0.0576 * pl_weight for the term: pl_weight = 2.4 balances them.
PL_WEIGHT_B = 2.4
PL_COST = {"pl_init": 0.0, "pl_portion": 0.5, "pl_momentum": 0.9}      # (pl_init is replaced by PL_TAU in _net)


@pytest.fixture(scope="module")
def case():
    """weights, one CT batch, and the oracle's graph in float32 and float64, kept alive: the pseudo-label term is teacher-forced with the
    DEVICE's class / selected map, so its gradient is taken once that map is known; the critics' part does not depend on it"""
    adv = pkg("adversarial")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(COST), network_config=dict(NETCFG), device="cpu", seed=1)
    sd = he_state(net, 7)
    rng = np.random.default_rng(5)
    ct = (rng.standard_normal((B, 256, 256, 3)) * 1.2 + 0.1).astype(np.float32)
    res = {}
    for dt in (torch.float32, torch.float64):
        V = make_vars(sd, dt, lambda k: k.startswith("adapt_"))
        o = nets_adv.adv_forward(V, None, torch.from_numpy(ct).to(dt), KEEP, ct_front_bn=True, seed=GEN_SEED)
        _, gen1 = nets_adv.wgan_losses(o, miu_gen=1.0, lam=LAM)
        names = [k for k in V if V[k].requires_grad]
        res[dt] = {"V": V, "names": names, "z": o["ct_logits"], "gen1": float(gen1.detach()),
                   "g_gen": _grads(gen1, V, names), "ct_logits": o["ct_logits"].detach()}
    return sd, ct, res


def _grads(root, V, names):
    gs = torch.autograd.grad(root, [V[k] for k in names], retain_graph=True, allow_unused=True)
    return {k: (g if g is not None else torch.zeros_like(V[k])) for k, g in zip(names, gs)}


def _oracle_term(r, labels):
    """the oracle's term on its own CT logits against the device's map: cross_entropy over the selected pixels, divided by P"""
    lab = labels.reshape(-1).astype(np.int64)
    target = torch.from_numpy(np.where(lab >= 0x80, lab & 0x7f, -100))
    z = r["z"].reshape(-1, 5)
    return torch.nn.functional.cross_entropy(z, target, ignore_index=-100, reduction="sum") / z.shape[0]


def _net(dev, sd, cost, tau=PL_TAU):
    adv = pkg("adversarial")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(COST, **cost), network_config=dict(NETCFG), device=dev, seed=1)
    net.store.load_state_dict(sd)
    if getattr(net, "pl_weight", 0) > 0 and tau is not None:
        net.pl_threshold.copy_(torch.tensor(tau, dtype=torch.float32))
    tr = adv.Trainer(net, None, None, None, None, num_cls=5, batch_size=B, opt_kwargs={"learning_rate": LR},
                     train_config={"dis_sub_iter": 1, "gen_sub_iter": 1})
    tr._get_optimizer()
    return net, tr


def _norm(gs):
    return float(sum(float((g.double() ** 2).sum()) for g in gs.values()) ** 0.5)


def test_oracle_logits_keep_clear_of_the_thresholds(case):
    """the condition of the map comparison below, checked where no device is needed: of the oracle's float32 logits, taken to float64, at
    most 1e-4 of the pixels lie within 2e-6 of their class's threshold (measured: PL_NEAR), and the float32 and float64 oracles disagree on
    the map in no more pixels than that"""
    _, _, res = case
    tau = np.array(PL_TAU, dtype=np.float32).astype(np.float64)
    r32 = pseudo_label_ref(res[torch.float32]["ct_logits"].numpy().reshape(-1, 5), tau)
    r64 = pseudo_label_ref(res[torch.float64]["ct_logits"].numpy().reshape(-1, 5), tau)
    near = int((np.abs(r32["conf"] - tau[r32["labels"] & 0x7f]) <= 2e-6).sum())
    differ = int((r32["labels"] != r64["labels"]).sum())
    P = r32["conf"].size
    print("oracle fp32 logits: %d of %d pixels within 2e-6 of their threshold (cap %d); fp32 and fp64 maps differ in %d; selected share %.4f"
          % (near, P, int(1e-4 * P), differ, r64["share"]))
    assert near <= 1e-4 * P and differ <= 1e-4 * P and 0.5 < r64["share"] < 0.95


# (a) miu_gen = 0: the adapt_* gradients come from the pseudo-label term alone — the new path and nothing else
# (b) the reference's miu_gen and lambda_mask_loss = 0.3: the mask critic, the feature critic and the term all feed ct_logits; PL_NORMS
@pytest.mark.parametrize("tag,miu_gen,pl_weight", [("a", 0.0, 1.0), ("b", COST["miu_gen"], "PL_WEIGHT_B")])
def test_gen_step_with_pseudo_labels_vs_oracle(dev, case, tag, miu_gen, pl_weight):
    K = pkg("kernels")
    sd, ct, res = case
    pl_weight = PL_WEIGHT_B if pl_weight == "PL_WEIGHT_B" else pl_weight
    net, tr = _net(dev, sd, dict(PL_COST, miu_gen=miu_gen, pl_weight=pl_weight))
    assert net.lambda_mask_loss == LAM and net.pl_weight == pl_weight
    tau0 = net.pl_threshold.clone()
    before = net.store.state_dict()
    loss = tr.gen_step(torch.from_numpy(ct).to(dev), KEEP, GEN_SEED)
    g_hip = {v.name: v.tensor.grad.detach().cpu().clone() for v in net.store.trainable() if v.name.startswith("adapt_")}
    for v in net.store.trainable():                 # variables outside adapt_* get zero gradient
        if not v.name.startswith("adapt_"):
            assert float(v.tensor.grad.abs().max()) == 0.0, v.name
    after = net.store.state_dict()
    labels = net.pl_labels.cpu().numpy()
    P = labels.size
    # the device's map = the restatement on the device's own fp32 logits, but for the pixels within 2e-6 of their threshold
    zdev = net.ct_logits.detach().cpu().numpy().reshape(-1, 5)
    tau = tau0.cpu().numpy().astype(np.float64)
    rdev = pseudo_label_ref(zdev, tau)
    near = np.abs(rdev["conf"] - tau[rdev["labels"] & 0x7f]) <= 2e-6
    print("gen+pl (%s): %d of %d pixels within 2e-6 of their threshold are left out of the map comparison (cap %d)" % (tag, near.sum(), P, int(1e-4 * P)))
    assert near.sum() <= 1e-4 * P
    assert np.array_equal(labels.reshape(-1)[~near], rdev["labels"][~near])
    assert np.array_equal(net.pl_counts.cpu().numpy()[0], np.bincount(labels.reshape(-1) & 0x7f, minlength=5))
    assert np.array_equal(net.pl_counts.cpu().numpy()[1], np.bincount((labels.reshape(-1) & 0x7f)[labels.reshape(-1) >= 0x80], minlength=5))
    assert abs(float(net.pl_share) - (labels >= 0x80).mean()) <= 1e-6 and 0.5 < float(net.pl_share) < 0.95
    # the oracle, teacher-forced with the device's map
    tot = {}
    for dt, r in res.items():
        term = _oracle_term(r, labels)
        g_pl = _grads(term, r["V"], r["names"])
        tot[dt] = (miu_gen * r["gen1"] + pl_weight * float(term.detach()), float(term.detach()),
                   {k: miu_gen * r["g_gen"][k] + pl_weight * g_pl[k] for k in g_pl}, g_pl)
    (l64, t64, g64, gpl64), (l32, t32, g32, _) = tot[torch.float64], tot[torch.float32]
    n_gen, n_pl = miu_gen * _norm(res[torch.float64]["g_gen"]), pl_weight * _norm(gpl64)
    print("gen+pl (%s): loss hip %.9g cpu32 %.9g fp64 %.9g | L_pl hip %.9g fp64 %.9g | float64 gradient norms: critics %.4g, pseudo-label %.4g"
          % (tag, float(loss), l32, l64, float(net.pl_value), t64, n_gen, n_pl))
    if tag == "a":
        assert n_gen == 0.0 and n_pl > 0.0
    else:
        assert 0.2 < n_gen / n_pl < 5.0             # both terms matter
    r64 = res[torch.float64]
    assert float((net.ct_logits.detach().cpu().double() - r64["ct_logits"]).abs().max()) < 1e-4 * float(r64["ct_logits"].abs().max())
    assert abs(float(loss) - l64) <= 1e-4 * abs(l64)
    assert float(loss) == float(net.ct_gen_loss)
    assert abs(float(net.pl_value) - t64) <= 1e-4 * t64
    # the kernel's value on the step's logits under the thresholds the step started from; the thresholds it left = one update
    v, _, _, lab2, conf2, _ = K.pseudo_label_loss(net.ct_logits.detach().contiguous(), tau0)
    assert torch.equal(net.pl_value, v) and torch.equal(lab2, net.pl_labels)
    t1 = tau0.clone()
    K.pseudo_label_update(lab2, conf2, t1, 0.5, 0.9)
    assert torch.equal(_bits(t1), _bits(net.pl_threshold)) and not torch.equal(_bits(t1), _bits(tau0))
    grad_report("gen+pl-" + tag, g_hip, g64, g32)
    worst = 0.0
    for k in g_hip:
        w = torch.from_numpy(before[k].copy())
        g = g_hip[k] + nets_adv.l2_coefficient(k, "gen", miu=miu_gen, lam=LAM) * w
        T.rmsprop_update(w, g, torch.ones_like(w), LR)
        worst = max(worst, float((w - torch.from_numpy(after[k])).abs().max()))
    print("gen+pl (%s) update: worst weight error %.3e" % (tag, worst))
    assert worst < 1e-7
    for v in net.store.trainable():                 # (the critics' batch-statistics BN layers move their moving averages, as in today's step)
        if not v.name.startswith("adapt_"):
            assert np.array_equal(before[v.name], after[v.name]), v.name


# ---- 4. pl_weight = 0 is today's step; determinism; next to the entropy term; bf16 arithmetic ----------------------------------------
def _one_step(dev, sd, ct, cost):
    net, tr = _net(dev, sd, cost)
    tr.gen_step(torch.from_numpy(ct).to(dev), KEEP, 17)
    torch.cuda.synchronize()
    return net.store.arena.detach().cpu().clone(), net.store.grad_arena.detach().cpu().clone(), net


def test_zero_pl_weight_is_todays_step(dev, case):
    sd, ct, _ = case
    w0, g0, n0 = _one_step(dev, sd, ct, {})
    wz, gz, nz = _one_step(dev, sd, ct, {"pl_weight": 0.0, "pl_init": 0.5, "pl_portion": 0.25})
    assert float(g0.abs().max()) > 0
    assert torch.equal(w0, wz) and torch.equal(g0, gz) and float(n0.ct_gen_loss) == float(nz.ct_gen_loss)
    for n in (n0, nz):
        assert n.pl_value is None and n.pl_share is None and n.pl_counts is None and not hasattr(n, "pl_threshold")
    w1, g1, n1 = _one_step(dev, sd, ct, dict(PL_COST, pl_weight=PL_WEIGHT_B))
    assert not torch.equal(g1, g0) and n1.pl_value is not None        # (and the term does change the step)


def test_gen_step_with_pseudo_labels_is_deterministic(dev, case):
    sd, ct, _ = case
    w1, g1, n1 = _one_step(dev, sd, ct, dict(PL_COST, pl_weight=PL_WEIGHT_B))
    w2, g2, n2 = _one_step(dev, sd, ct, dict(PL_COST, pl_weight=PL_WEIGHT_B))
    assert float(g1.abs().max()) > 0 and torch.equal(g1, g2) and torch.equal(w1, w2)
    assert float(n1.ct_gen_loss) == float(n2.ct_gen_loss) and float(n1.pl_value) == float(n2.pl_value) and float(n1.pl_share) == float(n2.pl_share)
    assert torch.equal(n1.pl_counts, n2.pl_counts) and torch.equal(_bits(n1.pl_threshold), _bits(n2.pl_threshold))


def test_pseudo_labels_next_to_the_entropy_term(dev, case):
    """both weights > 0: three roots in one backward; the gradient is today's plus the two single-term runs' extra gradients (the backward
    pass is linear in what arrives at the logits, the forward pass and its dropout masks are the same in all four runs)"""
    sd, ct, _ = case
    pl, ent = dict(PL_COST, pl_weight=PL_WEIGHT_B), {"ent_weight": 0.8}
    _, g0, n0 = _one_step(dev, sd, ct, {})
    _, ge, ne = _one_step(dev, sd, ct, ent)
    _, gp, np_ = _one_step(dev, sd, ct, pl)
    _, gb, nb = _one_step(dev, sd, ct, dict(pl, **ent))
    assert float(nb.ent_value) == float(ne.ent_value) and float(nb.pl_value) == float(np_.pl_value)
    assert torch.equal(_bits(nb.pl_threshold), _bits(np_.pl_threshold))
    want = float(n0.ct_gen_loss) + 0.8 * float(ne.ent_value) + PL_WEIGHT_B * float(np_.pl_value)
    assert abs(float(nb.ct_gen_loss) - want) <= 1e-6 * abs(want)
    e_ent, e_pl = (ge - g0).double(), (gp - g0).double()
    print("extra gradients: entropy max %.3e, pseudo-label max %.3e, today's max %.3e" % (float(e_ent.abs().max()), float(e_pl.abs().max()),
                                                                                          float(g0.abs().max())))
    assert float(e_ent.abs().max()) > 0 and float(e_pl.abs().max()) > 0
    _bar(gb.double() - g0.double(), e_ent + e_pl, "entropy + pseudo-label extra gradient")


def test_bf16_arithmetic_runs_the_term_on_fp32_logits(dev, case):
    F = pkg("functional")
    sd, ct, _ = case
    F.set_conv_dtype("bf16")
    try:
        _, g, net = _one_step(dev, sd, ct, dict(PL_COST, pl_weight=PL_WEIGHT_B))
    finally:
        F.set_conv_dtype("f32")
    assert net.ct_logits.dtype == torch.float32
    assert np.isfinite(float(net.pl_value)) and float(net.pl_value) > 0 and 0.0 < float(net.pl_share) < 1.0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(net.pl_threshold).all())


# ---- 5. step capture, fp32 -----------------------------------------------------------------------------------------------------------
def test_captured_gen_steps_with_pseudo_labels_equal_eager_bit_for_bit(dev, case):
    sd, ctn, _ = case
    rng = np.random.default_rng(0)
    mr = torch.from_numpy(rng.standard_normal((B, 256, 256, 3)).astype(np.float32)).to(dev)
    ct = torch.from_numpy(ctn).to(dev)
    cost = dict(PL_COST, pl_weight=PL_WEIGHT_B, pl_momentum=0.5)
    tau = torch.tensor(PL_TAU, dtype=torch.float32)

    def run(tr):
        out = []
        for i in range(2):
            out.append(float(tr.dis_step(mr, ct, KEEP, 2 * i + 1)))
            out.append(float(tr.gen_step(ct, KEEP, 2 * i + 2)))
            out += [float(tr.net.pl_value), float(tr.net.pl_share)] + tr.net.pl_counts.cpu().reshape(-1).tolist()
            out += _bits(tr.net.pl_threshold).tolist()              # the thresholds after every round, as bit patterns
        return out
    net_e, tr_e = _net(dev, sd, cost)
    le = run(tr_e)
    w_e = net_e.store.arena.detach().cpu().clone()
    net_c, tr_c = _net(dev, sd, cost)
    ptr = net_c.pl_threshold.data_ptr()
    tr_c.capture_steps(mr, ct, KEEP)
    assert not torch.equal(net_c.pl_threshold.cpu(), tau)        # the warm-up steps are real: they moved the thresholds
    net_c.store.load_state_dict(sd)
    for o in (tr_c.dis_optimizer, tr_c.gen_optimizer):          # RMSProp slots back to their initial value (ones: TF's initial ms)
        o.ms.copy_(torch.ones_like(o.ms))
    net_c.pl_threshold.copy_(tau)                                # and the thresholds, in place: the graph holds their address
    lc = run(tr_c)
    print("captured GAN steps with the pseudo-label term: eager %s captured %s" % (le, lc))
    assert tr_c._cap["dis"].replays == 2 and tr_c._cap["gen"].replays == 2 and net_c.pl_threshold.data_ptr() == ptr
    assert lc == le, (lc, le)
    assert torch.equal(net_c.store.arena.detach().cpu(), w_e)
    assert torch.equal(_bits(net_c.pl_threshold), _bits(net_e.pl_threshold)) and not torch.equal(net_e.pl_threshold.cpu(), tau)


# ---- 6. the entry point ---------------------------------------------------------------------------------------------------------------
def _scalar_rows(path):
    with open(os.path.join(path, "metrics.jsonl")) as f:
        return [r for r in map(json.loads, f) if "pl" in r]


def test_entry_point_with_pl_weight(dev, tmp_path, monkeypatch):
    """the synthetic chain of the entropy test: --phase pre-train (critic alone, no generator step), then train-gan from its checkpoint
    with the term (6 iterations: generator steps at 1 ... 5, the second Dice report at step 5 carries the term), then a second train-gan
    run from that output whose momentum of 1 keeps whatever thresholds it starts from.  The critic's 20 sub-iterations per step of the
    train-gan schedule are cut to 1: the schedule is not what this test is about, and 100 critic steps are most of its time."""
    ts, tg = pkg("train_segmenter"), pkg("train_gan")
    configure = tg.configure

    def short(phase):
        ck, nc, tc = configure(phase)
        if phase == "train-gan":
            assert tc["dis_sub_iter"] > 1
            tc["dis_sub_iter"] = 1
        return ck, nc, tc
    monkeypatch.setattr(tg, "configure", short)
    out1 = str(tmp_path / "seg")
    ts.main(["--synthetic", "6", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out1])
    ck = os.path.join(out1, "checkpoint.npz")
    out2 = str(tmp_path / "gan")
    common = ["--synthetic", "4", "--batch-size", "2", "--epochs", "1", "--output", out2, "--pl-weight", "0.01", "--pl-portion", "0.5"]
    t2 = tg.main("pre-train", common + ["--iters", "3", "--baseline", ck])
    assert t2.net.pl_weight == 0.01 and t2.net.pl_portion == 0.5 and t2.net.pl_value is None      # no generator step in this phase
    assert t2.net.pl_threshold.tolist() == [np.float32(0.9)] * 5
    t3 = tg.main("train-gan", common + ["--iters", "6"])
    assert np.isfinite(float(t3.net.pl_value)) and float(t3.net.pl_value) >= 0.0 and 0.0 <= float(t3.net.pl_share) <= 1.0
    assert np.isfinite(float(t3.net.ct_gen_loss)) and int(t3.net.pl_counts[0].sum()) == 2 * 256 * 256
    saved = t3.net.pl_threshold.cpu().numpy()
    assert np.isfinite(saved).all() and not np.array_equal(saved, np.full(5, 0.9, dtype=np.float32))      # the generator steps moved them
    with np.load(os.path.join(out2, "optimizer.npz")) as z:
        assert np.array_equal(z["pl_threshold"].view(np.uint32), saved.view(np.uint32))
    rows = _scalar_rows(out2)
    live = [r for r in rows if r["pl"] is not None]
    assert live, "no pl row with a value in the scalar log of %s" % out2
    assert all(np.isfinite(r["pl"]) and 0.0 <= r["pl_share"] <= 1.0 and len(r["pl_threshold"]) == 5 and r["kind"] in ("train_eval", "val_eval")
               for r in live)
    t4 = tg.main("train-gan", common + ["--iters", "2", "--pl-momentum", "1.0", "--pl-init", "0.25"])
    assert t4.net.pl_value is not None and t4.net.pl_init == 0.25
    assert np.array_equal(t4.net.pl_threshold.cpu().numpy().view(np.uint32), saved.view(np.uint32))      # from the checkpoint, not from pl_init
