"""-m gpu: the WGAN-GP gradient penalty (gradient_penalty.py, csrc/critic_gp.hip) against the oracle's own graph differentiated twice by
torch autograd in float64: the new kernels, critic_gradient_penalty for both critics, a penalty dis step of the Trainer, determinism,
gp_weight = 0 being today's step, the entry point and the capture refusal."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import nets_adv
from oracle import tf_ops as T
from test_gpu_adversarial import _rel, grad_report, he_state, make_vars

pytestmark = pytest.mark.gpu

KEEP = 0.75
MIU = 0.002
NETCFG = {"mr_front_trainable": False, "joint_trainable": False, "ct_front_trainable": False, "cls_trainable": True, "m_cls_trainable": True}


def _bar(got, ref, what, tol=1e-5):
    got = torch.as_tensor(got).detach().cpu().double()
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    print("%s: max err %.3e of max|ref| %.3e (%.2e)" % (what, err, scale, err / (scale + 1e-300)))
    assert err <= tol * scale + 1e-30, what


# ---- 1. the new kernels against float64 -------------------------------------------------------------------------------------------
def test_interpolation_kernel(dev):
    K = pkg("kernels")
    rng = np.random.default_rng(1)
    for shape in ((3, 8, 8, 32), (5, 7, 3, 5)):
        a = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
        b = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
        out, eps = K.gp_interpolate(a, b, 7, 123)
        e = eps.cpu().double()
        assert bool(((e >= 0) & (e < 1)).all()) and len(set(e.tolist())) == shape[0]
        ref = e.view(-1, 1, 1, 1) * a.cpu().double() + (1 - e.view(-1, 1, 1, 1)) * b.cpu().double()
        _bar(out, ref, "interp %s" % (shape,))
        out2, eps2 = K.gp_interpolate(a, b, 7, 124)
        assert not torch.equal(eps, eps2)                  # eps follows the stream id


def test_penalty_kernel_norms_value_adjoint(dev):
    K = pkg("kernels")
    rng = np.random.default_rng(2)
    for shape in ((4, 16, 16, 8), (3, 5, 7, 3)):
        g = rng.standard_normal(shape) * 0.3
        g[2] = 0.0                                          # an all-zero sample: zero adjoint, not NaN
        gt = torch.from_numpy(g.astype(np.float32)).to(dev)
        g64 = gt.cpu().double()
        coef, gscale = 10.0, 0.5
        pen, norms = K.gp_penalty_(gt, coef, gscale)
        n = g64.flatten(1).norm(dim=1)
        _bar(norms, n, "norms %s" % (shape,))
        ref_p = coef * ((n - 1) ** 2).mean()
        _bar(pen, ref_p.view(1), "penalty %s" % (shape,))
        x = g64.clone().requires_grad_(True)
        P = coef * ((x.flatten(1).norm(dim=1) - 1) ** 2).mean()
        (adj,) = torch.autograd.grad(P, x)
        adj = torch.nan_to_num(adj, nan=0.0) * gscale
        assert torch.isfinite(gt).all() and float(gt[2].abs().max()) == 0.0
        _bar(gt, adj, "adjoint %s" % (shape,))


@pytest.mark.parametrize("shape,keep,with_sc", [((16, 64, 64, 64), 0.75, True), ((16, 64, 64, 64), 1.0, False),
                                                ((3, 17, 19, 5), 0.75, True), ((3, 17, 19, 5), 1.0, False)])
def test_bn_double_backward_kernel(dev, shape, keep, with_sc):
    K = pkg("kernels")
    eps_bn, alpha, seed, sid = 1e-3, 0.2, 5, 9
    N, H, W, C = shape
    Cs = C // 2 + (C % 2) if with_sc else 0            # inc_dim shortcut: C = Cs + 2 * (Cs // 2)
    if with_sc:
        assert Cs + 2 * (Cs // 2) == C
    rng = np.random.default_rng(3)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    d = f32(rng.standard_normal(shape) * 1.3 + 0.2)
    gamma = f32(1.0 + 0.3 * rng.standard_normal(C))
    beta = f32(0.1 * rng.standard_normal(C))
    gy = f32(rng.standard_normal(shape))
    gcb = f32(rng.standard_normal(shape))
    sc = f32(rng.standard_normal((N, H, W, Cs))) if with_sc else None
    scb = f32(rng.standard_normal((N, H, W, Cs))) if with_sc else None
    mask = torch.from_numpy(T.dropout_mask(shape, keep, seed, sid)).double()
    kp = float(np.float32(keep))
    # float64 reference: L = <gcb, g_c> + <scb, crop(g_z)>, g_c = mask/keep * d(BN)/d(d)^T g_z, g_z = g_y * leaky'(z)
    d64, ga64, gy64 = d.double().requires_grad_(True), gamma.double().requires_grad_(True), gy.double().requires_grad_(True)
    mean = d64.mean(dim=(0, 1, 2))
    var = ((d64 - mean) ** 2).mean(dim=(0, 1, 2))
    zpre = (d64 - mean) * (ga64 / torch.sqrt(var + eps_bn)) + beta.double()
    z = zpre + (T.pad_channels(sc.double(), (C - Cs) // 2) if with_sc else 0)
    lk = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, alpha)).detach()
    y = torch.where(z > 0, z, z * alpha).detach()
    gz = gy64 * lk
    (gd,) = torch.autograd.grad(zpre, d64, grad_outputs=gz, create_graph=True)
    gc = gd * mask / kp
    L = (gcb.double() * gc).sum()
    if with_sc:
        c0 = (C - Cs) // 2
        L = L + (scb.double() * gz[..., c0:c0 + Cs]).sum()
    r_gy, r_d, r_ga = torch.autograd.grad(L, [gy64, d64, ga64])
    gb = torch.zeros(C, dtype=torch.float32, device=dev)
    dv = lambda t: t.to(dev) if t is not None else None
    gyb, xcb = K.bn_dbl_bwd(dv(gcb), dv(d), dv(y.float()), dv(gy), dv(mean.detach().float()), dv(var.detach().float()), dv(gamma),
                            dv(scb), eps_bn, alpha, keep, seed, sid, gamma_bar=gb)
    tag = "%s keep %.2f sc %s" % (shape, keep, with_sc)
    _bar(gyb, r_gy, "bn dbl gy_bar " + tag)
    _bar(xcb, r_d * mask / kp, "bn dbl xc_bar " + tag)
    _bar(gb, r_ga, "bn dbl gamma_bar " + tag)


# ---- oracle: the critic body from _Ctx, differentiated twice ---------------------------------------------------------------------
def _cls_body(c, x):
    """nets_adv._classifier after its input assembly"""
    p = "cls_scope/"
    h = x
    for k, kd, sd in [(1, 3, 2), (2, 5, 2), (3, 3, 2), (4, 3, 2), (5, 5, 4)]:
        s = p + "cls_%d/" % k
        h = c.rb(h, s + "Variable", s + "Variable_1", s + "cls_%d" % k, True, keep=c.critic_keep)
        h = c.cbr(h, s + "Variable_2", s + "cls_%d_3" % k, True, stride=sd, keep=c.critic_keep)
    h = c.cbr(h, p + "cls_6/Variable", p + "cls_6/cls_6", True, stride=2, padding="SYMMETRIC", keep=c.critic_keep)
    return c.fc(h, p + "cls_out/Variable")


def oracle_penalty(V, critic, xa, xb, eps, coef, seed, sid0):
    """coef * mean_i (|grad_{x_hat_i} sum_j miu f(x_hat_j)| - 1)^2 on the oracle's graph; BN moving statistics on copies (the oracle's
    batch_norm updates them on every training-mode call, the product's penalty pass does not).  -> (P, norms)"""
    Vc = {k: (v.detach().clone() if k.endswith(("moving_mean", "moving_variance")) else v) for k, v in V.items()}
    dt = xa.dtype
    e = eps.to(dt).view(-1, 1, 1, 1)
    xh = (e * xa + (1 - e) * xb).detach().requires_grad_(True)
    c = nets_adv._Ctx(Vc, KEEP, seed, critic_keep=KEEP)
    c.sid = sid0
    f = MIU * (_cls_body(c, xh) if critic == "cls" else nets_adv._mask_critic(c, xh))
    (g,) = torch.autograd.grad(f.sum(), xh, create_graph=True)
    n = g.flatten(1).norm(dim=1)
    return coef * ((n - 1) ** 2).mean(), n.detach()


@pytest.fixture(scope="module")
def critic_inputs():
    """real critic inputs of both domains: the oracle's float32 forward (its critic_input record and the segmenter logits)"""
    adv = pkg("adversarial")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=2, network_config=dict(NETCFG), device="cpu", seed=1)
    sd = he_state(net, 7)
    rng = np.random.default_rng(0)
    mr = torch.from_numpy(rng.standard_normal((2, 256, 256, 3)).astype(np.float32))
    ct = torch.from_numpy((rng.standard_normal((2, 256, 256, 3)) * 1.2 + 0.1).astype(np.float32))
    V = make_vars(sd, torch.float32, lambda k: False)
    units = []
    with torch.no_grad():
        o = nets_adv.adv_forward(V, mr, ct, KEEP, seed=11, segmenter_no_grad=True, units=units)
    cin = {r["branch"]: r["out"].detach() for r in units if r["kind"] == "critic_input"}
    return sd, {"cls": (cin["mr"], cin["ct"]), "mask": (o["mr_logits"].detach(), o["ct_logits"].detach())}


# ---- 2. critic_gradient_penalty for each critic at B = 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("critic", ["cls", "mask"])
def test_critic_gradient_penalty_vs_float64_oracle(dev, critic_inputs, critic):
    adv, gp = pkg("adversarial"), pkg("gradient_penalty")
    sd, ins = critic_inputs
    xa, xb = ins[critic]
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=2, cost_kwargs={"gp_weight": 10.0}, network_config=dict(NETCFG), device=dev, seed=1)
    net.store.load_state_dict(sd)
    net.store.zero_grad()
    coef, seed, s0 = 10.0, 21, 40
    stats0 = {k: v.tensor.detach().cpu().clone() for k, v in net.store.vars.items() if k.endswith(("moving_mean", "moving_variance"))}
    pen, norms, eps, nxt = gp.critic_gradient_penalty(net, critic, xa.to(dev), xb.to(dev), coef, seed, s0)
    units, fc = gp.unit_plan(critic, net.feature_base, net.n_class)
    assert nxt == s0 + len(units) + 1
    scope = "cls_scope/" if critic == "cls" else "mask_cls_scope/"
    g_hip = {v.name: v.tensor.grad.detach().cpu().clone() for v in net.store.trainable() if v.name.startswith(scope)}
    assert all(float(v.tensor.grad.abs().max()) == 0.0 for v in net.store.trainable() if not v.name.startswith(scope))
    for k, v in stats0.items():                     # the penalty pass leaves the moving statistics alone
        assert torch.equal(net.store.vars[k].tensor.detach().cpu(), v), k
    res = {}
    for dt in (torch.float32, torch.float64):
        V = make_vars(sd, dt, lambda k: k.startswith(scope))
        P, n = oracle_penalty(V, critic, xa.to(dt), xb.to(dt), eps.cpu(), coef, seed, s0)
        names = [k for k in V if V[k].requires_grad]
        gr = torch.autograd.grad(P, [V[k] for k in names], allow_unused=True)
        res[dt] = (P.detach(), n, {k: (g if g is not None else torch.zeros_like(V[k])) for k, g in zip(names, gr)},
                   {k for k, g in zip(names, gr) if g is None})
    P64, n64, g64, unused = res[torch.float64]
    P32, n32, g32, _ = res[torch.float32]
    print("%s penalty hip %.9g cpu32 %.9g fp64 %.9g | norms hip %s fp64 %s" % (critic, float(pen), float(P32), float(P64), norms.cpu().tolist(),
                                                                             n64.tolist()))
    assert abs(float(pen) - float(P64)) <= 1e-4 * abs(float(P64)) + 1e-9
    assert _rel(norms.cpu(), n64) < 1e-4
    for k in unused:                                # (torch: cls_6/beta only feeds a leaky-ReLU slope switch)
        assert float(g_hip[k].abs().max()) == 0.0, k
    print("%s: variables without a penalty gradient (torch: unused): %s" % (critic, sorted(unused)))
    grad_report("gp-" + critic, {k: g_hip[k] for k in g64 if k not in unused}, {k: v for k, v in g64.items() if k not in unused},
                {k: v for k, v in g32.items() if k not in unused})


# ---- 3. one Trainer.dis_step with gp_weight = 10 against the oracle (WGAN + L2 + penalty -> RMSProp, no clamp) ---------------------
def _trainer(adv, net):
    tr = adv.Trainer(net, None, None, None, None, num_cls=5, batch_size=2, opt_kwargs={"learning_rate": 3e-4}, train_config={"dis_sub_iter": 1})
    tr._get_optimizer()
    return tr


def _gp_net(adv, dev, sd, cost=None):
    ck = {"miu_dis": MIU, "lambda_mask_loss": 0.0}
    ck.update(cost or {})
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=2, cost_kwargs=ck, network_config=dict(NETCFG), device=dev, seed=1)
    net.store.load_state_dict(sd)
    return net


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(5)
    mr = rng.standard_normal((2, 256, 256, 3)).astype(np.float32)
    ct = (rng.standard_normal((2, 256, 256, 3)) * 1.2 + 0.1).astype(np.float32)
    return mr, ct


def test_dis_step_with_penalty_vs_oracle(dev, critic_inputs, batches):
    adv = pkg("adversarial")
    sd, _ = critic_inputs
    mr, ct = batches
    net = _gp_net(adv, dev, sd, {"gp_weight": 10.0})
    tr = _trainer(adv, net)
    before = net.store.state_dict()
    seed = 13
    tr.dis_step(torch.from_numpy(mr).to(dev), torch.from_numpy(ct).to(dev), KEEP, seed)
    g_hip = {v.name: v.tensor.grad.detach().cpu().clone() for v in net.store.trainable() if "cls" in v.name}
    after = net.store.state_dict()
    s0, eps = net.gp_stream0["cls"], net.gp_eps["cls"].cpu()
    assert set(net.gp_stream0) == {"cls"}          # lambda_mask_loss = 0 (--phase pre-train): the feature critic only
    res = {}
    for dt in (torch.float32, torch.float64):
        V = make_vars(sd, dt, lambda k: "cls" in k)
        units = []
        o = nets_adv.adv_forward(V, torch.from_numpy(mr).to(dt), torch.from_numpy(ct).to(dt), KEEP, seed=seed, segmenter_no_grad=True, units=units)
        dis, _ = nets_adv.wgan_losses(o, miu_dis=MIU, lam=0.0)
        cin = {r["branch"]: r["out"].detach() for r in units if r["kind"] == "critic_input"}
        P, _ = oracle_penalty(V, "cls", cin["mr"], cin["ct"], eps, 10.0, seed, s0)
        (dis + P).backward()
        res[dt] = (float((dis + P).detach()), {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in V.items() if v.requires_grad})
    (l64, g64), (l32, g32) = res[torch.float64], res[torch.float32]
    print("dis + gp loss hip %.9g cpu32 %.9g fp64 %.9g (gp %.6g)" % (float(net.dis_loss), l32, l64, float(net.gp_value)))
    assert abs(float(net.dis_loss) - l64) <= 1e-4 * abs(l64) + 1e-8
    for k in g_hip:                                  # lambda_mask_loss = 0: the mask critic takes no gradient at all
        if k.startswith("mask_cls_scope/"):
            assert float(g_hip[k].abs().max()) == 0.0 and float(g64[k].abs().max()) == 0.0, k
    fc = lambda d: {k: v for k, v in d.items() if k.startswith("cls_scope/")}
    grad_report("dis+gp", fc(g_hip), fc(g64), fc(g32))
    worst = 0.0
    for k in g_hip:
        w = torch.from_numpy(before[k].copy())
        g = g_hip[k] + nets_adv.l2_coefficient(k, "dis", miu=MIU, lam=0.0, sub_iter=1) * w
        T.rmsprop_update(w, g, torch.ones_like(w), 3e-4)         # no clamp: the penalty replaces the clip
        worst = max(worst, float((w - torch.from_numpy(after[k])).abs().max()))
    print("dis+gp update: worst weight error %.3e" % worst)
    assert worst < 1e-7
    big = max(float(np.abs(after[k]).max()) for k in after if "cls" in k and "Variable" in k)
    assert big > 0.03, big                           # the clip did not run


# ---- 4. determinism, 5. gp_weight = 0 is today's step ----------------------------------------------------------------------------
def _one_step(adv, dev, sd, batches, cost):
    mr, ct = batches
    net = _gp_net(adv, dev, sd, cost)
    tr = _trainer(adv, net)
    tr.dis_step(torch.from_numpy(mr).to(dev), torch.from_numpy(ct).to(dev), KEEP, 17)
    torch.cuda.synchronize()
    return net.store.arena.detach().cpu().clone(), net.store.grad_arena.detach().cpu().clone(), net


def test_penalty_dis_step_is_deterministic(dev, critic_inputs, batches):
    adv = pkg("adversarial")
    sd, _ = critic_inputs
    w1, g1, n1 = _one_step(adv, dev, sd, batches, {"gp_weight": 10.0, "lambda_mask_loss": 0.3})
    w2, g2, n2 = _one_step(adv, dev, sd, batches, {"gp_weight": 10.0, "lambda_mask_loss": 0.3})
    assert set(n1.gp_stream0) == {"cls", "mask"}
    assert float(g1.abs().max()) > 0 and torch.equal(g1, g2) and torch.equal(w1, w2)
    assert float(n1.dis_loss) == float(n2.dis_loss) and float(n1.gp_value) == float(n2.gp_value)


def test_zero_gp_weight_is_todays_step(dev, critic_inputs, batches):
    adv = pkg("adversarial")
    sd, _ = critic_inputs
    w0, g0, n0 = _one_step(adv, dev, sd, batches, None)
    wz, gz, nz = _one_step(adv, dev, sd, batches, {"gp_weight": 0.0})
    assert torch.equal(w0, wz) and torch.equal(g0, gz) and float(n0.dis_loss) == float(nz.dis_loss)
    assert getattr(nz, "gp_value", None) is None


# ---- 6. entry point, 7. capture refusal ------------------------------------------------------------------------------------------
def test_pretrain_entry_point_with_gp_weight(dev, tmp_path):
    ts, tg = pkg("train_segmenter"), pkg("train_gan")
    out1 = str(tmp_path / "seg")
    ts.main(["--synthetic", "6", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out1])
    ck = os.path.join(out1, "checkpoint.npz")
    out2 = str(tmp_path / "gan")
    t2 = tg.main("pre-train", ["--synthetic", "4", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out2, "--baseline", ck,
                               "--gp-weight", "10"])
    assert t2.net.gp_weight == 10.0 and t2.global_step == 2
    assert np.isfinite(float(t2.net.gp_value)) and float(t2.net.gp_value) > 0 and np.isfinite(float(t2.net.dis_loss))
    st = t2.net.store.state_dict()
    big = max(float(np.abs(v).max()) for k, v in st.items() if "cls" in k and "Variable" in k)
    assert big > 0.03 + 1e-9, big                   # not clipped


def test_capture_steps_refuses_the_penalty(dev):
    adv = pkg("adversarial")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=2, cost_kwargs={"gp_weight": 10.0}, network_config=dict(NETCFG), device=dev)
    tr = _trainer(adv, net)
    x = torch.zeros((2, 256, 256, 3), device=dev)
    with pytest.raises(RuntimeError, match="gradient-penalty"):
        tr.capture_steps(x, x, KEEP)
