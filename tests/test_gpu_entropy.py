"""-m gpu: entropy minimisation on the CT predictions (csrc/entropy.hip): the kernel against the float64 restatement of
tests/entropy_ref.py, the generator step with the term against the CPU oracle (oracle/nets_adv.py) with the term added in torch,
ent_weight = 0 being today's step, determinism, step capture, the label-free monitor and the entry point."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from entropy_ref import entropy_ref, special_rows
from kernel_bars import _bar, _value_bar
from oracle import nets_adv
from oracle import tf_ops as T
from test_gpu_adversarial import COST, NETCFG, grad_report, he_state, make_vars

pytestmark = pytest.mark.gpu

KEEP = 0.75
LR = 3e-4


# ---- 1. the kernel against float64 ------------------------------------------------------------------------------------------------
# C = 5: below one four-pixel group, one group, a group and a tail, many blocks with a tail, whole groups only; the other class counts on
# the generic path; 2 * 256 * 256 pixels: 64 blocks of 256 threads, every thread walks the grid-stride loop twice
SHAPES = [(P, 5) for P in (1, 3, 4, 7, 1021, 2 * 64 * 64)] + [(257, C) for C in (1, 2, 3, 8)] + [(2 * 256 * 256, 5)]


def _logits(P, C, seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((P, C)) * 3.0).astype(np.float32)
    return z, special_rows(z, rng)


def _check_against_reference(K, zd, z, idx, coef, what):
    ref_v, ref_g = entropy_ref(z, coef)
    v, g = K.softmax_entropy(zd, coef=coef, want_grad=True)
    v0, g0 = K.softmax_entropy(zd)
    v2, g2 = K.softmax_entropy(zd, coef=coef, want_grad=True)
    assert g0 is None and tuple(v.shape) == (1,) and g.shape == zd.shape
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all()), what
    C = z.shape[-1]
    if C == 1:
        assert float(v) == 0.0 and float(g.abs().max()) == 0.0          # one class: entropy 0, no normaliser
    else:
        _value_bar(v, ref_v, what)
        _bar(g, torch.from_numpy(ref_g), what + " gradient")
        assert 0.0 <= float(v) <= 1.0
    assert torch.equal(v0, v), "dlogits = NULL changes the value"      # bit for bit
    assert torch.equal(v2, v) and torch.equal(g2, g), "two runs differ"
    # the special rows, each on its own (P = 1: normalised entropy of that row, gradient at its largest scale 1 / ln C)
    for kind, rows in idx.items():
        for r in rows:
            vr, gr = K.softmax_entropy(zd[r:r + 1], want_grad=True)
            assert bool(torch.isfinite(vr).all()) and bool(torch.isfinite(gr).all()), (what, kind, r)
            assert bool(torch.isfinite(g[r]).all())
            if kind == "equal":
                assert abs(float(vr) - 1.0) <= 1e-6 and float(gr.abs().max()) <= 1e-6 and float(g[r].abs().max()) <= 1e-6, (what, kind, r)
            elif kind == "ahead":
                assert 0.0 <= float(vr) <= 1e-6 and float(gr.abs().max()) <= 1e-6, (what, kind, r)
            else:
                assert 0.0 <= float(vr) <= 1.0 + 1e-6, (what, kind, r)
    return v, g


@pytest.mark.parametrize("P,C", SHAPES)
def test_kernel_against_float64(dev, P, C):
    K = pkg("kernels")
    z, idx = _logits(P, C, 100 * C + P % 97)
    zd = torch.from_numpy(z).to(dev)
    assert zd.data_ptr() % 16 == 0
    _check_against_reference(K, zd, z, idx, 0.375 * 0.25, "P=%d C=%d" % (P, C))


@pytest.mark.parametrize("P", [7, 1021])
def test_kernel_misaligned_base_takes_the_fallback(dev, P):
    """logits that start one pixel (20 bytes) into an allocation: no float4 load is aligned, the launch takes the generic path"""
    K = pkg("kernels")
    z, idx = _logits(P, 5, 7 + P)
    base = torch.zeros((P + 1, 5), device=dev)
    base[1:] = torch.from_numpy(z).to(dev)
    zd = base[1:]
    assert zd.is_contiguous() and zd.data_ptr() % 16 != 0
    v, g = _check_against_reference(K, zd, z, idx, 1.0, "misaligned P=%d" % P)
    va, ga = K.softmax_entropy(zd.clone(), want_grad=True)         # the aligned copy on the vector path: the same numbers to the bar
    _bar(g, ga.detach().cpu(), "misaligned against aligned")
    assert abs(float(v) - float(va)) <= 1e-6 * float(va)


def test_autograd_function_scales_by_coef_and_gscale(dev):
    F = pkg("functional")
    z, _ = _logits(1021, 5, 3)
    for coef, gscale in ((1.0, 1.0), (0.01, 0.125), (2.5, 0.5)):
        zd = torch.from_numpy(z).to(dev).requires_grad_(True)
        val = F.EntropyLossFn.apply(zd, coef, gscale)
        val.backward(torch.ones(1, device=dev))
        ref_v, ref_g = entropy_ref(z, coef * gscale)
        _value_bar(val.detach(), ref_v, "EntropyLossFn coef %g gscale %g" % (coef, gscale))      # the value is not scaled
        _bar(zd.grad, torch.from_numpy(ref_g), "EntropyLossFn gradient coef %g gscale %g" % (coef, gscale))


def test_refusals_come_before_any_launch(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    with pytest.raises(L.PnpError, match="at most 8 classes"):
        K.softmax_entropy(torch.zeros((4, 9), device=dev))
    with pytest.raises(L.PnpError, match="CPU"):
        K.softmax_entropy(torch.zeros((4, 5)))
    P = 1021
    z = torch.zeros((P, 5), device=dev)
    out = torch.full((1,), -7.0, device=dev)
    dl = torch.full((P, 5), -7.0, device=dev)
    need = lib.pnp_softmax_entropy_workspace_bytes(P, 5)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    code = lib.pnp_softmax_entropy(p(z), P, 5, 1.0, p(dl), p(out), p(ws), need - 1, st)
    with pytest.raises(L.PnpError, match="workspace too small"):
        L.check(code, "pnp_softmax_entropy")
    torch.cuda.synchronize()
    assert float(out) == -7.0 and float(dl.min()) == -7.0 and float(dl.max()) == -7.0 and int(ws.min()) == 0x5A and int(ws.max()) == 0x5A
    L.check(lib.pnp_softmax_entropy(p(z), P, 5, 1.0, p(dl), p(out), p(ws), need, st), "pnp_softmax_entropy")      # exactly enough is enough
    assert abs(float(out) - 1.0) <= 1e-6 and float(dl.abs().max()) <= 1e-6


# ---- 2. the generator step with the term against the oracle, B = 2 ----------------------------------------------------------------
B = 2
LAM = COST["lambda_mask_loss"]
GEN_SEED = 23


@pytest.fixture(scope="module")
def case():
    """weights, one CT batch, and the oracle's two pieces in float32 and float64 — the graph does not depend on the cost, so one walk per
    type serves every weighting: gen(miu_gen) = miu_gen * gen(1), total gradient = miu_gen * d gen(1) + ent_weight * d L_ent"""
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
        z = o["ct_logits"]
        ent = -(torch.softmax(z, -1) * torch.log_softmax(z, -1)).sum(-1).mean() / float(np.log(5.0))
        names = [k for k in V if V[k].requires_grad]
        zero = lambda gs: {k: (g if g is not None else torch.zeros_like(V[k])) for k, g in zip(names, gs)}
        g_gen = zero(torch.autograd.grad(gen1, [V[k] for k in names], retain_graph=True, allow_unused=True))
        g_ent = zero(torch.autograd.grad(ent, [V[k] for k in names], allow_unused=True))
        res[dt] = {"gen1": float(gen1.detach()), "ent": float(ent.detach()), "g_gen": g_gen, "g_ent": g_ent, "ct_logits": z.detach()}
    return sd, ct, res


def _net(dev, sd, cost):
    adv = pkg("adversarial")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(COST, **cost), network_config=dict(NETCFG), device=dev, seed=1)
    net.store.load_state_dict(sd)
    tr = adv.Trainer(net, None, None, None, None, num_cls=5, batch_size=B, opt_kwargs={"learning_rate": LR},
                     train_config={"dis_sub_iter": 1, "gen_sub_iter": 1})
    tr._get_optimizer()
    return net, tr


def _norm(gs):
    return float(sum(float((g.double() ** 2).sum()) for g in gs.values()) ** 0.5)


# (a) miu_gen = 0: the adapt_* gradients come from the entropy alone — the new path and nothing else
# (b) the reference's miu_gen and lambda_mask_loss = 0.3: the mask critic, the feature critic and the entropy all feed ct_logits; at these
#     weights the float64 oracle's two gradient norms are 0.131 * (miu_gen / 0.002) and 0.157 * ent_weight: ent_weight = 0.8 balances them
@pytest.mark.parametrize("tag,miu_gen,ent_weight", [("a", 0.0, 1.0), ("b", COST["miu_gen"], 0.8)])
def test_gen_step_with_entropy_vs_oracle(dev, case, tag, miu_gen, ent_weight):
    K = pkg("kernels")
    sd, ct, res = case
    net, tr = _net(dev, sd, {"miu_gen": miu_gen, "ent_weight": ent_weight})
    assert net.lambda_mask_loss == LAM and net.ent_weight == ent_weight
    before = net.store.state_dict()
    loss = tr.gen_step(torch.from_numpy(ct).to(dev), KEEP, GEN_SEED)
    g_hip = {v.name: v.tensor.grad.detach().cpu().clone() for v in net.store.trainable() if v.name.startswith("adapt_")}
    for v in net.store.trainable():                 # variables outside adapt_* get zero gradient
        if not v.name.startswith("adapt_"):
            assert float(v.tensor.grad.abs().max()) == 0.0, v.name
    after = net.store.state_dict()
    tot = {}
    for dt, r in res.items():
        tot[dt] = (miu_gen * r["gen1"] + ent_weight * r["ent"],
                   {k: miu_gen * r["g_gen"][k] + ent_weight * r["g_ent"][k] for k in r["g_gen"]})
    (l64, g64), (l32, g32) = tot[torch.float64], tot[torch.float32]
    r64 = res[torch.float64]
    n_gen, n_ent = miu_gen * _norm(r64["g_gen"]), ent_weight * _norm(r64["g_ent"])
    print("gen+ent (%s): loss hip %.9g cpu32 %.9g fp64 %.9g | L_ent hip %.9g fp64 %.9g | float64 gradient norms: critics %.4g, entropy %.4g"
          % (tag, float(loss), l32, l64, float(net.ent_value), r64["ent"], n_gen, n_ent))
    if tag == "a":
        assert n_gen == 0.0 and n_ent > 0.0
    else:
        assert 0.2 < n_gen / n_ent < 5.0             # both terms matter
    assert float((net.ct_logits.detach().cpu().double() - r64["ct_logits"]).abs().max()) < 1e-4 * float(r64["ct_logits"].abs().max())
    assert abs(float(loss) - l64) <= 1e-4 * abs(l64)
    assert float(loss) == float(net.ct_gen_loss)
    assert abs(float(net.ent_value) - r64["ent"]) <= 1e-4 * r64["ent"]
    assert torch.equal(net.ent_value, K.softmax_entropy(net.ct_logits.detach().contiguous())[0])      # the kernel's value on the step's logits
    grad_report("gen+ent-" + tag, g_hip, g64, g32)
    worst = 0.0
    for k in g_hip:
        w = torch.from_numpy(before[k].copy())
        g = g_hip[k] + nets_adv.l2_coefficient(k, "gen", miu=miu_gen, lam=LAM) * w
        T.rmsprop_update(w, g, torch.ones_like(w), LR)
        worst = max(worst, float((w - torch.from_numpy(after[k])).abs().max()))
    print("gen+ent (%s) update: worst weight error %.3e" % (tag, worst))
    assert worst < 1e-7
    for v in net.store.trainable():                 # (the critics' batch-statistics BN layers move their moving averages, as in today's step)
        if not v.name.startswith("adapt_"):
            assert np.array_equal(before[v.name], after[v.name]), v.name


# ---- 3. ent_weight = 0 is today's step; the step with the term is deterministic -----------------------------------------------------
def _one_step(dev, sd, ct, cost):
    net, tr = _net(dev, sd, cost)
    tr.gen_step(torch.from_numpy(ct).to(dev), KEEP, 17)
    torch.cuda.synchronize()
    return net.store.arena.detach().cpu().clone(), net.store.grad_arena.detach().cpu().clone(), net


def test_zero_ent_weight_is_todays_step(dev, case):
    sd, ct, _ = case
    w0, g0, n0 = _one_step(dev, sd, ct, {})
    wz, gz, nz = _one_step(dev, sd, ct, {"ent_weight": 0.0})
    assert float(g0.abs().max()) > 0
    assert torch.equal(w0, wz) and torch.equal(g0, gz) and float(n0.ct_gen_loss) == float(nz.ct_gen_loss)
    assert n0.ent_value is None and nz.ent_value is None
    w1, g1, n1 = _one_step(dev, sd, ct, {"ent_weight": 0.8})
    assert not torch.equal(g1, g0) and n1.ent_value is not None        # (and the term does change the step)


def test_gen_step_with_entropy_is_deterministic(dev, case):
    sd, ct, _ = case
    w1, g1, n1 = _one_step(dev, sd, ct, {"ent_weight": 0.8})
    w2, g2, n2 = _one_step(dev, sd, ct, {"ent_weight": 0.8})
    assert float(g1.abs().max()) > 0 and torch.equal(g1, g2) and torch.equal(w1, w2)
    assert float(n1.ct_gen_loss) == float(n2.ct_gen_loss) and float(n1.ent_value) == float(n2.ent_value)


def test_bf16_arithmetic_keeps_fp32_logits(dev, case):
    """--dtype bf16: the logits convolution is not served by the bf16-resident kernels, ct_logits stays float32 and the term runs"""
    F = pkg("functional")
    sd, ct, _ = case
    F.set_conv_dtype("bf16")
    try:
        _, g, net = _one_step(dev, sd, ct, {"ent_weight": 0.8})
    finally:
        F.set_conv_dtype("f32")
    assert net.ct_logits.dtype == torch.float32
    assert np.isfinite(float(net.ent_value)) and 0.0 < float(net.ent_value) < 1.0 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


# ---- 4. step capture, fp32 -----------------------------------------------------------------------------------------------------------
def test_captured_gen_steps_with_entropy_equal_eager_bit_for_bit(dev, case):
    sd, ctn, _ = case
    rng = np.random.default_rng(0)
    mr = torch.from_numpy(rng.standard_normal((B, 256, 256, 3)).astype(np.float32)).to(dev)
    ct = torch.from_numpy(ctn).to(dev)

    def run(tr):
        out = []
        for i in range(2):
            out.append(float(tr.dis_step(mr, ct, KEEP, 2 * i + 1)))
            out.append(float(tr.gen_step(ct, KEEP, 2 * i + 2)))
            out.append(float(tr.net.ent_value))
        return out
    net_e, tr_e = _net(dev, sd, {"ent_weight": 0.8})
    le = run(tr_e)
    w_e = net_e.store.arena.detach().cpu().clone()
    net_c, tr_c = _net(dev, sd, {"ent_weight": 0.8})
    tr_c.capture_steps(mr, ct, KEEP)
    net_c.store.load_state_dict(sd)
    for o in (tr_c.dis_optimizer, tr_c.gen_optimizer):          # RMSProp slots back to their initial value (ones: TF's initial ms)
        o.ms.copy_(torch.ones_like(o.ms))
    lc = run(tr_c)
    print("captured GAN steps with the entropy term: eager %s captured %s" % (le, lc))
    assert tr_c._cap["dis"].replays == 2 and tr_c._cap["gen"].replays == 2
    assert lc == le, (lc, le)
    assert torch.equal(net_c.store.arena.detach().cpu(), w_e)


# ---- 5. the monitor ------------------------------------------------------------------------------------------------------------------
def test_evaluate_entropy_monitor(dev, case):
    K, lib = pkg("kernels"), pkg("lib")
    sd, ctn, _ = case
    net, _ = _net(dev, sd, {})
    rng = np.random.default_rng(1)
    ct = torch.from_numpy(ctn).to(dev)
    mr = torch.from_numpy(rng.standard_normal((B, 256, 256, 3)).astype(np.float32)).to(dev)
    y = lib.label_decomp_device(5, torch.from_numpy(rng.integers(0, 5, (B, 256, 256)).astype(np.float32)).to(dev))
    r0 = net.evaluate(ct, y, mr, y)
    assert not hasattr(net, "ct_entropy_eval") and not hasattr(net, "ct_logits_eval")
    pred0 = net.compact_pred.clone()
    r1 = net.evaluate(ct, y, mr, y, entropy=True)
    assert r1 == r0 and torch.equal(net.compact_pred, pred0)       # the return value does not change
    assert torch.equal(net.ct_entropy_eval, K.softmax_entropy(net.ct_logits_eval)[0])
    ref_v, _ = entropy_ref(net.ct_logits_eval.cpu().numpy())
    print("ct_entropy_eval %.6f (float64 of the same logits %.6f)" % (float(net.ct_entropy_eval), ref_v))
    assert 0.0 <= float(net.ct_entropy_eval) <= 1.0 and abs(float(net.ct_entropy_eval) - ref_v) <= 1e-5 * ref_v
    assert net.evaluate(ct, y, mr, y, ct_labelled=False, entropy=True)[0] is None and 0.0 <= float(net.ct_entropy_eval) <= 1.0


def _scalar_rows(path):
    with open(os.path.join(path, "metrics.jsonl")) as f:
        return [r for r in map(json.loads, f) if "ct_entropy" in r]


def test_entry_point_with_ent_weight_and_monitor(dev, tmp_path):
    """--phase pre-train trains the critic alone (gen_interval = 0): it shows the flags and the monitor; the train-gan phase that continues
    from its checkpoint runs generator steps with the term (3 iterations: steps 1 and 2 update)"""
    ts, tg = pkg("train_segmenter"), pkg("train_gan")
    out1 = str(tmp_path / "seg")
    ts.main(["--synthetic", "6", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out1])
    ck = os.path.join(out1, "checkpoint.npz")
    out2 = str(tmp_path / "gan")
    common = ["--synthetic", "4", "--batch-size", "2", "--iters", "3", "--epochs", "1", "--output", out2, "--ent-weight", "0.01", "--monitor-entropy"]
    t2 = tg.main("pre-train", common + ["--baseline", ck])
    assert t2.net.ent_weight == 0.01 and t2.train_config["monitor_entropy"] is True and t2.global_step == 2
    assert t2.net.ent_value is None                 # no generator step in this phase
    assert np.isfinite(float(t2.net.ct_entropy_eval)) and 0.0 <= float(t2.net.ct_entropy_eval) <= 1.0
    rows = _scalar_rows(out2)
    assert rows, "ct_entropy is not in the scalar log of %s" % out2
    assert all(0.0 <= r["ct_entropy"] <= 1.0 and r["kind"] in ("train_eval", "val_eval") for r in rows)
    t3 = tg.main("train-gan", common)
    assert t3.net.ent_value is not None and np.isfinite(float(t3.net.ent_value)) and 0.0 <= float(t3.net.ent_value) <= 1.0
    assert np.isfinite(float(t3.net.ct_gen_loss)) and len(_scalar_rows(out2)) > len(rows)
