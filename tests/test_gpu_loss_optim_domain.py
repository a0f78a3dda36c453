"""-m gpu: the loss, prediction and optimiser kernels (csrc/loss_optim.hip) over their whole domain, against the float64 references of
tests/elementwise_ref.py computed on the device.

The case lists are module-level: tests/test_elementwise_ref_host.py imports them without a GPU and asserts that every branch (class
counts 1 ... 8, absent classes, ragged pixel counts, the capped grid of 1024 workgroups, optimiser sizes around a chunk, more than 1024
chunks) is reached by at least one case.

Bars are the project's existing ones (tests/test_gpu_loss_optim.py): 1e-5 for losses, 1e-4 of max|ref| for dlogits, 1e-6 for optimiser
state and the softmax.  Every test prints its worst error per output (pytest -s -m gpu -k domain).
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import elementwise_ref as R
from conftest import GUARD_BYTES, pkg
from oracle import nets_adv
from parity_util import argmax_mismatches, rel

pytestmark = pytest.mark.gpu

# (ncls, P, logit scale, label map: "mixed" / "absent" (one class has no pixel) / "single" (every pixel in one class), (miu_cross, miu_dice))
SEG_CASES = [
    (1, 255, 1.0, "single", (1.0, 1.0)), (2, 1, 1.0, "single", (1.0, 1.0)), (2, 256, 4.0, "mixed", (0.1, 1.0)),
    (3, 257, 12.0, "absent", (1.0, 0.0)), (4, 4097, 0.1, "mixed", (0.0, 1.0)), (5, 4097, 4.0, "absent", (1.0, 1.0)),
    (6, 255, 12.0, "mixed", (1.0, 1.0)), (7, 257, 1.0, "single", (0.1, 1.0)), (8, 4097, 4.0, "mixed", (1.0, 1.0)),
    (5, 1 << 20, 1.0, "mixed", (1.0, 1.0)), (8, (1 << 20) + 1, 4.0, "absent", (0.1, 1.0)), (2, (1 << 22) + 5, 12.0, "mixed", (1.0, 1.0)),
    (5, (1 << 22) + 5, 0.1, "absent", (1.0, 1.0)),
]
# (ncls, P, logit scale)
PRED_CASES = [(1, 255, 1.0), (2, 256, 4.0), (3, 257, 12.0), (4, 1, 1.0), (5, 4097, 1.0), (8, 4097, 12.0), (5, 1 << 20, 4.0),
              (8, (1 << 20) + 1, 1.0)]
WGAN_B = (1, 2, 16, 63, 64, 65, 300)
WGAN_COEFS = (0.7, -1.3, 0.25, 2.0)
OPT_N = (1, 1000, 1024, 5000, (1 << 20) + 7)
OPT_COMBOS = ((False, False), (True, False), (False, True), (True, True))       # (chunk_l2, chunk_mask)
L2_N = (1, 1000, 1024, 5000, 1024 * 1500)

F32 = lambda v: float(np.float32(v))


def _gen(seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float32)


def _labels(g, P, ncls, mode):
    if mode == "single":
        return torch.full((P,), ncls - 1, dtype=torch.int64, device=g.device)
    lab = torch.randint(0, ncls, (P,), generator=g, device=g.device)
    lab[torch.rand(P, generator=g, device=g.device) < 0.6] = 0            # an unbalanced map: class weights far from uniform
    if mode == "absent":
        lab[lab == ncls - 2] = 0 if ncls > 2 else 1
    return lab


def _onehot(lab, ncls):
    return (lab.unsqueeze(-1) == torch.arange(ncls, device=lab.device)).float()


def _guarded(nbytes, dev):
    buf = torch.empty(nbytes + GUARD_BYTES, dtype=torch.uint8, device=dev)
    buf[:nbytes] = 0xFF                 # NaN bit patterns
    buf[nbytes:] = 0xA5
    return buf


def _seg_fwd_guarded(z, y, mc, md):
    """pnp_seg_loss_fwd on a buffer of EXACTLY the bytes its query asks for, followed by a guard zone"""
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    ncls = z.shape[-1]
    P = z.numel() // ncls
    need = int(lib.pnp_seg_loss_workspace_bytes(P, ncls))
    buf = _guarded(need, z.device)
    out = torch.full((3,), float("nan"), device=z.device)
    L.check(lib.pnp_seg_loss_fwd(K._p(z), K._p(y), K._p(out), P, ncls, float(mc), float(md), ctypes.c_void_p(buf.data_ptr()), need,
                                 K._stream()), "pnp_seg_loss_fwd")
    assert bool((buf[need:] == 0xA5).all()), "pnp_seg_loss_fwd wrote past the workspace it asked for"
    return out, buf[:need]


@pytest.mark.parametrize("case", SEG_CASES, ids=lambda c: "ncls%d-P%d-s%g-%s-m%g_%g" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1]))
def test_seg_loss_domain(dev, case):
    """forward (three losses and the 32 double sums) and backward (gscale 0.5; P_norm = 2P: the cross-entropy weight halves, the Dice
    term does not) against float64.  The gradient jumps where the true class's probability crosses the 0.005 clip: pixels whose float64
    probability is within 1e-4 (relative) of it are left out of the element-wise comparison — at most 1e-4 of the pixels — and must
    still be finite"""
    K = pkg("kernels")
    ncls, P, scale, mode, (mc, md) = case
    g = _gen(SEG_CASES.index(case), dev)
    z = _randn(g, 1, 1, P, ncls) * scale + 0.05
    lab = _labels(g, P, ncls, mode)
    y = _onehot(lab, ncls).reshape(1, 1, P, ncls)
    out, ws = _seg_fwd_guarded(z, y, mc, md)
    tot, xent, dice, sums = R.seg_loss(z, y, mc, md)
    o = out.double()
    e_fwd = (abs(float(o[0] - tot)), abs(float(o[1] - xent)), abs(float(o[2] - dice)))
    got = K.seg_loss_sums(ws).reshape(4, 8)
    assert torch.equal(got[0, :ncls], sums[0])                       # pixel counts: integers, exact
    assert not bool(got[:, ncls:].any())                             # classes beyond ncls: nothing
    e_sums = [float((got[q, :ncls] - sums[q]).abs().max() / (sums[q].abs().max() + 1e-300)) for q in (1, 2, 3)]
    out_w, _ = K.seg_loss_fwd(z, y, mc, md)                          # the wrapper: same kernels, its own buffer
    assert torch.equal(out_w, out)
    res = {}
    for name, gscale, Pn in (("gscale0.5", 0.5, None), ("P_norm2P", 1.0, 2 * P)):
        dz = K.seg_loss_bwd(z, y, ws, mc, md, gscale, Pn)
        rdz, p_true = R.seg_loss_bwd(z, y, mc, md, gscale, Pn)
        near = ((p_true - R.CLIP_P).abs() <= 1e-4 * R.CLIP_P).unsqueeze(-1)
        share = float(near.double().mean())
        assert share <= 1e-4, share
        assert bool(torch.isfinite(dz).all())
        keep = (~near).double()
        res[name] = float(((dz.double() - rdz) * keep).abs().max() / ((rdz * keep).abs().max() + 1e-300))
    if mc != 0 and ncls > 1 and mode != "single":
        # the halved cross-entropy weight is visible: P_norm = 2P is NOT the plain gradient
        assert rel(K.seg_loss_bwd(z, y, ws, mc, md, 1.0, None), R.seg_loss_bwd(z, y, mc, md, 1.0, 2 * P)[0]) > 1e-3
    print("seg loss %s: total %.2e xent %.2e dice %.2e | sums I %.2e S %.2e X %.2e | dlogits %s | near the clip: %.1e of the pixels" % (
        case, e_fwd[0], e_fwd[1], e_fwd[2], e_sums[0], e_sums[1], e_sums[2], " ".join("%s %.2e" % kv for kv in res.items()), share))
    assert e_fwd[1] < 1e-5 * max(1.0, abs(float(xent))) and e_fwd[2] < 1e-5 and e_fwd[0] < 2e-5, e_fwd
    assert max(e_sums) < 1e-5, e_sums
    assert max(res.values()) < 1e-4, res


@pytest.mark.parametrize("ncls,P,scale", PRED_CASES)
def test_prediction_kernels_domain(dev, ncls, P, scale):
    """softmax_argmax (with and without the probabilities), dice_eval (absent class, labels -1 and ncls), confusion_matrix (predictions
    outside the range are counted nowhere), label_decomp"""
    K, L = pkg("kernels"), pkg("_lib")
    g = _gen(100 + PRED_CASES.index((ncls, P, scale)), dev)
    z = _randn(g, 1, 1, P, ncls) * scale + 0.05
    ntie = min(P, 16)
    for i in range(ntie):                   # exact ties between every class from i % ncls on, the rest lower: the lowest index must win
        z[0, 0, i, :] = -1.0
        z[0, 0, i, i % ncls:] = 0.75
    prob, label = K.softmax_argmax(z)
    none, label2 = K.softmax_argmax(z, want_prob=False)
    assert none is None and torch.equal(label2, label)
    p64, lab64 = R.softmax_argmax(z)
    e_p = rel(prob, p64)
    assert e_p < 1e-6, e_p
    assert torch.equal(label[0, 0, :ntie], torch.arange(ntie, device=dev) % ncls) and torch.equal(label[0, 0, :ntie], lab64[0, 0, :ntie])
    assert int(label.min()) >= 0 and int(label.max()) < ncls
    if ncls == 1:
        n_mis, bad, worst, noise = int((label != 0).sum()), int((label != 0).sum()), 0.0, 0.0          # (no second class to tie with)
    else:
        n_mis, bad, worst, noise = argmax_mismatches(_onehot(label, ncls), p64, noise_rel=4e-7)
    print("softmax_argmax ncls=%d P=%d scale=%g: prob %.2e, %d label mismatches (largest float64 margin %.2e, noise %.2e), unexplained %d" % (
        ncls, P, scale, e_p, n_mis, worst, noise, bad))
    assert bad == 0 and n_mis <= 1e-4 * P, (n_mis, bad)

    # hard Dice: the truth lacks one class, the prediction carries labels outside [0, ncls)
    truth = _labels(g, P, ncls, "absent" if ncls > 1 else "single")
    y = _onehot(truth, ncls).reshape(1, 1, P, ncls)
    pred = label.clone()
    pred[0, 0, ::7] = -1
    pred[0, 0, 3::11] = ncls
    lib = L.load()
    nblk = min(max((P + 1023) // 1024, 1), 1024)
    buf = _guarded(nblk * 96, dev)
    out = torch.full((1 + ncls,), float("nan"), device=dev)
    L.check(lib.pnp_dice_eval(ctypes.c_void_p(pred.data_ptr()), K._p(y), K._p(out), P, ncls, ctypes.c_void_p(buf.data_ptr()), nblk * 96,
                              K._stream()), "pnp_dice_eval")
    assert bool((buf[nblk * 96:] == 0xA5).all()), "pnp_dice_eval wrote past nblk * 96 bytes"
    rd = R.dice_eval(pred, y)
    e_d = float((out.double() - rd).abs().max())
    assert torch.equal(K.dice_eval(pred, y), out)
    assert e_d < 1e-6, e_d
    if ncls > 2:
        assert float(rd[1 + ncls - 2]) == 0.0 and float(out[1 + ncls - 2]) == 0.0          # the absent class: 0 / 1e-7

    # confusion matrix of the same pair; rows without a label (all-zero one-hot) count as class 0
    y2 = y.clone()
    y2[0, 0, 5::13] = 0.0
    cy, cm = K.confusion_matrix(y2, pred)
    rcy, rcm = R.confusion_matrix(y2, pred)
    assert torch.equal(cy, rcy) and torch.equal(cm, rcm)
    n_in = int(((pred >= 0) & (pred < ncls)).sum())
    assert int(cm.sum()) == n_in
    assert P < 4 or n_in < P                                       # (some predictions really are outside the range)
    cy3, none = K.confusion_matrix(y2, None)
    assert none is None and torch.equal(cy3, cy)

    labf = pred.float()
    assert torch.equal(K.label_decomp(labf, ncls), _onehot(pred, ncls))
    print("dice_eval ncls=%d P=%d: %.2e" % (ncls, P, e_d))


@pytest.mark.parametrize("B", WGAN_B)
def test_wgan_loss_domain(dev, B):
    """every non-empty subset of the four critic outputs, unequal coefficients (one negative), against the float64 sum; the full set
    with the reference's coefficients against oracle.nets_adv.wgan_losses.  Two bars: the project's loss bar, 1e-5 * max(1, |ref|), and —
    because these sums cancel and the reference's coefficients are 0.002 — 1e-6 of the terms' size sum |coef| mean|x|: float32 rounding of
    the coefficients (6e-8 each) plus at most 11 additions per operand (5 per lane, 6 shuffle steps, 6e-8 each) stay below 7.2e-7 of it"""
    K = pkg("kernels")
    g = _gen(200 + B, dev)
    ops = [_randn(g, B, 1) + 0.3 * (i + 1) for i in range(4)]
    worst = 0.0
    for pick in itertools.product((False, True), repeat=4):
        if not any(pick):
            continue
        sel = [t if p else None for t, p in zip(ops, pick)]
        got = K.wgan_loss(sel[0], sel[1], sel[2], sel[3], WGAN_COEFS)
        ref = float(R.wgan_loss(sel, WGAN_COEFS))
        size = sum(abs(c) * float(t.abs().mean()) for t, c in zip(sel, WGAN_COEFS) if t is not None)
        e = abs(float(got) - ref) / size
        worst = max(worst, e)
        assert abs(float(got) - ref) < 1e-5 * max(1.0, abs(ref)) and e < 1e-6, (pick, e)
    miu, lam = 0.002, 0.3
    o = {"ct_cls": ops[0].double().cpu(), "mr_cls": ops[1].double().cpu(), "ct_mask": ops[2].double().cpu(), "mr_mask": ops[3].double().cpu()}
    dis, gen = nets_adv.wgan_losses(o, miu, miu, lam)
    got_d = float(K.wgan_loss(ops[0], ops[1], ops[2], ops[3], (miu, -miu, lam * miu, -lam * miu)))
    got_g = float(K.wgan_loss(ops[0], None, ops[2], None, (-miu, 0.0, -lam * miu, 0.0)))
    am = [float(t.abs().mean()) for t in ops]
    size_d = miu * (am[0] + am[1]) + lam * miu * (am[2] + am[3])
    size_g = miu * am[0] + lam * miu * am[2]
    e_d, e_g = abs(got_d - float(dis)) / size_d, abs(got_g - float(gen)) / size_g
    print("wgan_loss B=%d: subsets %.2e, dis %.2e gen %.2e" % (B, worst, e_d, e_g))
    assert abs(got_d - float(dis)) < 1e-5 and abs(got_g - float(gen)) < 1e-5 and e_d < 1e-6 and e_g < 1e-6


def _chunks(n, with_l2, with_mask, dev):
    nch = (n + R.OPT_CHUNK - 1) // R.OPT_CHUNK
    c = torch.arange(nch, device=dev)
    l2 = (0.125 * (1 + c % 3)).float()
    l2[2::5] = 0.0                                      # chunks without weight decay
    mask = torch.ones(nch, dtype=torch.uint8, device=dev)
    mask[3::5] = 0                                      # chunks outside the var list (their L2 is non-zero)
    return (l2 if with_l2 else None), (mask if with_mask else None)


@pytest.mark.parametrize("n", OPT_N)
@pytest.mark.parametrize("with_l2,with_mask", OPT_COMBOS)
def test_optimisers_domain(dev, n, with_l2, with_mask):
    """three steps of Adam / RMSProp / Momentum, and clip, with and without per-chunk L2 and var-list mask, against float64; a masked-out
    chunk keeps weights and state bit for bit"""
    K = pkg("kernels")
    g = _gen(300 + n % 1000, dev)
    l2, mask = _chunks(n, with_l2, with_mask, dev)
    sel = R.per_element(mask, n, 1.0).to(dev) != 0
    w0 = _randn(g, n) * 0.5 + 0.1
    grads = [_randn(g, n) + 0.2 for _ in range(3)]
    lr, b1, b2, eps = F32(1e-3), F32(0.9), F32(0.999), F32(1e-8)
    errs = {}

    def frozen(pairs):
        return all(torch.equal(a[~sel], b[~sel]) for a, b in pairs)

    w, m, v = w0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    rw, rm, rv = w0.double(), m.double(), v.double()
    for t in (1, 2, 3):
        prev = (w.clone(), m.clone(), v.clone())
        K.adam_step(w, grads[t - 1], m, v, l2, mask, lr, b1, b2, eps, t)
        rw, rm, rv = R.adam(rw, grads[t - 1], rm, rv, l2, mask, lr, b1, b2, eps, t)
        assert frozen(zip((w, m, v), prev))
    errs["adam"] = (rel(w, rw), rel(m, rm), rel(v, rv))

    lr_r, dec, eps_r = F32(3e-4), F32(0.9), F32(1e-10)
    w, ms = w0.clone(), torch.ones(n, device=dev)
    rw, rms = w0.double(), ms.double()
    for t in (1, 2, 3):
        prev = (w.clone(), ms.clone())
        K.rmsprop_step(w, grads[t - 1], ms, l2, mask, lr_r, dec, eps_r)
        rw, rms = R.rmsprop(rw, grads[t - 1], rms, l2, mask, lr_r, dec, eps_r)
        assert frozen(zip((w, ms), prev))
    errs["rmsprop"] = (rel(w, rw), rel(ms, rms))

    lr_m, mom = F32(0.2), F32(0.2)
    w, acc = w0.clone(), torch.zeros(n, device=dev)
    rw, racc = w0.double(), acc.double()
    for t in (1, 2, 3):
        prev = (w.clone(), acc.clone())
        K.momentum_step(w, grads[t - 1], acc, l2, mask, lr_m, mom)
        rw, racc = R.momentum(rw, grads[t - 1], racc, l2, mask, lr_m, mom)
        assert frozen(zip((w, acc), prev))
    errs["momentum"] = (rel(w, rw), rel(acc, racc))
    print("optimisers n=%d l2=%s mask=%s: %s" % (n, with_l2, with_mask, " | ".join("%s %s" % (k, " ".join("%.2e" % e for e in v_)) for k, v_ in errs.items())))
    assert all(e < 1e-6 for v_ in errs.values() for e in v_), errs

    w = w0.clone()
    K.clip(w, mask, -0.3, 0.25)
    want = torch.where(sel, torch.clamp(w0, -0.3, 0.25), w0)
    assert torch.equal(w, want) and torch.equal(want, R.clip(w0, mask, -0.3, 0.25))


@pytest.mark.parametrize("n", L2_N)
def test_l2_loss_domain(dev, n):
    """with per-chunk coefficients (some zero) and without (coefficient 1); 1500 chunks make the 1024 workgroups stride"""
    K = pkg("kernels")
    g = _gen(400 + n % 1000, dev)
    w = _randn(g, n) * 0.5 + 0.1
    l2, _ = _chunks(n, True, False, dev)
    e = []
    for coef in (l2, None):
        got, ref = float(K.l2_loss(w, coef)), float(R.l2_loss(w, coef))
        e.append(abs(got - ref) / abs(ref))
    print("l2_loss n=%d: per-chunk %.2e, plain %.2e" % (n, e[0], e[1]))
    assert max(e) < 1e-5, e


def test_bound_step_params_equal_by_value_arguments(dev):
    """with a pnp_step_params block bound, pnp_adam_step takes the bias-corrected learning rate and pnp_dropout the seed from device
    memory: the same bits as the unbound calls handed the same values (the by-value arguments of the bound calls are decoys)"""
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    g = _gen(500, dev)
    n = 5000
    w0, gr, x = _randn(g, n) * 0.5, _randn(g, n), _randn(g, n) + 0.5
    l2, mask = _chunks(n, True, True, dev)
    lr, b1, b2, eps, t, seed, sid = F32(1e-3), F32(0.9), F32(0.999), F32(1e-8), 3, 0x1234567890ABCDEF, 6
    lr_t = F32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
    wa, ma, va = w0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    K.adam_step(wa, gr, ma, va, l2, mask, lr, b1, b2, eps, t)
    ya = K.dropout(x, 0.75, seed, sid)
    block = torch.zeros(4, dtype=torch.float32, device=dev)
    bp = ctypes.c_void_p(block.data_ptr())
    wb, mb, vb = w0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    L.check(lib.pnp_step_params_bind(bp), "pnp_step_params_bind")
    try:
        L.check(lib.pnp_step_params_set(bp, seed, lr_t, K._stream()), "pnp_step_params_set")
        K.adam_step(wb, gr, mb, vb, l2, mask, 0.5, b1, b2, eps, 1)
        yb = K.dropout(x, 0.75, 42, sid)
        torch.cuda.synchronize()
    finally:
        L.check(lib.pnp_step_params_bind(None), "pnp_step_params_bind")            # process-global
    assert torch.equal(wb, wa) and torch.equal(mb, ma) and torch.equal(vb, va)
    assert torch.equal(yb, ya)
    assert not torch.equal(K.dropout(x, 0.75, 42, sid), ya)                        # unbound again: the by-value seed counts
