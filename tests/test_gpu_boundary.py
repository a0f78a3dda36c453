"""-m gpu: the boundary (distance-map) loss of the source segmenter (csrc/boundary.hip): the distance kernel and the loss
kernel against the exact restatement of tests/boundary_ref.py, the refusals, BoundaryLossFn, the training step with the term against the
CPU oracle (oracle/nets.py) with the term written in torch, bnd_weight = 0 being today's step, determinism, step capture and the entry
point."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from boundary_ref import boundary_ref, onehot_of_masks, patterns, phi_ref
from conftest import pkg
from kernel_bars import _bar, _value_bar
from oracle import nets
from oracle import tf_ops as T
from test_gpu_segmenter import COST, _blob_labels, _cos, _rel, he_scaled

pytestmark = pytest.mark.gpu


def _onehot(lab, C):
    return np.stack([(lab == c) for c in range(C)], axis=-1).astype(np.float32)


@pytest.fixture(scope="module")
def blob_case():
    """the labels of the segmenter tests (two slices of four ellipses) and their distance maps over all five classes, computed once"""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 256, 256, 3)).astype(np.float32)
    oh = _onehot(_blob_labels(rng, 2), 5)
    phi, d2 = phi_ref(oh, classes=range(5))
    return x, oh, phi, d2


# ---- 1. the distance kernel against the restatement ---------------------------------------------------------------------------------
# below, at and across a 64-column strip (the strip is narrower where the tiles of all classes would not fit: 8 classes at 63 rows, any
# class count at 1024 rows); extents that are no power of two; the extent cap in either direction; every class count from 1 to 8
SHAPES = [(1, 1, 1, 5), (1, 1, 7, 5), (1, 7, 1, 5), (2, 5, 9, 3), (1, 33, 65, 5), (1, 64, 64, 1), (1, 63, 130, 8), (2, 256, 256, 5),
          (1, 1024, 3, 2), (1, 3, 1024, 2), (1, 20, 70, 4), (1, 9, 129, 6), (1, 40, 31, 7)]
SUBSETS = (None, [0], [2, 4], [])


def _labels(B, H, W, C, rng):
    """a label map of coarse random blocks with a little salt: distances from 1 to a good part of the extent"""
    bh, bw = max(H // 5, 1), max(W // 5, 1)
    n = max(C, 2)                                        # (one class: label 1 is a pixel that belongs to no class)
    coarse = rng.integers(0, n, (B, -(-H // bh), -(-W // bw)))
    lab = np.repeat(np.repeat(coarse, bh, axis=1), bw, axis=2)[:, :H, :W]
    salt = rng.random((B, H, W)) < 0.02
    return np.where(salt, rng.integers(0, n, (B, H, W)), lab)


def _check_phi(K, dev, oh, ref_all, d2_all, classes, what):
    """ref_all, d2_all: the restatement over ALL classes; the classes that are not selected must come back exactly 0"""
    B, H, W, C = oh.shape
    sel = list(range(1, C)) if classes is None else list(classes)
    keep = np.zeros(C, bool)
    keep[sel] = True
    ref = np.where(keep, ref_all, 0.0)
    d2 = np.where(keep, d2_all, 0)
    ohd = torch.from_numpy(oh).to(dev)
    phi = K.signed_distance_2d(ohd, classes)
    phi2 = K.signed_distance_2d(ohd, classes)
    assert phi.shape == ohd.shape and phi.dtype == torch.float32
    assert torch.equal(phi, phi2), what + ": two runs differ"
    got = phi.cpu().double().numpy()
    assert np.isfinite(got).all(), what
    zero = d2 == 0                                       # not selected, absent from the slice, or filling it
    assert not got[zero].any(), what + ": a zero of the rule is not exactly 0"
    sq = np.where(oh > 0.5, (1.0 - got) ** 2, got ** 2)   # inside the class phi = -(d - 1)
    bad = np.rint(sq).astype(np.int64)[~zero] != d2[~zero]
    assert not bad.any(), "%s: %d squared distances differ from the exact integers" % (what, int(bad.sum()))
    err = np.abs(got - ref)
    print("%s: max |phi - ref| %.3e, max |ref| %.4g, %d non-zero entries" % (what, float(err.max()), float(np.abs(ref).max()), int((~zero).sum())))
    assert (err <= 1e-6 * np.abs(ref)).all(), what
    return phi


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distance_kernel_against_restatement(dev, blob_case, shape):
    K = pkg("kernels")
    B, H, W, C = shape
    if shape == (2, 256, 256, 5):
        _, oh, ref_all, d2_all = blob_case
    else:
        rng = np.random.default_rng(B * 7 + H * 3 + W + C)
        oh = _onehot(_labels(B, H, W, C, rng), C)
        ref_all, d2_all = phi_ref(oh, classes=range(C))
    for classes in SUBSETS:
        if classes is not None and any(c >= C for c in classes):
            continue
        _check_phi(K, dev, oh, ref_all, d2_all, classes, "%s classes %s" % (shape, classes))


@pytest.mark.parametrize("H,W,C,c", [(33, 65, 5, 2), (64, 130, 3, 1), (7, 9, 8, 7)])
def test_distance_kernel_label_patterns(dev, H, W, C, c):
    """every pattern as class c of one slice of a batch of two, the other slice random; then the two slices swapped"""
    K = pkg("kernels")
    rng = np.random.default_rng(H + W)
    other = rng.random((H, W)) < 0.35
    for name, m in patterns(H, W, rng).items():
        for i, masks in enumerate((np.stack([m, other]), np.stack([other, m]))):
            oh = onehot_of_masks(masks, C, c)
            ref_all, d2_all = phi_ref(oh, classes=range(C))
            _check_phi(K, dev, oh, ref_all, d2_all, None, "%s %dx%d" % (name, H, W))
            _check_phi(K, dev, oh, ref_all, d2_all, [c], "%s %dx%d alone" % (name, H, W))
            if name in ("absent", "full"):
                assert not d2_all[i, :, :, c].any() and d2_all[1 - i, :, :, c].all()      # the rule: 0 on that slice only


def test_far_blobs_take_the_minimum_from_the_far_end_of_a_column(dev):
    """two blobs in opposite corners of a 200 x 40 slice: for the pixels between them the nearest member is up to 160 rows away"""
    K = pkg("kernels")
    m = np.zeros((200, 40), bool)
    m[:8, :6] = True
    m[192:, 34:] = True
    oh = onehot_of_masks(np.stack([m, ~m]), 2, 1)
    ref_all, d2_all = phi_ref(oh, classes=range(2))
    assert d2_all[0, :, :, 1].max() > 90 ** 2
    _check_phi(K, dev, oh, ref_all, d2_all, None, "far blobs")
    _check_phi(K, dev, oh, ref_all, d2_all, [0, 1], "far blobs, both classes")


@pytest.mark.parametrize("shape,classes", [((1, 1024, 5, 8), list(range(8))), ((1, 1000, 9, 4), None), ((2, 300, 70, 5), [0, 1, 2, 3, 4]),
                                           ((2, 120, 70, 5), [0, 1, 2, 3, 4])])
def test_narrow_strips_where_the_tiles_of_all_classes_would_not_fit(dev, shape, classes):
    """the column pass halves its strip, down to two columns, until the int16 tiles of the selected classes fit 16 KB: 2 (at the floor,
    32 KB), 2, 4 and 8 columns here; 1000, 300 and 120 rows are no multiple of the 8 rows a thread takes"""
    K = pkg("kernels")
    B, H, W, C = shape
    rng = np.random.default_rng(H + W)
    oh = _onehot(_labels(B, H, W, C, rng), C)
    ref_all, d2_all = phi_ref(oh, classes=range(C))
    _check_phi(K, dev, oh, ref_all, d2_all, classes, "%s classes %s" % (shape, classes))


# ---- 2. the loss kernel against float64 ---------------------------------------------------------------------------------------------
LOSS_SHAPES = [(P, 5) for P in (1, 3, 4, 7, 1021, 2 * 256 * 256)] + [(257, C) for C in (1, 2, 3, 8)]


def _loss_inputs(P, C, seed, blob_case):
    """logits with a few rows far ahead, and distance maps of the restatement scaled to +-360"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((P, C)) * 3.0).astype(np.float32)
    if P >= 7:
        z[1, int(rng.integers(C))] += 300.0
        z[5, 0] += 700.0
        z[6, C - 1] -= 400.0
    if (P, C) == (2 * 256 * 256, 5):
        q = blob_case[2].reshape(-1, 5)
    else:
        h = max(int(np.ceil(np.sqrt(P))), 4)
        oh = _onehot(_labels(1, h, h, max(C, 2), rng), max(C, 2))[..., :C]
        q = phi_ref(oh, classes=range(C))[0].reshape(-1, C)[:P]
    q = (q * (360.0 / max(float(np.abs(q).max()), 1.0))).astype(np.float32)
    return z, q


def _check_loss(K, zd, qd, z, q, nsel, coef, what):
    ref_v, ref_g = boundary_ref(z, q, nsel, coef)
    v, g = K.boundary_loss(zd, qd, nsel, coef=coef, want_grad=True)
    v0, g0 = K.boundary_loss(zd, qd, nsel)
    v2, g2 = K.boundary_loss(zd, qd, nsel, coef=coef, want_grad=True)
    assert g0 is None and tuple(v.shape) == (1,) and g.shape == zd.shape
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all()), what
    if nsel == 0:
        assert float(v) == 0.0 and float(g.abs().max()) == 0.0
    else:
        _value_bar(v, ref_v, what)
        _bar(g, torch.from_numpy(ref_g), what + " gradient")
    assert torch.equal(v0, v), "dlogits = NULL changes the value"      # bit for bit
    assert torch.equal(v2, v) and torch.equal(g2, g), "two runs differ"
    return v, g


@pytest.mark.parametrize("P,C", LOSS_SHAPES)
def test_loss_kernel_against_float64(dev, blob_case, P, C):
    K = pkg("kernels")
    z, q = _loss_inputs(P, C, 100 * C + P % 97, blob_case)
    zd, qd = torch.from_numpy(z).to(dev), torch.from_numpy(q).to(dev)
    assert zd.data_ptr() % 16 == 0 and qd.data_ptr() % 16 == 0
    nsel = max(C - 1, 1)
    _check_loss(K, zd, qd, z, q, nsel, 0.375 * 0.25, "P=%d C=%d" % (P, C))
    if P == 1021:
        _check_loss(K, zd, qd, z, q, 0, 1.0, "P=%d C=%d nsel=0" % (P, C))
        _check_loss(K, zd, qd, z, q, 2, 1.0, "P=%d C=%d nsel=2" % (P, C))


@pytest.mark.parametrize("P", [7, 1021])
def test_loss_kernel_misaligned_base_takes_the_fallback(dev, blob_case, P):
    """logits and maps that start one pixel (20 bytes) into an allocation: no float4 load is aligned, the launch takes the generic path"""
    K = pkg("kernels")
    z, q = _loss_inputs(P, 5, 7 + P, blob_case)

    def off(a):
        base = torch.zeros((P + 1, 5), device=dev)
        base[1:] = torch.from_numpy(a).to(dev)
        return base[1:]
    zd, qd = off(z), off(q)
    assert zd.is_contiguous() and zd.data_ptr() % 16 != 0 and qd.data_ptr() % 16 != 0
    v, g = _check_loss(K, zd, qd, z, q, 4, 1.0, "misaligned P=%d" % P)
    va, ga = K.boundary_loss(zd.clone(), qd.clone(), 4, want_grad=True)      # the aligned copies on the vector path: the same to the bar
    _bar(g, ga.detach().cpu(), "misaligned against aligned")
    assert abs(float(v) - float(va)) <= 1e-6 * abs(float(va))
    _check_loss(K, zd, qd.clone(), z, q, 4, 1.0, "only the logits misaligned P=%d" % P)


def test_autograd_function_scales_by_coef_and_gscale(dev, blob_case):
    F, K = pkg("functional"), pkg("kernels")
    _, oh, phi_all, _ = blob_case
    rng = np.random.default_rng(3)
    z = (rng.standard_normal(oh.shape) * 2.0).astype(np.float32)
    yd = torch.from_numpy(oh).to(dev)
    for classes, coef, gscale in ((None, 1.0, 1.0), (None, 0.01, 0.125), ((1, 3), 2.5, 0.5)):
        sel = [1, 2, 3, 4] if classes is None else list(classes)
        keep = np.zeros(5, bool)
        keep[sel] = True
        zd = torch.from_numpy(z).to(dev).requires_grad_(True)
        val = F.BoundaryLossFn.apply(zd, yd, classes, coef, gscale)
        val.backward(torch.ones(1, device=dev))
        ref_v, ref_g = boundary_ref(z, np.where(keep, phi_all, 0.0), len(sel), coef * gscale)
        _value_bar(val.detach(), ref_v, "BoundaryLossFn %s coef %g gscale %g" % (classes, coef, gscale))      # the value is not scaled
        _bar(zd.grad, torch.from_numpy(ref_g), "BoundaryLossFn gradient %s coef %g gscale %g" % (classes, coef, gscale))
        assert torch.equal(val.detach(), K.boundary_loss(zd.detach(), K.signed_distance_2d(yd, classes), len(sel))[0])


def test_refusals_come_before_any_launch(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    with pytest.raises(L.PnpError, match="at most 8 classes"):
        K.signed_distance_2d(torch.zeros((1, 4, 4, 9), device=dev))
    with pytest.raises(L.PnpError, match="at most 1024"):
        K.signed_distance_2d(torch.zeros((1, 1025, 2, 5), device=dev))
    with pytest.raises(L.PnpError, match="at most 1024"):
        K.signed_distance_2d(torch.zeros((1, 2, 1025, 5), device=dev))
    with pytest.raises(L.PnpError, match="CPU"):
        K.signed_distance_2d(torch.zeros((1, 4, 4, 5)))
    with pytest.raises(L.PnpError, match="at most 8 classes"):
        K.boundary_loss(torch.zeros((4, 9), device=dev), torch.zeros((4, 9), device=dev), 4)
    with pytest.raises(L.PnpError, match="CPU"):
        K.boundary_loss(torch.zeros((4, 5)), torch.zeros((4, 5)), 4)
    with pytest.raises(ValueError):
        K.signed_distance_2d(torch.zeros((1, 4, 4, 5), device=dev), classes=[5])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    # the transform: a workspace one byte short, outputs and workspace pre-filled
    B, H, W, C, mask = 2, 9, 70, 5, 0b11110
    rng = np.random.default_rng(0)
    oh = _onehot(_labels(B, H, W, C, rng), C)
    y = torch.from_numpy(oh).to(dev)
    phi = torch.full((B, H, W, C), -7.0, device=dev)
    need = lib.pnp_signed_distance_2d_workspace_bytes(B, H, W, C, mask)
    assert need == B * 4 * H * W * 2
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    code = lib.pnp_signed_distance_2d(p(y), B, H, W, C, mask, p(phi), p(ws), need - 1, st)
    with pytest.raises(L.PnpError, match="workspace too small"):
        L.check(code, "pnp_signed_distance_2d")
    for bad in ((B, 1025, W, C), (B, H, W, 9)):
        with pytest.raises(L.PnpError):
            L.check(lib.pnp_signed_distance_2d(p(y), bad[0], bad[1], bad[2], bad[3], mask, p(phi), p(ws), need, st), "pnp_signed_distance_2d")
    torch.cuda.synchronize()
    assert float(phi.min()) == -7.0 and float(phi.max()) == -7.0 and int(ws.min()) == 0x5A and int(ws.max()) == 0x5A
    L.check(lib.pnp_signed_distance_2d(p(y), B, H, W, C, mask, p(phi), p(ws), need, st), "pnp_signed_distance_2d")      # exactly enough is enough
    ref, _ = phi_ref(oh)
    assert float(np.abs(phi.cpu().double().numpy() - ref).max()) <= 1e-6 * float(np.abs(ref).max())
    # the loss
    P = 1021
    z = torch.zeros((P, 5), device=dev)
    q = torch.ones((P, 5), device=dev)
    out = torch.full((1,), -7.0, device=dev)
    dl = torch.full((P, 5), -7.0, device=dev)
    need = lib.pnp_boundary_loss_workspace_bytes(P, 5)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    code = lib.pnp_boundary_loss(p(z), p(q), P, 5, 4, 1.0, p(dl), p(out), p(ws), need - 1, st)
    with pytest.raises(L.PnpError, match="workspace too small"):
        L.check(code, "pnp_boundary_loss")
    with pytest.raises(L.PnpError, match="at most 8 classes"):
        L.check(lib.pnp_boundary_loss(p(z), p(q), P, 9, 4, 1.0, p(dl), p(out), p(ws), need, st), "pnp_boundary_loss")
    torch.cuda.synchronize()
    assert float(out) == -7.0 and float(dl.min()) == -7.0 and float(dl.max()) == -7.0 and int(ws.min()) == 0x5A and int(ws.max()) == 0x5A
    L.check(lib.pnp_boundary_loss(p(z), p(q), P, 5, 4, 1.0, p(dl), p(out), p(ws), need, st), "pnp_boundary_loss")        # exactly enough is enough
    assert abs(float(out) - 0.25) <= 1e-6 and float(dl.abs().max()) <= 1e-9       # equal logits on a constant map: s = 1, L = 1 / nsel


# ---- 3. the training step with the term against the oracle, B = 2 ------------------------------------------------------------------
B = 2
LR = 1e-3
NSEL = 4


@pytest.fixture(scope="module")
def case(blob_case):
    """the setup of test_segmenter_train_step_parity at logit scale 0.05; per keep probability and type one walk of the oracle and the
    gradients of its two pieces — the graph does not depend on the weights of the cost: total = a * cost(1, 1) + w * L_bnd"""
    ss = pkg("source_segmenter")
    x, oh, phi_all, _ = blob_case
    phi = np.where(np.arange(5) >= 1, phi_all, 0.0)               # the default classes: all but the background
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, device="cpu", cost_kwargs=dict(COST), seed=3)
    sd = he_scaled(net.store.state_dict())
    sd["output/Variable"] = (sd["output/Variable"] * 0.05).astype(np.float32)
    res = {}
    for keep in (1.0, 0.75):
        for dt in (torch.float32, torch.float64):
            V = nets.make_variables(sd, dtype=dt)
            lo = nets.segmenter_forward(V, torch.from_numpy(x).to(dt), keep, True, True, 1)
            cost = nets.segmenter_cost(V, lo, torch.from_numpy(oh).to(dt))[0]
            bnd = (torch.softmax(lo, -1) * torch.from_numpy(phi).to(dt)).sum() / (B * 256 * 256 * NSEL)
            names = [k for k in V if V[k].requires_grad]
            zero = lambda gs: {k: (g if g is not None else torch.zeros_like(V[k])) for k, g in zip(names, gs)}
            g_seg = zero(torch.autograd.grad(cost, [V[k] for k in names], retain_graph=True, allow_unused=True))
            g_bnd = zero(torch.autograd.grad(bnd, [V[k] for k in names], allow_unused=True))
            res[(keep, dt)] = {"cost": float(cost.detach()), "bnd": float(bnd.detach()), "g_seg": g_seg, "g_bnd": g_bnd, "logits": lo.detach(),
                               "moving": {k: v.detach() for k, v in V.items() if k.endswith("moving_mean") or k.endswith("moving_variance")}}
    return sd, x, oh, res


def _net(dev, sd, cost):
    ss = pkg("source_segmenter")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, cost_kwargs=dict(COST, **cost), seed=3)
    net.store.load_state_dict(sd)
    tr = ss.Trainer(net, None, None, num_cls=5, batch_size=B, optimizer="adam", opt_kwargs={"learning_rate": LR})
    tr.opt = tr._get_optimizer(10)
    return net, tr


def _norm(gs):
    return float(sum(float((g.double() ** 2).sum()) for g in gs.values()) ** 0.5)


# (a) cross_flag = dice_flag = False: the gradients come from the boundary term alone — the new path and nothing else
# (b) the reference cost (weighted cross-entropy + Dice) plus BND_WEIGHT_B times the term.  On this setup the float64 oracle's gradient
#     norms are 0.1810 (region terms) and 5.411 (the un-weighted boundary term) at keep_prob 1.0, 0.1757 and 5.104 at 0.75: the weights
#     that balance them are 0.0335 and 0.0344, and 0.03 leaves region / boundary at 1.12 and 1.15 — asserted below within a factor 5
BND_WEIGHT_B = 0.03
@pytest.mark.parametrize("keep_prob", [1.0, 0.75])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_train_step_with_boundary_term_vs_oracle(dev, case, tag, keep_prob):
    K = pkg("kernels")
    sd, x, oh, res = case
    if tag == "a":
        a, w, cost = 0.0, 1.0, {"cross_flag": False, "dice_flag": False, "bnd_weight": 1.0}
    else:
        a, w, cost = 1.0, BND_WEIGHT_B, {"bnd_weight": BND_WEIGHT_B}
    net, tr = _net(dev, sd, cost)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(oh).to(dev)
    loss = tr.train_step(xd, yd, keep_prob, step=0)          # drop seed = step + 1 = 1
    logits = net.logits.detach().cpu()
    g_hip = {v.name: v.tensor.grad.detach().cpu().clone() for v in net.store.trainable()}
    after = net.store.state_dict()
    r64, r32 = res[(keep_prob, torch.float64)], res[(keep_prob, torch.float32)]
    l64 = a * r64["cost"] + w * r64["bnd"]
    g64 = {k: a * r64["g_seg"][k] + w * r64["g_bnd"][k] for k in r64["g_seg"]}
    g32 = {k: a * r32["g_seg"][k] + w * r32["g_bnd"][k] for k in r32["g_seg"]}
    n_seg, n_bnd = a * _norm(r64["g_seg"]), w * _norm(r64["g_bnd"])
    print("seg+bnd (%s, keep %.2f): loss hip %.9g fp64 %.9g | L_bnd hip %.9g fp64 %.9g | float64 gradient norms: region %.4g, boundary %.4g"
          % (tag, keep_prob, float(loss), l64, float(net.bnd_value), r64["bnd"], n_seg, n_bnd))
    if tag == "a":
        assert n_seg == 0.0 and n_bnd > 0.0
    else:
        assert 0.2 < n_seg / n_bnd < 5.0                     # both terms matter
    assert _rel(logits, r64["logits"]) < 1e-4
    assert abs(float(loss) - l64) < 1e-4 * max(1.0, abs(l64))
    assert float(loss) == float(net.cost)
    assert abs(float(net.bnd_value) - r64["bnd"]) <= 1e-4 * abs(r64["bnd"])
    # the kernel's value on the step's logits
    assert torch.equal(net.bnd_value, K.boundary_loss(net.logits.detach().contiguous(), K.signed_distance_2d(yd), NSEL)[0])
    if tag == "b":
        assert abs(float(net.weighted_loss) + float(net.dice_loss) + w * float(net.bnd_value) - float(loss)) <= 1e-5 * abs(float(loss))
    rows = [(k, _rel(g_hip[k], g), _rel(g32[k], g), _cos(g_hip[k], g)) for k, g in g64.items()]
    eh_all, ec_all = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    print("gradient error vs fp64 over %d variables: hip median %.3e max %.3e | cpu-fp32 median %.3e max %.3e | min cosine %.8f" % (
        len(rows), np.median(eh_all), eh_all.max(), np.median(ec_all), ec_all.max(), min(r[3] for r in rows)))
    for r in sorted(rows, key=lambda r: -r[1])[:5]:
        print("   %-28s hip %.3e cpu %.3e cos %.8f" % r)
    # the bars of test_segmenter_train_step_parity: the round-off class of the float32 CPU oracle, and the same direction
    assert np.median(eh_all) < 3.0 * np.median(ec_all) + 1e-4
    assert min(r[3] for r in rows) > 0.9999
    # the Adam update given the HIP path's own gradients (the L2 term is applied inside the optimiser kernel: add it back)
    upd_worst = 0.0
    for k in g64:
        wt = torch.from_numpy(sd[k].copy())
        g = g_hip[k] + COST["regularizer"] * nets.l2_multiplicity(k) * torch.from_numpy(sd[k])
        T.adam_update(wt, g, torch.zeros_like(wt), torch.zeros_like(wt), LR, 1)
        upd_worst = max(upd_worst, float((wt - torch.from_numpy(after[k])).abs().max() / LR))
    print("worst post-step weight error (fraction of lr): %.3e" % upd_worst)
    assert upd_worst < 1e-3
    for k, v in r64["moving"].items():
        assert _rel(after[k], v) < 1e-4, k


# ---- 4. bnd_weight = 0 is today's step; the step with the term is deterministic ---------------------------------------------------------
def _one_step(dev, sd, x, oh, cost):
    net, tr = _net(dev, sd, cost)
    tr.train_step(torch.from_numpy(x).to(dev), torch.from_numpy(oh).to(dev), 0.75, 16)
    torch.cuda.synchronize()
    return net.store.arena.detach().cpu().clone(), net.store.grad_arena.detach().cpu().clone(), net


def test_zero_bnd_weight_is_todays_step(dev, case):
    sd, x, oh, _ = case
    w0, g0, n0 = _one_step(dev, sd, x, oh, {})
    wz, gz, nz = _one_step(dev, sd, x, oh, {"bnd_weight": 0.0, "bnd_classes": [1, 2]})
    assert float(g0.abs().max()) > 0
    assert torch.equal(w0, wz) and torch.equal(g0, gz) and float(n0.cost) == float(nz.cost)
    assert n0.bnd_value is None and nz.bnd_value is None
    nz.evaluate(torch.from_numpy(x).to(dev), torch.from_numpy(oh).to(dev))
    assert nz.bnd_value is None
    w1, g1, n1 = _one_step(dev, sd, x, oh, {"bnd_weight": 0.05})
    assert not torch.equal(g1, g0) and n1.bnd_value is not None          # (and the term does change the step)
    assert float(n1.weighted_loss) == float(n0.weighted_loss) and float(n1.dice_loss) == float(n0.dice_loss)


def test_train_step_with_boundary_term_is_deterministic(dev, case):
    sd, x, oh, _ = case
    w1, g1, n1 = _one_step(dev, sd, x, oh, {"bnd_weight": 0.05})
    w2, g2, n2 = _one_step(dev, sd, x, oh, {"bnd_weight": 0.05})
    assert float(g1.abs().max()) > 0 and torch.equal(g1, g2) and torch.equal(w1, w2)
    assert float(n1.cost) == float(n2.cost) and float(n1.bnd_value) == float(n2.bnd_value)


def test_evaluate_adds_the_term_to_cost(dev, case):
    K = pkg("kernels")
    sd, x, oh, _ = case
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(oh).to(dev)
    net0, _ = _net(dev, sd, {})
    net1, _ = _net(dev, sd, {"bnd_weight": 0.05, "bnd_classes": [1, 3]})
    c0 = float(net0.evaluate(xd, yd, keep_prob=1.0, main_bn=False, adapt_bn=False))
    c1 = float(net1.evaluate(xd, yd, keep_prob=1.0, main_bn=False, adapt_bn=False))
    assert torch.equal(net0.logits, net1.logits)
    val = K.boundary_loss(net1.logits.contiguous(), K.signed_distance_2d(yd, [1, 3]), 2)[0]
    assert torch.equal(net1.bnd_value, val) and float(val) != 0.0
    assert abs(c1 - (c0 + 0.05 * float(val))) <= 1e-6 * abs(c1)
    assert float(net1.weighted_loss) == float(net0.weighted_loss) and float(net1.dice_loss) == float(net0.dice_loss)


# ---- 5. step capture, fp32 -----------------------------------------------------------------------------------------------------------------
def test_captured_steps_with_boundary_term_equal_eager_bit_for_bit(dev, case):
    sd, x, oh, _ = case
    rng = np.random.default_rng(9)
    xs = [torch.from_numpy(x).to(dev), torch.from_numpy(rng.standard_normal(x.shape).astype(np.float32)).to(dev)]
    ys = [torch.from_numpy(oh).to(dev), torch.from_numpy(np.ascontiguousarray(oh[::-1])).to(dev)]

    def run(tr):
        out = []
        for i in range(2):
            out.append(float(tr.train_step(xs[i], ys[i], 0.75, 10 + i)))
            out.append(float(tr.net.bnd_value))
        return out
    net_e, tr_e = _net(dev, sd, {"bnd_weight": 0.05})
    le = run(tr_e)
    w_e = net_e.store.arena.detach().cpu().clone()
    st_e = net_e.store.state_arena.detach().cpu().clone()
    net_c, tr_c = _net(dev, sd, {"bnd_weight": 0.05})
    tr_c.capture_step(xs[0], ys[0], 0.75)                      # two real warm-up steps + the recording
    net_c.store.load_state_dict(sd)                            # back to the start: weights, BN moving statistics, Adam slots, counters
    tr_c.opt.m.zero_(); tr_c.opt.v.zero_(); tr_c.opt.t = 0; tr_c.global_step = 0
    lc = run(tr_c)
    print("captured segmenter steps with the boundary term: eager %s captured %s" % (le, lc))
    assert tr_c._cap["step"].replays == 2
    assert lc == le, (lc, le)
    assert le[1] != le[3]                                      # the maps are computed inside the recorded step, from its own labels
    assert torch.equal(net_c.store.arena.detach().cpu(), w_e)
    assert torch.equal(net_c.store.state_arena.detach().cpu(), st_e)


# ---- 6. the entry point -------------------------------------------------------------------------------------------------------------------
def test_entry_point_with_bnd_weight_and_ramp(dev, tmp_path):
    ts = pkg("train_segmenter")
    out = str(tmp_path / "seg")
    tr = ts.main(["--synthetic", "8", "--batch-size", "2", "--iters", "2", "--epochs", "1", "--output", out, "--bnd-weight", "0.01",
                  "--bnd-ramp", "2"])
    assert tr.bnd_ramp == 2 and tr.bnd_weight == 0.01 and tr.net.bnd_weight == 0.005          # epoch 0 of a ramp of 2
    assert tr.net.bnd_value is not None and np.isfinite(float(tr.net.bnd_value)) and np.isfinite(float(tr.net.cost))
    with open(os.path.join(out, "metrics.jsonl")) as f:
        rows = [r for r in map(json.loads, f) if "bnd" in r]
    assert rows, "bnd is not in the scalar log of %s" % out
    assert all(r["kind"] in ("train_eval", "val_eval") and np.isfinite(r["bnd"]) and np.isfinite(r["cost"]) for r in rows)
    assert {r["kind"] for r in rows} == {"train_eval", "val_eval"}
    assert rows[-1]["kind"] == "val_eval" and rows[-1]["cost"] == tr.loss_dict["val"][1]
    # cost includes the term: the numbers the last step left
    assert abs(float(tr.net.cost) - (float(tr.net.weighted_loss) + float(tr.net.dice_loss) + 0.005 * float(tr.net.bnd_value))) <= 1e-5 * abs(float(tr.net.cost))
    out0 = str(tmp_path / "seg0")
    ts.main(["--synthetic", "8", "--batch-size", "2", "--iters", "2", "--epochs", "1", "--output", out0])
    with open(os.path.join(out0, "metrics.jsonl")) as f:
        assert not any("bnd" in r for r in map(json.loads, f))                                # without the flag the rows are today's
