"""CPU: (a) tests/elementwise_ref.py — the float64 references the -m gpu domain tests compare against — pinned to the oracle's own
functions under autograd, in float64 (both sides float64: 1e-12 relative); (b) the case lists of tests/test_gpu_elementwise_domain.py and
tests/test_gpu_loss_optim_domain.py pinned to the dispatch branches of csrc/elementwise.hip / csrc/loss_optim.hip, whose predicates are
restated here in a few lines each: a case list that stops reaching a branch fails here, without a GPU."""
import numpy as np
import pytest
import torch

import elementwise_ref as R
import test_gpu_elementwise_domain as ED
import test_gpu_loss_optim_domain as LD
from conftest import pkg
from oracle import nets_adv
from oracle import tf_ops as T

TOL = 1e-12


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _rng(seed):
    return np.random.default_rng(seed)


def _t(a, grad=False):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(grad)


# ---- (a) the references against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [-1.0, 0.0, 0.2])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C,Cs", [(8, 4), (8, 8), (6, 2), (8, 0)])          # (8, 4) and (6, 2): a pad of 2 channels per side, not a multiple of 4
def test_bn_reference_equals_the_oracle_under_autograd(alpha, training, C, Cs):
    rng = _rng(C + Cs)
    shape, keep, seed, sid = (2, 3, 5, C), 0.75, 9, 2
    mask = T.dropout_mask(shape, keep, seed, sid)
    xa, gamma, beta = _t(rng.standard_normal(shape) * 1.7 + 0.6, True), _t(1 + 0.1 * rng.standard_normal(C), True), _t(0.1 * rng.standard_normal(C), True)
    mm, mv = _t(0.3 * rng.standard_normal(C)), _t(1 + 0.2 * rng.random(C))
    sc = _t(rng.standard_normal(shape[:-1] + (Cs,)), True) if Cs else None
    dout = _t(rng.standard_normal(shape))
    xc = T.dropout(xa, keep, mask=mask)
    mm_o, mv_o = mm.clone(), mv.clone()
    z = T.batch_norm(xc, gamma, beta, mm_o, mv_o, training)
    if sc is not None:
        z = z + T.pad_channels(sc, (C - Cs) // 2)
    out_o = T.leaky_relu(z, alpha) if alpha >= 0 else z
    out_o.backward(dout)

    P = xc.numel() // C
    if training:
        mean, var = R.bn_stats(xc)
        mmr, mvr = R.bn_moving(mm, mv, mean, var, P)
        assert _rel(mmr, mm_o) < TOL and _rel(mvr, mv_o) < TOL
    else:
        mean, var = mm, mv
        assert torch.equal(mm_o, mm) and torch.equal(mv_o, mv)
    out = R.bn_apply(xc, mean, var, gamma, beta, sc, alpha)
    assert _rel(out, out_o) < TOL
    dx, dg, db, dsc = R.bn_bwd(dout, out, xc, mean, var, gamma, Cs, alpha, training, mask, keep)
    assert _rel(dx, xa.grad) < TOL and _rel(dg, gamma.grad) < TOL and _rel(db, beta.grad) < TOL
    if Cs:
        assert _rel(dsc, sc.grad) < TOL
    # P_norm: the two halves of the batch, handed the whole batch's sums and row count, give the whole batch's dx
    halves = [R.bn_bwd(dout[k:k + 1], out[k:k + 1], xc[k:k + 1], mean, var, gamma, Cs, alpha, training, mask[k:k + 1], keep, P_norm=P, sums=(dg, db))
              for k in (0, 1)]
    assert _rel(torch.cat([h[0] for h in halves]), dx) < TOL
    if training:
        assert _rel(halves[0][0], R.bn_bwd(dout[:1], out[:1], xc[:1], mean, var, gamma, Cs, alpha, True, mask[:1], keep)[0]) > 1e-3


def test_bn_reference_at_one_row():
    """P = 1: variance 0, Bessel factor 1 (the oracle's special case)"""
    x = _t([[[[0.5, -2.0, 3.0, 1.0]]]])
    mm, mv = _t(np.full(4, 0.25)), _t(np.full(4, 2.0))
    mm_o, mv_o = mm.clone(), mv.clone()
    T.batch_norm(x, _t(np.ones(4)), _t(np.zeros(4)), mm_o, mv_o, True)
    mean, var = R.bn_stats(x)
    assert torch.equal(var, torch.zeros(4, dtype=torch.float64))
    mmr, mvr = R.bn_moving(mm, mv, mean, var, 1)
    assert _rel(mmr, mm_o) < TOL and _rel(mvr, mv_o) < TOL


def test_maxpool_reference_routes_to_the_first_maximum():
    rng = _rng(1)
    x = _t(rng.integers(-2, 3, size=(2, 6, 4, 5)), True)          # ties in most windows
    dy = _t(rng.standard_normal((2, 3, 2, 5)))
    y = T.max_pool2(x)
    y.backward(dy)
    assert torch.equal(R.maxpool2_fwd(x), y.detach()) and torch.equal(R.maxpool2_bwd(x, dy), x.grad)
    t = _t([[[[1.0], [1.0]], [[1.0], [1.0]]]])                     # a fully tied window: the first element takes it all
    assert torch.equal(R.maxpool2_bwd(t, _t([[[[2.0]]]])).reshape(-1), _t([2.0, 0.0, 0.0, 0.0]))
    assert torch.equal(R.maxpool2_bwd(_t([[[[0.0], [1.0]], [[1.0], [0.0]]]]), _t([[[[2.0]]]])).reshape(-1), _t([0.0, 2.0, 0.0, 0.0]))


@pytest.mark.parametrize("N,A,B,r,nc", [(2, 3, 2, 2, 3), (1, 2, 3, 8, 2), (2, 1, 4, 1, 5), (3, 2, 2, 3, 4)])
def test_ps_reference(N, A, B, r, nc):
    x = _t(np.arange(N * A * B * nc * r * r).reshape(N, A, B, nc * r * r), True)
    y = T.PS(x, r, nc)
    assert torch.equal(R.ps_fwd(x, r, nc), y.detach())
    dy = _t(_rng(2).standard_normal(tuple(y.shape)))
    y.backward(dy)
    assert torch.equal(R.ps_bwd(dy, r, nc), x.grad)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4)])
def test_sympad_reference(H, W):
    rng = _rng(3)
    for p in range(0, min(H, W) + 1):
        x = _t(rng.standard_normal((2, H, W, 3)), True)
        xp = T.pad_symmetric(x, p, p)
        assert torch.equal(R.sympad_fwd(x, p), xp.detach())
        g = _t(rng.standard_normal(tuple(xp.shape)))
        xp.backward(g)
        assert _rel(R.sympad_bwd(g, p), x.grad) < TOL


@pytest.mark.parametrize("tile_a,ncls", [(3, 5), (1, 2), (3, 8)])
def test_critic_input_reference(tile_a, ncls):
    rng = _rng(4)
    sh = (2, 3, 4)
    ts = [_t(rng.standard_normal(sh + (n,)), True) for n in (2, 4, 3, 5, ncls)]
    with torch.no_grad():
        ts[4][0, 0, 0] = 1.0                                       # a tied maximum: the lowest index
        ts[4][0, 0, 1, 1:] = 7.0
    am = T.argmax_lowest(ts[4]).double().unsqueeze(-1)
    ref = torch.cat([ts[0].repeat(1, 1, 1, tile_a), ts[1], ts[2], ts[3], ts[4], am], dim=3)
    out = R.critic_input_fwd(ts[0], tile_a, ts[1], ts[2], ts[3], ts[4])
    assert torch.equal(out, ref.detach()) and float(out[0, 0, 0, -1]) == 0.0 and float(out[0, 0, 1, -1]) == 1.0
    g = _t(rng.standard_normal(tuple(ref.shape)))
    ref.backward(g)
    for got, t in zip(R.critic_input_bwd(g, (2, 4, 3, 5, ncls), tile_a), ts):
        assert _rel(got, t.grad) < TOL


def _seg_inputs(ncls, scale, absent, seed=5, shape=(2, 9, 7)):
    rng = _rng(seed)
    z = _t(rng.standard_normal(shape + (ncls,)) * scale, True)
    lab = rng.integers(0, ncls, size=shape)
    lab[rng.random(shape) < 0.5] = 0
    if absent:
        lab[lab == ncls - 2] = 0
    return z, _t(T.label_decomp(ncls, lab)), lab


@pytest.mark.parametrize("ncls,scale,absent", [(5, 1.0, False), (5, 4.0, True), (3, 8.0, True), (8, 4.0, False), (2, 1.0, False)])
@pytest.mark.parametrize("mius", [(1.0, 1.0), (0.1, 1.0), (1.0, 0.0), (0.0, 1.0)])
def test_seg_loss_reference_equals_the_oracle_under_autograd(ncls, scale, absent, mius):
    mc, md = mius
    z, y, lab = _seg_inputs(ncls, scale, absent)
    wl, dl = T.softmax_weighted_loss(z, y), T.dice_loss(z, y)
    tot, xent, dice, sums = R.seg_loss(z, y, mc, md)
    wl_f, dl_f = float(wl.detach()), float(dl.detach())
    assert abs(float(xent) - wl_f) < TOL * max(1, abs(wl_f)) and abs(float(dice) - dl_f) < TOL and abs(float(tot) - (mc * wl_f + md * dl_f)) < TOL
    p_true = (torch.softmax(z.detach(), -1) * y).sum(-1)
    if scale >= 4.0:
        assert bool((p_true < R.CLIP_P).any())                     # a pixel below the clip: no cross-entropy gradient there
    if absent:
        assert float(sums[0, ncls - 2]) == 0.0                     # the absent class: weight 1, Dice term 0 / (S + 1e-7)
    (0.5 * (mc * wl + md * dl)).backward(retain_graph=True)
    dz, pt = R.seg_loss_bwd(z, y, mc, md, 0.5)
    assert _rel(dz, z.grad) < TOL and _rel(pt, p_true) < TOL
    z.grad = None
    (mc * wl / 2 + md * dl).backward()                             # P_norm = 2P: the cross-entropy's mean halves, the Dice term does not
    assert _rel(R.seg_loss_bwd(z, y, mc, md, 1.0, 2 * p_true.numel())[0], z.grad) < TOL
    n, I, S, X = sums
    p = torch.softmax(z.detach(), -1).reshape(-1, ncls)
    assert _rel(n, y.reshape(-1, ncls).sum(0)) == 0 and _rel(S, (p * p).sum(0)) < TOL


def test_prediction_references():
    rng = _rng(6)
    z = _t(rng.standard_normal((2, 8, 8, 5)) * 3)
    z[0, 0, 0] = _t([1.0, 1.0, 0.5, 1.0, 0.0])
    z[0, 0, 1] = _t([0.0, 2.0, 0.5, 2.0, 2.0])
    p, lab = R.softmax_argmax(z)
    po = T.pixel_wise_softmax_2(z)
    assert _rel(p, po) < TOL and torch.equal(lab, T.argmax_lowest(po)) and int(lab[0, 0, 0]) == 0 and int(lab[0, 0, 1]) == 1
    truth = rng.integers(0, 5, size=(2, 8, 8))
    truth[truth == 3] = 0                                          # an absent class
    y = _t(T.label_decomp(5, truth))
    dm, arr = T.dice_eval(lab, y, 5)
    rd = R.dice_eval(lab, y)
    assert abs(float(rd[0] - dm)) < TOL and _rel(rd[1:], torch.stack(arr)) < TOL
    # labels outside [0, ncls): tf.one_hot gives a zero row — the same as dropping those pixels from the prediction's side only
    lab2 = lab.clone()
    lab2[0, 0, :4], lab2[1, 1, :4] = -1, 5
    inr = (lab2 >= 0) & (lab2 < 5)
    pred1h = torch.nn.functional.one_hot(lab2.clamp(0, 4), 5).double() * inr.unsqueeze(-1)
    want = torch.stack([2.0 * (pred1h[..., i] * y[..., i]).sum() / (pred1h[..., i].sum() + y[..., i].sum() + 1e-7) for i in range(5)])
    assert _rel(R.dice_eval(lab2, y)[1:], want) < TOL
    y0 = y.clone()
    y0[0, 0, 0] = 0.0                                              # a row without a label: class 0
    cy, cm = R.confusion_matrix(y0, lab2)
    cy_ref = y0.numpy().argmax(-1)
    cm_ref = np.zeros((5, 5), np.int64)
    np.add.at(cm_ref, (cy_ref[inr.numpy()], lab2.numpy()[inr.numpy()]), 1)
    assert np.array_equal(cy.numpy(), cy_ref) and np.array_equal(cm.numpy(), cm_ref) and int(cm.sum()) == int(inr.sum())


def test_optimiser_references():
    rng = _rng(7)
    n = 2500                                                       # three chunks, the last ragged
    w0, g = _t(rng.standard_normal(n) * 0.5), [_t(rng.standard_normal(n)) for _ in range(3)]
    l2, mask = _t([0.25, 0.0, 0.125]), torch.tensor([1, 0, 1], dtype=torch.uint8)
    for cl2, cm in ((None, None), (l2, None), (None, mask), (l2, mask)):
        l2e = R.per_element(cl2, n, 0.0)
        sel = R.per_element(cm, n, 1.0) != 0
        assert int(sel.sum()) == (n if cm is None else n - 1024)
        w, m, v = w0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        rw, rm, rv = w, m, v
        w2, ms = w0.clone(), torch.ones(n, dtype=torch.float64)
        rw2, rms = w2, ms
        w3, acc = w0.clone(), torch.zeros(n, dtype=torch.float64)
        rw3, racc = w3, acc
        for t in (1, 2, 3):
            rw, rm, rv = R.adam(rw, g[t - 1], rm, rv, cl2, cm, 1e-3, 0.9, 0.999, 1e-8, t)
            wn, mn, vn = w.clone(), m.clone(), v.clone()
            T.adam_update(wn, g[t - 1] + l2e * w, mn, vn, 1e-3, t)
            w, m, v = torch.where(sel, wn, w), torch.where(sel, mn, m), torch.where(sel, vn, v)
            rw2, rms = R.rmsprop(rw2, g[t - 1], rms, cl2, cm, 3e-4)
            wn, msn = w2.clone(), ms.clone()
            T.rmsprop_update(wn, g[t - 1] + l2e * w2, msn, 3e-4)
            w2, ms = torch.where(sel, wn, w2), torch.where(sel, msn, ms)
            rw3, racc = R.momentum(rw3, g[t - 1], racc, cl2, cm, 0.2, 0.2)
            wn, an = w3.clone(), acc.clone()
            T.momentum_update(wn, g[t - 1] + l2e * w3, an, 0.2, 0.2)
            w3, acc = torch.where(sel, wn, w3), torch.where(sel, an, acc)
        for a, b in ((rw, w), (rm, m), (rv, v), (rw2, w2), (rms, ms), (rw3, w3), (racc, acc)):
            assert _rel(a, b) < TOL
        if cm is not None:
            assert torch.equal(rw[1024:2048], w0[1024:2048]) and torch.equal(rms[1024:2048], torch.ones(1024, dtype=torch.float64))
        assert torch.equal(R.clip(w0, cm, -0.3, 0.25), torch.where(sel, w0.clamp(-0.3, 0.25), w0))
        want = sum(float(c) * float(T.l2_loss(w0[i * 1024:(i + 1) * 1024])) for i, c in enumerate((1.0, 1.0, 1.0) if cl2 is None else cl2.tolist()))
        assert abs(float(R.l2_loss(w0, cl2)) - want) < TOL * want


def test_wgan_reference():
    rng = _rng(8)
    o = {k: _t(rng.standard_normal((7, 1)) + 0.3) for k in ("ct_cls", "mr_cls", "ct_mask", "mr_mask")}
    miu, lam = 0.002, 0.3
    dis, gen = nets_adv.wgan_losses(o, miu, miu, lam)
    ops = [o["ct_cls"], o["mr_cls"], o["ct_mask"], o["mr_mask"]]
    assert abs(float(R.wgan_loss(ops, (miu, -miu, lam * miu, -lam * miu)) - dis)) < TOL
    assert abs(float(R.wgan_loss([ops[0], None, ops[2], None], (-miu, 5.0, -lam * miu, 5.0)) - gen)) < TOL


# ---- (b) the case lists against the dispatch predicates --------------------------------------------------------------------------------
NT = 256


def bn_vec(C, Cs):
    """pnp_bn_apply_h / pnp_bn_bwd_apply_h: the thread-owns-a-channel-quad kernels"""
    return C % 4 == 0 and (Cs == 0 or (Cs % 4 == 0 and ((C - Cs) // 2) % 4 == 0))


def bn_slices(C):
    """grid_rows: blockIdx.y slices of 256 channel quads"""
    return (C // 4 + NT - 1) // NT


def bn_rows_per_pass(C):
    return NT // min(C // 4, NT)


def colreduce_scalar(C):
    """run_colreduce: the one-thread-per-channel reduction"""
    return C % 4 != 0 or C > 1024


def grid_capped(nvec, cap=2048):
    """grid_for: more work than cap workgroups of 256 -> the grid-stride loop runs more than once"""
    return (nvec + NT - 1) // NT > cap


def ps_tile_T(B, Cin):
    if Cin > 4096:
        return 0
    T_ = min(4096 // Cin, B)
    while T_ > 1 and B % T_ != 0:
        T_ -= 1
    return T_


def loss_blocks(P):
    return min(max((P + NT * 4 - 1) // (NT * 4), 1), 1024)


def _require(branches):
    missing = [k for k, v in branches.items() if not v]
    assert not missing, "no case reaches: %s" % ", ".join(missing)


def test_bn_case_list_reaches_every_branch(built):
    lib = pkg("_lib").load()
    nblk = lambda P, C: int(lib.pnp_bn_workspace_bytes(P, C)) // (8 * C)
    cs = ED.BN_CASES
    assert 25 <= len(cs) <= 40 and len(set(cs)) == len(cs)
    assert all(Cs <= C and (C - Cs) % 2 == 0 for _, C, Cs, *_ in cs)
    vec = lambda c: bn_vec(c[1], c[2])
    nb = [nblk(c[0], c[1]) for c in cs]
    _require({
        "vector apply with a shortcut": any(vec(c) and c[2] for c in cs),
        "vector apply with a padded shortcut": any(vec(c) and 0 < c[2] < c[1] for c in cs),
        "scalar apply, shortcut channels not a multiple of 4": any(c[1] % 4 == 0 and c[2] % 4 != 0 for c in cs),
        "scalar apply, pad not a multiple of 4": any(c[1] % 4 == 0 and c[2] and c[2] % 4 == 0 and not vec(c) for c in cs),
        "scalar apply, C % 4 != 0 with a shortcut": any(c[1] % 4 != 0 and c[2] for c in cs),
        "scalar apply, C % 4 != 0 without a shortcut": any(c[1] % 4 != 0 and not c[2] for c in cs),
        "scalar apply with Cs = 2": any(c[2] == 2 for c in cs),
        "second blockIdx.y slice (vector, C > 1024)": any(vec(c) and bn_slices(c[1]) == 2 for c in cs),
        "second slice with a shortcut": any(vec(c) and bn_slices(c[1]) == 2 and c[2] for c in cs),
        "second slice narrower than the first (its own C4s / rpi)": any(vec(c) and bn_slices(c[1]) == 2 and (c[1] // 4) % NT != 0 for c in cs),
        "scalar apply at C > 1024": any(not vec(c) and c[1] > 1024 for c in cs),
        "scalar column reduction, C > 1024": any(c[1] > 1024 and c[1] % 4 == 0 for c in cs),
        "scalar column reduction, C % 4 != 0": any(c[1] % 4 != 0 for c in cs),
        "scalar column reduction over a long partial list": any(colreduce_scalar(c[1]) and n >= 512 for c, n in zip(cs, nb)),
        "P = 1 in training mode (Bessel factor 1)": any(c[0] == 1 and c[4] for c in cs),
        "1 < P < rows per pass (vector)": any(vec(c) and 1 < c[0] < bn_rows_per_pass(c[1]) for c in cs),
        "P not a multiple of the rows per pass": any(vec(c) and c[0] % bn_rows_per_pass(c[1]) != 0 and c[0] > bn_rows_per_pass(c[1]) for c in cs),
        "vector apply grid capped": any(vec(c) and -(-c[0] // bn_rows_per_pass(c[1])) > 2048 // bn_slices(c[1]) for c in cs),
        "scalar apply grid capped": any(not vec(c) and grid_capped(c[0] * c[1]) for c in cs),
        "partial list below 512": any(n < 512 for n in nb),
        "one partial": any(n == 1 for n in nb),
        "partial list compacted (>= 512)": any(n >= 512 for n in nb),
        "compacted with a last slab longer than 128": any(n >= 512 and n % 128 != 0 for n in nb),
        "2048 partials": any(n == 2048 for n in nb),
        "no activation": any(c[3] < 0 for c in cs), "ReLU": any(c[3] == 0 for c in cs), "leaky ReLU": any(c[3] == 0.2 for c in cs),
        "inference, vector": any(not c[4] and vec(c) for c in cs), "inference, scalar": any(not c[4] and not vec(c) for c in cs),
        "dropout mask, vector": any(c[5] < 1 and vec(c) for c in cs), "dropout mask, scalar": any(c[5] < 1 and not vec(c) for c in cs),
        "keep 0.5": any(c[5] == 0.5 for c in cs),
        "sign recomputed, training, vector": any(c[4] and not c[2] and c[3] >= 0 and vec(c) for c in cs),
        "sign recomputed, training, scalar": any(c[4] and not c[2] and c[3] >= 0 and not vec(c) for c in cs),
        "sign recomputed, inference, vector": any(not c[4] and not c[2] and c[3] >= 0 and vec(c) for c in cs),
        "sign recomputed, inference, scalar": any(not c[4] and not c[2] and c[3] >= 0 and not vec(c) for c in cs),
    })
    assert {c[1] for c in cs} >= {4, 6, 20, 24, 40, 64, 512, 1028, 1200} and {c[0] for c in cs} >= {1, 3, 63, 64, 1000, 40000}
    for C, Cv, Csc in ED.BN_TWIN_CASES:
        assert bn_vec(C, Cv) and not bn_vec(C, Csc) and Csc < Cv <= C
    _require({"twin at C > 1024": any(C > 1024 for C, _, _ in ED.BN_TWIN_CASES),
              "twin with a pad that is not a multiple of 4": any(Csc % 4 == 0 for _, _, Csc in ED.BN_TWIN_CASES),
              "twin with shortcut channels not a multiple of 4": any(Csc % 4 != 0 for _, _, Csc in ED.BN_TWIN_CASES),
              "bf16 side outputs, vector": any(bn_vec(C, Cs) for _, C, Cs in ED.BN_H_CASES),
              "bf16 side outputs, scalar with a shortcut": any(not bn_vec(C, Cs) and Cs for _, C, Cs in ED.BN_H_CASES),
              "bf16 side outputs, scalar C % 4 != 0": any(C % 4 != 0 for _, C, Cs in ED.BN_H_CASES),
              "bf16 side outputs, second slice": any(bn_vec(C, Cs) and bn_slices(C) == 2 for _, C, Cs in ED.BN_H_CASES),
              "SyncBN split, vector": any(bn_vec(C, Cs) for _, C, Cs in ED.SYNCBN_CASES),
              "SyncBN split, scalar": any(not bn_vec(C, Cs) for _, C, Cs in ED.SYNCBN_CASES),
              "SyncBN split over more than one partial per half": any(nblk(Ph, C) > 1 for Ph, C, _ in ED.SYNCBN_CASES)})
    assert all((Ph * C * 4) % 16 == 0 and (Ph * Cs * 4) % 16 == 0 for Ph, C, Cs in ED.SYNCBN_CASES)      # the second half stays 16-byte aligned


def test_data_movement_case_lists_reach_every_branch():
    work = lambda s: s[0] * (s[1] // 2) * (s[2] // 2) * (s[3] // 4 if s[3] % 4 == 0 else s[3])
    mp = ED.MAXPOOL_CASES
    _require({"max-pool vector form past the grid cap": any(s[3] % 4 == 0 and grid_capped(work(s)) for s in mp),
              "max-pool scalar form past the grid cap": any(s[3] % 4 != 0 and grid_capped(work(s)) for s in mp),
              "max-pool scalar form, small": any(s[3] % 4 != 0 and not grid_capped(work(s)) for s in mp),
              "max-pool H = 2": any(s[1] == 2 for s in mp), "max-pool W = 2": any(s[2] == 2 for s in mp)})
    ps = [(r, nc, B, nc * r * r, ps_tile_T(B, nc * r * r)) for r in ED.PS_R for nc in ED.PS_NC for B in ED.PS_B]
    assert set(ED.PS_R) >= {1, 2, 8} and set(ED.PS_NC) >= {1, 3, 5, 40, 63, 64, 65} and set(ED.PS_B) >= {1, 2, 7, 12, 13, 32}
    assert ED.PS_N * ED.PS_A * max(ED.PS_B) * max(ED.PS_NC) * max(ED.PS_R) ** 2 < 1 << 24            # arange stays exact in float32
    _require({"PS per-element kernel (Cin > 4096)": any(T_ == 0 for *_, T_ in ps),
              "PS Cin = 4096": any(Cin == 4096 and T_ == 1 for *_, Cin, T_ in ps),
              "PS Cin = 4032": any(Cin == 4032 for *_, Cin, T_ in ps), "PS Cin = 4160": any(Cin == 4160 for *_, Cin, T_ in ps),
              "PS T = 1 because B is prime": any(T_ == 1 and B > 1 and 4096 // Cin >= 2 for _, _, B, Cin, T_ in ps),
              "PS T = B": any(T_ == B and B > 1 for _, _, B, Cin, T_ in ps),
              "PS T cut by the divisor search": any(1 < T_ < min(4096 // Cin, B) for _, _, B, Cin, T_ in ps if T_),
              "PS T cut to 4096 / Cin": any(T_ == 4096 // Cin < B and T_ > 1 for _, _, B, Cin, T_ in ps if T_),
              "PS r = 1 (identity)": any(r == 1 for r, *_ in ps),
              "PS tile longer than one pass of 256 threads": any(T_ * Cin > NT for *_, Cin, T_ in ps),
              "PS tile shorter than 256": any(0 < T_ * Cin < NT for *_, Cin, T_ in ps)})
    _require({"sympad p = H": any(min(H, W) == H for H, W in ED.SYMPAD_HW), "sympad p = W < H": any(W < H for H, W in ED.SYMPAD_HW),
              "sympad 1 x 1": (1, 1) in ED.SYMPAD_HW, "sympad vector form": any(C % 4 == 0 for C in ED.SYMPAD_C),
              "sympad scalar form": any(C % 4 != 0 for C in ED.SYMPAD_C)})
    cr = [(Ca * ta + Cb + Cc + Cd + ncls + 1, Ca + Cb + Cc + Cd + ncls, ta, ncls, sh[0] * sh[1] * sh[2]) for Ca, ta, Cb, Cc, Cd, ncls, sh in ED.CRITIC_CASES]
    _require(dict([("critic Ctot %% 4 = %d" % k, any(ct % 4 == k for ct, *_ in cr)) for k in range(4)] + [
        ("critic tile_a = 1", any(ta == 1 for _, _, ta, _, _ in cr)), ("critic tile_a = 3", any(ta == 3 for _, _, ta, _, _ in cr)),
        ("critic ncls 2, 5, 8", {n for _, _, _, n, _ in cr} >= {2, 5, 8}),
        ("critic vector forward past the grid cap", any(ct % 4 == 0 and grid_capped(P * ct // 4, 4096) for ct, _, _, _, P in cr)),
        ("critic scalar forward past the grid cap", any(ct % 4 != 0 and grid_capped(P * ct, 4096) for ct, _, _, _, P in cr)),
        ("critic backward past the grid cap", any(grid_capped(P * cs, 4096) for _, cs, _, _, P in cr))]))
    ns = ED.STREAM_N
    assert set(ns) >= {1, 3, 4, 5, 1023, 1024, 1025, (1 << 21) + 3} and set(ED.DROP_KEEPS) >= {1.0, 0.75, 0.5}
    _require({"tail after a vector body": any(n > 4 and n % 4 for n in ns), "tail only": any(n < 4 for n in ns),
              "no tail": any(n % 4 == 0 for n in ns), "streaming grid capped": any(grid_capped(n // 4 + 1) for n in ns)})


def test_loss_and_optimiser_case_lists_reach_every_branch():
    sg = LD.SEG_CASES
    _require(dict([("seg loss ncls = %d" % k, any(c[0] == k for c in sg)) for k in range(1, 9)] + [
        ("seg loss P = %d" % P, any(c[1] == P for c in sg)) for P in (1, 255, 256, 257, 4097, 1 << 20, (1 << 20) + 1, (1 << 22) + 5)] + [
        ("seg loss scale %g" % s, any(c[2] == s for c in sg)) for s in (0.1, 1.0, 4.0, 12.0)] + [
        ("seg loss mius %s" % (m,), any(c[4] == m for c in sg)) for m in ((1.0, 1.0), (0.1, 1.0), (1.0, 0.0), (0.0, 1.0))] + [
        ("seg loss with an absent class", any(c[3] == "absent" and c[0] > 2 for c in sg)),
        ("seg loss with every pixel in one class", any(c[3] == "single" and c[0] > 1 for c in sg)),
        ("seg loss P not a multiple of 256", any(c[1] % 256 for c in sg)),
        ("seg loss one workgroup", any(loss_blocks(c[1]) == 1 for c in sg)),
        ("seg loss fewer than 32 workgroups", any(1 < loss_blocks(c[1]) < 32 for c in sg)),
        ("seg loss exactly 1024 workgroups, uncapped", any(loss_blocks(c[1]) == 1024 and c[1] <= 1024 * 1024 for c in sg)),
        ("seg loss grid capped at 1024", any(c[1] > 1024 * 1024 for c in sg)),
        ("seg loss 16 pixels per thread", any(c[1] > 16 * 1024 * 256 for c in sg)),
        ("seg loss MAXC classes past the cap", any(c[0] == 8 and c[1] > 1024 * 1024 for c in sg))]))
    pc = LD.PRED_CASES
    _require({"prediction ncls 1 and 8": {c[0] for c in pc} >= {1, 8}, "prediction grid capped": any(c[1] > 1024 * 1024 for c in pc),
              "prediction ragged P": any(c[1] % 256 for c in pc), "prediction P = 1": any(c[1] == 1 for c in pc),
              "prediction large logits": any(c[2] >= 12 for c in pc)})
    assert set(LD.WGAN_B) >= {1, 2, 16, 63, 64, 65, 300} and len(set(LD.WGAN_COEFS)) == 4 and min(LD.WGAN_COEFS) < 0
    ns = LD.OPT_N
    assert set(ns) >= {1, 1000, 1024, 5000, (1 << 20) + 7} and set(LD.OPT_COMBOS) == {(False, False), (True, False), (False, True), (True, True)}
    ch = [LD._chunks(n, True, True, torch.device("cpu")) for n in ns]
    _require({"n = 1": 1 in ns, "n below a chunk": any(1 < n < 1024 for n in ns), "n a multiple of 1024": any(n % 1024 == 0 for n in ns),
              "ragged last chunk after whole ones": any(n > 1024 and n % 1024 for n in ns),
              "masked-out chunk with L2": any(bool(((m == 0) & (l2 != 0)).any()) for l2, m in ch),
              "selected chunk with L2 = 0": any(bool(((m != 0) & (l2 == 0)).any()) for l2, m in ch),
              "masked-out ragged last chunk or selected one": any(n % 1024 and len(m) > 1 for n, (l2, m) in zip(ns, ch)),
              "l2_loss over more than 1024 chunks": any(n > 1024 * 1024 for n in LD.L2_N),
              "l2_loss of one element": 1 in LD.L2_N})
