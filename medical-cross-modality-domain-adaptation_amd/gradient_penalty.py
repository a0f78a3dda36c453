"""Opt-in WGAN-GP gradient penalty for the feature and mask critics (cost_kwargs["gp_weight"] > 0).  No reference parity
target: the reference bounds the critics only by clipping their weights to +-0.03 (adversarial.py:654, 861); with the penalty on, the
clip does not run.

With f = miu_dis * D (D a critic's raw score as _get_cost uses it, adversarial.py:455-458) and x_hat = eps_i x_MR + (1 - eps_i) x_CT:
    GP(f, x_hat) = mean_i ( |grad_{x_hat_i} sum_j f(x_hat_j)|_2 - 1 )^2
    dis_loss += gp_weight * [ GP(f_cls, x_hat_cls) + lambda_mask_loss * GP(f_mask, x_hat_mask) ]
so gp_weight = 10 is the WGAN-GP paper's value on the loss this project minimises.  The critics run batch statistics (of the
interpolated batch) and dropout at their keep probability; the moving averages are left alone.

The penalty differentiates the critic's backward pass a second time.  Instead of twice-differentiable autograd Functions, an explicit
walker runs four hand-scheduled passes over the critic's unit list (`unit_plan`, read from the same table as the graph builders):
  1. forward on x_hat, keeping each unit's input, BN input d, batch statistics and output y
  2. input-gradient backward from g_h = miu_dis * w_out per sample (bn_bwd + conv2d_dgrad, no filter gradients), keeping g_y and g_c
  3. penalty and its adjoint (pnp_gp_penalty), then the adjoint pass in forward order: g_c_bar = conv2d_fwd(g_x_bar, W),
     W_bar += wgrad(g_x_bar, g_c), BN double backward (pnp_bn_dbl_bwd) -> g_y_bar, gamma_bar, d_bar; w_out_bar += miu_dis sum_i g_h_bar_i
  4. ordinary backward with zero gradient at the critic output and d_bar added to the gradient of d in every unit (W, gamma, beta)
Every gradient is added into the store's gradient arena (scaled by the data-parallel 1/world like the loss's), so the optimiser and the
all-reduce see it with the WGAN loss's.
"""
import torch

from . import _lib
from . import kernels as K
from .functional import BN_EPS, LEAK


def critic_table(which, feature_base=16, num_cls=5):
    """THE topology of the two critics (adversarial.py:320-443), read by Full_DRN.create_classifier / create_mask_critic and by
    `unit_plan`.  [(variable scope, [layer, ...]), ...] with
      ("rb", bn scope, cin, cout, inc_dim)                          residual_block, filters Variable / Variable_1, 3x3, BN scope_1 / _2
      ("cbr", filter leaf, bn scope, k, cin, cout, stride, padding)  conv_bn_relu2d
      ("fc", D)                                                      the final matmul, filter Variable [D, 1]"""
    fb = feature_base
    if which == "cls":
        spec = [(1, fb * 2, fb * 4, 3, 2, True), (2, fb * 4, fb * 8, 5, 2, True), (3, fb * 8, fb * 16, 3, 2, True),
                (4, fb * 16, fb * 32, 3, 2, True), (5, fb * 32, fb * 32, 5, 4, False)]
        t = [("cls_%d" % k, [("rb", "cls_%d" % k, cin, cout, inc), ("cbr", "Variable_2", "cls_%d_3" % k, kd, cout, cout, sd, "SAME")])
             for k, cin, cout, kd, sd, inc in spec]
        t.append(("cls_6", [("cbr", "Variable", "cls_6", 3, fb * 32, fb * 32, 2, "SYMMETRIC")]))
        t.append(("cls_out", [("fc", fb * 32 * 4)]))
        return t
    if which == "mask":
        return [("mask_cls_1", [("cbr", "Variable", "mask_cls_1", 3, num_cls, fb, 2, "SAME")]),
                ("mask_cls_2", [("rb", "m_cls_2", fb, fb, False), ("cbr", "Variable_2", "m_cls_2_3", 5, fb, fb * 2, 4, "SAME")]),
                ("mask_cls_3", [("rb", "m_cls_3", fb * 2, fb * 4, True), ("cbr", "Variable_2", "m_cls_3_3", 5, fb * 4, fb * 8, 4, "SAME")]),
                ("mask_cls_4", [("cbr", "Variable", "m_cls_4", 5, fb * 8, fb * 16, 4, "SYMMETRIC")]),
                ("m_cls_out", [("fc", fb * 16 * 4)])]
    raise ValueError("critic must be 'cls' or 'mask', got %r" % (which,))


CRITIC_SCOPE = {"cls": "cls_scope", "mask": "mask_cls_scope"}


def unit_plan(which, feature_base=16, num_cls=5):
    """-> (units, fc): the critic's conv units in forward order, each {w, k, cin, cout, stride, padding, bn, shortcut, inc_dim} with
    full TF names (shortcut: index of the unit whose INPUT is added after this unit's BN, None otherwise), and the fc filter's name"""
    top = CRITIC_SCOPE[which]
    units, fc = [], None
    for scope, layers in critic_table(which, feature_base, num_cls):
        pre = "%s/%s/" % (top, scope)
        for L in layers:
            if L[0] == "rb":
                _, bn, cin, cout, inc = L
                head = len(units)
                units.append(dict(w=pre + "Variable", k=3, cin=cin, cout=cout, stride=1, padding="SAME", bn=pre + bn + "_1", shortcut=None,
                                  inc_dim=False))
                units.append(dict(w=pre + "Variable_1", k=3, cin=cout, cout=cout, stride=1, padding="SAME", bn=pre + bn + "_2", shortcut=head,
                                  inc_dim=bool(inc)))
            elif L[0] == "cbr":
                _, leaf, bn, k, cin, cout, stride, pad = L
                units.append(dict(w=pre + leaf, k=k, cin=cin, cout=cout, stride=stride, padding=pad, bn=pre + bn, shortcut=None, inc_dim=False))
            else:
                fc = pre + "Variable"
    return units, fc


def _slot(st, name):
    v = st.vars[name]
    if not v.trainable:
        raise RuntimeError("gradient penalty: critic variable %s is not trainable (cls_trainable / m_cls_trainable)" % name)
    return st.grad_arena[v.offset:v.offset + v.numel].view(v.shape)


def critic_gradient_penalty(net, critic, x_a, x_b, coef, seed, stream0, gscale=None, keep_prob=None):
    """coef * GP(miu_dis * D_critic, x_hat) for critic 'cls' (feature critic, inputs = the assembled 32-channel critic inputs) or 'mask'
    (inputs = the segmenter logits); x_a = MR, x_b = CT [B, H, W, C], constants.  Adds the penalty's gradients (times gscale, default
    1 / world_size) into net.store's gradient arena.  Dropout stream ids: units use stream0, stream0 + 1, ... in forward order (one id
    per conv call site, like the graph's own), eps is drawn from stream0 + n_units.
    -> (penalty [1] (coef included), norms [B] = |grad_{x_hat_i} sum_j f|, eps [B], next free stream id)"""
    with torch.no_grad():
        return _penalty(net, critic, x_a, x_b, coef, seed, stream0, gscale, keep_prob)


def _penalty(net, critic, x_a, x_b, coef, seed, stream0, gscale, keep_prob):
    from .adversarial import CRITIC_KEEP_PROB
    if K.CONV_DTYPE != _lib.DTYPE_F32:
        raise RuntimeError("gradient penalty: fp32 convolutions only (--dtype bf16 is not supported with gp_weight > 0)")
    keep = CRITIC_KEEP_PROB if keep_prob is None else float(keep_prob)
    gscale = 1.0 / net.world_size if gscale is None else float(gscale)
    st = net.store
    units, fc_name = unit_plan(critic, net.feature_base, net.n_class)
    var = lambda n: st.vars[n].tensor          # (raw kernels only: nothing here is recorded on a tape)
    bn_of = lambda u: tuple(var(u["bn"] + "/" + s) for s in ("gamma", "beta"))
    x_a, x_b = x_a.detach().contiguous(), x_b.detach().contiguous()
    B = x_a.shape[0]
    x0, eps = K.gp_interpolate(x_a, x_b, seed, stream0 + len(units))
    sids = [stream0 + i for i in range(len(units))]

    # ---- 1. forward on x_hat (batch statistics of x_hat, moving averages untouched)
    sv = []
    h = x0
    for i, u in enumerate(units):
        p = u["k"] // 2
        xp = K.sympad_fwd(h, p) if u["padding"] == "SYMMETRIC" else h
        g = K.conv_geom(tuple(xp.shape), (u["k"], u["k"], u["cin"], u["cout"]), u["stride"], 1,
                        "VALID" if u["padding"] == "SYMMETRIC" else "SAME")
        d = K.conv2d_fwd(xp, var(u["w"]), g, keep, seed, sids[i])
        mean, vr = K.bn_stats(d)
        gamma, beta = bn_of(u)
        sc = sv[u["shortcut"]]["x"] if u["shortcut"] is not None else None
        y = K.bn_apply(d, mean, vr, gamma, beta, sc, BN_EPS, LEAK)
        sv.append(dict(x=h, xp=xp, g=g, d=d, mean=mean, var=vr, y=y))
        h = y
    hL = h
    D = hL.numel() // B
    g_fc = K.conv_geom((B, 1, 1, D), (1, 1, D, 1), 1, 1, "VALID")
    w_out = var(fc_name).reshape(1, 1, D, 1)
    s = K.filled((B, 1, 1, 1), net.miu_dis, x0.device)

    # ---- 2. input-gradient backward from g_h = miu_dis * w_out per sample
    gy = K.conv2d_dgrad(s, w_out, g_fc).reshape(hL.shape)
    res = {}
    for i in reversed(range(len(units))):
        u, r = units[i], sv[i]
        Cs = sv[u["shortcut"]]["x"].shape[-1] if u["shortcut"] is not None else 0
        gc, _, _, dsc = K.bn_bwd(gy, r["y"], r["d"], r["mean"], r["var"], bn_of(u)[0], Cs, BN_EPS, LEAK, True, keep, seed, sids[i])
        r["gy"], r["gc"] = gy, gc
        if Cs:
            res[u["shortcut"]] = dsc
        gx = K.conv2d_dgrad(gc, var(u["w"]), r["g"], residual=res.pop(i, None))
        gy = K.sympad_bwd(gx, u["k"] // 2) if u["padding"] == "SYMMETRIC" else gx

    # ---- 3. penalty, its adjoint, and the adjoint pass in forward order
    gx0 = gy
    pen, norms = K.gp_penalty_(gx0, coef, gscale)          # gx0 now holds gscale * dP/d(grad_x)
    in_bar = [gx0]
    for i, u in enumerate(units):
        r = sv[i]
        gb = in_bar[i]
        gbp = K.sympad_fwd(gb, u["k"] // 2) if u["padding"] == "SYMMETRIC" else gb
        gc_bar = K.conv2d_fwd(gbp, var(u["w"]), r["g"])
        K.conv2d_wgrad(gbp, r["gc"], r["g"], into=_slot(st, u["w"]))
        sc_bar = in_bar[u["shortcut"]] if u["shortcut"] is not None else None
        gy_bar, r["xc_bar"] = K.bn_dbl_bwd(gc_bar, r["d"], r["y"], r["gy"], r["mean"], r["var"], bn_of(u)[0], sc_bar, BN_EPS, LEAK, keep,
                                           seed, sids[i], gamma_bar=_slot(st, u["bn"] + "/gamma"))
        del r["gy"], r["gc"]
        in_bar.append(gy_bar)
    K.conv2d_wgrad(in_bar[-1].reshape(B, 1, 1, D), s, g_fc, into=_slot(st, fc_name).view(1, 1, D, 1))
    del in_bar

    # ---- 4. ordinary backward: zero gradient at the critic output, d_bar added to the gradient of d in every unit
    gy = None
    res = {}
    for i in reversed(range(len(units))):
        u, r = units[i], sv[i]
        if gy is None:
            gc = r["xc_bar"]
        else:
            Cs = sv[u["shortcut"]]["x"].shape[-1] if u["shortcut"] is not None else 0
            gc, _, _, dsc = K.bn_bwd(gy, r["y"], r["d"], r["mean"], r["var"], bn_of(u)[0], Cs, BN_EPS, LEAK, True, keep, seed, sids[i],
                                     into=(_slot(st, u["bn"] + "/gamma"), _slot(st, u["bn"] + "/beta")))
            K.axpby(r["xc_bar"], gc, 1.0, 1.0)
            if Cs:
                res[u["shortcut"]] = dsc
        K.conv2d_wgrad(r["xp"], gc, r["g"], into=_slot(st, u["w"]))
        if i > 0:
            gx = K.conv2d_dgrad(gc, var(u["w"]), r["g"], residual=res.pop(i, None))
            gy = K.sympad_bwd(gx, u["k"] // 2) if u["padding"] == "SYMMETRIC" else gx
        sv[i] = None
    return pen, norms, eps, stream0 + len(units) + 1
