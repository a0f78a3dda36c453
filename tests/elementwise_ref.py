"""float64 references of the elementwise, loss and optimiser kernels (csrc/elementwise.hip, csrc/loss_optim.hip, the two sympad kernels).

Plain torch, written from the definitions in oracle/tf_ops.py and oracle/nets_adv.py (closed forms of their gradients, no autograd), and
device-agnostic like parity_util.rel: they compute wherever their inputs live, so the -m gpu tests get float64 references on the device.
tests/test_elementwise_ref_host.py pins every function to the oracle's own function under autograd, in float64, on the CPU.

Conventions: tensors are [..., C] with the channels last; every input is widened to float64; nothing is modified in place.
"""
import torch

BN_EPS = 1e-3
BN_DECAY = 0.9
OPT_CHUNK = 1024        # elements per optimiser chunk (include/pnp_hip.h: PNP_OPT_CHUNK)
CLIP_P = 0.005          # the cross-entropy's lower clip of the softmax


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().double()


def first_max(win):
    """{0,1} mask of the FIRST maximal element along the last axis (lowest index on ties)"""
    eq = win == win.max(dim=-1, keepdim=True).values
    return eq & (eq.cumsum(dim=-1) == 1)


def argmax_lowest(t):
    fm = first_max(t)
    return (fm.long() * torch.arange(t.shape[-1], device=t.device)).sum(-1)


# ---- batch norm (+ zero-padded shortcut, + leaky-ReLU, + the dropout mask of the convolution in front of it) ---------------------------
def bn_stats(x):
    """per-channel mean and BIASED variance over every leading axis"""
    x = _f64(x).reshape(-1, x.shape[-1])
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def bn_moving(mm, mv, mean, var, P, decay=BN_DECAY):
    """the moving averages after one training-mode execution: the moving variance receives the Bessel-corrected batch variance"""
    bessel = P / (P - 1.0) if P > 1 else 1.0
    mm, mv, mean, var = _f64(mm), _f64(mv), _f64(mean), _f64(var)
    return mm - (mm - mean) * (1.0 - decay), mv - (mv - var * bessel) * (1.0 - decay)


def pad_channels(s, C):
    """zero-pad the last axis of s symmetrically to C channels"""
    Cs = s.shape[-1]
    cpad = (C - Cs) // 2
    out = torch.zeros(s.shape[:-1] + (C,), dtype=s.dtype, device=s.device)
    out[..., cpad:cpad + Cs] = s
    return out


def act(z, alpha):
    """leaky-ReLU max(alpha z, z); alpha < 0: no activation"""
    return z if alpha < 0 else torch.where(z > 0, z, z * alpha)


def bn_apply(x, mean, var, gamma, beta, shortcut=None, alpha=0.2, eps=BN_EPS):
    """act((x - mean) * gamma / sqrt(var + eps) + beta + pad(shortcut)); (mean, var) = batch statistics (training) or the moving ones"""
    x, mean, var, gamma, beta = (_f64(t) for t in (x, mean, var, gamma, beta))
    z = (x - mean) * (gamma * torch.rsqrt(var + eps)) + beta
    if shortcut is not None:
        z = z + pad_channels(_f64(shortcut), x.shape[-1])
    return act(z, alpha)


def bn_bwd_sums(dout, out, x, mean, var, alpha=0.2, eps=BN_EPS):
    """(dgamma, dbeta) = (sum dz * xhat, sum dz) with dz = the activation's gradient, its sign read from the saved output `out`
    (LeakyReluGrad: features > 0)"""
    dout, x, mean, var = (_f64(t) for t in (dout, x, mean, var))
    C = x.shape[-1]
    g = dout if alpha < 0 else torch.where(_f64(out) > 0, dout, dout * alpha)
    xh = (x - mean) * torch.rsqrt(var + eps)
    return (g * xh).reshape(-1, C).sum(0), g.reshape(-1, C).sum(0), g, xh


def bn_bwd(dout, out, x, mean, var, gamma, shortcut_channels=0, alpha=0.2, training=True, mask=None, keep=1.0, P_norm=None, sums=None,
           eps=BN_EPS):
    """-> (dx, dgamma, dbeta, dshortcut).
    training: mean / var are functions of x, dx = gamma rs (dz - dbeta / P_norm - xhat dgamma / P_norm); `sums` = (dgamma, dbeta) over
    P_norm rows when they were reduced elsewhere (synchronised BN), default: this tensor's own sums and row count.
    inference: dx = gamma rs dz.  mask / keep: x was dropout(xa) = xa * mask / keep, dx is the gradient reaching xa."""
    gamma, var64 = _f64(gamma), _f64(var)
    C = x.shape[-1]
    P = x.numel() // C
    dgamma, dbeta, g, xh = bn_bwd_sums(dout, out, x, mean, var, alpha, eps)
    sg, sb = (dgamma, dbeta) if sums is None else (_f64(sums[0]), _f64(sums[1]))
    Pn = float(P if P_norm is None else P_norm)
    sc = gamma * torch.rsqrt(var64 + eps)
    dx = sc * (g - sb / Pn - xh * (sg / Pn)) if training else sc * g
    if mask is not None and keep < 1.0:
        dx = dx * _f64(mask) / keep
    dsc = None
    if shortcut_channels:
        cpad = (C - shortcut_channels) // 2
        dsc = g[..., cpad:cpad + shortcut_channels]
    return dx, dgamma, dbeta, dsc


# ---- 2x2 / 2 max-pool ------------------------------------------------------------------------------------------------------------------
def _windows(x):
    N, H, W, C = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)      # row-major window scan


def maxpool2_fwd(x):
    return _windows(_f64(x)).max(dim=-1).values


def maxpool2_bwd(x, dy):
    """the gradient goes to the first maximum of each window in row-major scan order"""
    N, H, W, C = x.shape
    d = first_max(_windows(_f64(x))).double() * _f64(dy).unsqueeze(-1)
    return d.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)


# ---- PS (phase shift): out[n, i*r+u, j*r+v, c] = x[n, i, j, c*r*r + v*r + u] -----------------------------------------------------------
def _ps_index(A, B, r, nc, device):
    ho = torch.arange(A * r, device=device).view(-1, 1, 1)
    wo = torch.arange(B * r, device=device).view(1, -1, 1)
    c = torch.arange(nc, device=device).view(1, 1, -1)
    i, u, j, v = ho // r, ho % r, wo // r, wo % r
    return i.expand(A * r, B * r, nc), j.expand(A * r, B * r, nc), (c * r * r + v * r + u).expand(A * r, B * r, nc)


def ps_fwd(x, r, nc):
    N, A, B, _ = x.shape
    i, j, ch = _ps_index(A, B, r, nc, x.device)
    return _f64(x)[:, i, j, ch]


def ps_bwd(dy, r, nc):
    N, Ar, Br, _ = dy.shape
    A, B = Ar // r, Br // r
    i, j, ch = _ps_index(A, B, r, nc, dy.device)
    dx = torch.zeros((N, A, B, nc * r * r), dtype=torch.float64, device=dy.device)
    dx[:, i, j, ch] = _f64(dy)         # a permutation: every element is written once
    return dx


# ---- tf.pad(..., 'SYMMETRIC') in H and W: the mirror includes the edge sample ----------------------------------------------------------
def _sym_index(n, p, device):
    a = torch.arange(n, device=device)
    return torch.cat([a[:p].flip(0), a, a.flip(0)[:p]])


def sympad_fwd(x, p):
    ih, iw = _sym_index(x.shape[1], p, x.device), _sym_index(x.shape[2], p, x.device)
    return _f64(x).index_select(1, ih).index_select(2, iw)


def sympad_bwd(dxp, p):
    """every padded position adds its gradient to the sample it mirrors"""
    N, Hp, Wp, C = dxp.shape
    H, W = Hp - 2 * p, Wp - 2 * p
    ih, iw = _sym_index(H, p, dxp.device), _sym_index(W, p, dxp.device)
    t = torch.zeros((N, H, Wp, C), dtype=torch.float64, device=dxp.device).index_add_(1, ih, _f64(dxp))
    return torch.zeros((N, H, W, C), dtype=torch.float64, device=dxp.device).index_add_(2, iw, t)


# ---- critic input: concat(tile(a), b, c, d, logits, float(argmax(logits))) -------------------------------------------------------------
def critic_input_fwd(a, tile_a, b, c, d, logits):
    a, b, c, d, logits = (_f64(t) for t in (a, b, c, d, logits))
    am = argmax_lowest(logits).double().unsqueeze(-1)
    return torch.cat([a] * tile_a + [b, c, d, logits, am], dim=-1)


def critic_input_bwd(dout, channels, tile_a):
    """channels = (Ca, Cb, Cc, Cd, ncls) -> (da, db, dc, dd, dlogits); the argmax channel carries no gradient"""
    dout = _f64(dout)
    Ca, Cb, Cc, Cd, ncls = channels
    da = sum(dout[..., t * Ca:(t + 1) * Ca] for t in range(tile_a))
    o = Ca * tile_a
    outs = [da]
    for n in (Cb, Cc, Cd, ncls):
        outs.append(dout[..., o:o + n])
        o += n
    return tuple(outs)


# ---- segmentation loss: class-weighted cross-entropy with the 0.005 clip + soft Dice ---------------------------------------------------
def seg_loss_sums(logits, y):
    """[4, ncls]: n_i = sum y_i, I_i = sum p_i y_i, S_i = sum p_i^2, X_i = sum -y_i log(clip(p_i, 0.005, 1)); also the softmax"""
    ncls = logits.shape[-1]
    z, y = _f64(logits).reshape(-1, ncls), _f64(y).reshape(-1, ncls)
    p = torch.softmax(z, dim=-1)
    sums = torch.stack([y.sum(0), (p * y).sum(0), (p * p).sum(0), -(y * torch.log(p.clamp(CLIP_P, 1.0))).sum(0)])
    return sums, p, y


def seg_loss(logits, y, miu_cross=1.0, miu_dice=1.0):
    """-> (total, xent, dice, sums[4, ncls])"""
    sums, p, y = seg_loss_sums(logits, y)
    n, I, S, X = sums
    P, ncls = p.shape
    w = 1.0 - n / n.sum()
    xent = (w * X).sum() / P
    dice = -(2.0 * I / (S + n + 1e-7)).sum() / ncls
    return miu_cross * xent + miu_dice * dice, xent, dice, sums


def seg_loss_bwd(logits, y, miu_cross=1.0, miu_dice=1.0, gscale=1.0, P_norm=None):
    """gradient of miu_cross * xent + miu_dice * dice with respect to the logits, times gscale.  The class weights depend on the labels
    only.  P_norm: the pixel count the cross-entropy's mean runs over (the Dice sums stay this tensor's own).
    -> (dlogits, p_true) with p_true = the softmax of each pixel's labelled class (where the clip makes the gradient jump)"""
    sums, p, y = seg_loss_sums(logits, y)
    n, I, S, X = sums
    P, ncls = p.shape
    Pn = float(P if P_norm is None else P_norm)
    w = 1.0 - n / n.sum()
    D = S + n + 1e-7
    gx = torch.where((p >= CLIP_P) & (p <= 1.0), -w * y / p / Pn, torch.zeros_like(p))      # clip_by_value passes the gradient inside
    gd = -(2.0 / ncls) * (y / D - 2.0 * I * p / (D * D))
    g = miu_cross * gx + miu_dice * gd
    dz = gscale * p * (g - (g * p).sum(-1, keepdim=True))
    return dz.reshape(logits.shape), (p * y).sum(-1).reshape(logits.shape[:-1])


# ---- prediction / monitoring -----------------------------------------------------------------------------------------------------------
def softmax_argmax(logits):
    """layers.pixel_wise_softmax_2: exp(z) / sum exp(z) without a max subtraction, clipped to +-1e15; tf.argmax: lowest index on ties"""
    e = torch.exp(_f64(logits))
    p = (e / e.sum(-1, keepdim=True)).clamp(-1e15, 1e15)
    return p, argmax_lowest(p)


def dice_eval(label, y):
    """lib._dice_eval: hard Dice per class against one-hot labels; a label outside [0, ncls) is in no class (tf.one_hot: a zero row)
    -> [1 + ncls] = (mean, per class)"""
    ncls = y.shape[-1]
    y = _f64(y).reshape(-1, ncls)
    pred = (label.reshape(-1, 1) == torch.arange(ncls, device=y.device)).double()
    d = 2.0 * (pred * y).sum(0) / (pred.sum(0) + y.sum(0) + 1e-7)
    return torch.cat([d.mean().reshape(1), d])


def confusion_matrix(y, pred):
    """(compact_y = lowest-index argmax of y, cm[truth, pred] as int64); a prediction outside [0, ncls) is counted nowhere"""
    ncls = y.shape[-1]
    cy = argmax_lowest(_f64(y))
    t, p = cy.reshape(-1), pred.reshape(-1)
    ok = (p >= 0) & (p < ncls)
    cm = torch.bincount(t[ok] * ncls + p[ok], minlength=ncls * ncls).reshape(ncls, ncls)
    return cy, cm


# ---- optimisers over a flat arena cut into chunks of 1024 elements ---------------------------------------------------------------------
def per_element(chunk_vec, n, default):
    """a per-chunk vector spread over the n elements (the last chunk may be ragged); None: `default` everywhere"""
    if chunk_vec is None:
        return torch.full((n,), float(default), dtype=torch.float64)
    return _f64(chunk_vec).repeat_interleave(OPT_CHUNK)[:n]


def _opt_common(w, g, chunk_l2, chunk_mask):
    w, g = _f64(w), _f64(g)
    n = w.numel()
    l2 = per_element(chunk_l2, n, 0.0).to(w.device)
    sel = per_element(chunk_mask, n, 1.0).to(w.device) != 0
    return w, g + l2 * w, sel


def adam(w, g, m, v, chunk_l2, chunk_mask, lr, beta1, beta2, eps, t):
    """tf.train.AdamOptimizer on g + l2 w; a masked-out chunk keeps weights and state -> (w, m, v)"""
    w, ge, sel = _opt_common(w, g, chunk_l2, chunk_mask)
    m, v = _f64(m), _f64(v)
    lr_t = lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)
    mn = m + (ge - m) * (1.0 - beta1)
    vn = v + (ge * ge - v) * (1.0 - beta2)
    wn = w - lr_t * mn / (torch.sqrt(vn) + eps)
    return torch.where(sel, wn, w), torch.where(sel, mn, m), torch.where(sel, vn, v)


def rmsprop(w, g, ms, chunk_l2, chunk_mask, lr, decay=0.9, eps=1e-10):
    """tf.train.RMSPropOptimizer(momentum=0) -> (w, ms)"""
    w, ge, sel = _opt_common(w, g, chunk_l2, chunk_mask)
    ms = _f64(ms)
    msn = ms + (ge * ge - ms) * (1.0 - decay)
    wn = w - lr * ge / torch.sqrt(msn + eps)
    return torch.where(sel, wn, w), torch.where(sel, msn, ms)


def momentum(w, g, acc, chunk_l2, chunk_mask, lr, mom):
    """tf.train.MomentumOptimizer -> (w, acc)"""
    w, ge, sel = _opt_common(w, g, chunk_l2, chunk_mask)
    acc = _f64(acc)
    an = acc * mom + ge
    return torch.where(sel, w - lr * an, w), torch.where(sel, an, acc)


def clip(w, chunk_mask, lo, hi):
    """clip_by_value on the selected chunks, in the tensor's own type (pure selection: exact)"""
    sel = per_element(chunk_mask, w.numel(), 1.0).to(w.device) != 0
    return torch.where(sel, w.clamp(lo, hi), w)


def l2_loss(w, chunk_l2):
    """sum over chunks of l2_c * sum(w^2) / 2; None: coefficient 1 (tf.nn.l2_loss)"""
    w = _f64(w)
    return (per_element(chunk_l2, w.numel(), 1.0).to(w.device) * w * w).sum() / 2.0


def wgan_loss(operands, coefs):
    """sum_i coef_i * mean(operand_i) over the operands that are not None"""
    return sum(float(c) * _f64(t).mean() for t, c in zip(operands, coefs) if t is not None)
