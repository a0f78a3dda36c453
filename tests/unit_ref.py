"""Float64 restatement of what layers.py / ops.PS_conv2d build, and the case lists of tests/test_gpu_units.py and tests/test_units_host.py.

The restatement is written from oracle/tf_ops.py alone (conv2d, pad_symmetric, dropout, batch_norm, leaky_relu, pad_channels, max_pool2,
PS, softmax_weighted_loss, dice_loss) and runs under torch autograd in float64: it is the reference the autograd Functions of
functional.py and the blocks of layers.py are held to.  Dropout uses the product's documented (seed, stream id) counter hash
(tf_ops.dropout_mask), so both sides drop the same elements by construction; the functions take the stream id as an argument, and
`RefLayers` hands the ids out in call order exactly as a VariableStore does (one per convolution call site, also at keep_prob 1).

A case is plain data.  Its `seed` is part of it: it is chosen so that the float64 forward keeps every tensor that enters an activation
clear of zero and every 2x2 pool window clear of a tie (`clearance`), which is what lets the float32 product be compared at the
per-kernel bar without excluding a pixel.  tests/test_units_host.py asserts that on the CPU, tests/test_gpu_units.py on the reference it
computes.

A `program` is the graph of a case written once against the names of layers.py; it runs on `RefLayers` (float64, this file) and on the
product's layers module (tests/test_gpu_units.py::ProductLayers).  The two share the sequence of calls and nothing else.
"""
import zlib

import numpy as np
import torch

from oracle import tf_ops as T

LEAK = T.LEAK
MARGIN = 1e-4          # min|v| >= MARGIN * max|v| for every pre-activation; top-2 gap of every pool window >= MARGIN * max|v|


# ---- operand rounding (bf16 budget) ----------------------------------------------------------------------------------------------------
def round_bf16(t):
    """tf_ops.round_bf16 on a float64 tensor (through float32, as the product's operands are float32 before they are rounded);
    differentiable: the casts hand the gradient through"""
    return T.round_bf16(t.float()).to(t.dtype)


def _r(t, rnd):
    return t if rnd is None else rnd(t)


# ---- layers.py, restated ----------------------------------------------------------------------------------------------------------------
def _conv(x, W, stride, dil, padding, rnd=None):
    return T.conv2d(_r(x, rnd), _r(W, rnd), stride, dil, padding)


def conv2d(x, W, keep_prob, seed, sid, stride=1, padding="SAME", rnd=None):
    """layers.conv2d: conv -> dropout"""
    return T.dropout(_conv(x, W, stride, 1, padding, rnd), keep_prob, seed, sid)


def dilate_conv2d(x, W, keep_prob, seed, sid, rate=2, padding="SAME", rnd=None):
    """layers.dilate_conv2d: atrous conv -> dropout"""
    return T.dropout(_conv(x, W, 1, rate, padding, rnd), keep_prob, seed, sid)


def batch_norm(x, bn, is_training):
    """layers.batch_norm.  bn: dict gamma, beta, moving_mean, moving_variance; the moving statistics are updated in place"""
    return T.batch_norm(x, bn["gamma"], bn["beta"], bn["moving_mean"], bn["moving_variance"], bool(is_training))


def conv_bn(x, W, bn, keep_prob, seed, sid, stride=1, dil=1, padding="SAME", is_train=True, alpha=-1.0, shortcut=None, rec=None, rnd=None):
    """act( BN( dropout( conv(x, W) ) ) + pad_channels(shortcut) ); alpha < 0: no activation.  rec: list that receives ("act", v) for
    every tensor entering an activation"""
    y = T.dropout(_conv(x, W, stride, dil, padding, rnd), keep_prob, seed, sid)
    y = batch_norm(y, bn, is_train)
    if shortcut is not None:
        cin, cout = shortcut.shape[-1], y.shape[-1]
        y = (T.pad_channels(shortcut, cin // 2) if cout != cin else shortcut) + y
    if alpha < 0:
        return y
    if rec is not None:
        rec.append(("act", y.detach()))
    return T.leaky_relu(y, alpha)


def conv_bn_2d(x, W, bn, keep_prob, seed, sid, padding="SAME", stride=1, is_train=True, **kw):
    return conv_bn(x, W, bn, keep_prob, seed, sid, stride, 1, padding, is_train, -1.0, **kw)


def conv_bn_relu2d(x, W, bn, keep_prob, seed, sid, padding="SAME", stride=1, is_train=True, leak=False, **kw):
    return conv_bn(x, W, bn, keep_prob, seed, sid, stride, 1, padding, is_train, LEAK if leak is True else 0.0, **kw)


def dilate_conv_bn(x, W, bn, keep_prob, seed, sid, padding="SAME", rate=2, is_train=True, **kw):
    return conv_bn(x, W, bn, keep_prob, seed, sid, 1, rate, padding, is_train, -1.0, **kw)


def dilate_conv_bn_relu2d(x, W, bn, keep_prob, seed, sid, padding="SAME", rate=2, is_train=True, leak=False, **kw):
    return conv_bn(x, W, bn, keep_prob, seed, sid, 1, rate, padding, is_train, LEAK if leak is True else 0.0, **kw)


def max_pool2d(x, rec=None):
    if rec is not None:
        rec.append(("pool", x.detach()))
    return T.max_pool2(x)


def residual_block(x, w1, w2, bn1, bn2, keep_prob, seed, sids, inc_dim=False, is_train=True, leak=False, padding="SAME", rate=1, **kw):
    """layers.residual_block (rate 1) / layers.DR_block: conv-BN-act -> conv-BN -> + x (zero-padded C/2 each side when inc_dim) -> act"""
    alpha = LEAK if leak is True else 0.0
    inner = conv_bn(x, w1, bn1, keep_prob, seed, sids[0], 1, rate, padding, is_train, alpha, **kw)
    assert w2.shape[-1] == (x.shape[-1] + 2 * (x.shape[-1] // 2) if inc_dim else x.shape[-1])
    return conv_bn(inner, w2, bn2, keep_prob, seed, sids[1], 1, rate, padding, is_train, alpha, shortcut=x, **kw)


def DR_block(x, w1, w2, bn1, bn2, rate, keep_prob, seed, sids, inc_dim=False, is_train=True, leak=False, **kw):
    return residual_block(x, w1, w2, bn1, bn2, keep_prob, seed, sids, inc_dim, is_train, leak, "SAME", rate, **kw)


def PS_conv2d(X, W, r, n_channel, keep_prob, seed, sid, rnd=None):
    """ops.PS_conv2d: conv2d(PS(X, r, n_channel), W, keep_prob, padding='SYMMETRIC')"""
    return conv2d(T.PS(X, r, n_channel), W, keep_prob, seed, sid, 1, "SYMMETRIC", rnd)


def seg_loss(logits, y, miu_cross, miu_dice):
    """(total, cross-entropy, Dice) of functional.SegLossFn"""
    wl, dl = T.softmax_weighted_loss(logits, y), T.dice_loss(logits, y)
    return miu_cross * wl + miu_dice * dl, wl, dl


def wgan_loss(ts, coefs):
    """functional.WganLossFn: sum_i coef_i * mean(t_i) over the inputs that are not None"""
    return sum(c * t.mean() for t, c in zip(ts, coefs) if t is not None)


# ---- the clear-of-zero condition ----------------------------------------------------------------------------------------------------------
def clearance(rec):
    """smallest margin over the records of one float64 forward: min|v| / max|v| of a pre-activation, (top1 - top2) / max|v| of a 2x2 pool
    window.  The case is usable when this is >= MARGIN (inf: the graph has no activation and no pool)"""
    worst = float("inf")
    for kind, v in rec:
        top = float(v.abs().max())
        if kind == "act":
            worst = min(worst, float(v.abs().min()) / top)
        else:
            N, H, W, C = v.shape
            win = v.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
            t2 = torch.topk(win, 2, dim=1).values
            worst = min(worst, float((t2[:, 0] - t2[:, 1]).min()) / top)
    return worst


# ---- values ----------------------------------------------------------------------------------------------------------------------------------
def init_value(seed, name, shape):
    """float32 initial value of a variable or an input: a function of (case seed, name) only, so that neither side depends on the order
    in which the other creates its variables"""
    rng = np.random.default_rng([int(seed), zlib.crc32(name.encode())])
    leaf = name.rsplit("/", 1)[-1]
    if leaf == "gamma":
        a = rng.uniform(0.5, 1.5, shape)
    elif leaf == "beta":
        a = rng.standard_normal(shape) * 0.5
    elif leaf == "moving_mean":
        a = rng.standard_normal(shape) * 0.3
    elif leaf == "moving_variance":
        a = rng.uniform(0.5, 1.5, shape)
    elif len(shape) == 4 and name.startswith("w"):           # a filter [R, S, C, K]: He-scaled
        a = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))
    else:
        a = rng.standard_normal(shape)
    return a.astype(np.float32)


def onehot_labels(seed, shape, ncls):
    """[N, H, W, ncls] float32 one-hot labels in vertical bands with a ragged edge (every class present)"""
    rng = np.random.default_rng([int(seed), 77])
    N, H, W = shape
    lab = (np.arange(W)[None, None, :] * ncls // W + rng.integers(0, 2, (N, H, 1))) % ncls
    return np.eye(ncls, dtype=np.float32)[np.broadcast_to(lab, (N, H, W))]


def clip_margin(logits, y):
    """distance of the label class's probability from the 0.005 clip of the weighted cross-entropy, smallest over the pixels: the one
    place where the segmentation loss has a kink"""
    return float(((torch.softmax(logits.detach(), -1) * y).sum(-1) - 0.005).abs().min())


# ---- the reference side of a program ----------------------------------------------------------------------------------------------------
class RefLayers(object):
    """layers.py's names over the restatement above.  Variables are float64 leaves made from init_value; stream ids and nothing else are
    handed out in call order.  `calls` records every convolution call site (what the host test asks the planner about), `rec` the
    tensors of the clear-of-zero condition."""

    def __init__(self, seed, drop_seed, rnd=None):
        self.seed, self.drop_seed, self.rnd = seed, drop_seed, rnd
        self.V, self.trainable = {}, {}
        self.rec, self.calls = [], []
        self._sid = 0

    def var(self, name, shape, trainable=True):
        if name not in self.V:
            t = torch.from_numpy(init_value(self.seed, name, tuple(shape))).double()
            self.V[name] = t.requires_grad_(True) if trainable else t
            self.trainable[name] = trainable
        return self.V[name]

    def _bn(self, scope, C, trainable):
        return {leaf: self.var("%s/%s" % (scope, leaf), (C,), trainable and leaf in ("gamma", "beta"))
                for leaf in ("beta", "gamma", "moving_mean", "moving_variance")}

    def _next(self):
        self._sid += 1
        return self._sid - 1

    def _call(self, x, W, stride, dil, padding, **kw):
        self.calls.append(dict(x=tuple(x.shape), w=tuple(W.shape), stride=stride, dil=dil, padding=padding, **kw))

    def conv2d(self, x, W, keep_prob_, strides=(1, 1, 1, 1), padding="SAME"):
        self._call(x, W, strides[1], 1, padding, bn=False)
        return conv2d(x, W, keep_prob_, self.drop_seed, self._next(), strides[1], padding, self.rnd)

    def dilate_conv2d(self, x, W, keep_prob_, rate=2, padding="SAME"):
        self._call(x, W, 1, rate, padding, bn=False)
        return dilate_conv2d(x, W, keep_prob_, self.drop_seed, self._next(), rate, padding, self.rnd)

    def _conv_bn(self, x, W, keep_prob, padding, stride, dil, is_train, scope, bn_trainable, alpha, shortcut=None, link=None):
        self._call(x, W, stride, dil, padding, bn=True, is_train=bool(is_train), bn_trainable=bool(bn_trainable), alpha=alpha,
                   sc=None if shortcut is None else shortcut.shape[-1], link=link, keep=keep_prob)
        return conv_bn(x, W, self._bn(scope, W.shape[-1], bn_trainable), keep_prob, self.drop_seed, self._next(), stride, dil, padding,
                       is_train, alpha, shortcut, self.rec, self.rnd)

    def conv_bn_2d(self, x, W, keep_prob, padding="SAME", strides=(1, 1, 1, 1), is_train=True, scope=None, bn_trainable=True):
        return self._conv_bn(x, W, keep_prob, padding, strides[1], 1, is_train, scope, bn_trainable, -1.0)

    def conv_bn_relu2d(self, x, W, keep_prob, padding="SAME", strides=(1, 1, 1, 1), is_train=True, scope=None, bn_trainable=True, leak=False):
        return self._conv_bn(x, W, keep_prob, padding, strides[1], 1, is_train, scope, bn_trainable, LEAK if leak is True else 0.0)

    def dilate_conv_bn(self, x, W, keep_prob, padding="SAME", rate=2, is_train=True, scope=None, bn_trainable=True):
        return self._conv_bn(x, W, keep_prob, padding, 1, rate, is_train, scope, bn_trainable, -1.0)

    def dilate_conv_bn_relu2d(self, x, W, keep_prob, padding="SAME", rate=2, is_train=True, scope=None, bn_trainable=True, leak=False):
        return self._conv_bn(x, W, keep_prob, padding, 1, rate, is_train, scope, bn_trainable, LEAK if leak is True else 0.0)

    def batch_norm(self, x, is_training=True, scope=None, trainable=True):
        return batch_norm(x, self._bn(scope, x.shape[-1], trainable), is_training)

    def max_pool2d(self, x, n):
        assert n == 2
        return max_pool2d(x, self.rec)

    def residual_block(self, x, w1, w2, keep_prob, inc_dim=False, is_train=True, scope=None, bn_trainable=True, leak=False, padding="SAME"):
        alpha = LEAK if leak is True else 0.0
        role = ("head", "tail") if padding == "SAME" else (None, None)
        inner = self._conv_bn(x, w1, keep_prob, padding, 1, 1, is_train, scope + "_1", bn_trainable, alpha, link=role[0])
        return self._conv_bn(inner, w2, keep_prob, padding, 1, 1, is_train, scope + "_2", bn_trainable, alpha, shortcut=x, link=role[1])

    def DR_block(self, x, w1, w2, rate, keep_prob, inc_dim=False, is_train=True, bn_trainable=True, scope=None, leak=False):
        alpha = LEAK if leak is True else 0.0
        inner = self._conv_bn(x, w1, keep_prob, "SAME", 1, rate, is_train, scope + "_1", bn_trainable, alpha, link="head")
        return self._conv_bn(inner, w2, keep_prob, "SAME", 1, rate, is_train, scope + "_2", bn_trainable, alpha, shortcut=x, link="tail")

    def PS_conv2d(self, X, W, r, n_channel, keep_prob_):
        self._call(T.PS(X, r, n_channel), W, 1, 1, "SYMMETRIC", bn=False)
        return PS_conv2d(X, W, r, n_channel, keep_prob_, self.drop_seed, self._next(), self.rnd)

    def fan_out(self, x):
        return x, x


# ---- programs: one graph, written against the names of layers.py ---------------------------------------------------------------------------
def prog_unit(L, X, c):
    """one conv-BN unit through layers._conv_bn"""
    N, H, W, C, K = c["shape"]
    k = c["k"]
    w = L.var("w", (k, k, C, K), c.get("w_trainable", True))
    return [L._conv_bn(X["x"], w, c["keep"], c["padding"], c["stride"], c["dil"], c["is_train"], "u", c["bn_trainable"], c["alpha"],
                       shortcut=X.get("sc"))]


def prog_res(L, X, c):
    C, K = c["shape"][3], c["shape"][4]
    w1, w2 = L.var("w1", (3, 3, C, K)), L.var("w2", (3, 3, K, K))
    return [L.residual_block(X["x"], w1, w2, c["keep"], inc_dim=c["inc_dim"], is_train=c["is_train"], scope="b", bn_trainable=True,
                             leak=c["leak"], padding=c["padding"])]


def prog_dr(L, X, c):
    C, K = c["shape"][3], c["shape"][4]
    w1, w2 = L.var("w1", (3, 3, C, K)), L.var("w2", (3, 3, K, K))
    return [L.DR_block(X["x"], w1, w2, 2, c["keep"], inc_dim=c["inc_dim"], is_train=c["is_train"], scope="d", leak=c["leak"])]


def prog_chain(L, X, c):
    """residual block (inc_dim) -> max-pool -> DR block -> conv2d tail with dropout"""
    C, K = c["shape"][3], c["shape"][4]
    h = L.residual_block(X["x"], L.var("w1", (3, 3, C, K)), L.var("w2", (3, 3, K, K)), c["keep"], inc_dim=True, is_train=True, scope="b",
                         leak=True)
    h = L.max_pool2d(h, 2)
    h = L.DR_block(h, L.var("w3", (3, 3, K, K)), L.var("w4", (3, 3, K, K)), 2, c["keep"], is_train=True, scope="d", leak=True)
    return [L.conv2d(h, L.var("w5", (3, 3, K, 6)), 0.75)]


def prog_plain(L, X, c):
    """the layers without an activation of their own, and layers.batch_norm"""
    C, K = c["shape"][3], c["shape"][4]
    h = L.dilate_conv2d(X["x"], L.var("w1", (3, 3, C, K)), c["keep"], rate=2)
    h = L.batch_norm(h, is_training=True, scope="n0")
    h = L.conv_bn_2d(h, L.var("w2", (3, 3, K, K)), c["keep"], padding="SYMMETRIC", is_train=True, scope="n1")
    h = L.dilate_conv_bn(h, L.var("w3", (3, 3, K, K)), 1.0, rate=2, is_train=False, scope="n2", bn_trainable=False)
    h = L.conv_bn_relu2d(h, L.var("w4", (3, 3, K, K)), 1.0, strides=[1, 2, 2, 1], is_train=True, scope="n3", leak=False)
    return [L.dilate_conv_bn_relu2d(h, L.var("w5", (3, 3, K, K)), 1.0, rate=2, is_train=True, scope="n4", leak=True)]


def prog_fan(L, X, c):
    """one tensor through fan_out into a residual block and into a dilated unit"""
    C, K = c["shape"][3], c["shape"][4]
    h = L.conv_bn_relu2d(X["x"], L.var("w0", (3, 3, C, K)), 1.0, is_train=True, scope="f0", leak=True)
    a, b = L.fan_out(h)
    ya = L.residual_block(a, L.var("w1", (3, 3, K, K)), L.var("w2", (3, 3, K, K)), c["keep"], is_train=True, scope="fa", leak=True)
    yb = L.dilate_conv_bn_relu2d(b, L.var("w3", (3, 3, K, K)), 1.0, rate=2, is_train=True, scope="fb", leak=True)
    return [ya, yb]


def prog_shared(L, X, c):
    """ONE filter variable consumed by two call sites of one step (the critics' shared filters)"""
    C = c["shape"][3]
    w = L.var("wsh", (3, 3, C, C))
    h = L.conv_bn_relu2d(X["x"], w, c["keep"], is_train=True, scope="s0", leak=True)
    return [L.conv_bn_relu2d(h, w, c["keep"], is_train=True, scope="s1", leak=True)]


def prog_head(L, X, c):
    """a unit, then the segmenter head: PS + mirror pad + 5x5 logits convolution"""
    C, K = c["shape"][3], c["shape"][4]
    h = L.conv_bn_relu2d(X["x"], L.var("w0", (3, 3, C, K)), c["keep"], is_train=True, scope="h0", leak=True)
    return [L.PS_conv2d(h, L.var("w1", (5, 5, K // 4, c["ncls"])), 2, K // 4, 1.0)]


PROGRAMS = {"unit": prog_unit, "res": prog_res, "dr": prog_dr, "chain": prog_chain, "plain": prog_plain, "fan": prog_fan,
            "shared": prog_shared, "head": prog_head}


def out_hw(c):
    N, H, W, C, K = c["shape"]
    if c["padding"] == "SYMMETRIC":
        return H, W
    return T.same_pad(H, c["k"], c["stride"], c["dil"])[0], T.same_pad(W, c["k"], c["stride"], c["dil"])[0]


def input_shapes(c):
    N, H, W, C, K = c["shape"]
    out = {"x": (N, H, W, C)}
    if c.get("sc", "none") != "none":
        oh, ow = out_hw(c)
        out["sc"] = (N, oh, ow, K if c["sc"] == "same" else K // 2)
    return out


def ref_inputs(c):
    return {k: torch.from_numpy(init_value(c["seed"], "in_" + k, s)).double().requires_grad_(True) for k, s in input_shapes(c).items()}


def run_ref(c, rnd=None):
    """float64 forward of a case (rnd: applied to both operands of every convolution) and the upstream gradients
    init_value(seed, 'dout<i>') a test hands to backward.  -> dict(L, X, outs, douts)"""
    L = RefLayers(c["seed"], c["drop_seed"], rnd)
    X = ref_inputs(c)
    outs = PROGRAMS[c["prog"]](L, X, c)
    douts = [torch.from_numpy(init_value(c["seed"], "dout%d" % i, tuple(o.shape))).double() for i, o in enumerate(outs)]
    return dict(L=L, X=X, outs=outs, douts=douts)


# ---- case lists -------------------------------------------------------------------------------------------------------------------------
def _u(id, shape, seed, is_train=True, bn_trainable=True, alpha=LEAK, keep=1.0, sc="none", padding="SAME", k=3, stride=1, dil=1, **kw):
    return dict(id=id, prog="unit", shape=shape, seed=seed, drop_seed=1000 + seed, is_train=is_train, bn_trainable=bn_trainable, alpha=alpha,
                keep=keep, sc=sc, padding=padding, k=k, stride=stride, dil=dil, **kw)


A, B_ = (2, 8, 8, 8, 16), (2, 7, 9, 5, 7)
# every value of every factor; every pair among is_train, shortcut kind and keep_prob (the first twelve)
UNIT_CASES = [
    _u("train-none-1.0", A, 9),
    _u("train-none-.75-relu", B_, 0, alpha=0.0, keep=0.75),
    _u("train-same-1.0", A, 3, sc="same"),
    _u("train-same-.75-noact", B_, 0, alpha=-1.0, keep=0.75, sc="same"),
    _u("train-half-1.0-relu-dil2", A, 0, alpha=0.0, sc="half", dil=2),
    _u("train-half-.75", A, 0, keep=0.75, sc="half"),
    _u("infer-none-1.0-fused", A, 2, is_train=False, bn_trainable=False),
    _u("infer-none-.75-unfused", B_, 2, is_train=False, keep=0.75),
    _u("infer-same-1.0-fused-relu", B_, 3, is_train=False, bn_trainable=False, alpha=0.0, sc="same"),
    _u("infer-same-.75-unfused", A, 3, is_train=False, keep=0.75, sc="same"),
    _u("infer-half-1.0-unfused-noact-s2", A, 0, is_train=False, alpha=-1.0, sc="half", stride=2),
    _u("infer-half-.75-fused", A, 2, is_train=False, bn_trainable=False, keep=0.75, sc="half"),
    _u("train-sym5", A, 2, padding="SYMMETRIC", k=5),
    _u("infer-sym5-.75-fused-relu", B_, 0, is_train=False, bn_trainable=False, alpha=0.0, keep=0.75, padding="SYMMETRIC", k=5),
    _u("train-s2-.75", B_, 0, keep=0.75, stride=2),
    _u("train-frozen-bn-same", A, 3, bn_trainable=False, sc="same"),
    _u("train-stats-parts", (2, 16, 16, 32, 64), 0, alpha=-1.0, keep=0.75, parts=True),
    _u("train-no-stats-parts", (2, 8, 8, 64, 64), 0, alpha=-1.0, sc="same", parts=False),
]

# (b) which gradients are asked for, on one unit with a shortcut
GRAD_SUBSETS = {"all": ("x", "w", "gamma", "beta", "sc"), "x-only": ("x",), "params-only": ("w", "gamma", "beta"),
                "no-shortcut": ("x", "w", "gamma", "beta")}
SUBSET_CASES = [_u("subset-train-half-.75", A, 0, keep=0.75, sc="half"), _u("subset-infer-same", A, 2, is_train=False, sc="same")]


def _b(id, prog, shape, seed, keep=1.0, **kw):
    d = dict(id=id, prog=prog, shape=shape, seed=seed, drop_seed=2000 + seed, keep=keep, padding="SAME", k=3, stride=1, dil=1,
             is_train=True, leak=True, inc_dim=False)
    d.update(kw)
    return d


BLOCK_CASES = [
    _b("res", "res", (2, 8, 8, 8, 8), 3, keep=0.75),
    _b("res-inc", "res", A, 1, keep=0.75, inc_dim=True),
    _b("res-infer-relu", "res", (2, 7, 9, 6, 6), 1, is_train=False, leak=False),
    _b("res-sym", "res", (2, 8, 8, 8, 8), 2, padding="SYMMETRIC"),
    _b("dr", "dr", (2, 8, 8, 8, 8), 1, keep=0.75),
    _b("dr-inc", "dr", A, 5, inc_dim=True),
    _b("chain", "chain", A, 11),
    _b("plain", "plain", A, 0, keep=0.75),
]
FAN_CASE = _b("fan", "fan", (2, 8, 8, 8, 8), 0, keep=0.75)
SHARED_CASE = _b("shared", "shared", (2, 8, 8, 8, 8), 0, keep=0.75)
HEAD_CASE = _b("head", "head", (2, 8, 8, 8, 16), 6, keep=0.75, ncls=3)
DEST_CASE = BLOCK_CASES[1]            # (e): the same block with leaf tensors, with sinks, with sinks on the side stream

# (h) bf16 mode.  The resident kernels serve no geometry below 4096 output pixels (conv_bf16r.hip::served), so the small cases above run
# whatever the typed dispatch gives them; these are the smallest the resident family serves: wholly; forward and filter gradient only
# (5x5: the data gradient stays on the staged kernels, so the BN backward writes float32 AND bf16 — want_h without only_h); and one
# two-unit block.  At 4096 x 64 elements no seed keeps an activation clear of zero and bf16 rounding moves signs anyway: `clear` False,
# the budget E carries the reference's own flips
BF16_RESIDENT_CASES = [
    _u("bf16r-served", (4, 32, 32, 64, 64), 0, alpha=-1.0, keep=0.75, sc="same", served=(True, True, True)),
    _u("bf16r-partly-5x5", (4, 32, 32, 64, 64), 0, alpha=-1.0, keep=0.75, k=5, served=(True, False, True)),
]
BF16_BLOCK_CASE = _b("bf16r-res", "res", (4, 32, 32, 64, 64), 0, keep=0.75, served=(True, True, True), clear=False)
BF16_BLOCK_IDS = ("res", "res-inc", "dr")

ALL_CASES = UNIT_CASES + SUBSET_CASES + BLOCK_CASES + [FAN_CASE, SHARED_CASE, HEAD_CASE] + BF16_RESIDENT_CASES + [BF16_BLOCK_CASE]
