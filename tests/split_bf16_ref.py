"""Host restatement of the split-bf16 arithmetic of csrc/conv_x3_direct.hip, conv_x3_wgrad.hip and conv_x3_narrow.hip, the operands of
the per-element tests (tests/test_gpu_split_bf16_exact.py) and the assertion both sides make.  numpy + torch on the CPU only.

The kernels split each fp32 operand into three bf16 planes (split3) and keep six of the nine plane products, smallest first (kTermX /
kTermW), one MFMA and therefore one fp32 addition per product.  A test whose outputs are ONE product each (one operand nonzero on a lattice
of pixels, or one impulse per channel) sees that arithmetic per element: the six-term product of two fp32 values is within 1.87 * 2^-24 of
the exact product (relative; 1.71 over 2^20 random pairs, 1.87 over every case below), any five-term product misses by more than 2^-21 on
75 .. 100 % of the pairs.  BOUND = 4 * 2^-24 is what the GPU tests assert: the factor over the emulation's 1.87 covers accumulate
rounding inside the matrix pipe that the emulation does not model (measured on MI355X: up to 2.69 * 2^-24), and stays 2x
under the 2^-21 at which a dropped term shows.
tests/test_split_bf16_host.py holds the emulation to these figures on the very arrays of every GPU case."""
import math

import numpy as np
import torch

from oracle import tf_ops as T

BOUND = 4.0 * 2.0 ** -24          # per element, relative to the float64 product: what the GPU tests assert
VISIBLE = 2.0 ** -21              # a dropped plane product moves at least a quarter of a case's outputs further than this
TERMS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # (kTermX[i], kTermW[i]): plane of the activation, plane of the filter / dy
TERMS_OF_PLANE0 = {"w": (0, 3, 5), "x": (2, 4, 5)}            # the terms that plane 0 (the only nonzero plane of a power of two) of a side is in


def bf16(v):
    """fp32 -> nearest bfloat16, ties to even (v_cvt_pk_bf16_f32), as fp32"""
    return torch.from_numpy(np.array(v, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def split3(v):
    """split3 of the kernels: h = bf16(v), m = bf16(v - h), l = bf16(v - h - m); both differences are exact in fp32"""
    v = np.asarray(v, np.float32)
    h = bf16(v)
    r1 = v - h
    m = bf16(r1)
    return h, m, bf16(r1 - m)


def product6(a, b, drop=None):
    """the kept plane products of a (activation side, kTermX) and b (filter / dy side, kTermW) in the kernels' order, each exact in fp32
    (8 x 8 significand bits), one fp32 addition per product; drop = index of a term to leave out.  a, b: fp32 arrays, or their split3()"""
    pa, pb = (a if isinstance(a, tuple) else split3(a)), (b if isinstance(b, tuple) else split3(b))
    acc = np.zeros(np.broadcast(pa[0], pb[0]).shape, np.float32)
    for i, (ia, ib) in enumerate(TERMS):
        if i != drop:
            acc = acc + pa[ia] * pb[ib]
    return acc


def rel_err(got, ref):
    """|got - ref| / |ref| per element in float64 (ref != 0)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.abs(ref)


def check_per_element(got, ref, bound=BOUND):
    """THE assertion of the per-element tests: where the float64 reference is 0 the result is 0 by value, elsewhere |got - ref| <= bound *
    |ref|.  -> (largest relative error in units of 2^-24, number of nonzero outputs); raises AssertionError"""
    got = np.asarray(got, np.float64).ravel()
    ref = np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nz = ref != 0
    bad0 = np.flatnonzero(~nz & (got != 0))
    assert bad0.size == 0, "%d outputs whose reference is 0 are not 0 (first: flat index %s)" % (bad0.size, bad0[:1].tolist())
    assert nz.any(), "no nonzero output"
    e = rel_err(got[nz], ref[nz])
    worst = int(np.argmax(e))
    assert e[worst] <= bound, "%d of %d nonzero outputs outside %.2f * 2^-24 (worst %.2f * 2^-24: got %r, reference %r)" % (
        int((e > bound).sum()), e.size, bound * 2 ** 24, e[worst] * 2 ** 24, got[nz][worst], ref[nz][worst])
    return float(e[worst] * 2 ** 24), int(nz.sum())


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def values(rng, shape):
    """full-mantissa fp32 values, random sign, magnitudes 1e-3 .. 1e3 (log-uniform): nothing near the denormals, also not the third plane
    of the smallest value times the third plane of another"""
    return (rng.choice((-1.0, 1.0), shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)).astype(np.float32)


def pow2(rng, shape):
    """signed powers of two, exponents -4 .. 4: one nonzero bf16 plane"""
    return (rng.choice((-1.0, 1.0), shape) * 2.0 ** rng.integers(-4, 5, shape)).astype(np.float32)


def lattice(rng, shape, pitch):
    """[N, H, W, C] zero but for the pixels (i, j) = offset mod pitch; there ONE channel holds a value, the channel cycling over all of them
    with the lattice pixel's index.  Image n has the offset (pitch - 1 - n) mod pitch: the first image's lattice starts as far from the
    top left corner as it can (under zero padding the windows there hold no lattice point), later images walk through the other offsets,
    and no two consecutive images have their values at the same place of a tile."""
    N, H, W, C = shape
    ph, pw = pitch
    a = np.zeros(shape, np.float32)
    count = 0
    for n in range(N):
        i, j = (g.ravel() for g in np.meshgrid(np.arange((ph - 1 - n) % ph, H, ph), np.arange((pw - 1 - n) % pw, W, pw), indexing="ij"))
        a[n, i, j, (count + np.arange(i.size)) % C] = values(rng, i.size)
        count += i.size
    return a


def impulses(rng, shape):
    """[N, H, W, C] zero but for one value per channel, each at a pixel of its own: channel 0 at the first pixel of the batch, channel 1 at
    the last, the others anywhere"""
    N, H, W, C = shape
    a = np.zeros(shape, np.float32)
    px = np.concatenate(([0, N * H * W - 1], 1 + rng.choice(N * H * W - 2, C - 2, replace=False)))
    a.reshape(N * H * W, C)[px, np.arange(C)] = values(rng, C)
    return a


def _geom(H, W, R, S, s, padding):
    if padding == "SAME":
        (OH, pt, _), (OW, pl, _) = T.same_pad(H, R, s), T.same_pad(W, S, s)
    else:
        OH, pt, OW, pl = (H - R) // s + 1, 0, (W - S) // s + 1, 0
    return OH, OW, pt, pl


class Case:
    """one launch of the per-element tests.  family: "x3d" (stride 1), "x3s" (strided), "x3n" (logits), "x3w" (filter gradient); kind 0
    forward / 1 data gradient / 2 filter gradient; layer = (N, H, W, C, K, R, S, stride, padding); sparse: which operand carries the
    lattice / the impulses; dense: "values" or "pow2".  operands() -> (x, w, dy) with None for the one the kind does not read."""

    def __init__(self, family, kind, layer, sparse, dense="values", seed=0):
        self.family, self.kind, self.layer, self.sparse, self.dense, self.seed = family, kind, tuple(layer), sparse, dense, seed
        N, H, W, C, K, R, S, s, padding = self.layer
        self.OH, self.OW, self.pt, self.pl = _geom(H, W, R, S, s, padding)
        self.id = "%s-%s-%s-%s%s-%d" % (family, ("fwd", "dgrad", "wgrad")[kind], "x".join(str(v) for v in self.layer), sparse,
                                        "-pow2" if dense == "pow2" else "", seed)

    def operands(self):
        """the same arrays on every call (seeded by the case), read-only; nothing is kept"""
        N, H, W, C, K, R, S, s, padding = self.layer
        rng = np.random.default_rng([self.kind, self.seed, len(self.dense)] + [v for v in self.layer[:8]])
        fill = values if self.dense == "values" else pow2
        x = w = dy = None
        if self.kind == 0:
            x, w = lattice(rng, (N, H, W, C), (R, S)), fill(rng, (R, S, C, K))
        elif self.kind == 1:          # every dx pixel reads ceil(R / s) x ceil(S / s) pixels of dy
            dy, w = lattice(rng, (N, self.OH, self.OW, K), (-(-R // s), -(-S // s))), fill(rng, (R, S, C, K))
        elif self.sparse == "x":
            x, dy = impulses(rng, (N, H, W, C)), fill(rng, (N, self.OH, self.OW, K))
        else:
            x, dy = fill(rng, (N, H, W, C)), impulses(rng, (N, self.OH, self.OW, K))
        for a in (x, w, dy):
            if a is not None:
                a.setflags(write=False)
        return x, w, dy

    def pow2_side(self):
        """which side of a product (TERMS_OF_PLANE0) the dense operand is"""
        return "x" if self.kind == 2 and self.sparse == "dy" else "w"

    def pairs(self, ops):
        """ops = operands() -> (a, b): the two factors of every output that is one product, a on the activation side of TERMS (x, or dy for a data
        gradient), b on the other (w, or dy for the filter gradient); found from the indices, no convolution"""
        N, H, W, C, K, R, S, s, padding = self.layer
        x, w, dy = ops
        av, bv = [], []
        if self.kind == 2:
            sp = x if self.sparse == "x" else dy
            n, i, j, c = np.nonzero(sp)
            for r in range(R):
                for t in range(S):
                    # dw[r, t, c, k] += x[n, oh + r - pt, ow + t - pl, c] dy[n, oh, ow, k]
                    oi, oj = (i - r + self.pt, j - t + self.pl) if self.sparse == "x" else (i + r - self.pt, j + t - self.pl)
                    lim = (self.OH, self.OW) if self.sparse == "x" else (H, W)
                    ok = (oi >= 0) & (oi < lim[0]) & (oj >= 0) & (oj < lim[1])
                    if self.sparse == "x":
                        b = dy[n[ok], oi[ok], oj[ok], :]
                        av.append(np.repeat(x[n[ok], i[ok], j[ok], c[ok]], b.shape[1])); bv.append(b.ravel())
                    else:
                        a = x[n[ok], oi[ok], oj[ok], :]
                        av.append(a.ravel()); bv.append(np.repeat(dy[n[ok], i[ok], j[ok], c[ok]], a.shape[1]))
        else:
            sp = x if self.kind == 0 else dy
            n, i, j, c = np.nonzero(sp)
            for r in range(R):
                for t in range(S):
                    if self.kind == 0:           # y[oh, ow, k] += x[oh s - pt + r, ow s - pl + t, c] w[r, t, c, k]
                        ok = ((i + self.pt - r) % s == 0) & ((j + self.pl - t) % s == 0)
                        oi, oj = (i + self.pt - r) // s, (j + self.pl - t) // s
                        ok &= (oi >= 0) & (oi < self.OH) & (oj >= 0) & (oj < self.OW)
                        b = w[r, t, c[ok], :]
                    else:                        # dx[oh s - pt + r, ow s - pl + t, c] += dy[oh, ow, k] w[r, t, c, k]
                        oi, oj = i * s - self.pt + r, j * s - self.pl + t
                        ok = (oi >= 0) & (oi < H) & (oj >= 0) & (oj < W)
                        b = w[r, t, :, c[ok]]
                    av.append(np.repeat(sp[n[ok], i[ok], j[ok], c[ok]], b.shape[1])); bv.append(b.ravel())
        return np.concatenate(av), np.concatenate(bv)

    def products_per_output(self, ops):
        """-> float64 counts: the convolution (of the case's direction) of the nonzero indicators of its two operands.  The dense operand
        is nonzero everywhere (asserted), so its indicator is constant over its channels and the indicator convolution is computed with
        that axis collapsed: [.., 1] stands for each of the K (C) equal slices."""
        N, H, W, C, K, R, S, s, padding = self.layer
        x, w, dy = ops
        ind = lambda a: torch.from_numpy((a != 0).astype(np.float64))
        one = lambda *shape: torch.ones(shape, dtype=torch.float64)
        if self.kind == 0:
            assert (w != 0).all()
            return T.conv2d(ind(x).sum(-1, keepdim=True), one(R, S, 1, 1), s, 1, padding).numpy()
        if self.kind == 1:
            assert (w != 0).all()
            xg = torch.zeros((N, H, W, 1), dtype=torch.float64, requires_grad=True)
            T.conv2d(xg, one(R, S, 1, 1), s, 1, padding).backward(ind(dy).sum(-1, keepdim=True))
            return xg.grad.numpy()
        if self.sparse == "x":
            assert (dy != 0).all()
            wg = torch.zeros((R, S, C, 1), dtype=torch.float64, requires_grad=True)
            T.conv2d(ind(x), wg, s, 1, padding).backward(one(N, self.OH, self.OW, 1))
        else:
            assert (x != 0).all()
            wg = torch.zeros((R, S, 1, K), dtype=torch.float64, requires_grad=True)
            T.conv2d(one(N, H, W, 1), wg, s, 1, padding).backward(ind(dy))
        return wg.grad.numpy()

    def reference(self, ops):
        """float64: y, dx or dw of the case, the float64 convolution (oracle.tf_ops.conv2d + autograd) of the float32 operands"""
        N, H, W, C, K, R, S, s, padding = self.layer
        x, w, dy = (None if a is None else torch.from_numpy(np.array(a)).double() for a in ops)
        if self.kind == 0:
            return T.conv2d(x, w, s, 1, padding)
        if self.kind == 1:
            xg = torch.zeros((N, H, W, C), dtype=torch.float64, requires_grad=True)
            T.conv2d(xg, w, s, 1, padding).backward(dy)
            return xg.grad
        wg = torch.zeros((R, S, C, K), dtype=torch.float64, requires_grad=True)
        T.conv2d(x, wg, s, 1, padding).backward(dy)
        return wg.grad

    def collapsed(self):
        """how many equal slices one entry of products_per_output() stands for"""
        N, H, W, C, K = self.layer[:5]
        return {0: K, 1: C}.get(self.kind, K if self.sparse == "x" else C)


def _both(family, layer, **kw):
    return [Case(family, 0, layer, "x", **kw), Case(family, 1, layer, "dy", **kw)]


def _l3(N, H, W, C, K):
    return (N, H, W, C, K, 3, 3, 1, "SAME")


def _ln(N, H, W, padding):
    return (N, H, W, 40, 5, 5, 5, 1, padding)


# conv_x3_direct_kernel<NH, KW, KIND> on 256 persistent workgroups: every multi-item layer has more items than that and no multiple of it
# (300, 300, 275, 300; 360 with two filter blocks per tile), so the loaders cross item boundaries and the last round is partial.
# 64 -> 64 cannot have more than 256 items under 2.4 GMAC (9.4 MMAC per item): (5, 80, 176) has 275.
X3D_LAYERS = [
    _l3(5, 96, 160, 32, 64),      # forward <1, 64, 0>, data gradient <2, 32, 1>
    _l3(5, 96, 160, 64, 32),      # forward <2, 32, 0>, data gradient <1, 64, 1>
    _l3(5, 80, 176, 64, 64),      # forward <2, 64, 0>, data gradient <2, 64, 1>
    _l3(5, 96, 160, 32, 32),      # forward <1, 32, 0>, data gradient <1, 32, 1>
    _l3(1, 16, 16, 32, 64),       # a single tile
]
X3D_FWD_ONLY = [_l3(3, 96, 160, 64, 128)]     # 180 tiles x two filter blocks = 360 items (a data gradient of 128 filters is another route's)
X3S_LAYERS = [
    (3, 32, 96, 64, 64, 3, 3, 2, "SAME"),        # the model's k3s2
    (2, 96, 48, 64, 64, 5, 5, 3, "SAME"),        # stride 3: nine phases
    (3, 160, 192, 64, 64, 5, 5, 2, "SAME"),      # 90 / 360 items: workgroups that cross group boundaries
]
X3N_LAYERS = [_ln(65, 20, 100, "VALID"), _ln(48, 32, 96, "SAME")]      # 780 / 910 and 1152 / 576 items on 512 workgroups
# 330 tiles on 256 workgroups: static shares of one or two tiles
X3W_LAYERS = [_l3(3, 160, 176, 32, 64), _l3(3, 160, 176, 64, 64)]

CASES = []
for _l in X3D_LAYERS:
    CASES += _both("x3d", _l)
CASES += [Case("x3d", 0, _l, "x") for _l in X3D_FWD_ONLY]
for _l in X3S_LAYERS:
    CASES += _both("x3s", _l)
for _l in X3N_LAYERS:
    CASES += _both("x3n", _l)
for _l in X3W_LAYERS:
    for _seed in (0, 1, 2):
        CASES += [Case("x3w", 2, _l, "x", seed=_seed), Case("x3w", 2, _l, "dy", seed=_seed)]
# one bit-exact case per kernel: the dense operand a signed power of two
CASES += _both("x3d", X3D_LAYERS[0], dense="pow2") + _both("x3d", X3D_LAYERS[2], dense="pow2")
CASES += _both("x3s", X3S_LAYERS[0], dense="pow2") + _both("x3n", X3N_LAYERS[0], dense="pow2")
CASES += [Case("x3w", 2, _l, _sp, dense="pow2") for _l in X3W_LAYERS for _sp in ("x", "dy")]

assert len({c.id for c in CASES}) == len(CASES)


def fp32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def units(e):
    return "%.2f * 2^-24" % (e * 2 ** 24) if math.isfinite(e) else str(e)
