"""-m gpu: the elementwise kernels (csrc/elementwise.hip, the two sympad kernels) over their whole domain, against the float64 references
of tests/elementwise_ref.py computed on the device.

The case lists are module-level: tests/test_elementwise_ref_host.py imports them without a GPU and asserts that every dispatch branch
(vector / scalar apply kernels, the second blockIdx.y slice, the scalar column reduction, partial-list compaction, the tiled and the
per-element PS kernels, every grid cap) is reached by at least one case.

Bars are the project's existing ones for the same outputs (tests/test_gpu_elementwise.py): 2e-5 of max|ref| for the BN output, 1e-4 for
dx / dgamma / dbeta, 1e-5 for dshortcut, 1e-6 / 1e-5 absolute for mean / variance, 1e-5 for the moving statistics.  Pure data movement is
bit-exact.  Every test prints its worst error per output (pytest -s -m gpu -k domain).
"""
import numpy as np
import pytest
import torch

import elementwise_ref as R
from conftest import pkg
from oracle import tf_ops as T
from parity_util import rel

pytestmark = pytest.mark.gpu

# (P, C, Cs, alpha, training, keep): rows, channels, shortcut channels (0: none), leaky slope (-1: no activation), mode, dropout keep
BN_CASES = [
    (1, 4, 0, 0.2, True, 1.0), (1, 6, 2, 0.2, True, 0.75), (1, 1200, 1200, 0.2, True, 1.0),
    (3, 4, 2, 0.2, True, 1.0), (3, 20, 10, 0.2, True, 0.75), (3, 64, 32, 0.2, True, 0.75), (3, 1028, 0, 0.2, True, 1.0),
    (63, 24, 12, 0.0, True, 0.75), (63, 40, 20, 0.2, True, 1.0), (63, 512, 0, 0.2, False, 1.0), (63, 1028, 514, 0.2, True, 1.0),
    (64, 40, 40, 0.2, True, 0.75), (64, 6, 6, -1.0, True, 1.0), (64, 20, 2, 0.2, False, 1.0), (64, 24, 24, 0.2, True, 0.5),
    (64, 6, 0, 0.2, False, 1.0),
    (1000, 64, 32, 0.2, True, 0.75), (1000, 64, 62, 0.2, False, 0.75), (1000, 512, 256, 0.2, True, 0.5),
    (1000, 1028, 1028, 0.2, True, 1.0), (1000, 1200, 600, 0.0, False, 0.75), (1000, 1200, 1198, 0.2, True, 1.0),
    (1000, 20, 20, 0.0, True, 1.0), (1000, 40, 38, 0.2, True, 0.75),
    (40000, 4, 0, 0.2, True, 0.75), (40000, 6, 2, 0.2, True, 1.0), (40000, 24, 12, 0.2, False, 1.0), (40000, 64, 64, -1.0, True, 0.75),
    (40000, 512, 510, 0.2, True, 0.75), (40000, 1200, 0, 0.2, True, 1.0),
    (131072, 4, 4, 0.2, True, 1.0), (131072, 6, 0, 0.0, True, 0.75),
]
# (C, Cs of the vector-kernel run, Cs of the scalar-kernel run): both kernels are legal for the channels the two shortcuts share
BN_TWIN_CASES = [(40, 40, 20), (24, 24, 12), (1200, 1200, 1198)]
# (P, C, Cs): bf16 side outputs on a scalar-path and a vector-path case
BN_H_CASES = [(1000, 40, 20), (1000, 64, 32), (63, 6, 0), (1000, 1200, 600)]
SYNCBN_CASES = [(500, 64, 32), (500, 40, 20), (4100, 24, 24)]           # (rows per half, C, Cs)

MAXPOOL_CASES = [(1, 2, 2, 3), (1, 2, 2, 4), (2, 2, 64, 5), (1, 6, 2, 8), (2, 16, 16, 16), (3, 256, 256, 64), (2, 512, 512, 6)]
PS_R, PS_NC, PS_B = (1, 2, 8), (1, 3, 5, 40, 63, 64, 65), (1, 2, 7, 12, 13, 32)
PS_N, PS_A = 2, 3
SYMPAD_HW, SYMPAD_C = ((1, 1), (2, 3), (5, 4), (7, 7)), (3, 4, 8)
# (Ca, tile_a, Cb, Cc, Cd, ncls, (N, H, W))
CRITIC_CASES = [(2, 3, 4, 8, 8, 5, (2, 8, 8)), (3, 1, 4, 8, 8, 8, (1, 5, 7)), (2, 1, 4, 8, 8, 2, (2, 8, 8)), (3, 3, 4, 8, 8, 8, (1, 9, 3)),
                (2, 1, 4, 8, 8, 8, (2, 4, 4)), (2, 3, 4, 8, 8, 5, (2, 300, 300)), (2, 1, 4, 8, 8, 2, (1, 300, 300))]
STREAM_N = (1, 3, 4, 5, 1023, 1024, 1025, (1 << 21) + 3)
DROP_KEEPS = (1.0, 0.75, 0.5)

NAN = float("nan")


def _gen(seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=g.device, dtype=torch.float32)


def _bn_inputs(P, C, Cs, seed, dev):
    g = _gen(seed, dev)
    shape = (1, 1, P, C)
    x = _randn(g, *shape) * 1.7 + 0.6
    gamma, beta = 1.0 + 0.1 * _randn(g, C), 0.1 * _randn(g, C) + 0.05
    mm, mv = 0.3 * _randn(g, C) + 0.1, 1.0 + 0.2 * torch.rand(C, generator=g, device=dev)
    sc = (_randn(g, 1, 1, P, Cs) + 0.2) if Cs else None
    dout = _randn(g, *shape) + 0.1
    return x, gamma, beta, mm, mv, sc, dout


def _mask(shape, keep, seed, sid, dev):
    return torch.from_numpy(T.dropout_mask(shape, keep, seed, sid)).to(dev) if keep < 1.0 else None


@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "P%d-C%d-Cs%d-a%g-%s-k%g" % (c[0], c[1], c[2], c[3], "train" if c[4] else "infer", c[5]))
def test_bn_domain(dev, case):
    """statistics (+ moving update), apply and backward (also with the sums added into caller-owned slots, and with the activation's sign
    recomputed instead of read) of every (P, C, Cs) class against float64"""
    K = pkg("kernels")
    P, C, Cs, alpha, training, keep = case
    seed, sid = 99 + P + C, 3
    x, gamma, beta, mm, mv, sc, dout = _bn_inputs(P, C, Cs, BN_CASES.index(case), dev)
    errs = {}
    if training:
        mm1, mv1 = mm.clone(), mv.clone()
        mean, var = K.bn_stats_update(x, mm1, mv1, 0.9)
        mean2, var2 = K.bn_stats(x)
        assert torch.equal(mean, mean2) and torch.equal(var, var2)
        m64, v64 = R.bn_stats(x)
        mmr, mvr = R.bn_moving(mm, mv, m64, v64, P)
        errs["mean_abs"], errs["var_abs"] = float((mean.double() - m64).abs().max()), float((var.double() - v64).abs().max())
        errs["mm"], errs["mv"] = rel(mm1, mmr), rel(mv1, mvr)
        assert errs["mean_abs"] < 1e-6 and errs["var_abs"] < 1e-5, errs
        assert errs["mm"] < 1e-5 and errs["mv"] < 1e-5, errs
        mm3, mv3 = mm.clone(), mv.clone()
        K.bn_update_moving(mm3, mv3, mean, var, P, 0.9)            # the separate update: the same expressions
        assert torch.equal(mm3, mm1) and torch.equal(mv3, mv1)
    else:
        mean, var = mm.clone(), mv.clone()
    out = K.bn_apply(x, mean, var, gamma, beta, sc, 1e-3, alpha)
    errs["out"] = rel(out, R.bn_apply(x, mean, var, gamma, beta, sc, alpha))
    assert errs["out"] < 2e-5, errs
    dx, dg, db, dsc = K.bn_bwd(dout, out, x, mean, var, gamma, Cs, 1e-3, alpha, training, keep, seed, sid)
    mask = _mask((1, 1, P, C), keep, seed, sid, dev)
    rdx, rdg, rdb, rdsc = R.bn_bwd(dout, out, x, mean, var, gamma, Cs, alpha, training, mask, keep)
    errs["dx"], errs["dgamma"], errs["dbeta"] = rel(dx, rdx), rel(dg, rdg), rel(db, rdb)
    if Cs:
        errs["dshortcut"] = rel(dsc, rdsc)
    print("bn %s: %s" % (case, " ".join("%s %.2e" % kv for kv in errs.items())))
    assert bool(torch.isfinite(dx).all())
    assert errs["dx"] < 1e-4 and errs["dgamma"] < 1e-4 and errs["dbeta"] < 1e-4, errs
    assert not Cs or errs["dshortcut"] < 1e-5, errs
    if keep < 1.0:
        assert bool((dx[mask == 0] == 0).all())             # the mask's zeros
    # the sums also ADDED into caller-owned slots, twice
    sg, sb = torch.full((C,), 2.0, device=dev), torch.full((C,), -1.0, device=dev)
    for rep in (1, 2):
        dx2, dg2, db2, dsc2 = K.bn_bwd(dout, out, x, mean, var, gamma, Cs, 1e-3, alpha, training, keep, seed, sid, into=(sg, sb))
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db) and (not Cs or torch.equal(dsc2, dsc))
        assert rel(sg, 2.0 + rep * dg.double()) < 1e-6 and rel(sb, -1.0 + rep * db.double()) < 1e-6
    if not Cs and alpha >= 0:
        # `out` not handed in: the sign is recomputed from x, bit for bit, in training and in inference mode
        dxr, dgr, dbr, _ = K.bn_bwd(dout, None, x, mean, var, gamma, 0, 1e-3, alpha, training, keep, seed, sid, beta=beta)
        assert torch.equal(dxr, dx) and torch.equal(dgr, dg) and torch.equal(dbr, db)


@pytest.mark.parametrize("C,Cv,Csc", BN_TWIN_CASES)
@pytest.mark.parametrize("training", [True, False])
def test_bn_vector_and_scalar_apply_kernels_agree_bit_for_bit(dev, C, Cv, Csc, training):
    """"same expressions in the same order": the vector kernels (shortcut of Cv channels) and the scalar kernels (the middle Csc channels
    of the same shortcut) must give identical bits on the columns the two shortcuts share, in out, dx and dshortcut; the scalar run's pad
    columns must equal a run without a shortcut"""
    K = pkg("kernels")
    P, alpha, keep, seed, sid = 1000, 0.2, 0.75, 5, 1
    x, gamma, beta, mm, mv, sc, dout = _bn_inputs(P, C, Cv, 1000 + C, dev)
    mean, var = K.bn_stats(x) if training else (mm, mv)
    cpad = (C - Csc) // 2
    sc_mid = sc[..., cpad - (C - Cv) // 2:cpad - (C - Cv) // 2 + Csc].contiguous()
    res = {}
    for name, s in (("vec", sc), ("scalar", sc_mid), ("none", None)):
        out = K.bn_apply(x, mean, var, gamma, beta, s, 1e-3, alpha)
        ncs = s.shape[-1] if s is not None else 0
        dx, dg, db, dsc = K.bn_bwd(dout, out, x, mean, var, gamma, ncs, 1e-3, alpha, training, keep, seed, sid)
        res[name] = (out, dx, dsc, dg, db)
    mid = slice(cpad, cpad + Csc)
    for i, what in enumerate(("out", "dx")):
        assert torch.equal(res["vec"][i][..., mid], res["scalar"][i][..., mid]), what
        for edge in (slice(0, cpad), slice(cpad + Csc, C)):
            assert torch.equal(res["scalar"][i][..., edge], res["none"][i][..., edge]), what + " (pad columns)"
    off = cpad - (C - Cv) // 2
    assert torch.equal(res["vec"][2][..., off:off + Csc], res["scalar"][2]), "dshortcut"
    assert torch.equal(res["vec"][3][mid], res["scalar"][3][mid]) and torch.equal(res["vec"][4][mid], res["scalar"][4][mid])
    # and the float64 reference of the scalar run, shortcut columns and pad columns alike
    out_s, dx_s, dsc_s = res["scalar"][:3]
    mask = _mask((1, 1, P, C), keep, seed, sid, dev)
    rdx, _, _, rdsc = R.bn_bwd(dout, out_s, x, mean, var, gamma, Csc, alpha, training, mask, keep)
    e = (rel(out_s, R.bn_apply(x, mean, var, gamma, beta, sc_mid, alpha)), rel(dx_s, rdx), rel(dsc_s, rdsc))
    print("bn twin C=%d Cs=%d/%d %s: out %.2e dx %.2e dshortcut %.2e" % (C, Cv, Csc, "train" if training else "infer", e[0], e[1], e[2]))
    assert e[0] < 2e-5 and e[1] < 1e-4 and e[2] < 1e-5, e


@pytest.mark.parametrize("P,C,Cs", BN_H_CASES)
def test_bn_bf16_side_outputs(dev, P, C, Cs):
    """want_h / only_h: the float32 results are unchanged bit for bit and the bf16 copy is the result rounded once (nearest-even)"""
    K = pkg("kernels")
    alpha, keep, seed, sid = 0.2, 0.75, 11, 2
    x, gamma, beta, mm, mv, sc, dout = _bn_inputs(P, C, Cs, 2000 + C, dev)
    mean, var = K.bn_stats(x)
    out = K.bn_apply(x, mean, var, gamma, beta, sc, 1e-3, alpha)
    outh = K.bn_apply(x, mean, var, gamma, beta, sc, 1e-3, alpha, want_h=True)
    assert torch.equal(outh, out) and torch.equal(outh._pnp_h[0], out.to(torch.bfloat16))
    dx, dg, db, dsc = K.bn_bwd(dout, out, x, mean, var, gamma, Cs, 1e-3, alpha, True, keep, seed, sid)
    dxw, dgw, dbw, dscw = K.bn_bwd(dout, out, x, mean, var, gamma, Cs, 1e-3, alpha, True, keep, seed, sid, want_h=True)
    assert torch.equal(dxw, dx) and torch.equal(dgw, dg) and torch.equal(dbw, db) and (not Cs or torch.equal(dscw, dsc))
    assert torch.equal(dxw._pnp_h[0], dx.to(torch.bfloat16))
    dxo, dgo, dbo, dsco = K.bn_bwd(dout, out, x, mean, var, gamma, Cs, 1e-3, alpha, True, keep, seed, sid, only_h=True)
    assert isinstance(dxo, K.HalfOnly) and torch.equal(dxo.h, dx.to(torch.bfloat16))
    assert torch.equal(dgo, dg) and torch.equal(dbo, db) and (not Cs or torch.equal(dsco, dsc))
    sums = torch.stack([dg, db])
    dxa, dsca = K.bn_bwd_apply(dout, out, x, mean, var, gamma, sums, P, Cs, 1e-3, alpha, True, keep, seed, sid, only_h=True)
    assert torch.equal(dxa.h, dxo.h) and (not Cs or torch.equal(dsca, dsc))


@pytest.mark.parametrize("Ph,C,Cs", SYNCBN_CASES)
def test_syncbn_split_on_one_gpu(dev, Ph, C, Cs):
    """pnp_bn_bwd_reduce on two half batches, the two [2, C] sums added, pnp_bn_bwd_apply(P_norm = 2P) on each half == the full batch's
    backward.  The dropout mask index is the LOCAL flat index: each half carries the mask of a Ph x C tensor"""
    K = pkg("kernels")
    alpha, seed, sid = 0.2, 7, 4
    g = _gen(3000 + C, dev)
    x = _randn(g, 2, 1, Ph, C) * 1.7 + 0.6
    dout = _randn(g, 2, 1, Ph, C) + 0.1
    gamma, beta = 1.0 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)
    sc = _randn(g, 2, 1, Ph, Cs)
    mean, var = K.bn_stats(x)
    out = K.bn_apply(x, mean, var, gamma, beta, sc, 1e-3, alpha)
    halves = [(dout[k:k + 1], out[k:k + 1], x[k:k + 1]) for k in (0, 1)]
    sums = [K.bn_bwd_reduce(d, o, xx, mean, var, 1e-3, alpha) for d, o, xx in halves]
    tot = sums[0] + sums[1]
    full = K.bn_bwd(dout, out, x, mean, var, gamma, Cs, 1e-3, alpha, True, 1.0, seed, sid)
    e_sum = (rel(tot[0], full[1]), rel(tot[1], full[2]))
    for keep in (1.0, 0.75):
        parts = [K.bn_bwd_apply(d, o, xx, mean, var, gamma, tot, 2 * Ph, Cs, 1e-3, alpha, True, keep, seed, sid) for d, o, xx in halves]
        dx, dsc = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        mh = _mask((1, 1, Ph, C), keep, seed, sid, dev)
        mask = torch.cat([mh, mh]) if mh is not None else None
        rdx, rdg, rdb, rdsc = R.bn_bwd(dout, out, x, mean, var, gamma, Cs, alpha, True, mask, keep)
        e64 = rel(dx, rdx)
        assert e64 < 1e-4, e64
        assert torch.equal(dsc, full[3])                   # the activation's gradient does not depend on the sums
        if keep == 1.0:
            e32 = rel(dx, full[0])
            # two float32 evaluations whose only difference is the summation order of dgamma / dbeta (each a few 1e-7 of its value)
            assert e32 < 1e-5, e32
        else:
            mfull = _mask((2, 1, Ph, C), keep, seed, sid, dev)
            assert bool((dx[1][mh[0] == 0] == 0).all()) and not torch.equal(mfull[1], mh[0])
            assert float(((dx == 0) & (mask != 0)).float().mean()) < 1e-3
    print("syncbn split Ph=%d C=%d Cs=%d: summed dgamma %.2e dbeta %.2e vs full batch; dx vs float64 %.2e, vs full-batch kernel %.2e" % (
        Ph, C, Cs, e_sum[0], e_sum[1], e64, e32))
    assert e_sum[0] < 1e-5 and e_sum[1] < 1e-5
    # a wrong normaliser must be visible: P_norm = P instead of 2P moves dx by far more than the bar
    wrong = torch.cat([K.bn_bwd_apply(d, o, xx, mean, var, gamma, tot, Ph, Cs, 1e-3, alpha, True, 1.0, seed, sid)[0] for d, o, xx in halves])
    assert rel(wrong, full[0]) > 1e-3


@pytest.mark.parametrize("shape", MAXPOOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_domain(dev, shape):
    """integer-valued inputs full of ties: forward and first-maximum backward are bit-exact"""
    K = pkg("kernels")
    g = _gen(sum(shape), dev)
    x = torch.randint(-3, 4, shape, generator=g, device=dev).float()
    dy = _randn(g, shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    assert torch.equal(K.maxpool2_fwd(x), R.maxpool2_fwd(x).float())
    assert torch.equal(K.maxpool2_bwd(x, dy), R.maxpool2_bwd(x, dy).float())


@pytest.mark.parametrize("r", PS_R)
def test_ps_domain(dev, r):
    """every (nc, B) of the grid, forward and backward, on arange input (every element distinguishable): bit-exact"""
    K = pkg("kernels")
    for nc in PS_NC:
        for B in PS_B:
            n = PS_N * PS_A * B * nc * r * r
            x = torch.arange(n, dtype=torch.float32, device=dev).reshape(PS_N, PS_A, B, nc * r * r)
            y = K.ps_fwd(x, r, nc)
            assert torch.equal(y, R.ps_fwd(x, r, nc).float()), (r, nc, B)
            dy = torch.arange(n, dtype=torch.float32, device=dev).reshape(PS_N, PS_A * r, B * r, nc) * 2.0 + 1.0
            assert torch.equal(K.ps_bwd(dy, r, nc), R.ps_bwd(dy, r, nc).float()), (r, nc, B)
            assert torch.equal(K.ps_bwd(y, r, nc), x), (r, nc, B)


@pytest.mark.parametrize("H,W", SYMPAD_HW)
def test_sympad_domain(dev, H, W):
    """every legal pad 0 ... min(H, W) (at p = H every row collects three mirrored rows): forward bit-exact, backward against float64"""
    K = pkg("kernels")
    worst = 0.0
    for C in SYMPAD_C:
        for p in range(0, min(H, W) + 1):
            g = _gen(100 * H + 10 * C + p, dev)
            x = _randn(g, 2, H, W, C) + 0.3
            assert torch.equal(K.sympad_fwd(x, p), R.sympad_fwd(x, p).float()), (H, W, C, p)
            dxp = _randn(g, 2, H + 2 * p, W + 2 * p, C) + 0.3
            e = rel(K.sympad_bwd(dxp, p), R.sympad_bwd(dxp, p))
            worst = max(worst, e)
            assert e < 1e-6, (H, W, C, p, e)
    print("sympad bwd %dx%d: worst %.2e" % (H, W, worst))


@pytest.mark.parametrize("case", CRITIC_CASES, ids=lambda c: "-".join(map(str, c[:6])) + "-" + "x".join(map(str, c[6])))
def test_critic_input_domain(dev, case):
    K = pkg("kernels")
    Ca, tile_a, Cb, Cc, Cd, ncls, sh = case
    g = _gen(CRITIC_CASES.index(case), dev)
    a, b, c, d, lg = (_randn(g, *sh, n) + 0.1 for n in (Ca, Cb, Cc, Cd, ncls))
    lg[0, 0, 0] = 1.5                                       # every class tied: class 0
    lg[0, 0, 1] = -1.0
    lg[0, 0, 1, 1::2] = 2.0                                 # the odd classes tied: class 1
    out = K.critic_input_fwd(a, tile_a, b, c, d, lg)
    ref = R.critic_input_fwd(a, tile_a, b, c, d, lg)
    assert out.shape[-1] == Ca * tile_a + Cb + Cc + Cd + ncls + 1
    assert float(ref[0, 0, 0, -1]) == 0.0 and float(ref[0, 0, 1, -1]) == (1.0 if ncls > 1 else 0.0)
    assert torch.equal(out, ref.float())
    dout = _randn(g, *out.shape)
    shapes = tuple(tuple(t.shape) for t in (a, b, c, d, lg))
    full = K.critic_input_bwd(dout, shapes, tile_a)
    refs = R.critic_input_bwd(dout, (Ca, Cb, Cc, Cd, ncls), tile_a)
    errs = [rel(got, want) for got, want in zip(full, refs)]
    print("critic input %s: backward %s" % (case, " ".join("%.2e" % e for e in errs)))
    assert max(errs) < 1e-6, errs
    for i in range(1, 5):
        assert torch.equal(full[i], refs[i].float())        # copies
    # need=: one output switched off, and all but one — the outputs still asked for do not change
    needs = [tuple(j != i for j in range(5)) for i in range(5)] + [tuple(j == i for j in range(5)) for i in range(5)]
    for need in needs:
        got = K.critic_input_bwd(dout, shapes, tile_a, need=need)
        for j in range(5):
            assert (got[j] is None) == (not need[j])
            assert got[j] is None or torch.equal(got[j], full[j]), need


@pytest.mark.parametrize("n", STREAM_N)
def test_streaming_ops_domain(dev, n):
    """dropout (also with its bf16 copy), axpby, add, fill at sizes around the vector body / tail split.  Every tensor is a fresh allocation
    (16-byte aligned: the kernels' contract)"""
    K = pkg("kernels")
    g = _gen(n % 9973, dev)
    x, y0 = _randn(g, n) + 0.5, _randn(g, n) - 0.25
    for keep in DROP_KEEPS:
        for want_h in (False, True):
            y = K.dropout(x, keep, 1234 + n, 5, want_h=want_h)
            if keep < 1.0:
                m = T.dropout_mask((n,), keep, 1234 + n, 5)
                want = np.where(m != 0, x.cpu().numpy() / np.float32(keep), np.float32(0))      # one correctly rounded float32 division
            else:
                want = x.cpu().numpy()
            assert torch.equal(y.cpu(), torch.from_numpy(want.astype(np.float32))), (n, keep)
            if want_h:
                assert torch.equal(y._pnp_h[0], y.to(torch.bfloat16))
    assert torch.equal(K.add(x, y0), x + y0)
    yy = y0.clone()
    assert K.axpby(x, yy, 2.5, -0.75) is yy
    e = rel(yy, 2.5 * x.double() - 0.75 * y0.double())
    print("axpby n=%d: %.2e" % (n, e))
    assert e < 1e-6
    t = torch.full((n,), NAN, device=dev)
    K.fill_(t, -3.25)
    assert torch.equal(t, torch.full((n,), -3.25, device=dev))
    f = K.filled((n,), 0.125, dev)
    assert torch.equal(f, torch.full((n,), 0.125, device=dev))
