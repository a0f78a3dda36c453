"""-m gpu: the kernels of csrc/critic_gp.hip (pnp_gp_interpolate, pnp_gp_penalty, pnp_bn_dbl_bwd) over everything their launchers can
produce, against the float64 references of tests/gp_ref.py on the same float32 operands: both load widths, every blockIdx.y slice shape
of group_map, the row-slab and apply-grid caps, every shortcut placement, the three activations, the three keep probabilities, planted
samples and signed zeros, gamma_bar null / pre-filled, determinism, the refusals, and the gscale / keep_prob arguments of the walker.
tests/test_gp_ref_host.py proves (without a GPU) that the module-level case lists below reach every one of those branches.

Bars.  Interpolation: |got - ref| <= 2^-22 (|eps a| + |(1 - eps) b|) per element (1 - eps is exact in float32, one product and one fused
multiply-add are rounded: 2^-23 of that sum, a factor 2 over it).  Penalty: 1e-6 relative per sample norm, for the value and per element of
the adjoint (a few float32 roundings of values accumulated in double), exact zeros where the reference is zero.  A sample of 1e20s has
(|g| - 1)^2 >= 1e40 — beyond float32 — so a batch holding one has the penalty slot's correctly rounded value +inf for coef > 0 (asserted;
never NaN) and exactly 0 for coef = 0; its norms and adjoint are finite and held to the same 1e-6.  BN double backward, ordinary operands:
the project's 1e-5 of max|ref| per output.  P = 1: every reference is zero and the kernel returns the rounding of terms that cancel —
gy_bar = k2 v + k0 with k2 = gamma/sigma, k0 = -(gamma/sigma) m_v, gamma_bar = P (m_vg - m_v m_g) / sigma, xc_bar the sum of
-(gamma/sigma^2) m_gx (v - m_v) and its siblings with xhat = 0; the bars are 1e-6 of max|gamma/sigma v|, max|P m_vg / sigma| and
max|gamma/sigma^2 v g_z|.  Hard operands: 2 x max(error of gp_ref.bn_dbl_closed_f32 on the same tensors, 1e-6) of max|ref|, the rule of
tests/test_gpu_x3_wgrad.py (2x: a differently ordered, equally long float32 chain).

Measured on one MI355X, hard operands, worst of gy_bar / xc_bar / gamma_bar over the four shapes, kernel | float32 restatement, of
max|ref|: d = 100 +- 1.3: 1.6e-7 | 2.4e-7; d = 5 +- 0.01: 1.7e-7 | 2.4e-7; gc_bar = 50 + noise: 1.3e-5 | 1.5e-5 (1000 x 1028, xc_bar; the
other shapes 1.6e-6 | 1.9e-6 and below); g_y = 50 + noise: 5.7e-7 | 7.0e-7; both = 1 + noise: 1.2e-6 | 3.3e-5 (gamma_bar at P = 131073:
9.2e-7 | 3.3e-5); wide: 1.7e-7 | 2.0e-7.  Ordinary operands: gy_bar <= 1.4e-7, xc_bar <= 5.4e-7, gamma_bar <= 5.2e-7."""
import ctypes

import numpy as np
import pytest
import torch

import gp_ref as R
from conftest import pkg
from oracle import nets_adv
from oracle import tf_ops as T
from test_gpu_adversarial import _rel, grad_report, make_vars
from test_gpu_gradient_penalty import MIU, NETCFG, critic_inputs  # noqa: F401  (critic_inputs: the existing file's fixture)

pytestmark = pytest.mark.gpu

BN_EPS, SEED, SID = 1e-3, 5, 9

# ---- case lists (module level: tests/test_gp_ref_host.py reads them) -----------------------------------------------------------------
# (B, n, a = -b)
INTERP_CASES = [(1, 1, False), (2, 3, False), (300, 4, False), (2, 105, False), (3, 8188, False), (2, 8188, True),
                (2, (1 << 21) + 8, False), (1, (1 << 21) + 3, False), (1, (1 << 21) + 5, False), (65535, 3, False)]

# (B, n, coef, gscale, plants): plants are written over samples 0, 1, ... in this order (as far as B goes)
PLANTS = ("zero", "onehot", "tiny")
PLANTS_HUGE = ("zero", "onehot", "tiny", "huge")
PEN_CASES = [
    (1, 105, 10.0, 1.0, ()),
    (1, 64, 10.0, 0.125, ("onehot",)),
    (3, 105, 10.0, 0.125, PLANTS),                     # one element per lane
    (5, 105, 10.0, 1.0, PLANTS_HUGE),
    (4, 8188, 0.0, 1.0, PLANTS_HUGE),                  # coef 0: penalty and adjoint exactly zero
    (4, 8188, 10.0, 1.0, PLANTS),                      # 16 bytes per lane
    (4, 64 * 256 * 4 + 4, 10.0, 0.125, PLANTS_HUGE),   # one lane of the norm kernel makes a second pass
    (4, 64 * 256 + 3, 10.0, 1.0, PLANTS),              # the same in the scalar form
    (4, (1 << 21) + 8, 10.0, 1.0, PLANTS),             # the scale kernel's cap of 256 workgroups per sample
    (2, (1 << 21) + 5, 10.0, 0.125, ("tiny", "huge")),    # the same, one element per lane
    (300, 12, 10.0, 1.0, PLANTS_HUGE),                 # gp_final_kernel's loop over the samples
    (300, 7, 10.0, 0.125, PLANTS),
    (300, 7, 10.0, 1.0, ("onehot",) * 300),            # a batch of one-hots: penalty exactly 0
]

# (P, C, Cs, alpha (< 0: no activation, y = None), keep)
DBL_CASES = [
    (3, 4, 0, 0.2, 0.75),               # P < rows per pass (256)
    (3, 3, 1, 0.0, 1.0),                # one channel per lane, Cs = C - 2
    (3, 1028, 0, 0.2, 1.0),             # two slices: the second is one channel group wide, 256 rows per pass over 3 rows
    (63, 4, 4, 0.2, 0.5),
    (63, 20, 18, 0.2, 0.75),            # 5 channel groups: 51 rows per pass, one idle lane; a pad of one channel
    (64, 24, 0, -1.0, 1.0),             # 6 groups: 4 idle lanes
    (64, 5, 5, 0.0, 0.75),
    (64, 1, 1, 0.2, 1.0),
    (200, 24, 12, 0.2, 0.75),           # 4 row slabs: a combine with fewer than 8
    (1000, 8, 4, 0.2, 0.75),            # a pad of 2 channels in the 16-byte kernel
    (1000, 40, 2, 0.2, 0.5),            # 10 groups: 6 idle lanes; two shortcut channels inside a wide C
    (1000, 64, 64, 0.2, 0.75),          # the mask critic's residual block: Cs = C
    (1000, 6, 4, -1.0, 0.75),
    (1000, 257, 0, 0.2, 1.0),           # scalar, two slices, the last one channel wide
    (1000, 1028, 1026, 0.0, 0.75),      # vector, two slices, the last one group wide; the shortcut crosses the boundary
    (1000, 1030, 1028, 0.2, 0.75),      # scalar, five slices, the last 6 channels wide
    (1000, 1200, 600, 0.2, 1.0),        # vector, second slice 44 groups wide: 5 rows per pass, 36 idle lanes
    (3000, 1200, 1198, 0.2, 0.75),      # the apply grid's cap of 2048 / 2
    (3000, 8, 0, 0.2, 1.0),
    (131073, 4, 2, 0.2, 0.75),          # 2049 slabs of 64 rows wanted: the cap of 2048
    (131073, 6, 6, 0.0, 0.5),           # the same, scalar; the apply grid's cap of 2048
]
# (P, C, Cs): one row — every reference is zero, but for gy_bar under a shortcut adjoint (its slope-weighted copy)
P1_CASES = [(1, 1, 0), (1, 5, 0), (1, 8, 0), (1, 8, 8), (1, 6, 4), (1, 257, 0), (1, 1028, 0)]
GBAR_CASES = [(64, 5, 5, 0.0, 0.75), (1000, 40, 2, 0.2, 0.5), (1000, 1028, 1026, 0.0, 0.75)]
DET_CASES = [(1000, 6, 4, -1.0, 0.75), (1000, 64, 64, 0.2, 0.75), (1000, 1028, 1026, 0.0, 0.75)]
# hard operands: d100 / d5: mean >> spread; gc_off / gy_off / both_off: a common offset on gc_bar, on g_y, on both; wide: gc_bar, g_y and
# the shortcut adjoint span 1e-6 .. 1e3 with 75 % exact zeros
HARD_KINDS = ("d100", "d5", "gc_off", "gy_off", "both_off", "wide")
HARD_OFFSET = {"gc_off": 50.0, "gy_off": 50.0, "both_off": 1.0}
HARD_SHAPES = [(1000, 64, 32, 0.2, 0.75), (3000, 6, 4, 0.2, 0.75), (1000, 1028, 0, 0.2, 1.0), (131073, 4, 0, 0.2, 0.75)]
HARD_CASES = [s + (k,) for s in HARD_SHAPES for k in HARD_KINDS]


# ---- operands (numpy on the host: tests/test_gp_ref_host.py builds the same tensors without a GPU) ----------------------------------
def _wide(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-6.0, 3.0, shape) * (rng.random(shape) < 0.25)


def dbl_operands(case, kind="normal", device="cpu"):
    """float32 operands of pnp_bn_dbl_bwd for (P, C, Cs, alpha, keep), distributed as in test_bn_double_backward_kernel; for P > 1 channel
    C // 2 of d is constant over the rows; with an activation, y = leaky(z) of these operands with +0.0 and -0.0 planted under a non-zero
    g_y.  mean / var: float64 statistics of the float32 d, rounded to float32.  -> dict of tensors on `device` (mask: float64 or None)"""
    P, C, Cs, alpha, keep = case
    rng = np.random.default_rng(1000003 * P + 1009 * C + Cs + (sum(map(ord, kind)) if kind != "normal" else 0))
    shape = (P, C)
    nrm = lambda s: rng.standard_normal(s)
    d = nrm(shape) * 1.3 + 0.2
    gy, gcb = nrm(shape), nrm(shape)
    scb = nrm((P, Cs)) if Cs else None
    if kind == "d100":
        d = nrm(shape) * 1.3 + 100.0
    elif kind == "d5":
        d = nrm(shape) * 0.01 + 5.0
    elif kind in ("gc_off", "both_off", "gy_off"):
        gcb = gcb + (HARD_OFFSET[kind] if kind != "gy_off" else 0.0)
        gy = gy + (HARD_OFFSET[kind] if kind != "gc_off" else 0.0)
    elif kind == "wide":
        gy, gcb = _wide(rng, shape), _wide(rng, shape)
        scb = _wide(rng, (P, Cs)) if Cs else None
    else:
        assert kind == "normal", kind
    if P > 1 and kind == "normal":
        d[:, C // 2] = 0.75
    gamma, beta = 1.0 + 0.3 * nrm(C), 0.1 * nrm(C)
    sc = nrm((P, Cs)) if Cs else None
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if a is not None else None
    o = {"d": f32(d), "gy": f32(gy), "gcb": f32(gcb), "scb": f32(scb), "gamma": f32(gamma)}
    d64 = o["d"].double()
    mean = d64.mean(0)
    var = ((d64 - mean) ** 2).mean(0)
    o["mean"], o["var"] = mean.float(), var.float()
    o["y"] = None
    if alpha >= 0:
        z = (d64 - mean) * (o["gamma"].double() / torch.sqrt(var + BN_EPS)) + f32(beta).double()
        if Cs:
            z = z + T.pad_channels(f32(sc).double(), (C - Cs) // 2)
        y = torch.where(z > 0, z, z * alpha).float().reshape(-1)
        k = rng.permutation(P * C)[:max(2, min(P * C // 8, 64))]
        y[torch.from_numpy(k[0::2])] = 0.0
        y[torch.from_numpy(k[1::2])] = -0.0
        if kind in ("normal", "gy_off", "both_off"):
            assert bool((o["gy"].reshape(-1)[torch.from_numpy(k)] != 0).all())
        o["y"] = y.reshape(P, C)
    o["mask"] = torch.from_numpy(T.dropout_mask(shape, keep, SEED, SID)).double() if keep < 1 else None
    return {k_: (v.to(device) if v is not None else None) for k_, v in o.items()}


def _run_dbl(K, o, case, gamma_bar="zeros"):
    P, C, Cs, alpha, keep = case
    gb = torch.zeros(C, dtype=torch.float32, device=o["d"].device) if isinstance(gamma_bar, str) else gamma_bar
    gyb, xcb = K.bn_dbl_bwd(o["gcb"], o["d"], o["y"], o["gy"], o["mean"], o["var"], o["gamma"], o["scb"], BN_EPS, alpha, keep, SEED, SID,
                            gamma_bar=gb)
    return gyb, xcb, gb


def _refs(o, case, fn=R.bn_dbl_closed):
    P, C, Cs, alpha, keep = case
    return fn(o["gcb"], o["d"], o["y"], o["gy"], o["mean"], o["var"], o["gamma"], o["scb"], BN_EPS, alpha, keep, o["mask"])


def _errs(got, ref):
    """max |got - ref| / max |ref| per output, on the device in float64"""
    return [float((g.double().reshape(r.shape) - r).abs().max() / (r.abs().max() + 1e-300)) for g, r in zip(got, ref)]


# ---- interpolation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", INTERP_CASES, ids=lambda c: "%dx%d%s" % (c[0], c[1], "-neg" if c[2] else ""))
def test_interpolation_over_its_domain(dev, case):
    K = pkg("kernels")
    B, n, neg = case
    g = torch.Generator(device=dev).manual_seed(B * 31 + n)
    a = torch.randn((B, n), generator=g, device=dev)
    b = -a if neg else torch.randn((B, n), generator=g, device=dev) * 1.2 + 0.1
    out, eps = K.gp_interpolate(a, b, 7, 123)
    want = torch.from_numpy(R.gp_eps(B, 7, 123))
    assert torch.equal(eps.cpu(), want), "eps is not the numpy restatement's"
    out2, eps2 = K.gp_interpolate(a, b, 7, 123)
    assert torch.equal(out, out2) and torch.equal(eps, eps2), "two calls differ"
    _, eps3 = K.gp_interpolate(a, b, 7, 124)
    assert torch.equal(eps3.cpu(), torch.from_numpy(R.gp_eps(B, 7, 124)))
    assert not torch.equal(eps, eps3)                              # eps follows the stream id
    ta, tb = R.interp_terms(a, b, eps)
    err = (out.double() - (ta + tb)).abs()
    bound = 2.0 ** -22 * (ta.abs() + tb.abs())
    worst = float((err / (bound + 1e-300)).max())
    print("interp B %d n %d%s: worst error %.3f of its bound, max err %.3e" % (B, n, " a = -b" if neg else "", worst, float(err.max())))
    assert bool((err <= bound).all()), worst


# ---- penalty ---------------------------------------------------------------------------------------------------------------------------------
def _pen_operand(case, dev):
    B, n, coef, gscale, plants = case
    g = torch.Generator(device=dev).manual_seed(B * 131 + n)
    x = torch.randn((B, n), generator=g, device=dev) * 0.3
    for i, kind in enumerate(plants[:B]):
        if kind == "zero":
            x[i] = 0.0
        elif kind == "onehot":
            x[i] = 0.0
            x[i, (7 * i + n // 2) % n] = -1.0 if i % 2 else 1.0
        elif kind == "tiny":
            x[i] = torch.randn(n, generator=g, device=dev) * 1e-25 + 1e-25
        elif kind == "huge":
            x[i] = torch.randn(n, generator=g, device=dev) * 1e20 + 1e20
    return x


@pytest.mark.parametrize("case", PEN_CASES, ids=lambda c: "%dx%d-c%g-s%g-%d" % (c[0], c[1], c[2], c[3], len(c[4])))
def test_penalty_over_its_domain(dev, case):
    K = pkg("kernels")
    B, n, coef, gscale, plants = case
    x = _pen_operand(case, dev)
    nrm, pen_ref, adj = R.penalty_ref(x, coef, gscale)
    gt = x.clone()
    pen, norms = K.gp_penalty_(gt, coef, gscale)
    got_p = float(pen)
    e_n = float(((norms.double() - nrm).abs() / nrm.clamp_min(1e-300)).max())
    e_a = float(((gt.double() - adj).abs() / adj.abs().clamp_min(1e-300))[adj != 0].max()) if bool((adj != 0).any()) else 0.0
    print("penalty B %d n %d coef %g gscale %g plants %d: norms %.2e, adjoint %.2e (per element), penalty %.9g vs %.9g" % (
        B, n, coef, gscale, len(plants), e_n, e_a, got_p, float(pen_ref)))
    assert bool(torch.isfinite(norms).all()) and bool(torch.isfinite(gt).all())
    assert bool(((norms.double() - nrm).abs() <= 1e-6 * nrm).all())
    assert bool(((gt.double() - adj).abs() <= 1e-6 * adj.abs()).all())                 # (exact zeros where the reference is zero)
    for i, kind in enumerate(plants[:B]):
        if kind in ("zero", "onehot"):
            assert float(gt[i].abs().max()) == 0.0, (i, kind)
            assert float(norms[i]) == (0.0 if kind == "zero" else 1.0), (i, kind)
    if float(pen_ref) > float(np.finfo(np.float32).max):
        assert "huge" in plants[:B] and coef > 0 and got_p == float("inf"), got_p       # the float32 slot's correctly rounded value
    elif float(pen_ref) == 0.0:
        assert got_p == 0.0, got_p
    else:
        assert np.isfinite(got_p) and abs(got_p - float(pen_ref)) <= 1e-6 * float(pen_ref), (got_p, float(pen_ref))
    x2 = x.clone()
    pen2, norms2 = K.gp_penalty_(x2, coef, gscale)
    assert torch.equal(x2, gt) and torch.equal(norms2, norms) and torch.equal(pen2, pen), "two calls differ"


# ---- BN double backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DBL_CASES, ids=lambda c: "P%d-C%d-Cs%d-a%g-k%g" % c)
def test_bn_double_backward_over_its_domain(dev, case):
    K = pkg("kernels")
    P, C, Cs, alpha, keep = case
    o = dbl_operands(case, "normal", dev)
    got = _run_dbl(K, o, case)
    ref = _refs(o, case)
    e = _errs(got, ref)
    print("bn dbl %s: gy_bar %.3e xc_bar %.3e gamma_bar %.3e of max|ref| (%.2e / %.2e / %.2e)" % (
        (case,) + tuple(e) + tuple(float(r.abs().max()) for r in ref)))
    assert all(bool(torch.isfinite(t).all()) for t in got)
    if o["mask"] is not None:
        assert bool((o["mask"] == 0).any()) and float(got[1][o["mask"] == 0].abs().max()) == 0.0
    if o["y"] is not None:
        assert int((o["y"] == 0).sum()) >= 2
    assert max(e) <= 1e-5, e


@pytest.mark.parametrize("P,C,Cs", P1_CASES)
@pytest.mark.parametrize("alpha,keep", [(0.2, 1.0), (-1.0, 0.75)])
def test_bn_double_backward_one_row(dev, P, C, Cs, alpha, keep):
    """P = 1: every reference is identically zero (gy_bar: the slope-weighted shortcut adjoint alone); the bars are 1e-6 of the largest
    cancelling term — max|gamma/sigma v| for gy_bar (k2 v + k0), max|P m_vg / sigma| for gamma_bar (m_vg - m_v m_g),
    max|gamma/sigma^2 v g_z| for xc_bar"""
    K = pkg("kernels")
    case = (P, C, Cs, alpha, keep)
    o = dbl_operands(case, "normal", dev)
    got = _run_dbl(K, o, case)
    ref = _refs(o, case)
    assert all(float(r.abs().max()) <= 1e-12 for r in ref[1:]) and (float(ref[0].abs().max()) > 0) == (Cs > 0)
    sig = torch.sqrt(o["var"].double() + float(np.float32(BN_EPS)))
    v = o["gcb"].double() * (o["mask"] / float(np.float32(keep)) if o["mask"] is not None else 1.0)
    gz = o["gy"].double() * (R._slope(o["y"], o["gy"], alpha, torch.float64))
    ga = o["gamma"].double()
    t_gy, t_gb, t_xc = float((ga / sig * v).abs().max()), float((P * v * gz / sig).abs().max()), float((ga / sig ** 2 * v * gz).abs().max())
    e = [float((g.double().reshape(r.shape) - r).abs().max()) for g, r in zip(got, ref)]
    print("bn dbl one row C %d Cs %d alpha %g keep %g: gy_bar off by %.2e, term %.2e; xc_bar %.2e, term %.2e; gamma_bar %.2e, term %.2e" % (
        C, Cs, alpha, keep, e[0], t_gy, e[1], t_xc, e[2], t_gb))
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert e[0] <= 1e-6 * t_gy and e[1] <= 1e-6 * t_xc and e[2] <= 1e-6 * t_gb


@pytest.mark.parametrize("case", GBAR_CASES, ids=lambda c: "P%d-C%d-Cs%d-a%g-k%g" % c)
def test_gamma_bar_null_and_accumulating(dev, case):
    K = pkg("kernels")
    P, C = case[:2]
    o = dbl_operands(case, "normal", dev)
    gy0, xc0, gb0 = _run_dbl(K, o, case)
    gy1, xc1, _ = _run_dbl(K, o, case, gamma_bar=None)
    assert torch.equal(gy0, gy1) and torch.equal(xc0, xc1), "gamma_bar = null changes the other outputs"
    slot = torch.randn(C, generator=torch.Generator(device=dev).manual_seed(C), device=dev) * 3.0
    gy2, xc2, gb2 = _run_dbl(K, o, case, gamma_bar=slot.clone())
    assert torch.equal(gy0, gy2) and torch.equal(xc0, xc2)
    assert float(gb0.abs().max()) > 0 and torch.equal(gb2, slot + gb0), "slot + gamma_bar is not one float32 addition"
    ref = _refs(o, case)[2] + slot.double()
    err = float((gb2.double() - ref).abs().max() / ref.abs().max())
    print("gamma_bar into a filled slot %s: %.3e of max|ref|" % (case, err))
    assert err <= 1e-5


@pytest.mark.parametrize("case", DET_CASES, ids=lambda c: "P%d-C%d-Cs%d-a%g-k%g" % c)
def test_bn_double_backward_is_deterministic(dev, case):
    K = pkg("kernels")
    o = dbl_operands(case, "normal", dev)
    a, b = _run_dbl(K, o, case), _run_dbl(K, o, case)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("case", HARD_CASES, ids=lambda c: "P%d-C%d-Cs%d-a%g-k%g-%s" % c)
def test_bn_double_backward_hard_operands(dev, case):
    K = pkg("kernels")
    shape, kind = case[:5], case[5]
    o = dbl_operands(shape, kind, dev)
    got = _run_dbl(K, o, shape)
    ref = _refs(o, shape)
    e_k, e_r = _errs(got, ref), _errs(_refs(o, shape, R.bn_dbl_closed_f32), ref)
    print("bn dbl hard %s: kernel %.2e %.2e %.2e | float32 restatement %.2e %.2e %.2e of max|ref| (gy_bar, xc_bar, gamma_bar)" % (
        (case,) + tuple(e_k) + tuple(e_r)))
    assert all(bool(torch.isfinite(t).all()) for t in got)
    for name, k, r in zip(("gy_bar", "xc_bar", "gamma_bar"), e_k, e_r):
        assert k <= 2.0 * max(r, 1e-6), (name, k, r)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -77.25


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _refused(L, code, name, outs):
    with pytest.raises(L.PnpError, match=name):
        L.check(code, name)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), "a refused call wrote an output"


def test_interpolate_and_penalty_refusals(dev):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    a = torch.ones((4, 8), device=dev)
    b = torch.ones((4, 8), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.pnp_gp_workspace_bytes(4, 8))
    assert need == R.gp_dispatch(4, 8)["workspace"]
    for B, n in ((0, 8), (65536, 8), (4, 0)):
        assert int(lib.pnp_gp_workspace_bytes(B, n)) == 0
        out, eps = torch.full((4, 8), SENTINEL, device=dev), torch.full((4,), SENTINEL, device=dev)
        _refused(L, lib.pnp_gp_interpolate(_vp(a), _vp(b), _vp(out), _vp(eps), B, n, 7, 1, st), "pnp_gp_interpolate", (out, eps))
        g, norms, pen = torch.full((4, 8), SENTINEL, device=dev), torch.full((4,), SENTINEL, device=dev), torch.full((1,), SENTINEL, device=dev)
        ws = K.workspace(need, dev)
        _refused(L, lib.pnp_gp_penalty(_vp(g), B, n, 10.0, 1.0, _vp(norms), _vp(pen), _vp(ws), need, st), "pnp_gp_penalty", (g, norms, pen))
    g, norms, pen = torch.full((4, 8), SENTINEL, device=dev), torch.full((4,), SENTINEL, device=dev), torch.full((1,), SENTINEL, device=dev)
    ws = K.workspace(need, dev)
    _refused(L, lib.pnp_gp_penalty(_vp(g), 4, 8, 10.0, 1.0, _vp(norms), _vp(pen), _vp(ws), need - 1, st), "pnp_gp_penalty", (g, norms, pen))


# what differs from a valid call (P = 6, C = 8, Cs = 4, eps 1e-3, alpha 0.2, keep 0.75, every pointer set)
DBL_REFUSALS = [("C = 65536", dict(C=65536)), ("P * C > 2^32", dict(P=(1 << 30) + 1, C=4, Cs=0)), ("C - Cs odd", dict(Cs=3)), ("Cs > C", dict(Cs=10)),
                ("shortcut adjoint null", dict(scb=None)), ("keep = 0", dict(keep=0.0)), ("keep = 1.5", dict(keep=1.5)), ("eps = 0", dict(eps=0.0)),
                ("alpha = 0.2 with y null", dict(y=None)), ("alpha = 0 with y null", dict(y=None, alpha=0.0)), ("workspace one byte short", dict(short=1))]


@pytest.mark.parametrize("what,change", DBL_REFUSALS, ids=[w for w, _ in DBL_REFUSALS])
def test_bn_double_backward_refusals(dev, what, change):
    K, L = pkg("kernels"), pkg("_lib")
    lib = L.load()
    a = dict(P=6, C=8, Cs=4, eps=1e-3, alpha=0.2, keep=0.75, short=0)
    t = {k: torch.ones((6, 8), device=dev) for k in ("gcb", "d", "y", "gy")}
    t["scb"] = torch.ones((6, 4), device=dev)
    a.update(t)
    a.update(change)
    vec = {k: torch.ones(8, device=dev) for k in ("mean", "var", "gamma")}
    gyb, xcb, gb = (torch.full((6, 8), SENTINEL, device=dev), torch.full((6, 8), SENTINEL, device=dev), torch.full((8,), SENTINEL, device=dev))
    need = int(lib.pnp_bn_dbl_bwd_workspace_bytes(a["P"], a["C"]))
    assert need == (R.dbl_dispatch(a["P"], a["C"])["workspace"] if a["C"] <= 65535 else 0)
    nbytes = need if need else int(lib.pnp_bn_dbl_bwd_workspace_bytes(6, 8))
    ws = K.workspace(nbytes, dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = lib.pnp_bn_dbl_bwd(_vp(a["gcb"]), _vp(a["d"]), _vp(a["y"]), _vp(a["gy"]), _vp(vec["mean"]), _vp(vec["var"]), _vp(vec["gamma"]),
                              _vp(a["scb"]), a["Cs"], _vp(gyb), _vp(xcb), _vp(gb), a["P"], a["C"], a["eps"], a["alpha"], a["keep"], SEED, SID,
                              _vp(ws), nbytes - a["short"], st)
    _refused(L, code, "pnp_bn_dbl_bwd", (gyb, xcb, gb))


# ---- the walker's gscale and keep_prob ---------------------------------------------------------------------------------------------------
def _walk(dev, sd, xa, xb, coef, seed, s0, **kw):
    adv, gp = pkg("adversarial"), pkg("gradient_penalty")
    net = adv.Full_DRN(channels=3, n_class=5, batch_size=2, cost_kwargs={"gp_weight": 10.0}, network_config=dict(NETCFG), device=dev, seed=1)
    net.store.load_state_dict(sd)
    net.store.zero_grad()
    pen, norms, eps, _ = gp.critic_gradient_penalty(net, "mask", xa.to(dev), xb.to(dev), coef, seed, s0, **kw)
    torch.cuda.synchronize()
    grads = {v.name: v.tensor.grad.detach().cpu().clone() for v in net.store.trainable() if v.name.startswith("mask_cls_scope/")}
    return pen.cpu(), norms.cpu(), eps.cpu(), net.store.grad_arena.detach().cpu().clone(), grads


def test_walker_gscale_halves_every_gradient_bit_for_bit(dev, critic_inputs):
    """everything after gp_final_kernel is linear in gscale and a power of two commutes with rounding"""
    sd, ins = critic_inputs
    xa, xb = ins["mask"]
    p1, n1, e1, g1, _ = _walk(dev, sd, xa, xb, 10.0, 21, 40, gscale=1.0)
    p2, n2, e2, g2, _ = _walk(dev, sd, xa, xb, 10.0, 21, 40, gscale=0.5)
    assert torch.equal(e1, e2) and torch.equal(n1, n2) and torch.equal(p1, p2)
    assert float(g1.abs().max()) > 0
    diff = float((g2.double() * 2.0 - g1.double()).abs().max() / g1.double().abs().max())
    print("walker gscale 0.5 against 1.0: 2 g(0.5) - g(1.0) is %.3e of max|g|" % diff)
    assert torch.equal(g2 * 2.0, g1)


def _oracle_penalty_mask(V, xa, xb, eps, coef, seed, sid0, keep):
    """test_gpu_gradient_penalty.oracle_penalty for the mask critic at another keep probability"""
    Vc = {k: (v.detach().clone() if k.endswith(("moving_mean", "moving_variance")) else v) for k, v in V.items()}
    e = eps.to(xa.dtype).view(-1, 1, 1, 1)
    xh = (e * xa + (1 - e) * xb).detach().requires_grad_(True)
    c = nets_adv._Ctx(Vc, keep, seed, critic_keep=keep)
    c.sid = sid0
    f = MIU * nets_adv._mask_critic(c, xh)
    (g,) = torch.autograd.grad(f.sum(), xh, create_graph=True)
    n = g.flatten(1).norm(dim=1)
    return coef * ((n - 1) ** 2).mean(), n.detach()


def test_walker_keep_one_and_gscale_quarter_vs_float64_oracle(dev, critic_inputs):
    sd, ins = critic_inputs
    xa, xb = ins["mask"]
    coef, seed, s0, gs = 10.0, 21, 40, 0.25
    pen, norms, eps, _, g_hip = _walk(dev, sd, xa, xb, coef, seed, s0, gscale=gs, keep_prob=1.0)
    n_units = len(pkg("gradient_penalty").unit_plan("mask")[0])
    assert torch.equal(eps, torch.from_numpy(R.gp_eps(2, seed, s0 + n_units)))          # eps is drawn from stream0 + the number of units
    res = {}
    for dt in (torch.float32, torch.float64):
        V = make_vars(sd, dt, lambda k: k.startswith("mask_cls_scope/"))
        P, n = _oracle_penalty_mask(V, xa.to(dt), xb.to(dt), eps, coef, seed, s0, 1.0)
        names = [k for k in V if V[k].requires_grad]
        gr = torch.autograd.grad(P, [V[k] for k in names], allow_unused=True)
        res[dt] = (P.detach(), n, {k: (g * gs if g is not None else torch.zeros_like(V[k])) for k, g in zip(names, gr)},
                   {k for k, g in zip(names, gr) if g is None})
    P64, n64, g64, unused = res[torch.float64]
    g32 = res[torch.float32][2]
    print("mask keep 1 gscale %.2f: penalty hip %.9g fp64 %.9g | norms hip %s fp64 %s" % (gs, float(pen), float(P64), norms.tolist(), n64.tolist()))
    assert abs(float(pen) - float(P64)) <= 1e-4 * abs(float(P64)) + 1e-9
    assert _rel(norms, n64) < 1e-4
    for k in unused:
        assert float(g_hip[k].abs().max()) == 0.0, k
    grad_report("gp-mask keep 1", {k: g_hip[k] for k in g64 if k not in unused}, {k: v for k, v in g64.items() if k not in unused},
                {k: v for k, v in g32.items() if k not in unused})
