"""References and dispatch facts of csrc/critic_gp.hip for tests/test_gpu_gp_domain.py and tests/test_gp_ref_host.py (no GPU needed):
(a) the per-sample uniform of pnp_gp_interpolate restated in numpy; (b) float64 references of the interpolation, of the penalty (norms,
value, adjoint) and of the BN double backward — once through torch autograd, once as the closed form of the kernel file's comment;
(c) the same closed form run in float32 (the yardstick of the hard-operand bar: the reference's arithmetic at the kernels' precision);
(d) dbl_dispatch / gp_dispatch, the launch arithmetic of pnp_bn_dbl_bwd and of pnp_gp_interpolate / pnp_gp_penalty in Python.
Every tensor function runs on whichever device its operands live on."""
import numpy as np
import torch

from oracle import tf_ops as T

NT = 256               # threads per workgroup of every kernel of the file
GP_BLOCKS = 64         # partial sums per sample of the norm reduction
DBL_SUMS, DBL_COEF = 5, 8
GRID_CAP = 2048        # row slabs of the reduction / workgroups of the apply grid


# ---- (a) eps ---------------------------------------------------------------------------------------------------------------------------
def gp_eps(B, seed, stream_id):
    """gp_uniform: 24 bits of fmix32((i * 0xCC9E2D51) ^ key(seed, stream id)) times 2^-24 -> float32 [B] (exact: 24 bits fit the mantissa)"""
    with np.errstate(over="ignore"):
        i = np.arange(B, dtype=np.uint32)
        h = T._fmix32((i * np.uint32(0xCC9E2D51)) ^ T.drop_key(seed, stream_id))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---- (b) float64 references ------------------------------------------------------------------------------------------------------------
def interp_terms(a, b, eps):
    """eps_i * a and (1 - eps_i) * b in float64, [B, n] (their sum is the reference, the sum of their magnitudes scales its bound)"""
    B = a.shape[0]
    e = eps.double().view(B, 1)
    return e * a.double().reshape(B, -1), (1.0 - e) * b.double().reshape(B, -1)


def penalty_ref(g, coef, gscale):
    """g [B, ...] -> (norms [B], penalty, gscale * dP/dg [B, n]) in float64, P = coef * mean_i (|g_i| - 1)^2; a sample of norm 0 has no
    direction: its adjoint is exactly zero"""
    B = g.shape[0]
    g = g.double().reshape(B, -1)
    nrm = (g * g).sum(dim=1).sqrt()
    pen = float(coef) * ((nrm - 1.0) ** 2).mean()
    safe = torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    k = torch.where(nrm > 0, float(coef) * float(gscale) * 2.0 / B * (nrm - 1.0) / safe, torch.zeros_like(nrm))
    return nrm, pen, k.view(B, 1) * g


def _f32(v):
    return float(np.float32(v))


def _slope(y, gy, alpha, dtype):
    """leaky'(z) read from the sign of the y the kernel is given (slope alpha at y == +-0); alpha < 0: no activation"""
    if alpha < 0:
        return torch.ones_like(gy, dtype=dtype)
    one = torch.ones((), dtype=dtype, device=gy.device)
    return torch.where(y > 0, one, one * _f32(alpha)).to(dtype)


def bn_dbl_closed(gcb, d, y, gy, mean, var, gamma, scb, eps, alpha, keep, mask, dtype=torch.float64):
    """the closed form of csrc/critic_gp.hip (comment above DblArgs) on [P, C] operands in `dtype`:
        v = gcb * mask / keep, g_z = g_y * leaky'(z), m_* the per-channel means over the P rows, sigma = sqrt(var + eps)
        gzb = (gamma/sigma) (v - m_v - xhat m_vx) [+ pad(scb)], gyb = gzb * leaky'(z)
        gamma_bar = P (m_vg - m_v m_g - m_vx m_gx) / sigma
        xd = -(gamma/sigma^2) [xhat (m_vg - m_v m_g - 3 m_vx m_gx) + m_gx (v - m_v) + m_vx (g_z - m_g)], xcb = xd * mask / keep
    mean / var are the float32 tensors the kernel reads; mask is a {0, 1} tensor or None (keep = 1).  -> (gyb, xcb, gamma_bar)"""
    C = d.shape[-1]
    P = d.numel() // C
    c = lambda t: t.to(dtype).reshape(P, -1)
    gcb, d_, gy_ = c(gcb), c(d), c(gy)
    lk = _slope(y.reshape(P, C) if y is not None else None, gy_, alpha, dtype)
    kp = _f32(keep)
    mk = c(mask) if mask is not None else None
    sig2 = var.to(dtype) + _f32(eps)
    sig = sig2.sqrt()
    ga = gamma.to(dtype)
    xh = (d_ - mean.to(dtype)) / sig
    gz = gy_ * lk
    v = gcb * mk / kp if mk is not None else gcb
    m_v, m_vx, m_vg, m_g, m_gx = v.mean(0), (v * xh).mean(0), (v * gz).mean(0), gz.mean(0), (gz * xh).mean(0)
    gzb = (ga / sig) * (v - m_v - xh * m_vx)
    if scb is not None:
        Cs = scb.shape[-1]
        c0 = (C - Cs) // 2
        gzb = torch.cat([gzb[:, :c0], gzb[:, c0:c0 + Cs] + c(scb), gzb[:, c0 + Cs:]], dim=1)
    gyb = gzb * lk
    gbar = P * (m_vg - m_v * m_g - m_vx * m_gx) / sig
    xd = -(ga / sig2) * (xh * (m_vg - m_v * m_g - 3.0 * m_vx * m_gx) + m_gx * (v - m_v) + m_vx * (gz - m_g))
    xcb = xd * mk / kp if mk is not None else xd
    return gyb, xcb, gbar


def bn_dbl_autograd(gcb, d, y, gy, mean, var, gamma, scb, eps, alpha, keep, mask):
    """float64, by torch autograd: L = <gcb, g_c> + <scb, crop(g_z)> with g_z = g_y * leaky'(z), g_d = d(BN(d))/d(d)^T g_z taken with
    create_graph=True, g_c = g_d * mask / keep; -> dL/d(g_y), dL/d(d) * mask / keep, dL/d(gamma).  The statistics are functions of d whose
    VALUES are the float32 mean / var the kernel reads (a constant offset is added to each), the slope comes from the given y."""
    C = d.shape[-1]
    P = d.numel() // C
    c = lambda t: t.double().reshape(P, -1)
    d64, gy64, ga64 = c(d).requires_grad_(True), c(gy).requires_grad_(True), gamma.double().clone().requires_grad_(True)
    lk = _slope(y.reshape(P, C) if y is not None else None, gy64, alpha, torch.float64).detach()
    kp = _f32(keep)
    mk = c(mask) if mask is not None else None
    m0 = d64.mean(0)
    v0 = ((d64 - m0) ** 2).mean(0)
    m = m0 + (mean.double() - m0).detach()
    vr = v0 + (var.double() - v0).detach()
    zpre = (d64 - m) * (ga64 / torch.sqrt(vr + _f32(eps)))
    gz = gy64 * lk
    (gd,) = torch.autograd.grad(zpre, d64, grad_outputs=gz, create_graph=True)
    gc = gd * mk / kp if mk is not None else gd
    L = (c(gcb) * gc).sum()
    if scb is not None:
        Cs = scb.shape[-1]
        c0 = (C - Cs) // 2
        L = L + (c(scb) * gz[:, c0:c0 + Cs]).sum()
    r_gy, r_d, r_ga = torch.autograd.grad(L, [gy64, d64, ga64])
    return r_gy, (r_d * mk / kp if mk is not None else r_d), r_ga


# ---- (c) the closed form at the kernels' precision -------------------------------------------------------------------------------------
def bn_dbl_closed_f32(gcb, d, y, gy, mean, var, gamma, scb, eps, alpha, keep, mask):
    """bn_dbl_closed in plain torch float32 throughout (means included)"""
    return bn_dbl_closed(gcb, d, y, gy, mean, var, gamma, scb, eps, alpha, keep, mask, dtype=torch.float32)


# ---- (d) dispatch ----------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def dbl_dispatch(P, C):
    """dbl_plan, group_map and the launch code of pnp_bn_dbl_bwd.  slices: per blockIdx.y (channel groups, rows per pass rpi, idle lanes:
    those with rsub >= rpi)"""
    vec = C % 4 == 0
    CG = C // 4 if vec else C
    ny = _cdiv(CG, NT)
    slices = []
    for s in range(ny):
        cgs = min(CG - s * NT, NT)
        rpi = NT // cgs
        slices.append({"groups": cgs, "rpi": rpi, "idle": NT - rpi * cgs})
    b = min(max(_cdiv(P, 64), 1), GRID_CAP)
    rpb = _cdiv(P, b)
    nblk = _cdiv(P, rpb)
    rpi0 = NT // min(CG, NT)
    cap = max(GRID_CAP // ny, 1)
    bx = max(_cdiv(P, rpi0), 1)
    return {"vector": vec, "ny": ny, "slices": slices, "nblk": nblk, "rows_per_block": rpb, "nblk_capped": _cdiv(P, 64) > GRID_CAP,
            "bx": min(bx, cap), "apply_capped": bx > cap,
            "workspace": _align(nblk * DBL_SUMS * C * 8) + _align(C * DBL_COEF * 4)}


def _align(v):
    return (v + 255) & ~255


def gp_dispatch(B, n):
    """gp_blocks_per_sample and the loops of the four gp_* kernels: the 16-byte path, workgroups per sample of the interpolation and the
    scale kernel, whether their cap of 256 bound, passes of the norm kernel's 64 x 256 lanes, and whether gp_final_kernel's one workgroup
    loops over the samples"""
    vec = n % 4 == 0
    want = max(_cdiv(n // 4, NT * 8), 1)
    return {"vector": vec, "blocks": min(want, 256), "capped": want > 256, "norm_passes": _cdiv(n // 4 if vec else n, GP_BLOCKS * NT),
            "final_loops": B > NT, "workspace": _align(B * GP_BLOCKS * 8) + _align(B * 4)}
