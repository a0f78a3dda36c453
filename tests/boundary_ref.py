"""numpy restatement, in exact integers and float64, of the boundary term of DESIGN.md §28 (kernels.signed_distance_2d and
kernels.boundary_loss): the reference of the kernel tests.

    phi_c = edt(~m_c) * ~m_c - (edt(m_c) - 1) * m_c    (one_hot2dist of the boundary-loss paper's code; edt = distance to the nearest
                                                         zero of its argument), 0 where m_c is empty or full, per slice
    p_i = softmax(z_i),  s_i = sum_k p_ik phi_ik,  L = sum_i s_i / (P nsel),  dL/dz_ij = p_ij (phi_ij - s_i) / (P nsel)

The transform is separable: per row the distance to the nearest member and to the nearest non-member, then per column the minimum of
row distance squared plus row offset squared, all in int64."""
import numpy as np

BIG = 1 << 40      # "no such pixel in this row": above any squared distance, and BIG + 1023^2 fits an int64


def _row_dist(target):
    """target [H, W] bool -> int64 [H, W]: |w - w'| to the nearest w' of the same row with target[h, w'] (0 on a target pixel), BIG for
    a row without one"""
    H, W = target.shape
    idx = np.broadcast_to(np.arange(W, dtype=np.int64), (H, W))
    left = np.maximum.accumulate(np.where(target, idx, -BIG), axis=1)                       # the last target at or before w
    right = np.minimum.accumulate(np.where(target, idx, 2 * BIG)[:, ::-1], axis=1)[:, ::-1]  # the first target at or after w
    return np.minimum(np.minimum(idx - left, right - idx), BIG)


def sq_dist_to(target):
    """target [H, W] bool -> int64 [H, W]: exact squared Euclidean distance to the nearest target pixel (>= BIG: there is none)"""
    H, W = target.shape
    g = _row_dist(target)                                             # [k, w]
    g2 = np.where(g >= BIG, BIG, g * g)
    hh = np.arange(H, dtype=np.int64)
    out = np.empty((H, W), np.int64)
    for h0 in range(0, H, 32):                                        # (blocks of rows: the broadcast is [32, H, W])
        dh2 = (hh[h0:h0 + 32, None] - hh[None, :]) ** 2               # [h, k]
        out[h0:h0 + 32] = (g2[None, :, :] + dh2[:, :, None]).min(axis=1)
    return out


def class_list(classes, ncls):
    return list(range(1, ncls)) if classes is None else [int(c) for c in classes]


def phi_ref(onehot, classes=None):
    """onehot [B, H, W, C] -> (phi float64 [B, H, W, C], d2 int64 [B, H, W, C]).  d2 is the squared distance to the nearest pixel of the
    other membership (0 where phi is 0 by rule: class not selected, absent from the slice or filling it); phi = sqrt(d2) outside the
    class and -(sqrt(d2) - 1) inside it."""
    onehot = np.asarray(onehot)
    B, H, W, C = onehot.shape
    phi = np.zeros((B, H, W, C), np.float64)
    d2 = np.zeros((B, H, W, C), np.int64)
    for c in sorted(set(class_list(classes, C))):
        for b in range(B):
            m = onehot[b, :, :, c] > 0.5
            if not m.any() or m.all():
                continue
            q = np.where(m, sq_dist_to(~m), sq_dist_to(m))
            d2[b, :, :, c] = q
            r = np.sqrt(q.astype(np.float64))
            phi[b, :, :, c] = np.where(m, -(r - 1.0), r)
    return phi, d2


def boundary_ref(z, phi, nsel, coef=1.0):
    """z, phi: [..., C] (computed in float64) -> (L: float, coef * dL/dz: float64 array of z's shape)"""
    z = np.asarray(z, dtype=np.float64)
    q = np.asarray(phi, dtype=np.float64).reshape(-1, z.shape[-1])
    C = z.shape[-1]
    z2 = z.reshape(-1, C)
    P = z2.shape[0]
    if nsel == 0:
        return 0.0, np.zeros_like(z)
    zs = z2 - z2.max(axis=1, keepdims=True)
    e = np.exp(zs)
    p = e / e.sum(axis=1, keepdims=True)
    s = (p * q).sum(axis=1, keepdims=True)
    k = 1.0 / (P * float(nsel))
    grad = k * p * (q - s)
    return float(s.sum() * k), (coef * grad).reshape(z.shape)


# ---- label patterns of the kernel tests ------------------------------------------------------------------------------------------------
def patterns(H, W, rng):
    """{name: bool mask [H, W]} — the membership of ONE class on one slice"""
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"absent": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}
    m = np.zeros((H, W), bool)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    out["corners"] = m
    m = np.zeros((H, W), bool)
    m[0, :] = m[H - 1, :] = True
    m[:, 0] = m[:, W - 1] = True
    out["border"] = m
    out["checker"] = ((yy + xx) % 2) == 0
    rr = ((yy - (H - 1) / 2.0) / max(H / 2.0 - 1.0, 1.0)) ** 2 + ((xx - (W - 1) / 2.0) / max(W / 2.0 - 1.0, 1.0)) ** 2
    out["ring"] = (rr <= 1.0) & (rr >= 0.3)                          # a hole inside the class
    m = np.zeros((H, W), bool)
    bh, bw = max(H // 6, 1), max(W // 6, 1)
    m[:bh, :bw] = True
    m[H - bh:, W - bw:] = True
    out["far_blobs"] = m
    out["random"] = rng.random((H, W)) < 0.3
    return out


def onehot_of_masks(masks, C, c):
    """per-slice bool masks [B, H, W] of class c -> one-hot [B, H, W, C] float32: class c where the mask is set, else the other classes in
    vertical bands (class 0 alone when C == 1 cannot be expressed: then the pixel belongs to no class)"""
    B, H, W = masks.shape
    oh = np.zeros((B, H, W, C), np.float32)
    others = [k for k in range(C) if k != c]
    band = (np.arange(W) * max(len(others), 1) // max(W, 1))
    for b in range(B):
        oh[b, :, :, c] = masks[b]
        for j, k in enumerate(others):
            oh[b, :, :, k] = (~masks[b]) & (band[None, :] == j)
    return oh
