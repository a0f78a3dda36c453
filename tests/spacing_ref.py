"""float64 numpy restatements of the millimetre-grid sampling — the reference of tests/test_gpu_spacing.py, pinned on the
host in tests/test_spacing_host.py.  Built on augment_ref / paste_ref, which it does not change (the ensemble's bounds stay ensemble_ref's).

  compose_mm(...)                    the plane map s = c_src + S^-1 (t_mm + (1 / scale) R F P (p - c_out)) from 2 x 2 matrices, unrounded
  frame_positions(frame, dz, Z)      the clamped frame coordinates of channels 0 and 2, from the float32 dz the kernel gets
  frame_at(vol, zf)                  [X, Y] float64: the volume interpolated linearly between the two frames around zf
  gather_image_z(...)                z-lerp first, then augment_ref.gather_image's bilinear-with-fill on the three resulting frames
  z_eps / frame_gap / image_bound    the terms of the image bound (restated at image_bound)
  covered / border_margin            pnp_paste_*_fov's coverage rule in float64, and the distance of the nearest coordinate to its border
  GEOMETRIES                         the five field-of-view cases of the paste tests
"""
import math

import numpy as np

import augment_ref as A
import paste_ref as P

U = 2.0 ** -24


def compose_mm(src_xy, out_hw, spacing_xy, pixel_mm, rotate=0.0, scale=1.0, translate=(0.0, 0.0), flip=False):
    """six float64 entries, from the matrices of the formula (volume_source.compose_matrix composes the entries one by one)"""
    X, Y = src_xy
    H, W = out_hw
    r = math.radians(rotate)
    R = np.array([[math.cos(r), -math.sin(r)], [math.sin(r), math.cos(r)]])
    F = np.diag([1.0, -1.0 if flip else 1.0])
    Pm = np.diag([float(pixel_mm[0]), float(pixel_mm[1])])
    Sinv = np.diag([1.0 / float(spacing_xy[0]), 1.0 / float(spacing_xy[1])])
    A2 = Sinv @ (R @ F @ Pm) / float(scale)
    c_src = np.array([(X - 1) / 2.0, (Y - 1) / 2.0])
    c_out = np.array([(H - 1) / 2.0, (W - 1) / 2.0])
    t = c_src + Sinv @ np.asarray(translate, dtype=np.float64) - A2 @ c_out
    return np.array([A2[0, 0], A2[0, 1], t[0], A2[1, 0], A2[1, 1], t[1]])


def frame_positions(frame, dz, Z):
    """(zf of channel 0, zf of channel 2) in float64: frame -+ dz clamped into [0, Z - 1], dz being the float32 the record holds"""
    dz = float(np.float32(dz))
    return min(max(frame - dz, 0.0), Z - 1.0), min(max(frame + dz, 0.0), Z - 1.0)


def frame_at(vol, zf):
    v = np.asarray(vol, dtype=np.float64)
    Z = v.shape[2]
    z0 = int(math.floor(zf))
    z1 = min(z0 + 1, Z - 1)
    t = zf - z0
    return v[:, :, z0] + t * (v[:, :, z1] - v[:, :, z0])


def frames_of(vol, frame, dz):
    """[X, Y, 3] float64: what the three channels read before the in-plane interpolation"""
    v = np.asarray(vol, dtype=np.float64)
    lo, hi = frame_positions(frame, dz, v.shape[2])
    return np.stack([frame_at(v, lo), v[:, :, frame], frame_at(v, hi)], axis=-1)


def gather_image_z(vol, frame, dz, sx, sy, fill):
    """[H, W, 3]: pnp_aug_slices_z's image of one sample"""
    return A.gather_image(frames_of(vol, frame, dz), 1, sx, sy, fill)


def z_eps(Z):
    """4 float32 ulps at the largest frame coordinate that is not clamped away (the subtraction / addition rounds once: half an ulp)"""
    return 4.0 * float(np.spacing(np.float32(max(Z - 1, 1))))


def frame_gap(vol):
    """the largest absolute difference between voxels adjacent along z"""
    v = np.asarray(vol, dtype=np.float64)
    return float(np.abs(np.diff(v, axis=2)).max()) if v.shape[2] > 1 else 0.0


def image_bound(vol, fill, ms, H, W):
    """|got - ref| <= eps (Gx + Gy) + 4 u max|v|        (augment_ref's: §13)
                     + eps_z Gz + 4 u max|v|           (the z term)
    z term: the lerp is Lipschitz in zf with the largest gap between adjacent frames as its constant, and zf carries the one rounding of
    (float)frame -+ dz (z_eps has margin); the lerp itself rounds v[z1] - v[z0] (<= 2 u max|v| after the product with t <= 1) and the
    fmaf (u max|v|): 3 u max|v| <= 4 u max|v|.  Both enter the bilinear chain with weights that sum to 1.  The in-plane gaps of the
    lerped frames are no larger than those of the volume (a convex combination of frames), so Gx, Gy of the volume hold."""
    v = np.asarray(vol, dtype=np.float64)
    Gx, Gy = A.adjacent_gap(v, fill)
    top = max(float(np.abs(v).max()), abs(float(fill)))
    return A.coord_eps(ms, H, W) * (Gx + Gy) + 4 * U * top + z_eps(v.shape[2]) * frame_gap(v) + 4 * U * top


# ---- the field of view -----------------------------------------------------------------------------------------------------------------
def covered(invs, X, Y, H, W):
    """[X, Y] bool: the columns whose unclamped plane coordinates lie in [-0.5, H - 0.5] x [-0.5, W - 0.5] for EVERY map (float64 of the
    float32 entries the kernel gets)"""
    invs = np.asarray(invs, dtype=np.float32).reshape(-1, 6)
    ok = np.ones((X, Y), dtype=bool)
    for inv in invs:
        pi, pj = P.coords(inv, X, Y)
        ok &= (pi >= -0.5) & (pi <= H - 0.5) & (pj >= -0.5) & (pj <= W - 0.5)
    return ok


def border_margin(invs, X, Y, H, W):
    """the smallest distance, in plane pixels, of any column's coordinate to a coverage border: the exact comparison of the written set
    needs it far above the float32 coordinate error (paste_ref.coord_eps)"""
    invs = np.asarray(invs, dtype=np.float32).reshape(-1, 6)
    best = np.inf
    for inv in invs:
        pi, pj = P.coords(inv, X, Y)
        best = min(best, float(np.abs(pi + 0.5).min()), float(np.abs(pi - (H - 0.5)).min()),
                   float(np.abs(pj + 0.5).min()), float(np.abs(pj - (W - 0.5)).min()))
    return best


#              (X, Y)   spacing (mm)  pixel (mm)   (H, W)    compose_matrix keywords                     margin (px)  coverage
GEOMETRIES = {1: ((23, 19), (0.7, 1.3), (1.0, 1.0), (16, 16), {}, 0.20, 0.68),
              2: ((23, 19), (0.7, 1.3), (1.0, 1.0), (16, 16), {"rotate": 7.5}, 0.0074, 0.62),
              3: ((37, 41), (0.35, 0.35), (1.0, 1.0), (12, 12), {}, 0.05, 0.81),
              4: ((9, 11), (2.0, 1.5), (1.0, 1.0), (24, 24), {}, 4.0, 1.00),
              5: ((23, 19), (0.7, 1.3), (1.25, 0.8), (16, 20), {"flip": True, "scale": 1.1, "translate": (1.5, -2.0)}, 0.096, 0.60)}


def smooth_plane_logits(B, H, W, ncls, seed):
    """[B, H, W, ncls] float32, smooth like ensemble_ref.smooth_logits (a coarse normal grid upsampled bilinearly, max|logit| = 10)"""
    h, w = max(2, H // 4), max(2, W // 4)
    coarse = np.random.default_rng(seed).standard_normal((B, h, w, ncls))
    pi, pj = np.meshgrid(np.linspace(0, h - 1, H), np.linspace(0, w - 1, W), indexing="ij")
    up = np.stack([P.interpolate(coarse[b], pi, pj) for b in range(B)])
    return (up * (10.0 / np.abs(up).max())).astype(np.float32)

