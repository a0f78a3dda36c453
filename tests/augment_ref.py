"""float64 numpy restatements of csrc/augment.hip — the reference of tests/test_gpu_augment.py, pinned to
scipy.ndimage.map_coordinates in tests/test_augment_host.py where scipy is installed.

  preprocess(v, percentile)        clip at the exact order statistic np.partition(v, k)[k], k = (percentile (n - 1) + 99) // 100, then the
                                   z-score with the population std; all zeros when std == 0
  coords(m, H, W)                  source coordinates of every output pixel from the SAME six float32 matrix entries the kernel gets
  gather_image / gather_label      per-corner bilinear with fill (order=1, grid-constant) / floor(s + 0.5) nearest, 0 outside (order=0)
  coord_eps, adjacent_gap          the terms of the image bound |got - ref| <= eps (Gx + Gy) + 4 * 2^-24 max|v|
  label_candidates                 the labels at floor(s + 0.5) for s -+ eps on either axis (at most four)
"""
import numpy as np


def clip_index(n, percentile=98):
    return (int(percentile) * (int(n) - 1) + 99) // 100


def preprocess(v, percentile=98):
    """-> (normalised float64 array of v's shape, {clip, mean, std})"""
    v = np.asarray(v, dtype=np.float32)
    flat = v.ravel()
    k = clip_index(flat.size, percentile)
    clip = np.partition(flat, k)[k]
    c = np.minimum(flat.astype(np.float64), np.float64(clip))
    mean, std = c.mean(), c.std()
    out = np.zeros_like(c) if std == 0 else (c - mean) / std
    return out.reshape(v.shape), {"clip": float(clip), "mean": float(mean), "std": float(std)}


def coords(m, H, W):
    """(sx, sy) [H, W] float64 of the float32 entries m = (m00, m01, m02, m10, m11, m12)"""
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    i = np.arange(H, dtype=np.float64)[:, None]
    j = np.arange(W, dtype=np.float64)[None, :]
    return m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]


def _at(frames, x, y, fill):
    X, Y = frames.shape[:2]
    inside = (x >= 0) & (x < X) & (y >= 0) & (y < Y)
    val = frames[np.clip(x, 0, X - 1), np.clip(y, 0, Y - 1)]
    return np.where(inside[..., None], val, fill)


def gather_image(vol, z, sx, sy, fill):
    """[H, W, 3]: frames z-1, z, z+1 of vol [X, Y, Z], bilinear between the four corners around (sx, sy); a corner outside contributes fill"""
    frames = np.asarray(vol, dtype=np.float64)[:, :, z - 1:z + 2]
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    tx, ty = (sx - x0)[..., None], (sy - y0)[..., None]
    a = _at(frames, x0, y0, fill) * (1 - ty) + _at(frames, x0, y0 + 1, fill) * ty
    b = _at(frames, x0 + 1, y0, fill) * (1 - ty) + _at(frames, x0 + 1, y0 + 1, fill) * ty
    return a * (1 - tx) + b * tx


def gather_label(lab, z, sx, sy):
    """[H, W] float64: the label at (floor(sx + 0.5), floor(sy + 0.5), z), 0 outside"""
    lab = np.asarray(lab)
    X, Y = lab.shape[:2]
    x, y = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
    inside = (x >= 0) & (x < X) & (y >= 0) & (y < Y)
    return np.where(inside, lab[np.clip(x, 0, X - 1), np.clip(y, 0, Y - 1), z], 0).astype(np.float64)


def coord_eps(ms, H, W):
    """4 float32 ulps at the largest coordinate term of the batch (the two fmaf roundings are half an ulp each; the rest is margin)"""
    ms = np.abs(np.asarray(ms, dtype=np.float32).astype(np.float64).reshape(-1, 6))
    t = max(float((ms[:, [0, 3]] * (H - 1)).max()), float((ms[:, [1, 4]] * (W - 1)).max()), float(ms[:, [2, 5]].max()))
    return 4.0 * float(np.spacing(np.float32(t)))


def adjacent_gap(vol, fill):
    """(Gx, Gy): the largest absolute difference between face-adjacent voxels along x and along y, the fill at the border included"""
    v = np.asarray(vol, dtype=np.float64)
    px = np.concatenate([np.full((1,) + v.shape[1:], fill), v, np.full((1,) + v.shape[1:], fill)], axis=0)
    py = np.concatenate([np.full((v.shape[0], 1, v.shape[2]), fill), v, np.full((v.shape[0], 1, v.shape[2]), fill)], axis=1)
    return float(np.abs(np.diff(px, axis=0)).max()), float(np.abs(np.diff(py, axis=1)).max())


def label_candidates(lab, z, sx, sy, eps):
    """[4, H, W]: gather_label at (sx -+ eps, sy -+ eps)"""
    return np.stack([gather_label(lab, z, sx + dx, sy + dy) for dx in (-eps, eps) for dy in (-eps, eps)])


def onehot(label, ncls):
    """the rows of lib._label_decomp: a label >= ncls gives an all-zero row"""
    return (np.asarray(label)[..., None] == np.arange(ncls)).astype(np.float32)
