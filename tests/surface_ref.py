"""float64 reference of the surface-distance metrics (surface.py / csrc/surface.hip; medpy.metric.binary semantics, connectivity 1),
written from the definitions: borders by an explicit 6-neighbour check with zero padding, distances by chunked brute-force pairwise
minima between border point sets in physical coordinates, the per-voxel EDT by brute force over the feature points.  Small volumes only.

`pairmin` (optional) replaces the chunked numpy minimum: (points A [n, 3] float64, points B [m, 3] float64) -> min distance per row of A."""
import numpy as np


def border(a):
    """voxels of `a` with one of their 6 face neighbours outside `a` (outside the volume counts as outside)"""
    a = np.asarray(a, dtype=bool)
    p = np.pad(a, 1, constant_values=False)
    c = p[1:-1, 1:-1, 1:-1]
    inner = (c & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return a & ~inner


def _spacing(spacing):
    return np.array([1.0, 1.0, 1.0] if spacing is None else [float(s) for s in spacing], dtype=np.float64)


def pairmin_numpy(pa, pb, chunk=2048):
    out = np.empty(len(pa), dtype=np.float64)
    for i in range(0, len(pa), chunk):
        d2 = ((pa[i:i + chunk, None, :] - pb[None, :, :]) ** 2).sum(-1)
        out[i:i + chunk] = np.sqrt(d2.min(axis=1))
    return out


def sds(a, b, spacing=None, pairmin=None):
    """for each voxel of border(a): the distance to the nearest voxel of border(b), physical units"""
    s = _spacing(spacing)
    pa = np.argwhere(border(a)).astype(np.float64) * s
    pb = np.argwhere(border(b)).astype(np.float64) * s
    return (pairmin or pairmin_numpy)(pa, pb)


def edt_sq(mask, spacing=None, chunk=2048):
    """squared distance of every voxel to the nearest non-zero voxel of `mask` (+inf if there is none)"""
    mask = np.asarray(mask) != 0
    s = _spacing(spacing)
    out = np.full(mask.shape, np.inf)
    feat = np.argwhere(mask).astype(np.float64) * s
    if len(feat) == 0:
        return out
    allp = np.argwhere(np.ones(mask.shape, dtype=bool)).astype(np.float64) * s
    flat = out.reshape(-1)
    for i in range(0, len(allp), chunk):
        flat[i:i + chunk] = ((allp[i:i + chunk, None, :] - feat[None, :, :]) ** 2).sum(-1).min(axis=1)
    return out


def metrics(pred, gt, num_cls, spacing=None, pairmin=None):
    """{field: float64 [num_cls]} with the fields of surface.FIELDS; class 0 NaN, NaN distances for a class empty on either side"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    f = {k: np.full(num_cls, np.nan) for k in ("asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95", "n_border_pred", "n_border_gt")}
    for c in range(1, num_cls):
        P, G = pred == c, gt == c
        f["n_border_pred"][c] = border(P).sum()
        f["n_border_gt"][c] = border(G).sum()
        if not P.any() or not G.any():
            continue
        d_pg, d_gp = sds(P, G, spacing, pairmin), sds(G, P, spacing, pairmin)
        f["asd_pred_gt"][c] = d_pg.mean()
        f["asd_gt_pred"][c] = d_gp.mean()
        f["assd"][c] = np.mean((d_pg.mean(), d_gp.mean()))
        f["hd"][c] = max(d_pg.max(), d_gp.max())
        f["hd95"][c] = np.percentile(np.hstack((d_pg, d_gp)), 95)
    return f


def ellipsoids(shape, num_cls, seed, per_class=2):
    """seeded union of ellipsoids, one label per class (later ones overwrite earlier)"""
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, np.int32)
    g = np.indices(shape).astype(np.float64)
    for c in range(1, num_cls):
        for _ in range(per_class):
            ctr = rng.uniform(0, 1, 3) * np.array(shape)
            rad = rng.uniform(0.08, 0.3, 3) * np.array(shape) + 1.0
            inside = (((g - ctr[:, None, None, None]) / rad[:, None, None, None]) ** 2).sum(0) <= 1.0
            vol[inside] = c
    return vol
