"""Surface-distance metrics of 3-D label volumes: average surface distance (ASD / ASSD), Hausdorff distance (HD) and its 95th
percentile (HD95) with the semantics of `medpy.metric.binary` (connectivity 1), which SIFA's evaluate.py — the evaluation the reference's
README points to — uses next to Dice.  medpy is not available to this package; every distance comes from libpnp_hip.so
(csrc/surface.hip) and the host does only bookkeeping: sum / n, the mean of the two ASDs, the larger of the two maxima.

For a label volume V [X, Y, Z] (array axis order of nifti.load), spacing s per array axis and class c:
  A = (V == c); a label outside [0, num_cls) is in no class
  border(A)   voxels of A with one of their 6 face neighbours outside A (outside the volume counts as outside A)
  sds(A->B)   for each voxel of border(A), the Euclidean distance (physical units) to the nearest voxel of border(B)
  asd(A, B)   mean sds(A->B);  assd = (asd(P, G) + asd(G, P)) / 2;  hd = max over both directions
  hd95        numpy.percentile(hstack(sds(P->G), sds(G->P)), 95)
Class 0 (background) is not a structure: its entries are NaN.  A class that is empty in the prediction or in the ground truth has NaN
distances; its border counts are still reported.
"""
import numpy as np
import torch

from . import _lib
from . import kernels as K

FIELDS = ("asd_pred_gt", "asd_gt_pred", "assd", "hd", "hd95", "n_border_pred", "n_border_gt")


def spacing_of(affine):
    """voxel spacing per array axis of a NIfTI affine: the column norms of affine[:3, :3] (the zooms nifti.save writes)"""
    a = np.asarray(affine, dtype=np.float64)
    return tuple(float(v) for v in np.sqrt((a[:3, :3] ** 2).sum(axis=0)))


def _spacing(spacing):
    if spacing is None:
        return (1.0, 1.0, 1.0)
    if np.isscalar(spacing):
        return (float(spacing),) * 3
    s = tuple(float(v) for v in spacing)
    if len(s) != 3:
        raise ValueError("spacing: one value per array axis (3) expected, got %r" % (spacing,))
    return s


def _host_labels(x, what):
    """numpy label volume -> contiguous int32 (labels outside the int32 range become -1: in no class); non-integer values raise"""
    a = np.asarray(x)
    if a.ndim != 3:
        raise ValueError("%s: a 3-D label volume expected, got shape %s" % (what, a.shape))
    if a.dtype.kind == "b":
        return np.ascontiguousarray(a, dtype=np.int32)
    if a.dtype.kind == "f":
        if not np.all(np.isfinite(a)) or not np.all(a == np.floor(a)):
            raise ValueError("%s: labels must be integer-valued" % what)
    elif a.dtype.kind not in "iu":
        raise ValueError("%s: labels must be integer-valued, got dtype %s" % (what, a.dtype))
    info = np.iinfo(np.int32)
    out = np.where((a < info.min) | (a > info.max), -1, a) if a.size and (a.min() < info.min or a.max() > info.max) else a
    return np.ascontiguousarray(out, dtype=np.int32)


def _device_labels(pred, gt):
    """both volumes as int32 CUDA tensors.  CUDA tensors are used as they are (int32, contiguous: kernels.surface_distances checks);
    a CPU tensor raises PnpError (no CPU fallback); numpy arrays are checked on the host, then copied to the current device."""
    for t in (pred, gt):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise _lib.PnpError("surface_metrics: pnp kernels need CUDA/HIP tensors (got a CPU tensor) — there is no CPU fallback")
    for t, what in ((pred, "prediction"), (gt, "ground truth")):
        if isinstance(t, torch.Tensor) and (t.is_floating_point() or t.is_complex()):
            raise ValueError("surface_metrics: %s labels must have an integer dtype, got %s" % (what, t.dtype))
    hp = None if isinstance(pred, torch.Tensor) else _host_labels(pred, "prediction")
    hg = None if isinstance(gt, torch.Tensor) else _host_labels(gt, "ground truth")
    dev = pred.device if isinstance(pred, torch.Tensor) else gt.device if isinstance(gt, torch.Tensor) else \
        torch.device("cuda", torch.cuda.current_device())
    dp = pred if hp is None else torch.from_numpy(hp).to(dev)
    dg = gt if hg is None else torch.from_numpy(hg).to(dev)
    return dp, dg


def rows_to_metrics(rows):
    """[num_cls, 7] rows of pnp_surface_distances (host float64) -> {field: per-class float64 array}"""
    rows = np.asarray(rows, dtype=np.float64)
    n_p, n_g = rows[:, 0], rows[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        asd_pg = rows[:, 2] / n_p
        asd_gp = rows[:, 3] / n_g
        assd = (asd_pg + asd_gp) / 2.0
    return {"asd_pred_gt": asd_pg, "asd_gt_pred": asd_gp, "assd": assd, "hd": np.maximum(rows[:, 4], rows[:, 5]), "hd95": rows[:, 6].copy(),
            "n_border_pred": n_p.copy(), "n_border_gt": n_g.copy()}


def surface_metrics(pred, gt, num_cls, spacing=None):
    """per-class surface distances of a predicted and a ground-truth label volume [X, Y, Z] (numpy arrays or int32 CUDA tensors).
    spacing: per array axis; None = voxel units (medpy's default).  -> {field: float64 array [num_cls]} for the FIELDS; row 0 is NaN."""
    s = _spacing(spacing)
    dp, dg = _device_labels(pred, gt)
    rows = K.surface_distances(dp, dg, int(num_cls), s)
    return rows_to_metrics(rows.cpu().numpy())


# ---- medpy.metric.binary-shaped wrappers of binary masks ------------------------------------------------------------------------------
def _binary(result, reference, voxelspacing, connectivity):
    if connectivity != 1:
        raise ValueError("connectivity %r: only 1 (6 face neighbours) is supported" % (connectivity,))
    bits = []
    for t in (result, reference):
        if isinstance(t, torch.Tensor):
            bits.append(t)                         # a CUDA int32 0/1 mask (a CPU tensor raises PnpError in surface_metrics)
        else:
            bits.append(np.asarray(t).astype(bool))
    m = surface_metrics(bits[0], bits[1], 2, voxelspacing)
    if not m["n_border_pred"][1] > 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not m["n_border_gt"][1] > 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return m


def asd(result, reference, voxelspacing=None, connectivity=1):
    """medpy.metric.binary.asd: mean distance from the border of `result` to the border of `reference`"""
    return float(_binary(result, reference, voxelspacing, connectivity)["asd_pred_gt"][1])


def assd(result, reference, voxelspacing=None, connectivity=1):
    """medpy.metric.binary.assd: mean of asd(result, reference) and asd(reference, result)"""
    return float(_binary(result, reference, voxelspacing, connectivity)["assd"][1])


def hd(result, reference, voxelspacing=None, connectivity=1):
    """medpy.metric.binary.hd: Hausdorff distance (the larger of the two directed maxima)"""
    return float(_binary(result, reference, voxelspacing, connectivity)["hd"][1])


def hd95(result, reference, voxelspacing=None, connectivity=1):
    """medpy.metric.binary.hd95: 95th percentile of the pooled distances of both directions"""
    return float(_binary(result, reference, voxelspacing, connectivity)["hd95"][1])


# ---- per-subject bookkeeping of the trainers' test_eval -------------------------------------------------------------------------------
class SurfaceLog(object):
    """collects surface_metrics per subject for Trainer.test_eval(surface=True): rows for surface.csv (one per subject x organ, organ
    names from contour_map) and a per-organ mean +- std over the subjects whose metrics are defined"""
    HEADER = "subject,organ,label,n_border_pred,n_border_gt,asd_pred_gt,asd_gt_pred,assd,hd,hd95"

    def __init__(self, num_cls, contour_map, spacing_mode="unit"):
        if spacing_mode not in ("unit", "header"):
            raise ValueError("spacing must be 'unit' or 'header', got %r" % (spacing_mode,))
        self.num_cls = num_cls
        self.organs = sorted(((int(i), o) for o, i in contour_map.items() if 0 < int(i) < num_cls))
        self.spacing_mode = spacing_mode
        self.entries = []

    def add(self, subject, pred, gt, label_fid=None):
        spacing = None
        if self.spacing_mode == "header":
            from .lib import read_nii_object
            spacing = spacing_of(read_nii_object(label_fid).get_affine())
        m = surface_metrics(pred, gt, self.num_cls, spacing)
        m["subject"] = subject
        m["spacing"] = spacing if spacing is not None else (1.0, 1.0, 1.0)
        self.entries.append(m)
        return m

    def csv_lines(self):
        out = [self.HEADER]
        for m in self.entries:
            for ind, organ in self.organs:
                vals = [m["n_border_pred"][ind], m["n_border_gt"][ind], m["asd_pred_gt"][ind], m["asd_gt_pred"][ind], m["assd"][ind],
                        m["hd"][ind], m["hd95"][ind]]
                out.append(",".join([m["subject"], organ, str(ind)] + ["%d" % v if f.startswith("n_") else repr(float(v))
                                                                       for f, v in zip(FIELDS[5:] + FIELDS[:5], vals)]))
        return out

    def write_csv(self, path):
        with open(path, "w") as f:
            f.write("\n".join(self.csv_lines()) + "\n")
        return path

    def summary(self):
        """{organ: {assd_mean, assd_std, hd95_mean, hd95_std, defined, undefined}} over the subjects"""
        res = {}
        for ind, organ in self.organs:
            a = np.array([m["assd"][ind] for m in self.entries])
            h = np.array([m["hd95"][ind] for m in self.entries])
            ok = np.isfinite(a)
            res[organ] = {"assd_mean": float(np.mean(a[ok])) if ok.any() else float("nan"),
                          "assd_std": float(np.std(a[ok])) if ok.any() else float("nan"),
                          "hd95_mean": float(np.mean(h[ok])) if ok.any() else float("nan"),
                          "hd95_std": float(np.std(h[ok])) if ok.any() else float("nan"),
                          "defined": int(ok.sum()), "undefined": int((~ok).sum())}
        return res

    def print_summary(self):
        print("------- surface distances (%s spacing), mean +- std over subjects ------- " % self.spacing_mode)
        for organ, r in self.summary().items():
            print("organ: %s  assd: %.4f +- %.4f  hd95: %.4f +- %.4f  (%d subjects, %d undefined left out)" % (
                organ, r["assd_mean"], r["assd_std"], r["hd95_mean"], r["hd95_std"], r["defined"], r["undefined"]))
