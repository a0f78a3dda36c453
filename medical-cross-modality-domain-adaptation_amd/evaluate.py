"""Volume evaluation from NIfTI files — the drop-in for SIFA's evaluate.py, which the reference's README points to for scoring: per-organ
3-D Dice and surface distances (ASSD, HD95; surface.py) as mean +- std over the subjects.

    python -m "medical-cross-modality-domain-adaptation_amd.evaluate" --pred a.nii.gz b.nii.gz --gt ga.nii.gz gb.nii.gz
    python -m "medical-cross-modality-domain-adaptation_amd.evaluate" --pred-dir OUT/test_pred [--num-cls 5] [--spacing unit|header]
                                                                       [--json result.json]
                                                                       [--keep-largest [K]] [--min-size N] [--connectivity 1|2|3]
                                                                       [--fill-holes [MAX]] [--fill-classes C,C]

--pred-dir takes the `dense_pred_*` / `gth_dense_pred_*` pairs that Trainer.test_eval(save_result=True) writes.  3-D Dice runs on the
existing kernels (label_decomp -> confusion_matrix -> lib._dice); every distance comes from csrc/surface.hip.  Subjects whose surface
distance is undefined for an organ (the organ is empty on one side) are left out of that organ's mean and counted.

--keep-largest / --min-size / --connectivity (components.py) filter every PREDICTION on the device before it is scored (the
ground truth is left alone), so one output folder can be scored with and without the filter; the JSON records the options and, per
subject, the filter's stats rows.  --fill-holes [MAX] / --fill-classes C,C then fill the enclosed background holes of the
prediction, after the component filter; the JSON records these options and per subject the fill's stats rows likewise.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

from . import kernels as K
from . import lib
from .source_segmenter import contour_map
from .surface import SurfaceLog, spacing_of


def pairs_of_dir(pred_dir):
    """[(prediction, ground truth)] of the dense_pred_* / gth_dense_pred_* files of a test_eval output folder"""
    out = []
    for p in sorted(glob.glob(os.path.join(pred_dir, "dense_pred_*"))):
        g = os.path.join(os.path.dirname(p), "gth_" + os.path.basename(p))
        if not os.path.isfile(g):
            raise FileNotFoundError("no ground truth %s for %s" % (g, p))
        out.append((p, g))
    if not out:
        raise FileNotFoundError("no dense_pred_* files in %s" % pred_dir)
    return out


def dice_3d(pred, gt, num_cls, device):
    """per-class 3-D Dice of two label volumes on the device: one-hot ground truth (pnp_label_decomp), confusion matrix
    (pnp_confusion_matrix), Dice from the matrix (lib._dice)"""
    y = K.label_decomp(torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).to(device), num_cls)
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int64)).to(device)
    _, cm = K.confusion_matrix(y.view(-1, num_cls), p.view(-1), want_compact=False)
    return lib._dice(cm.cpu().numpy())


def evaluate(pairs, num_cls=5, spacing="unit", device=None, keep_largest=None, fill_holes=None):
    """-> {"subjects": [...], "organs": {organ: {dice_mean, dice_std, assd_mean, assd_std, hd95_mean, hd95_std, defined, undefined}}}
    keep_largest: None, an int K or a dict of components.keep_largest's keywords — every prediction is filtered on the device before it is
    scored; the result then carries "keep_largest" (the options) and per subject "component_stats" ([num_cls][4])
    fill_holes: None, True, a size limit or a dict of components.fill_holes' keywords — the holes of every prediction are filled on the
    device, after the component filter; the result then carries "fill_holes" (the options) and per subject "hole_stats" ([num_cls][4])"""
    from . import components
    post = components.parse_option(keep_largest, num_cls)
    fill = components.parse_fill_option(fill_holes, num_cls)
    device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    slog = SurfaceLog(num_cls, contour_map, spacing)
    subjects = []
    for pf, gf in pairs:
        pred = np.asarray(lib.read_nii_image(pf))
        gt_obj = lib.read_nii_object(gf)
        gt = np.asarray(gt_obj.get_data())
        if pred.shape != gt.shape:
            raise ValueError("%s %s and %s %s differ in shape" % (pf, pred.shape, gf, gt.shape))
        cstats = hstats = None
        if post is not None or fill is not None:
            if pred.ndim != 3 or pred.min() < 0 or pred.max() > 255 or np.any(pred != np.floor(pred)):
                raise ValueError("%s: the component filter takes a 3-D volume of integer labels in [0, 255]" % pf)
            filt = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.uint8)).to(device)
            if post is not None:
                filt, st = components.keep_largest(filt, num_cls=num_cls, **post)
                cstats = st.cpu().tolist()
            if fill is not None:
                filt, st = components.fill_holes(filt, num_cls=num_cls, out=filt, **fill)
                hstats = st.cpu().tolist()
            pred = filt.cpu().numpy()
        dice = dice_3d(pred, gt, num_cls, device)
        m = slog.add(os.path.basename(pf), pred, gt, gf)
        subjects.append({"pred": pf, "gt": gf, "spacing": list(m["spacing"]), "dice": dice.tolist(),
                         **{k: [None if not np.isfinite(v) else float(v) for v in m[k]] for k in ("assd", "hd95", "asd_pred_gt", "asd_gt_pred", "hd")},
                         "n_border_pred": [None if not np.isfinite(v) else int(v) for v in m["n_border_pred"]],
                         "n_border_gt": [None if not np.isfinite(v) else int(v) for v in m["n_border_gt"]]})
        if cstats is not None:
            subjects[-1]["component_stats"] = cstats
        if hstats is not None:
            subjects[-1]["hole_stats"] = hstats
    organs = slog.summary()
    for ind, organ in slog.organs:
        d = np.array([s["dice"][ind] for s in subjects])
        organs[organ]["dice_mean"], organs[organ]["dice_std"] = float(np.mean(d)), float(np.std(d))
    res = {"num_cls": num_cls, "spacing": spacing, "subjects": subjects, "organs": organs}
    if post is not None:
        res["keep_largest"] = post
    if fill is not None:
        res["fill_holes"] = fill
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pred", nargs="+", help="predicted label volumes (.nii / .nii.gz)")
    ap.add_argument("--gt", nargs="+", help="ground-truth label volumes, in the order of --pred")
    ap.add_argument("--pred-dir", help="a test_eval output folder with dense_pred_* / gth_dense_pred_* pairs")
    ap.add_argument("--num-cls", type=int, default=5)
    ap.add_argument("--spacing", choices=("unit", "header"), default="unit", help="voxel units, or the ground truth's NIfTI zooms")
    ap.add_argument("--json", help="write the full result here")
    from . import components
    components.add_cli_arguments(ap)
    a = ap.parse_args(argv)
    post = components.cli_option(ap, a, a.num_cls)
    fill = components.cli_fill_option(ap, a, a.num_cls)
    if a.pred_dir:
        if a.pred or a.gt:
            ap.error("--pred-dir excludes --pred / --gt")
        pairs = pairs_of_dir(a.pred_dir)
    else:
        if not a.pred or not a.gt or len(a.pred) != len(a.gt):
            ap.error("--pred and --gt need the same number of files (or use --pred-dir)")
        pairs = list(zip(a.pred, a.gt))
    res = evaluate(pairs, a.num_cls, a.spacing, keep_largest=post, fill_holes=fill)
    print("%d subjects, %s spacing" % (len(pairs), a.spacing))
    if post is not None:
        print("predictions filtered: %s" % ", ".join("%s %s" % kv for kv in sorted(post.items())))
        for s in res["subjects"]:
            print("  %s  %s" % (os.path.basename(s["pred"]), components.stats_line(s["component_stats"])))
    if fill is not None:
        print("holes filled: %s" % (", ".join("%s %s" % kv for kv in sorted(fill.items())) or "of any size, every class"))
        for s in res["subjects"]:
            print("  %s  %s" % (os.path.basename(s["pred"]), components.fill_stats_line(s["hole_stats"])))
    for organ, r in res["organs"].items():
        print("%-9s dice %.4f +- %.4f   assd %.4f +- %.4f   hd95 %.4f +- %.4f   (%d undefined)" % (
            organ, r["dice_mean"], r["dice_std"], r["assd_mean"], r["assd_std"], r["hd95_mean"], r["hd95_std"], r["undefined"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
