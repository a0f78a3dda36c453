"""Entry point mirroring the reference's train_segmenter.py (same hard-coded config dicts, train_segmenter.py:22-80): trains the
source segmenter.  Extra flags (defaults keep the reference behaviour): --synthetic N writes N synthetic tfrecords and trains on
them, --batch-size, --iters, --epochs, --output; --nii-train LIST --nii-val LIST train from NIfTI volumes kept on the device
(volume_source.py: one `image.nii[.gz] label.nii[.gz]` pair per line; --augment JSON / --no-augment; --sample-mm MM|PI,PJ,FRAME samples them on
a millimetre grid; --prefilter auto|off|SX,SY,SZ low-passes them first; --axes 0,1,2 trains on slices of
every listed orientation; --crop-body [N] crops every volume to its body, found without a label, --crop-margin N to its
label bounding box); --bnd-weight W adds W times the boundary (distance-map) loss of Kervadec et al. to the cost
(default 0 = the reference), --bnd-ramp EPOCHS raises that weight linearly over the first EPOCHS epochs, --bnd-classes 1,3
restricts it to the listed classes (default: every class but the background); --fda-target LIST --fda-beta B|LO,HI --fda-prob P
stylise every training batch with the low-frequency amplitude spectra of target slices (Fourier domain adaptation).  Launched under `python -m torch.distributed.run --nproc-per-node N` it trains data-parallel:
one process per GPU over RCCL, --batch-size slices PER RANK, file lists sharded by rank, rank 0 writes the checkpoint.
  python -m "medical-cross-modality-domain-adaptation_amd.train_segmenter" --synthetic 8 --batch-size 4 --iters 2 --epochs 1
"""
import argparse
import logging
import os

from . import source_segmenter as drn
from .lib import _read_lists
from .parallel import GradReducer, barrier, enable_sync_stats, init_distributed

logging.basicConfig(level=logging.INFO)


NUM_CLS = 5


def parse_args(argv=None):
    """the command line -> (parser, args); the flags of the boundary term are checked here, the volume flags by main()"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=5000)
    ap.add_argument("--output", default="./tmp_exps/mr_baseline")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--sync-stats", action="store_true", help="data parallel only: all-reduce BN statistics and loss normalisers "
                    "(exactly the single-GPU step on the concatenated batch; ~2 tiny collectives per BN layer per pass)")
    ap.add_argument("--restore", action="store_true")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32", help="arithmetic of the convolution operands: f32 = the reference's "
                    "(default); bf16 = BASELINE configs[4]: bf16 MFMA operands, fp32 accumulation / master weights / BN")
    ap.add_argument("--nii-train", default=None, metavar="LIST", help="train from NIfTI volumes resident on the device: a list file with one "
                    "`image.nii[.gz] label.nii[.gz]` pair per line (volume_source.py); needs --nii-val")
    ap.add_argument("--nii-val", default=None, metavar="LIST", help="validation volumes (never augmented)")
    from .volume_source import (add_augment_flags, add_axes_flag, add_prefilter_flag, add_sample_mm_flag, add_sampling_flags, augment_from_args,
                                axes_from_args, prefilter_from_args, sample_mm_from_args, sampling_from_args)
    add_augment_flags(ap)
    add_sample_mm_flag(ap)
    add_prefilter_flag(ap)
    add_axes_flag(ap)
    add_sampling_flags(ap)
    from . import body
    body.add_crop_flags(ap)
    from .fda import add_fda_flags, fda_from_args
    add_fda_flags(ap)
    ap.add_argument("--bnd-weight", type=float, default=0.0, help="weight of the boundary (distance-map) loss of the logits against the "
                    "labels' signed distance maps, computed on the device every step (DESIGN.md §28); default 0 = the reference")
    ap.add_argument("--bnd-ramp", type=int, default=None, metavar="EPOCHS", help="raise --bnd-weight linearly over the first EPOCHS epochs "
                    "(epoch e trains with W * min(1, (e + 1) / EPOCHS)); default: W throughout")
    ap.add_argument("--bnd-classes", default=None, metavar="C,C", help="classes of the boundary loss, e.g. 1,3; default: every class but "
                    "the background")
    args = ap.parse_args(argv)
    if not args.bnd_weight >= 0.0:
        ap.error("--bnd-weight must be >= 0, got %r" % args.bnd_weight)
    if args.bnd_ramp is not None and args.bnd_ramp < 1:
        ap.error("--bnd-ramp must be a positive number of epochs, got %r" % args.bnd_ramp)
    if (args.bnd_ramp is not None or args.bnd_classes is not None) and not args.bnd_weight > 0:
        ap.error("--bnd-ramp and --bnd-classes go with --bnd-weight > 0")
    if args.bnd_classes is not None:
        try:
            args.bnd_classes = tuple(int(c) for c in args.bnd_classes.split(","))
        except ValueError:
            ap.error("--bnd-classes takes class indices separated by commas, got %r" % args.bnd_classes)
        if not args.bnd_classes or not all(0 <= c < NUM_CLS for c in args.bnd_classes):
            ap.error("--bnd-classes must name classes in 0 ... %d, got %r" % (NUM_CLS - 1, args.bnd_classes))
    fda_from_args(ap, args)
    return ap, args


def cost_kwargs_from_args(args):
    """the reference's cost dict (train_segmenter.py:60-66); the keys of the boundary term enter it only when --bnd-weight is > 0"""
    ck = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}
    if args.bnd_weight > 0:
        ck["bnd_weight"] = float(args.bnd_weight)
        if args.bnd_classes is not None:
            ck["bnd_classes"] = tuple(args.bnd_classes)
    return ck


def main(argv=None):
    from .volume_source import augment_from_args, axes_from_args, prefilter_from_args, sample_mm_from_args, sampling_from_args
    from . import body
    ap, args = parse_args(argv)
    crop = body.crop_from_args(ap, args, have_lists=bool(args.nii_train))
    sample_mm = sample_mm_from_args(ap, args)
    prefilter = prefilter_from_args(ap, args)
    axes = axes_from_args(ap, args)
    sampling = sampling_from_args(ap, args)
    if args.foreground is not None and not args.nii_train:
        ap.error("--foreground goes with --nii-train / --nii-val")
    if axes is not None and not args.nii_train:
        ap.error("--axes goes with --nii-train / --nii-val")
    if sample_mm is not None and not args.nii_train:
        ap.error("--sample-mm goes with --nii-train / --nii-val")
    if prefilter is not None and not args.nii_train:
        ap.error("--prefilter goes with --nii-train / --nii-val")
    if (args.nii_train is None) != (args.nii_val is None):
        ap.error("--nii-train and --nii-val go together")
    if args.nii_train and args.synthetic:
        ap.error("--nii-train and --synthetic exclude each other")
    from .functional import set_conv_dtype
    set_conv_dtype(args.dtype)

    train_fid, val_fid = "./lists/mr_train_list", "./lists/mr_val_list"
    output_path = args.output
    num_cls = NUM_CLS
    batch_size = args.batch_size
    training_iters, epochs = args.iters, args.epochs
    checkpoint_space = 1500
    optimizer = 'adam'
    cost_kwargs = cost_kwargs_from_args(args)
    opt_kwargs = {"learning_rate": 1e-3}
    rank, local, world = init_distributed()
    if args.sync_stats:
        enable_sync_stats()
    if os.environ.get("PNP_SAME_DEVICE"):       # test mode: several gloo ranks on one GPU (tests/test_gpu_dp.py)
        local = 0
    device = "cuda:%d" % local if (world > 1 and args.device == "cuda") else args.device
    os.makedirs(output_path, exist_ok=True)

    if args.nii_train:
        from .volume_source import sources_from_lists
        train_list, val_list = sources_from_lists(args.nii_train, args.nii_val, device, batch_size, num_cls, augment=augment_from_args(args),
                                                  shard=(rank, world) if world > 1 else None, sample_mm=sample_mm,
                                                  prefilter=prefilter, axes=axes, sampling=sampling, crop=crop)
    elif args.synthetic:
        from .synthetic import write_dataset
        # next to (not inside) output_path: Trainer.train(restore=False) clears output_path like the reference (source_segmenter.py:416-418)
        data_root = output_path.rstrip("/") + "_data"
        if rank == 0:
            write_dataset(os.path.join(data_root, "synthetic_train"), args.synthetic, seed=0)
            write_dataset(os.path.join(data_root, "synthetic_val"), max(batch_size, args.synthetic // 4), seed=100)
        barrier()
        train_list = _read_lists(os.path.join(data_root, "synthetic_train", "slice_list"))
        val_list = _read_lists(os.path.join(data_root, "synthetic_val", "slice_list"))
    else:
        train_list, val_list = _read_lists(train_fid), _read_lists(val_fid)
        if not train_list:
            raise SystemExit("no training list at %s (use --synthetic N)" % train_fid)

    fda = None
    if args.fda_target:          # the target list is sharded by rank like the training list
        from .fda import FdaStylizer, nifti_target_source
        shard = (rank, world) if world > 1 else None
        if args.nii_train:
            target = nifti_target_source(args.fda_target, device, batch_size, sample_mm=sample_mm, prefilter=prefilter, axes=axes, crop=crop,
                                         shard=shard)
        else:
            target = _read_lists(args.fda_target)
            if not target:
                raise SystemExit("no target slice list at %s" % args.fda_target)
        fda = FdaStylizer(target, beta=args.fda_beta, prob=args.fda_prob, shard=shard)

    net = drn.Full_DRN(channels=3, batch_size=batch_size, n_class=num_cls, cost_kwargs=cost_kwargs, device=device, world_size=world)
    print("Network has been built!")
    trainer = drn.Trainer(net, train_list=train_list, val_list=val_list, num_cls=num_cls, batch_size=batch_size, opt_kwargs=opt_kwargs,
                          checkpoint_space=checkpoint_space, optimizer=optimizer, lr_update_flag=False,
                          reducer=GradReducer(net.store) if world > 1 else None, shard=(rank, world) if world > 1 else None,
                          **({"bnd_ramp": args.bnd_ramp} if args.bnd_weight > 0 and args.bnd_ramp else {}),
                          **({"fda": fda} if fda is not None else {}))
    print("Now start training...")
    try:
        trainer.train(output_path=output_path, training_iters=training_iters, epochs=epochs, restore=args.restore, restored_path=output_path)
    finally:
        if fda is not None:
            fda.close()
    return trainer


if __name__ == "__main__":
    main()
