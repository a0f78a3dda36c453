"""Entry point mirroring the reference's train_gan.py (config dicts and --phase switch, train_gan.py:27-157).
  --phase pre-train : warm up the feature critic (dis only, 1 sub-iteration, lambda_mask_loss = 0, CT front frozen)
  --phase train-gan : joint training (20 dis : 1 gen, lambda_mask_loss = rate, dis_sub_iter += 1 every 300 steps)
  --phase fine-tune : continue from a breakpoint (the reference's `training_config` NameError at train_gan.py:121 is fixed)
Extra flags: --synthetic N, --batch-size, --iters, --epochs, --output, --baseline (source-segmenter .npz for the pre-train hand-off),
--mr-nii-train / --mr-nii-val / --ct-nii-train / --ct-nii-val LIST (all four: train from NIfTI volumes kept on the device,
volume_source.py; the two CT lists may name images alone — unlabelled target scans; --crop-body [N] / --crop-margin N crop
every volume of both domains to its body / label box; --augment JSON / --no-augment; --axes 0,1,2: slices of every listed orientation, one value for MR and CT), --gp-weight L (opt-in WGAN-GP penalty of the critics instead of the +-0.03 weight clip; gradient_penalty.py; default 0 = the reference),
--ent-weight W (opt-in entropy minimisation on the CT predictions in the gen step: gen loss + W * normalised mean entropy, DESIGN.md §27;
default 0 = the reference), --monitor-entropy (log ct_entropy, the label-free monitor, with every Dice report; implied by --ent-weight > 0),
--pl-weight W --pl-portion R --pl-momentum B --pl-init T --pl-classes C,C (opt-in class-balanced pseudo-label self-training on the CT
predictions in the gen step, DESIGN.md §29: gen loss + W * cross-entropy against the arg-max on the pixels whose confidence reaches their
class's threshold; the thresholds follow each batch's per-class R-quantile with momentum B from T; default W = 0 = the reference).
"""
import argparse
import datetime
import logging
import os

import numpy as np

from . import adversarial as drn
from .lib import _read_lists
from .parallel import GradReducer, barrier, enable_sync_stats, init_distributed

logging.basicConfig(level=logging.INFO)
rate = 0.3
date = datetime.datetime.now().strftime('%m%d')

cost_kwargs = {"regularizer": 1e-4, "gan_regularizer": 1e-4, "miu_gen": 0.002, "miu_dis": 0.002, "lambda_mask_loss": None}
opt_kwargs = {"learning_rate": 3e-4}
network_config = {"mr_front_trainable": False, "joint_trainable": False, "ct_front_trainable": None, "cls_trainable": True,
                  "m_cls_trainable": True, "restore_skip_kwd": ["Adam", "RMS", "cls"]}
train_config = {"restore_from_baseline": None, "copy_main": None, "clear_rms": None, "lr_update": None, "dis_interval": 1, "gen_interval": 1,
                "dis_sub_iter": 20, "gen_sub_iter": 1, "tag": "gan-" + str(rate) + "_" + date, "iter_upd_interval": 300, "dis_sub_iter_inc": 1,
                "gen_sub_iter_inc": 0, "lr_decay_factor": 0.98, "checkpoint_space": 100, "training_iters": 200, "epochs": 600}


def configure(phase):
    """train_gan.py:85-126"""
    ck, nc, tc = dict(cost_kwargs), dict(network_config), dict(train_config)
    if phase == 'pre-train':
        nc["ct_front_trainable"] = False
        tc.update(restore_from_baseline=True, copy_main=True, clear_rms=True, lr_update=True, gen_interval=0, dis_sub_iter=1,
                  dis_sub_iter_inc=0, checkpoint_space=2000, training_iters=201, epochs=100)
        ck["lambda_mask_loss"] = 0
    elif phase == 'train-gan':
        nc["ct_front_trainable"] = True
        tc.update(restore_from_baseline=False, copy_main=False, clear_rms=False, lr_update=True, tag=tc["tag"] + "-gan")
        ck["lambda_mask_loss"] = rate
    elif phase == 'fine-tune':
        nc["ct_front_trainable"] = True
        tc.update(restore_from_baseline=False, copy_main=False, clear_rms=False, lr_update=False, gen_interval=1, dis_sub_iter=30,
                  tag=tc["tag"] + "-fine_tune")
        ck["lambda_mask_loss"] = rate
    else:
        raise Exception("Please set a training phase!")
    return ck, nc, tc


NII_FLAGS = ("mr_nii_train", "mr_nii_val", "ct_nii_train", "ct_nii_val")


def parse_args(phase, argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", default=phase)
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=6)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--output", default="./tmp_exps/mr2ct" + date)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--sync-stats", action="store_true", help="data parallel only: all-reduce BN statistics and loss normalisers "
                    "(exactly the single-GPU step on the concatenated batch; ~2 tiny collectives per BN layer per pass)")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32", help="arithmetic of the convolution operands: f32 = the reference's "
                    "(default); bf16 = BASELINE configs[4]: bf16 MFMA operands, fp32 accumulation / master weights / BN")
    ap.add_argument("--gp-weight", type=float, default=0.0, help="WGAN-GP gradient penalty weight of the critics (f = miu_dis * D; 10 = "
                    "the WGAN-GP paper's value); > 0 replaces the +-0.03 weight clip.  fp32, without --sync-stats; default 0")
    ap.add_argument("--ent-weight", type=float, default=0.0, help="weight of the normalised mean entropy of the CT predictions in the "
                    "generator loss (entropy minimisation on the unlabelled target, DESIGN.md §27); default 0 = the reference")
    ap.add_argument("--monitor-entropy", action="store_true", help="log ct_entropy (normalised mean entropy of the CT batch, BN in "
                    "inference mode) next to the Dice monitor and write it to the scalar log; implied by --ent-weight > 0")
    ap.add_argument("--pl-weight", type=float, default=0.0, help="weight of the class-balanced pseudo-label term of the CT predictions in "
                    "the generator loss (self-training on the unlabelled target, DESIGN.md §29); default 0 = the reference")
    ap.add_argument("--pl-portion", type=float, default=0.5, help="portion of each predicted class's pixels, taken from the most confident "
                    "down, that a batch's threshold admits; in (0, 1], default 0.5")
    ap.add_argument("--pl-momentum", type=float, default=0.9, help="momentum of the thresholds: tau <- q + B (tau - q) per gen step; in "
                    "[0, 1], default 0.9")
    ap.add_argument("--pl-init", type=float, default=0.9, help="starting threshold of every class (a checkpoint that holds thresholds "
                    "replaces it); default 0.9")
    ap.add_argument("--pl-classes", default=None, metavar="C,C", help="restrict the pseudo-label term to these classes (default: every "
                    "class, the background included)")
    for flag in NII_FLAGS:
        ap.add_argument("--" + flag.replace("_", "-"), default=None, metavar="LIST", help="NIfTI list file (one `image.nii[.gz] "
                        "label.nii[.gz]` pair per line, volume_source.py); the four --*-nii-* flags go together")
    from .volume_source import (add_augment_flags, add_axes_flag, add_prefilter_flag, add_sample_mm_flag, add_sampling_flags, axes_from_args,
                                prefilter_from_args, sample_mm_from_args, sampling_from_args)
    add_augment_flags(ap)
    add_sample_mm_flag(ap)
    add_prefilter_flag(ap)
    add_axes_flag(ap)
    add_sampling_flags(ap, what="the source-domain (MR) training volumes ONLY: the target's labels must not steer an unsupervised adaptation, "
                                "so the CT volumes and both validation sets stay uniform")
    from . import body
    body.add_crop_flags(ap)
    args = ap.parse_args(argv)
    args.axes = axes_from_args(ap, args)                    # one value serves MR and CT
    args.sample_mm = sample_mm_from_args(ap, args)          # one grid for both modalities: that is the point
    args.prefilter = prefilter_from_args(ap, args)          # one setting for both: the per-volume sigmas differ through the spacings
    args.sampling = sampling_from_args(ap, args)            # the MR training set's alone
    given = [getattr(args, f) is not None for f in NII_FLAGS]
    args.crop = body.crop_from_args(ap, args, have_lists=all(given))         # one crop for both domains
    if any(given) and not all(given):
        ap.error("--mr-nii-train, --mr-nii-val, --ct-nii-train and --ct-nii-val go together")
    if all(given) and args.synthetic:
        ap.error("the --*-nii-* lists and --synthetic exclude each other")
    if args.sample_mm is not None and not all(given):
        ap.error("--sample-mm goes with the --*-nii-* lists")
    if args.prefilter is not None and not all(given):
        ap.error("--prefilter goes with the --*-nii-* lists")
    if args.axes is not None and not all(given):
        ap.error("--axes goes with the --*-nii-* lists")
    if args.foreground is not None and not all(given):
        ap.error("--foreground goes with the --*-nii-* lists")
    if not args.gp_weight >= 0.0:
        ap.error("--gp-weight must be >= 0, got %r" % args.gp_weight)
    if not args.ent_weight >= 0.0:
        ap.error("--ent-weight must be >= 0, got %r" % args.ent_weight)
    if not args.pl_weight >= 0.0:
        ap.error("--pl-weight must be >= 0, got %r" % args.pl_weight)
    if not 0.0 < args.pl_portion <= 1.0:
        ap.error("--pl-portion must be in (0, 1], got %r" % args.pl_portion)
    if not 0.0 <= args.pl_momentum <= 1.0:
        ap.error("--pl-momentum must be in [0, 1], got %r" % args.pl_momentum)
    if not 0.0 <= args.pl_init < float("inf"):
        ap.error("--pl-init must be a finite value >= 0, got %r" % args.pl_init)
    if args.pl_classes is not None:
        try:
            args.pl_classes = tuple(int(c) for c in args.pl_classes.split(","))
        except ValueError:
            ap.error("--pl-classes takes class indices separated by commas, got %r" % args.pl_classes)
    if args.gp_weight > 0 and args.dtype != "f32":
        ap.error("--gp-weight > 0 runs fp32 convolutions only: the gradient penalty is not implemented for --dtype %s" % args.dtype)
    if args.gp_weight > 0 and args.sync_stats:
        ap.error("--gp-weight > 0 with --sync-stats: the gradient penalty's pass uses per-replica batch statistics and is not "
                 "implemented with synchronised ones")
    return args


def configure_args(args):
    """configure(args.phase) plus the flags that change the cost: gp_weight, ent_weight and the pl_* keys enter cost_kwargs only when
    their weight is > 0"""
    ck, nc, tc = configure(args.phase)
    if args.gp_weight > 0:
        ck["gp_weight"] = float(args.gp_weight)
    if args.ent_weight > 0:
        ck["ent_weight"] = float(args.ent_weight)
    if args.pl_weight > 0:
        ck.update(pl_weight=float(args.pl_weight), pl_portion=float(args.pl_portion), pl_momentum=float(args.pl_momentum),
                  pl_init=float(args.pl_init))
        if args.pl_classes is not None:
            ck["pl_classes"] = args.pl_classes
    if args.monitor_entropy:
        tc["monitor_entropy"] = True
    return ck, nc, tc


def main(phase, argv=None):
    args = parse_args(phase, argv)
    from .functional import set_conv_dtype
    set_conv_dtype(args.dtype)
    ck, nc, tc = configure_args(args)
    num_cls, batch_size = 5, args.batch_size
    output_path = args.output
    rank, local, world = init_distributed()     # >1 only under torch.distributed.run: data-parallel, --batch-size slices per rank
    if args.sync_stats:
        enable_sync_stats()
    if os.environ.get("PNP_SAME_DEVICE"):       # test mode: several gloo ranks on one GPU (tests/test_gpu_dp.py)
        local = 0
    device = "cuda:%d" % local if (world > 1 and args.device == "cuda") else args.device
    os.makedirs(output_path, exist_ok=True)
    if args.mr_nii_train:
        from .volume_source import augment_from_args, sources_from_lists
        shard = (rank, world) if world > 1 else None
        mr_train, mr_val = sources_from_lists(args.mr_nii_train, args.mr_nii_val, device, batch_size, num_cls, augment=augment_from_args(args),
                                              seed=0, shard=shard, sample_mm=args.sample_mm, prefilter=args.prefilter, axes=args.axes,
                                              sampling=args.sampling, crop=args.crop)
        # the target lists may name images alone: dis_step and gen_step never read a CT label, the Dice monitor skips such a source
        ct_train, ct_val = sources_from_lists(args.ct_nii_train, args.ct_nii_val, device, batch_size, num_cls, augment=augment_from_args(args),
                                              seed=2, shard=shard, sample_mm=args.sample_mm, prefilter=args.prefilter, axes=args.axes,
                                              crop=args.crop, labels="optional")
    elif args.synthetic:
        from .synthetic import write_dataset
        sets = (("syn_mr_train", args.synthetic, 0, "mr"), ("syn_ct_train", args.synthetic, 1, "ct"),
                ("syn_mr_val", batch_size, 100, "mr"), ("syn_ct_val", batch_size, 101, "ct"))
        if rank == 0:
            for folder, n, seed, prefix in sets:
                write_dataset(os.path.join(output_path, folder), n, seed=seed, prefix=prefix)
        barrier()
        mr_train, ct_train, mr_val, ct_val = [_read_lists(os.path.join(output_path, folder, prefix + "_list")) for folder, _, _, prefix in sets]
    else:
        mr_train, mr_val = _read_lists("./lists/mr_train_list"), _read_lists("./lists/mr_val_list")
        ct_train, ct_val = _read_lists("./lists/ct_train_list"), _read_lists("./lists/ct_val_list")
        if not mr_train or not ct_train:
            raise SystemExit("no ./lists/*_train_list found (use --synthetic N)")
    adapt_var_list, mr_var_list = _read_lists("./lists/half_zip_ct_vars"), _read_lists("./lists/half_zip_mri_vars")
    old_bn_list, new_bn_list = _read_lists("./lists/old_bn_list"), _read_lists("./lists/pred_bn_list")

    net = drn.Full_DRN(channels=3, batch_size=batch_size, n_class=num_cls, cost_kwargs=ck, network_config=nc, device=device, world_size=world)
    print("Network has been built ...")
    if tc["restore_from_baseline"] and not args.baseline:
        # the reference cannot get past this point either: _load_batch_norm_weights / restore raise without a baseline checkpoint
        # (adversarial.py:706-765, 790-801); warming a critic up against a randomly initialised segmenter is never what was asked for
        raise SystemExit("--phase %s starts from the source segmenter: pass --baseline <train_segmenter output>/checkpoint.npz" % args.phase)
    if tc["restore_from_baseline"]:
        with np.load(args.baseline) as z:
            seg = {k.replace("|", "/"): z[k] for k in z.files}
        net.load_baseline(seg, old_bn_list, new_bn_list, adapt_var_list, mr_var_list)
        print("initializing from baseline model!")
    trainer = drn.Trainer(net, mr_train, mr_val, ct_train, ct_val, adapt_var_list=adapt_var_list, mr_var_list=mr_var_list,
                          old_bn_list=old_bn_list, new_bn_list=new_bn_list, num_cls=num_cls, batch_size=batch_size, opt_kwargs=dict(opt_kwargs),
                          train_config=tc, reducer=GradReducer(net.store) if world > 1 else None, shard=(rank, world) if world > 1 else None)
    print("Now start training...")
    trainer.train(output_path=output_path, restored_path=output_path, restore=not tc["restore_from_baseline"],
                  training_iters=args.iters or tc["training_iters"], epochs=args.epochs or tc["epochs"])
    return trainer


if __name__ == "__main__":
    import sys
    ph = "train-gan"
    for i, a in enumerate(sys.argv):
        if a == "--phase" and i + 1 < len(sys.argv):
            ph = sys.argv[i + 1]
    main(phase=ph)
