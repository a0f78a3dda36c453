"""gpu: Fourier domain adaptation in the source segmenter's training loop: prob = 0 is the run without it bit for bit,
the batch a step receives is the amplitude swap of the feeder's batch, and train_segmenter runs with --fda-target on a tfrecord list and
on an image-only NIfTI list."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

B = 2
COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}


class Slices(object):
    """synthetic [B, 256, 256, 4] batches (image channels 0:3, label map in channel 3), the same stream for every instance of a seed;
    fixed: the same batch every time"""

    def __init__(self, seed, fixed=False):
        self.rng, self.fixed, self.first = np.random.default_rng(seed), fixed, None

    def next_batch(self, batch_size):
        if self.fixed and self.first is not None:
            return self.first.copy(), ["fixed"] * batch_size
        syn = pkg("synthetic")
        out = []
        for _ in range(batch_size):
            img, lab = syn.make_slice(self.rng)
            out.append(np.concatenate([img, lab[:, :, 1:2]], axis=-1))
        self.first = np.stack(out).astype(np.float32)
        return self.first.copy(), ["slice"] * batch_size


def _trainer(dev, fda=None):
    ss = pkg("source_segmenter")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, cost_kwargs=dict(COST), seed=3)
    tr = ss.Trainer(net, Slices(0), Slices(100), num_cls=5, batch_size=B, optimizer="adam", opt_kwargs={"learning_rate": 1e-3}, fda=fda)
    return net, tr


def test_prob_zero_is_the_run_without_fda(dev, tmp_path):
    F = pkg("fda")
    res = []
    for fda in (None, F.FdaStylizer(Slices(7, fixed=True), beta=0.09, prob=0.0)):
        net, tr = _trainer(dev, fda)
        tr.train(output_path=str(tmp_path / ("run%d" % len(res))), training_iters=3, epochs=1)
        torch.cuda.synchronize()
        res.append((net.store.arena.detach().cpu().clone(), net.store.state_arena.detach().cpu().clone()))
        if fda is not None:
            assert (fda.last_band == -1).all()
            fda.close()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


class _Recorder(object):
    def __init__(self, sty):
        self.sty, self.inputs = sty, []

    def __call__(self, x):
        self.inputs.append(x.clone())
        return self.sty(x)


def test_step_receives_the_amplitude_swap_of_the_feeder_batch(dev, tmp_path):
    F, K = pkg("fda"), pkg("kernels")
    target = Slices(7, fixed=True)
    tgt = torch.from_numpy(target.next_batch(B)[0][..., :3].copy()).to(dev)
    sty = F.FdaStylizer(target, beta=(0.01, 0.09), prob=1.0, seed=4)
    rec = _Recorder(sty)
    net, tr = _trainer(dev, rec)
    seen, stats = {}, []
    step0, stats0 = tr.train_step, tr.output_minibatch_stats

    def step(bx, by, dropout, step):
        seen.update(x=bx.clone(), y=by.clone(), args=(dropout, step))
        loss = step0(bx, by, dropout, step)
        seen.update(w=net.store.arena.detach().clone(), s=net.store.state_arena.detach().clone())
        return loss

    def stats_(step, bx, by):
        stats.append(bx.clone())
        return stats0(step, bx, by)
    tr.train_step, tr.output_minibatch_stats = step, stats_
    try:
        tr.train(output_path=str(tmp_path / "fda"), training_iters=1, epochs=1)
    finally:
        sty.close()
    assert len(rec.inputs) == 1 and len(stats) == 1
    band, pair = sty.last_band, sty.last_pair
    print("bands %s pairs %s" % (band, pair))
    assert ((band >= 2) & (band <= 23)).all() and ((pair >= 0) & (pair < B)).all()
    want = K.fda_amplitude_swap(rec.inputs[0], tgt, band, pair)
    assert torch.equal(seen["x"], want) and not torch.equal(seen["x"], rec.inputs[0])
    assert torch.equal(stats[0], seen["x"])                  # output_minibatch_stats sees the stylised batch
    # a twin fed that batch directly takes the same step
    net2, tr2 = _trainer(dev)
    tr2.opt = tr2._get_optimizer(1)
    tr2.train_step(want, seen["y"], *seen["args"])
    torch.cuda.synchronize()
    assert torch.equal(net2.store.arena, seen["w"]) and torch.equal(net2.store.state_arena, seen["s"])


def test_entry_point_with_a_tfrecord_target_list(dev, tmp_path):
    ts, syn = pkg("train_segmenter"), pkg("synthetic")
    syn.write_dataset(str(tmp_path / "ct"), 4, seed=1)
    out = str(tmp_path / "seg")
    tr = ts.main(["--synthetic", "8", "--batch-size", "2", "--iters", "2", "--epochs", "1", "--output", out,
                  "--fda-target", str(tmp_path / "ct" / "slice_list"), "--fda-beta", "0.01,0.09"])
    assert os.path.exists(os.path.join(out, "checkpoint.npz"))
    assert (tr.fda.lo, tr.fda.hi, tr.fda.prob) == (0.01, 0.09, 1.0)
    assert ((tr.fda.last_band >= 2) & (tr.fda.last_band <= 23)).all() and np.isfinite(tr.loss_dict["train"][1])


def test_entry_point_with_an_image_only_nifti_target_list(dev, tmp_path):
    ts, nifti = pkg("train_segmenter"), pkg("nifti")
    rng = np.random.default_rng(5)
    aff = np.diag([1.0, 1.0, 2.0, 1.0])
    shape = (48, 40, 12)
    for name in ("mr0", "mr1", "ct0", "ct1"):
        v = rng.normal(0.0, 1.0, shape).astype(np.float32)
        v[8:40, 8:32] += 3.0
        nifti.save(nifti.Nifti1Image(v, aff), str(tmp_path / (name + "_image.nii.gz")))
        lab = np.zeros(shape, np.int16)
        lab[10:24, 10:20], lab[24:38, 10:20], lab[10:24, 20:30], lab[24:38, 20:30] = 1, 2, 3, 4
        nifti.save(nifti.Nifti1Image(lab, aff), str(tmp_path / (name + "_label.nii.gz")))
    (tmp_path / "mr_train").write_text("mr0_image.nii.gz mr0_label.nii.gz\nmr1_image.nii.gz mr1_label.nii.gz\n")
    (tmp_path / "mr_val").write_text("mr1_image.nii.gz mr1_label.nii.gz\n")
    (tmp_path / "ct_train").write_text("ct0_image.nii.gz\nct1_image.nii.gz\n")          # images alone
    out = str(tmp_path / "seg")
    tr = ts.main(["--nii-train", str(tmp_path / "mr_train"), "--nii-val", str(tmp_path / "mr_val"), "--batch-size", "2", "--iters", "2",
                  "--epochs", "1", "--output", out, "--fda-target", str(tmp_path / "ct_train"), "--fda-beta", "0.05", "--fda-prob", "0.5"])
    assert os.path.exists(os.path.join(out, "checkpoint.npz"))
    assert tr.fda.source.augment is None and not tr.fda.source.labelled
    assert set(tr.fda.last_band.tolist()) <= {-1, 12} and np.isfinite(tr.loss_dict["train"][1])
