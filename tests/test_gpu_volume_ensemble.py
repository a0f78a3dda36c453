"""-m gpu: ensemble inference through the product (volume_predict.py, predict.py) with the real networks, randomly
initialised the way tests/test_gpu_volume_predict.py does (He-scaled weights, the logits layer rescaled to peak at 10, B = 2; the small
helpers are copies of that file's).

A single identity member against the default path, a net listed twice against the net listed once (bit for bit), a three-member tta and two
nets with different seeds against tests/ensemble_ref.py on the captured logits within the bounds of tests/test_gpu_ensemble.py, the crop
box, the adapted net through Trainer.predict_volumes, and the command line.

The command line: the members are checkpoints x views and at most 8, so `--tta default --ensemble CKPT` (2 x 5 = 10 members) must end
in SystemExit before any GPU work; the three files are written with `--tta default` alone (5 members) and with a three-view `--tta` plus
`--ensemble CKPT` (6 members)."""
import json
import os

import numpy as np
import pytest
import torch

import ensemble_ref as E
from conftest import pkg

pytestmark = pytest.mark.gpu

B = 2
COST = {"cross_flag": True, "miu_cross": 1.0, "dice_flag": True, "miu_dice": 1.0, "regularizer": 1e-4}
ADV_COST = {"regularizer": 1e-4, "gan_regularizer": 1e-4, "miu_gen": 0.002, "miu_dis": 0.002, "lambda_mask_loss": 0.3}
NETCFG = {"mr_front_trainable": False, "joint_trainable": False, "ct_front_trainable": True, "cls_trainable": True, "m_cls_trainable": True}


def _random_state(net, seed, logits_fn):
    """He-scaled conv weights, BN statistics off the identity; then the logits convolution is rescaled so that the logits of a probe batch
    peak at 10"""
    rng = np.random.default_rng(seed)
    sd = net.store.state_dict()
    for k, a in sd.items():
        if "Variable" in k:
            sd[k] = (rng.standard_normal(a.shape) * np.sqrt(2.0 / np.prod(a.shape[:-1])) * 0.9).astype(np.float32)
        elif k.endswith("moving_mean"):
            sd[k] = (0.05 * rng.standard_normal(a.shape)).astype(np.float32)
        elif k.endswith("moving_variance"):
            sd[k] = (1.0 + 0.2 * rng.random(a.shape)).astype(np.float32)
        elif k.endswith("gamma"):
            sd[k] = (1.0 + 0.05 * rng.standard_normal(a.shape)).astype(np.float32)
    net.store.load_state_dict(sd)
    probe = torch.from_numpy((1.5 * rng.standard_normal((B, 256, 256, 3))).astype(np.float32)).to(net.device)
    peak = float(logits_fn(net)(probe).abs().max())
    last = [k for k in sd if "output" in k and "Variable" in k]
    assert len(last) == 1 and np.isfinite(peak) and peak > 0, (last, peak)
    sd[last[0]] = (sd[last[0]] * (10.0 / peak)).astype(np.float32)
    net.store.load_state_dict(sd)
    return net


def _segmenter(dev, seed):
    ss = pkg("source_segmenter")
    return _random_state(ss.Full_DRN(channels=3, n_class=5, batch_size=B, device=dev, seed=0, cost_kwargs=dict(COST)), seed, pkg("volume_predict").segmenter_logits)


@pytest.fixture(scope="module")
def seg(dev):
    return _segmenter(dev, 5)


@pytest.fixture(scope="module")
def seg2(dev):
    return _segmenter(dev, 6)


def _scan(shape, seed):
    """a smooth-ish int16 scan with a bright tail: blobs over noise"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    v = 400 * np.exp(-4 * (g[0] ** 2 + g[1] ** 2 + 0.5 * g[2] ** 2)) + 60 * rng.standard_normal(shape) + 100 * np.sin(5 * g[0]) * np.cos(3 * g[1])
    return v.astype(np.int16)


def _to_slicing(a, flip, axis):
    if flip:
        a = np.flip(np.flip(a, 0), 1)
    return np.moveaxis(a, axis, -1)


def _capturing(fn, store):
    def wrapped(x):
        out = fn(x)
        store.append(out.detach().clone())
        return out
    return wrapped


def _against_the_restatement(res, captured, per_batch, invs_of_batch, XYZ, flip, axis, what):
    """res: Ensemble of device tensors in file order; captured: the logits in call order, per_batch members per batch (member order)"""
    X, Y, Z = XYZ
    lab_s = _to_slicing(res.label.cpu().numpy(), flip, axis)
    prob_s = np.stack([_to_slicing(p, flip, axis) for p in res.prob.cpu().numpy()], -1)          # [X, Y, Z, ncls]
    ent_s = _to_slicing(res.entropy.cpu().numpy(), flip, axis)
    assert len(captured) % per_batch == 0
    bad = differ = multi = 0
    perr = herr = serr = 0.0
    dp_max = hb_max = 0.0
    for k in range(len(captured) // per_batch):
        lgs = [t.cpu().numpy() for t in captured[k * per_batch:(k + 1) * per_batch]]
        nb = min(B, Z - k * B)
        ref = E.ensemble(lgs, invs_of_batch, X, Y, nb)
        dp = E.delta_p(lgs, invs_of_batch, X, Y, nb)
        hb = E.entropy_bound(dp, 5)
        dp_max, hb_max = max(dp_max, dp), max(hb_max, hb)
        sl = slice(k * B, k * B + nb)
        mine = np.moveaxis(lab_s[:, :, sl], 2, 0)
        adm = E.admissible(ref.prob, dp)
        ok = np.take_along_axis(adm, mine[..., None].astype(np.int64), axis=-1)[..., 0]
        bad += int((~ok).sum())
        differ += int((mine != ref.label).sum())
        multi += int((adm.sum(-1) > 1).sum())
        P = np.moveaxis(prob_s[:, :, sl], 2, 0).astype(np.float64)
        e1, e2 = float(np.abs(P - ref.prob).max()), float(np.abs(np.moveaxis(ent_s[:, :, sl], 2, 0) - ref.entropy).max())
        assert e1 <= dp and e2 <= hb, "%s, batch %d: max|dP| %.3g (bound %.3g), max|dH| %.3g (bound %.3g)" % (what, k, e1, dp, e2, hb)
        perr, herr, serr = max(perr, e1), max(herr, e2), max(serr, float(np.abs(P.sum(-1) - 1).max()))
    print("%s: %d of %d labels differ from the float64 argmax, %d outside the bound (%d voxels admit more than one class); max|dP| %.3g "
          "(bound %.3g), max|dH| %.3g (bound %.3g), max|sum P - 1| %.3g" % (what, differ, X * Y * Z, bad, multi, perr, dp_max, herr, hb_max, serr))
    assert bad == 0 and serr <= 5 * 2.0 ** -23
    assert len(np.unique(lab_s)) > 1, "a constant prediction shows nothing"


def test_single_identity_member_against_the_default_path(dev, seg):
    """256 x 256 x 6, tta=[{}] with prob=True: the default call's labels, except where the float64 top-2 PROBABILITY gap is below
    2 delta_p (interpolation is exact for the identity map: delta_p is its rounding term, 20 * 2^-24); such voxels must be <= 1e-4 of all"""
    vp = pkg("volume_predict")
    image = _scan((256, 256, 6), 0)
    captured = []
    fn = _capturing(vp.segmenter_logits(seg), captured)
    plain = vp.segment_volume(fn, image, batch_size=B, device=dev)
    assert isinstance(plain, torch.Tensor) and plain.dtype == torch.uint8
    n_plain = len(captured)
    res = vp.segment_volume(fn, image, batch_size=B, device=dev, tta=[{}], prob=True)
    assert isinstance(res, vp.Ensemble) and res.entropy is None and res.label.dtype == torch.uint8 and tuple(res.label.shape) == image.shape
    assert res.prob.dtype == torch.float32 and tuple(res.prob.shape) == (5,) + image.shape and res.prob.is_cuda
    assert n_plain == 3 and len(captured) == 6                                   # one forward per batch and member
    logits = torch.cat(captured[:3]).cpu().numpy().astype(np.float64)            # [6, 256, 256, 5]: frames in slicing order
    P = np.sort(E.softmax(logits), -1)
    dp = E.K_ROUND * E.U
    close = np.moveaxis((P[..., -1] - P[..., -2]) < 2 * dp, 0, 2)                # [X, Y, Z] slicing order
    diff = _to_slicing((res.label != plain).cpu().numpy(), True, 2)
    print("identity member: %d of %d labels differ from the default path, %d voxels with a top-2 probability gap < %.3g" % (int(diff.sum()), diff.size, int(close.sum()), 2 * dp))
    assert not np.any(diff & ~close) and close.sum() <= 1e-4 * close.size
    got = np.stack([_to_slicing(p, True, 2) for p in res.prob.cpu().numpy()], -1)          # [X, Y, Z, 5]
    assert np.abs(np.moveaxis(got, 2, 0) - E.softmax(logits)).max() <= dp
    assert len(np.unique(plain.cpu().numpy())) > 1


def test_a_net_listed_twice_is_the_net_listed_once(dev, seg):
    """bit for bit, all three outputs, also listed 4 and 8 times (one map: the members are copies of ONE member, whose sum in two runs of
    four is exact; with several views the copies interleave with other members and only the bounds hold)"""
    vp = pkg("volume_predict")
    image = _scan((200, 5, 232), 1)
    fn = vp.segmenter_logits(seg)
    kw = dict(flip_correction=True, axis=1, batch_size=B, device=dev, prob=True, entropy=True)
    once = vp.segment_volume([fn], image, **kw)
    assert len(torch.unique(once.label)) > 1
    for n in (2, 4, 8):
        many = vp.segment_volume([fn] * n, image, **kw)
        for a, b, name in zip(once, many, once._fields):
            assert torch.equal(a, b), "listed %d times: %s differs" % (n, name)


def _the_plan_has(n_callables, options, shape, invs):
    """the hand-built inverse maps are the ones segment_volume's plan holds for these options (axis 1, batches of B), member for member"""
    vp = pkg("volume_predict")
    plan = vp.plan_view(vp.parse_request(n_callables, axis=1, batch_size=B, **options), shape, 1, ((0, 200), (0, 232), (0, 5)), None)
    assert plan.dims == (200, 232, 5) and plan.kind == "ensemble" and plan.members == len(invs)
    assert all(np.array_equal(a, b) for a, b in zip(plan.invs, invs))


def test_three_member_tta_against_the_restatement(dev, seg):
    """200 x 232 x 5 in slicing order, stored with the slicing axis in the middle and flipped: batches of 2, 2 and 1 frames"""
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    image = _scan((200, 5, 232), 1)
    tta = [{}, {"rotate": 7.5, "translate": (2.0, -1.5)}, {"scale": 1.05, "flip": True}]
    captured = []
    res = vp.segment_volume(_capturing(vp.segmenter_logits(seg), captured), image, flip_correction=True, axis=1, batch_size=B, device=dev,
                            tta=tta, prob=True, entropy=True)
    assert len(captured) == 9 and tuple(res.prob.shape) == (5, 200, 5, 232) and tuple(res.entropy.shape) == image.shape
    invs = [vp.invert_matrix(vs.compose_matrix((200, 232), (256, 256), **e)) for e in tta]
    _the_plan_has(None, dict(tta=tta, prob=True, entropy=True), image.shape, invs)
    _against_the_restatement(res, captured, 3, invs, (200, 232, 5), True, 1, "three-member tta, 200 x 232 x 5")


def test_two_nets_against_the_restatement(dev, seg, seg2):
    vp, vs = pkg("volume_predict"), pkg("volume_source")
    image = _scan((200, 5, 232), 3)
    captured = []
    fns = [_capturing(vp.segmenter_logits(n), captured) for n in (seg, seg2)]
    res = vp.segment_volume(fns, image, flip_correction=True, axis=1, batch_size=B, device=dev, prob=True, entropy=True)
    assert len(captured) == 6
    assert not torch.equal(captured[0], captured[1]), "two seeds, two nets"
    inv = vp.invert_matrix(vs.compose_matrix((200, 232), (256, 256)))
    _the_plan_has(2, dict(prob=True, entropy=True), image.shape, [inv, inv])
    _against_the_restatement(res, captured, 2, [inv, inv], (200, 232, 5), True, 1, "two nets, 200 x 232 x 5")


def test_crop_box(dev, seg):
    vp = pkg("volume_predict")
    image = _scan((200, 5, 232), 2)
    box = ((10, 150), (21, 200), (1, 5))
    res = vp.segment_volume(vp.segmenter_logits(seg), image, crop=box, flip_correction=True, axis=1, batch_size=B, device=dev,
                            tta=[{}, {"rotate": -7.5}], prob=True, entropy=True)
    inside = np.zeros((200, 232, 5), bool)
    inside[tuple(slice(a, b) for a, b in box)] = True
    lab, ent = _to_slicing(res.label.cpu().numpy(), True, 1), _to_slicing(res.entropy.cpu().numpy(), True, 1)
    prob = np.stack([_to_slicing(p, True, 1) for p in res.prob.cpu().numpy()], -1)
    assert not lab[~inside].any() and not ent[~inside].any() and not prob[~inside].any()
    assert np.abs(prob[inside].sum(-1) - 1).max() <= 5 * 2.0 ** -23 and ent[inside].min() >= 0 and ent[inside].max() <= 1 + 1e-6
    assert len(np.unique(lab[inside])) > 1


def _check_files(nifti, out, base, shape, aff):
    names = sorted(os.listdir(out))
    assert names == sorted(k + "_" + base for k in ("pred", "prob", "entropy")), names
    pred, prob, ent = (nifti.load(os.path.join(out, k + "_" + base)) for k in ("pred", "prob", "entropy"))
    assert pred.shape == shape and pred.get_data().dtype == np.uint8 and np.allclose(pred.affine, aff) and pred.get_data().max() < 5
    assert prob.shape == shape + (5,) and prob.get_data().dtype == np.float32 and np.allclose(prob.affine, aff)
    assert ent.shape == shape and ent.get_data().dtype == np.float32 and np.allclose(ent.affine, aff)
    P, Hn = prob.get_data(), ent.get_data()
    assert np.abs(P.sum(-1) - 1).max() <= 5 * 2.0 ** -23 and Hn.min() >= 0 and Hn.max() <= 1 + 1e-6
    lab = pred.get_data()
    top = np.sort(P, -1)
    clear = top[..., -1] - top[..., -2] > 1e-6                     # the file's label is the argmax of the file's probabilities
    assert np.array_equal(np.argmax(P, -1)[clear], lab[clear]) and clear.mean() > 0.99
    return lab, P, Hn


def test_adapted_net_through_the_trainer(dev, tmp_path):
    adv, vp, nifti = pkg("adversarial"), pkg("volume_predict"), pkg("nifti")
    net = _random_state(adv.Full_DRN(channels=3, n_class=5, batch_size=B, cost_kwargs=dict(ADV_COST), network_config=dict(NETCFG), device=dev, seed=1), 9,
                        vp.adapted_logits)
    aff = np.array([[0.0, -1.5, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, 3.0, 5.0], [0.0, 0.0, 0.0, 1.0]])
    a = str(tmp_path / "a.nii.gz")
    nifti.save(nifti.Nifti1Image(_scan((40, 36, 4), 4), aff), a)
    tr = adv.Trainer(net, [], [], [], [], num_cls=5, batch_size=B)
    out = str(tmp_path / "out")
    paths = tr.predict_volumes([a], out, tta="default", prob=True, entropy=True)
    assert paths == [os.path.join(out, "pred_a.nii.gz")]
    _check_files(nifti, out, "a.nii.gz", (40, 36, 4), aff)


def test_command_line(dev, seg, seg2, tmp_path):
    ss, nifti, pr = pkg("source_segmenter"), pkg("nifti"), pkg("predict")
    aff = np.diag([0.8, 0.8, 2.5, 1.0])
    b = str(tmp_path / "b.nii")
    nifti.save(nifti.Nifti1Image(_scan((33, 47, 3), 5), aff), b)
    cks = []
    for net, name in ((seg, "ckpt1.npz"), (seg2, "ckpt2.npz")):
        ck = net.save(str(tmp_path / name))
        cks.append(ck if isinstance(ck, str) and os.path.isfile(ck) else str(tmp_path / name))
        assert os.path.isfile(cks[-1])
    ck1, ck2 = cks
    base = ["--model", ck1, "--net", "segmenter", "--images", b, "--batch-size", str(B)]
    # 2 checkpoints x 5 views = 10 members: refused as an argument error, nothing is written
    with pytest.raises(SystemExit):
        pr.main(base + ["--out", str(tmp_path / "refused"), "--tta", "default", "--prob", "--entropy", "--ensemble", ck2])
    assert not os.path.exists(str(tmp_path / "refused"))
    out1 = str(tmp_path / "tta")
    res = pr.main(base + ["--out", out1, "--tta", "default", "--prob", "--entropy"])
    assert res["paths"] == [os.path.join(out1, "pred_b.nii")]
    _check_files(nifti, out1, "b.nii", (33, 47, 3), aff)
    out2 = str(tmp_path / "ens")
    tta = [{}, {"rotate": 7.5}, {"rotate": -7.5}]
    res = pr.main(base + ["--out", out2, "--tta", json.dumps(tta), "--prob", "--entropy", "--ensemble", ck2])
    lab, P, Hn = _check_files(nifti, out2, "b.nii", (33, 47, 3), aff)
    # the same six members through the method, bit for bit
    tr = ss.Trainer(seg, train_list=[], val_list=[], num_cls=5, batch_size=B)
    out3 = str(tmp_path / "method")
    tr.predict_volumes([b], out3, ensemble=[seg2], tta=tta, prob=True, entropy=True)
    lab3, P3, H3 = _check_files(nifti, out3, "b.nii", (33, 47, 3), aff)
    assert np.array_equal(lab, lab3) and np.array_equal(P, P3) and np.array_equal(Hn, H3)
    # and the default command line still writes the label file alone
    out4 = str(tmp_path / "plain")
    pr.main(base + ["--out", out4])
    assert os.listdir(out4) == ["pred_b.nii"]
