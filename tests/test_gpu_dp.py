"""-m gpu: data-parallel gradient reduction with 2 ranks sharing the one GPU of the test box (gloo transport): the overlapped,
bucketed, side-stream all-reduce must equal a plain all-reduce of the same gradients; bench.py's N=2 launch line works end to end."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(args, extra_env, timeout=600):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="4", **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29741"] + args
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_overlapped_allreduce_equals_plain(dev):
    p = _run([os.path.join(ROOT, "tests", "dp_worker.py")], {})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.count(" ok ") == 2


def test_native_rccl_single_rank(dev):
    """pnp_comm_* (csrc/comm.hip) on the one GPU of the test box: bring-up through the unique id, a sum all-reduce over a 1-rank
    communicator enqueued on a SIDE stream behind an event (the GradReducer pattern), float32 and float64, tear-down"""
    import torch
    from conftest import pkg
    par = pkg("parallel")
    comm = par.NativeComm(0, 1).prepare().connect()
    assert comm.version >= 20000 and bool(comm.handle)
    side = torch.cuda.Stream()
    for dt in (torch.float32, torch.float64):
        t = torch.randn(3 << 20, device=dev, dtype=dt)
        ref = t.clone()
        t.mul_(2.0)                                   # producer on the current stream
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        comm.allreduce_(t, side)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(t, ref * 2.0)
    with pytest.raises(pkg("_lib").PnpError):
        comm.allreduce_(torch.zeros(4, device=dev, dtype=torch.int32))
    comm.destroy()


def test_native_rccl_two_ranks(dev):
    """the production transport end to end: 2 ranks on 2 GPUs, overlapped bucketed pnp_comm_allreduce == one plain all-reduce
    (skipped on 1-GPU boxes: RCCL refuses two ranks on one device)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    p = _run([os.path.join(ROOT, "tests", "dp_worker.py")], {"PNP_DP_NATIVE": "1"})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.count(" ok ") == 2


def test_bench_two_rank_launch_line(dev, tmp_path):
    """the plain line: the timed steps, rank 0's --dump-outputs, the record — none of what --full adds"""
    import numpy as np
    out = str(tmp_path / "outputs")
    p = _run([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4", "--no-cpu-baseline", "--workload", "segmenter",
              "--no-sub", "--dump-outputs", out],
             {"PNP_DIST_BACKEND": "gloo", "PNP_SAME_DEVICE": "1"})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    r = json.loads(line)
    assert r["n_gpus"] == 2 and r["config"]["global_batch"] == 8 and r["scaling"] == "weak" and r["value"] > 0
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and "roofline" not in r and "kernels_file" not in r and r["config"]["comm"] is None
    assert sorted(os.listdir(out)) == ["loss.npy", "trainable_variables.npy"]
    loss, v = np.load(os.path.join(out, "loss.npy")), np.load(os.path.join(out, "trainable_variables.npy"))
    assert loss.dtype == np.float64 and np.isclose(float(loss), r["config"]["final_loss"], rtol=1e-3) and v.dtype == np.float32 and np.isfinite(v).all()


def test_bench_two_rank_gan_workload(dev):
    """config 4 launch line: joint dis + gen step, 2 ranks, gradient buckets of the frozen groups skipped"""
    p = _run([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--batch", "2", "--workload", "gan", "--full"],
             {"PNP_DIST_BACKEND": "gloo", "PNP_SAME_DEVICE": "1"})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    last = p.stdout.rstrip("\n").splitlines()[-1]              # the driver parses the LAST stdout line (out of a ~2000-character tail)
    assert len(last) < 1700, len(last)
    r = json.loads(last)
    assert r["n_gpus"] == 2 and "joint" in r["metric"] and r["value"] > 0 and "cpu_baseline" not in r
    assert r["segmenter_step"]["value"] > 0 and r["roofline"]["launches"] > 0 and "roofline_kernels" not in r
    assert r["config"]["comm"]["buckets"] >= 1 and r["config"]["per_gpu_batch"] == 2
    full = json.load(open(os.path.join(ROOT, r["kernels_file"])))             # the per-symbol table: side file
    assert len(full["roofline_kernels"]) >= 3 and full["config"]["comm"]["dis_step"]["launch_order"] is not None


def test_train_segmenter_two_ranks(dev, tmp_path):
    """the entry point itself under torch.distributed.run: sharded file lists, per-rank feeders, overlapped reduction, rank-0 checkpoint"""
    out = str(tmp_path / "seg_dp")
    p = _run(["-m", "medical-cross-modality-domain-adaptation_amd.train_segmenter", "--synthetic", "8", "--batch-size", "2", "--iters", "3",
              "--epochs", "1", "--output", out], {"PNP_DIST_BACKEND": "gloo", "PNP_SAME_DEVICE": "1"})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert os.path.exists(os.path.join(out, "checkpoint.npz"))
    assert (p.stdout + p.stderr).count("Optimization Finished!") == 2


def test_two_ranks_equal_one_gpu(dev, tmp_path):
    """SURVEY.md §8e 'N GPUs == 1 GPU': with synchronised batch statistics and loss normalisers, 2 ranks x 2 slices reproduce the
    gradients, BN moving statistics and Adam update of one process on the 4 slices (fp32 summation-order differences only)."""
    import numpy as np
    import torch
    from conftest import pkg
    from dp_sync_common import COST, make_batch, scaled_state
    ss = pkg("source_segmenter")
    net = ss.Full_DRN(channels=3, n_class=5, batch_size=4, device=dev, cost_kwargs=dict(COST), seed=0)
    net.store.load_state_dict(scaled_state(net))
    x, y = make_batch(4)
    tr = ss.Trainer(net, None, None, num_cls=5, batch_size=4, optimizer="adam", opt_kwargs={"learning_rate": 1e-3})
    tr.opt = tr._get_optimizer(10)
    net.loss_and_grads(x.to(dev), y.to(dev), 1.0)
    g1 = net.store.grad_arena.detach().cpu().numpy().copy()
    tr.opt.step()
    torch.cuda.synchronize()
    sd1 = net.store.state_dict()
    def compare(path):
        with np.load(path) as z:
            g2 = z["grads"]
            sd2 = {k.replace("|", "/"): z[k] for k in z.files if k != "grads"}
        errs = []
        for v in net.store.trainable():
            a, b = g1[v.offset:v.offset + v.numel], g2[v.offset:v.offset + v.numel]
            errs.append(float(np.abs(a - b).max() / (np.abs(a).max() + 1e-30)))
        cos = float((g1.astype(np.float64) * g2).sum() / (np.linalg.norm(g1.astype(np.float64)) * np.linalg.norm(g2.astype(np.float64))))
        mv = max(float(np.abs(sd1[k] - sd2[k]).max() / (np.abs(sd1[k]).max() + 1e-30)) for k in sd1 if k.endswith("moving_variance"))
        return float(np.median(errs)), max(errs), cos, mv

    res = {}
    for tag, extra in (("sync", {}), ("per_replica", {"PNP_SYNC_OFF": "1"})):
        out = str(tmp_path / (tag + ".npz"))
        p = _run([os.path.join(ROOT, "tests", "dp_sync_worker.py")], dict(extra, PNP_SYNC_OUT=out))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        res[tag] = compare(out)
        print("2 ranks x 2 slices vs 1 GPU x 4 slices [%s]: gradient error median %.2e max %.2e, cosine %.8f, moving-variance error %.2e"
              % ((tag,) + res[tag]))
    # synchronised: what is left is fp32 summation order through 30 BN layers (different tiles / splits at B=2 and B=4);
    # per-replica statistics and normalisers are a different function of the batch — an order of magnitude away
    assert res["sync"][2] > 0.99999 and res["sync"][3] < 1e-4
    assert res["per_replica"][0] > 10 * res["sync"][0] and (1 - res["per_replica"][2]) > 10 * (1 - res["sync"][2])
    # the halves differ in class proportions by construction, so per-replica loss normalisers cannot agree with the global ones
    lab = y.argmax(3)
    f0 = [(lab[:2] == c).float().mean().item() for c in range(5)]
    f1 = [(lab[2:] == c).float().mean().item() for c in range(5)]
    assert max(abs(a - b) for a, b in zip(f0, f1)) > 1e-3
