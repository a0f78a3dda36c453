"""Bit-for-bit A/B of the batch-norm kernels (csrc/elementwise.hip: column reductions, combine, apply, backward) between two builds of the library.

    PNP_LIB=<one libpnp_hip.so>     python tools/bn_ab.py dump a.npz
    PNP_LIB=<another libpnp_hip.so> python tools/bn_ab.py dump b.npz
    python tools/bn_ab.py compare a.npz b.npz        # one line per array (dtype, shape and bytes), exit status 1 if any differs

`dump` writes EVERY output of bn_stats, bn_stats_update and bn_update_moving; of bn_apply with and without the bf16 copy; of bn_bwd with
`out` handed in and with the sign recomputed, with into= and with the bf16 side output; of bn_bwd_reduce and bn_bwd_apply (P_norm = 2 P) —
over BN_CASES, BN_TWIN_CASES, BN_H_CASES and SYNCBN_CASES of tests/test_gpu_elementwise_domain.py, the six shapes of
test_bn_reductions_with_long_partial_lists and the overflowing tensor of tests/test_gpu_elementwise.py — and of bn_stats_finish on
synthetic partial lists of FINISH_ROWS rows at FINISH_C channels (the list itself, which the combine consumes, included).  An array above
16 MB is kept as its SHA-256."""
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_elementwise_domain as D      # noqa: E402

LONG_LISTS = [(16384, 64), (65536, 64), (300000, 32), (262144, 5), (1048576, 16), (40000, 512)]
FINISH_ROWS, FINISH_C = (1, 2, 511, 512, 513, 640, 1000), (5, 32, 64, 1028)


def _put(out, name, t):
    if t is None:
        return
    a = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()
    if a.nbytes > (16 << 20):
        name, a = name + " (sha256 of %s %s)" % (a.dtype, a.shape), np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
    assert name not in out, name
    out[name] = a


def _case(K, out, tag, P, C, Cs, alpha, training, keep, seed, dev):
    x, gamma, beta, mm, mv, sc, dout = D._bn_inputs(P, C, Cs, seed, dev)
    put = lambda name, t: _put(out, "%s %s" % (tag, name), t)
    mean, var = K.bn_stats(x)
    mm1, mv1 = mm.clone(), mv.clone()
    mean_u, var_u = K.bn_stats_update(x, mm1, mv1, 0.9)
    mm2, mv2 = mm.clone(), mv.clone()
    K.bn_update_moving(mm2, mv2, mean, var, P, 0.9)
    for name, t in (("stats mean", mean), ("stats var", var), ("stats_update mean", mean_u), ("stats_update var", var_u), ("stats_update mm", mm1),
                    ("stats_update mv", mv1), ("update_moving mm", mm2), ("update_moving mv", mv2)):
        put(name, t)
    if not training:
        mean, var = mm.clone(), mv.clone()
    y = K.bn_apply(x, mean, var, gamma, beta, sc, 1e-3, alpha)
    yh = K.bn_apply(x, mean, var, gamma, beta, sc, 1e-3, alpha, want_h=True)
    put("apply y", y)
    put("apply want_h y", yh)
    put("apply want_h bf16", yh._pnp_h[0])
    sid = 3
    runs = [("bwd", dict(out=y))]
    if not Cs and alpha >= 0:
        runs.append(("bwd recomputed", dict(out=None, beta=beta)))
    for name, kw in runs:
        o = kw.pop("out")
        dx, dg, db, dsc = K.bn_bwd(dout, o, x, mean, var, gamma, Cs, 1e-3, alpha, training, keep, seed, sid, **kw)
        for n2, t in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("dshortcut", dsc)):
            put("%s %s" % (name, n2), t)
    sg, sb = torch.full((C,), 2.0, device=dev), torch.full((C,), -1.0, device=dev)
    dx, dg, db, dsc = K.bn_bwd(dout, y, x, mean, var, gamma, Cs, 1e-3, alpha, training, keep, seed, sid, into=(sg, sb), want_h=True)
    for n2, t in (("dx", dx), ("dx bf16", dx._pnp_h[0]), ("dgamma", dg), ("dbeta", db), ("dshortcut", dsc), ("slot dgamma", sg), ("slot dbeta", sb)):
        put("bwd into want_h %s" % n2, t)
    sums = K.bn_bwd_reduce(dout, y, x, mean, var, 1e-3, alpha)
    put("bwd_reduce sums", sums)
    if not Cs and alpha >= 0:
        put("bwd_reduce recomputed sums", K.bn_bwd_reduce(dout, None, x, mean, var, 1e-3, alpha, gamma=gamma, beta=beta))
    dxa, dsca = K.bn_bwd_apply(dout, y, x, mean, var, gamma, sums, 2 * P, Cs, 1e-3, alpha, training, keep, seed, sid, want_h=True)
    put("bwd_apply dx", dxa)
    put("bwd_apply dx bf16", dxa._pnp_h[0])
    put("bwd_apply dshortcut", dsca)


def _finish(K, out, nparts, C, dev):
    g = D._gen(7000 + nparts + C, dev)
    parts = torch.cat([D._randn(g, nparts, 1, C) * 9.0, D._randn(g, nparts, 1, C).abs() * 70.0 + 40.0], 1).contiguous()      # [row][q][c]
    shift, mm, mv = 0.3 * D._randn(g, C), 0.2 * D._randn(g, C), 1.0 + 0.1 * torch.rand(C, generator=g, device=dev)
    for name, m_, v_ in (("plain", None, None), ("moving", mm.clone(), mv.clone())):
        p = parts.clone()
        mean, var = K.bn_stats_finish((p, nparts), shift, 64 * nparts, m_, v_, 0.9)
        for n2, t in (("mean", mean), ("var", var), ("mm", m_), ("mv", v_), ("list", p)):
            _put(out, "stats_finish rows%d C%d %s %s" % (nparts, C, name, n2), t)


def dump(path):
    K = importlib.import_module("medical-cross-modality-domain-adaptation_amd.kernels")
    dev = torch.device("cuda:0")
    out = {}
    for n, (P, C, Cs, alpha, training, keep) in enumerate(D.BN_CASES):
        _case(K, out, "domain P%d C%d Cs%d a%g %s k%g" % (P, C, Cs, alpha, "train" if training else "infer", keep), P, C, Cs, alpha, training,
              keep, n, dev)
    for C, Cv, Csc in D.BN_TWIN_CASES:
        for training in (True, False):
            for Cs in (Cv, Csc):
                _case(K, out, "twin C%d Cs%d %s" % (C, Cs, "train" if training else "infer"), 1000, C, Cs, 0.2, training, 0.75, 1000 + C, dev)
    for P, C, Cs in D.BN_H_CASES:
        _case(K, out, "sideout P%d C%d Cs%d" % (P, C, Cs), P, C, Cs, 0.2, True, 0.75, 2000 + C, dev)
    for Ph, C, Cs in D.SYNCBN_CASES:
        for P in (Ph, 2 * Ph):
            _case(K, out, "syncbn P%d C%d Cs%d" % (P, C, Cs), P, C, Cs, 0.2, True, 0.75, 3000 + C, dev)
    for P, C in LONG_LISTS:
        _case(K, out, "long P%d C%d" % (P, C), P, C, 0, 0.2, True, 1.0, P % 1000 + C, dev)
    x = torch.full((1, 1, 65536, 32), 1e25, device=dev)
    x[0, 0, 0, :] = 0.0
    mean, var = K.bn_stats(x)
    _put(out, "overflow mean", mean)
    _put(out, "overflow var", var)
    for nparts in FINISH_ROWS:
        for C in FINISH_C:
            _finish(K, out, nparts, C, dev)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("%s: %d arrays, %.1f MB, library %s" % (path, len(out), sum(a.nbytes for a in out.values()) / 1e6, os.environ.get("PNP_LIB", "(the tree's)")))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    differ = sorted(set(a.files) ^ set(b.files))
    for name in differ:
        print("MISSING   %s (in one file only)" % name)
    n = len(differ)
    for name in sorted(set(a.files) & set(b.files)):
        x, y = a[name], b[name]
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        n += not same
        print("%-9s %-72s %s %s" % ("equal" if same else "DIFFERS", name, x.dtype, x.shape))
    print("VERDICT: %d arrays, %d differ" % (len(set(a.files) | set(b.files)), n))
    return 1 if n else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
