"""Bit-for-bit A/B of the per-pixel loss terms (csrc/pixel_loss.h: entropy, boundary, pseudo-label) between two builds of the library.

    PNP_LIB=<one libpnp_hip.so>     python tools/pixel_loss_ab.py dump a.npz
    PNP_LIB=<another libpnp_hip.so> python tools/pixel_loss_ab.py dump b.npz
    python tools/pixel_loss_ab.py compare a.npz b.npz        # one line per array (dtype, shape and bytes), exit status 1 if any differs

`dump` writes EVERY output of the three terms — value, gradient, and for the pseudo-label term share, counts, class / selected bytes and
confidences — with and without want_grad, over the case tables of tests/pixel_loss_cases.py: GEOMETRY (1 to 2 048 workgroups, the ragged
third trip at the grid cap, both paths), ELEMENT_SHAPES (the SHAPES / LOSS_SHAPES of the three feature files), every operand of
MISALIGNED moved off its alignment alone at P = 7 and 1021 (through ctypes), and one pseudo_label_update after a loss (q and the
thresholds).  The file holds about 0.9 GB: the cap cases keep their whole gradients."""
import ctypes
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pixel_loss_cases as X      # noqa: E402

TERMS = ("entropy", "boundary", "pseudo_label")


def _place(a, dev, path):
    t = torch.from_numpy(a).to(dev)
    if path != "offset":
        return t
    base = torch.zeros((a.shape[0] + 1, a.shape[1]), device=dev)
    base[1:] = t
    return base[1:]


def _terms(K, out, tag, z, q, path, dev):
    P, C = z.shape
    nsel = max(C - 1, 1)
    zd, qd = _place(z, dev, path), _place(q, dev, path)
    tau = torch.from_numpy(X.tau_of(C).astype(np.float32)).to(dev)
    runs = {"entropy": lambda **kw: K.softmax_entropy(zd, **kw), "boundary": lambda **kw: K.boundary_loss(zd, qd, nsel, **kw),
            "pseudo_label": lambda **kw: K.pseudo_label_loss(zd, tau, **kw)}
    names = {"entropy": ("value", "grad"), "boundary": ("value", "grad"), "pseudo_label": ("value", "share", "counts", "labels", "conf", "grad")}
    for term in TERMS:
        coef = X.coef_of(term, P, C, nsel)[0]
        for suffix, res in (("", runs[term](coef=coef, want_grad=True)), (" nograd", runs[term]())):
            for name, t in zip(names[term], res):
                if t is not None:
                    out["%s %s %s%s" % (term, tag, name, suffix)] = t.cpu().numpy()


def _buffer(dev, nbytes, off, src=None):
    """nbytes that start 256 + off bytes into an allocation of their own -> (allocation, view of the bytes)"""
    base = torch.zeros(256 + off + nbytes, dtype=torch.uint8, device=dev)
    view = base[256 + off:256 + off + nbytes]
    if src is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(-1)).to(dev))
    return base, view


def _misaligned(lib, check, out, dev, term, P, name, off):
    z, q = X.element_inputs(P, 5)
    C = 5
    offs = {name: off}
    B = {"logits": _buffer(dev, z.nbytes, offs.get("logits", 0), z), "dlogits": _buffer(dev, z.nbytes, offs.get("dlogits", 0)),
         "phi": _buffer(dev, q.nbytes, offs.get("phi", 0), q), "tau": _buffer(dev, 4 * C, 0, X.tau_of(C).astype(np.float32)),
         "labels": _buffer(dev, P, offs.get("labels", 0)), "conf": _buffer(dev, 4 * P, offs.get("conf", 0)), "out": _buffer(dev, 8, 0),
         "counts": _buffer(dev, 8 * C, 0)}
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in B.items()}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    coef = X.coef_of(term, P, C, 4)[0]
    if term == "entropy":
        need = lib.pnp_softmax_entropy_workspace_bytes(P, C)
        ws = _buffer(dev, need, 0)
        code = lib.pnp_softmax_entropy(p["logits"], P, C, coef, p["dlogits"], p["out"], ctypes.c_void_p(ws[1].data_ptr()), need, st)
        outs = {"dlogits": np.float32, "out": np.float32}
    elif term == "boundary":
        need = lib.pnp_boundary_loss_workspace_bytes(P, C)
        ws = _buffer(dev, need, 0)
        code = lib.pnp_boundary_loss(p["logits"], p["phi"], P, C, 4, coef, p["dlogits"], p["out"], ctypes.c_void_p(ws[1].data_ptr()), need, st)
        outs = {"dlogits": np.float32, "out": np.float32}
    else:
        need = lib.pnp_pseudo_label_loss_workspace_bytes(P, C)
        ws = _buffer(dev, need, 0)
        code = lib.pnp_pseudo_label_loss(p["logits"], p["tau"], P, C, (1 << C) - 1, coef, p["dlogits"], p["labels"], p["conf"], p["out"],
                                         p["counts"], ctypes.c_void_p(ws[1].data_ptr()), need, st)
        outs = {"dlogits": np.float32, "out": np.float32, "labels": np.uint8, "conf": np.float32, "counts": np.int32}
    torch.cuda.synchronize()
    check(code, term)
    for o, dt in outs.items():
        a = B[o][1].cpu().numpy().view(dt)
        out["%s misaligned P%d %s+%d %s" % (term, P, name, off, o)] = a[:1] if o == "out" and term != "pseudo_label" else a


def dump(path):
    K = importlib.import_module("medical-cross-modality-domain-adaptation_amd.kernels")
    L = importlib.import_module("medical-cross-modality-domain-adaptation_amd._lib")
    dev = torch.device("cuda:0")
    out = {}
    for P, C, where in X.GEOMETRY:
        z, q = X.geometry_inputs(P, C)
        _terms(K, out, "geometry P%d C%d %s" % (P, C, where), z, q, where, dev)
    X.geometry_inputs.cache_clear()
    for P, C in X.ELEMENT_SHAPES:
        z, q = X.element_inputs(P, C)
        _terms(K, out, "shapes P%d C%d" % (P, C), z, q, "aligned", dev)
    for term in TERMS:
        for P in X.MISALIGNED_P:
            for name, off in X.MISALIGNED[term]:
                _misaligned(L.load(), L.check, out, dev, term, P, name, off)
    z, _ = X.element_inputs(2 * 256 * 256, 5)
    tau = torch.from_numpy(X.tau_of(5).astype(np.float32)).to(dev)
    _, _, _, labels, conf, _ = K.pseudo_label_loss(torch.from_numpy(z).to(dev), tau)
    out["pseudo_label update q"] = K.pseudo_label_update(labels, conf, tau, 0.5, 0.9).cpu().numpy()
    out["pseudo_label update thresholds"] = tau.cpu().numpy()
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
        print("%-9s %-64s %s %s" % ("equal" if same else "DIFFERS", name, x.dtype, x.shape))
    print("VERDICT: %d arrays, %d differ" % (len(set(a.files) | set(b.files)), n))
    return 1 if n else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
