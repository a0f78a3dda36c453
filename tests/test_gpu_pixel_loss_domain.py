"""-m gpu: the per-pixel loss terms over their domain (csrc/pixel_loss.h, csrc/block_sum.h, csrc/entropy.hip, csrc/boundary.hip,
csrc/pseudo_label.hip).  The cases and the host restatements are tests/pixel_loss_cases.py; tests/
test_pixel_loss_domain_host.py holds them to the branches they are there for.

1. launch geometry: partial lists of 256 and 257 entries, the grid cap with a ragged third trip, every P mod 4, both paths
2. the per-element bound on the shapes and special rows of the feature tests, and on rows 20 ... 104 logits behind their leader
3. one operand misaligned at a time, every output between guards
4. the selection rule on logits that are not filtered, and at the threshold's own bits
5. the threshold update on maps made directly
6. the workspace extent of the four entry points
7. the column pass of the signed distance with 5, 6 and 7 blocks a strip, inputs that are not one-hot, five slices"""
import ctypes

import numpy as np
import pytest
import torch

import pixel_loss_cases as X
from boundary_ref import phi_ref
from conftest import pkg
from kernel_bars import _element_bar, _value_bar
from pseudo_label_ref import order_statistic, pseudo_label_ref, rank_of, update_ref
from test_gpu_boundary import LOSS_SHAPES as BOUNDARY_SHAPES
from test_gpu_boundary import _check_phi
from test_gpu_entropy import SHAPES as ENTROPY_SHAPES
from test_gpu_pseudo_label import SHAPES as PSEUDO_LABEL_SHAPES

pytestmark = pytest.mark.gpu

TERMS = ("entropy", "boundary", "pseudo_label")


def _bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def _place(a, dev, path):
    """"offset": one pixel into an allocation (no 16-byte aligned base: the generic path); else a fresh allocation"""
    t = torch.from_numpy(a).to(dev)
    if path != "offset":
        assert t.data_ptr() % 16 == 0
        return t
    base = torch.zeros((a.shape[0] + 1, a.shape[1]), device=dev)
    base[1:] = t
    assert base[1:].is_contiguous() and base[1:].data_ptr() % 16 != 0
    return base[1:]


def _nsel(C):
    return max(C - 1, 1)


def _check_term(K, dev, term, z, q, path, what):
    """value to _value_bar and gradient to the per-element bar against float64; the value bit for bit without dlogits; two runs bit for
    bit; pseudo-label: the class / selected bytes, the counts, the confidence and the share against the reference's map"""
    P, C = z.shape
    zd = _place(z, dev, path)
    if term == "entropy":
        coef, gk = X.coef_of(term, P, C)
        ref_v, ref_g, scale = X.entropy_elem(z, gk)
        run = lambda **kw: K.softmax_entropy(zd, **kw)
    elif term == "boundary":
        coef, gk = X.coef_of(term, P, C, _nsel(C))
        ref_v, ref_g, scale = X.boundary_elem(z, q, _nsel(C), gk)
        qd = torch.from_numpy(q).to(dev)
        run = lambda **kw: K.boundary_loss(zd, qd, _nsel(C), **kw)
    else:
        return _check_pseudo_label(K, dev, z, zd, what)
    v, g = run(coef=coef, want_grad=True)
    v0, g0 = run()
    v2, g2 = run(coef=coef, want_grad=True)
    assert g0 is None and tuple(v.shape) == (1,) and g.shape == zd.shape
    if C == 1 and term == "entropy":
        assert float(v) == 0.0
    else:
        _value_bar(v, ref_v, what)
    _element_bar(g.cpu().numpy(), ref_g, scale, X.FACTOR, what + " gradient")
    assert torch.equal(_bits(v0), _bits(v)), what + ": dlogits = NULL changes the value"
    assert torch.equal(_bits(v2), _bits(v)) and torch.equal(_bits(g2), _bits(g)), what + ": two runs differ"


def _check_pseudo_label(K, dev, z, zd, what, strict_map=True):
    P, C = z.shape
    tau = X.tau_of(C)
    taud = torch.from_numpy(tau.astype(np.float32)).to(dev)
    coef, gk = X.coef_of("pseudo_label", P, C)
    ref = pseudo_label_ref(z, tau)
    v, share, counts, labels, conf, g = K.pseudo_label_loss(zd, taud, coef=coef, want_grad=True)
    v0, share0, counts0, labels0, conf0, g0 = K.pseudo_label_loss(zd, taud)
    v2, share2, counts2, labels2, conf2, g2 = K.pseudo_label_loss(zd, taud, coef=coef, want_grad=True)
    assert g0 is None and tuple(v.shape) == (1,) and g.shape == zd.shape and tuple(counts.shape) == (2, C)
    lab = labels.cpu().numpy()
    if strict_map:                    # logits kept clear of thresholds and ties: the map is the reference's, byte for byte
        assert np.array_equal(lab, ref["labels"]), what + ": class / selected bytes"
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref["counts"]), what + ": counts"
        assert abs(float(share) - ref["share"]) <= 1e-6
    else:                             # special rows (ties, a confidence of exactly 1): only where the reference is not near an edge
        differ = lab != ref["labels"]
        assert not (differ & ~X.near(z, tau)).any(), what + ": the map differs from float64 away from every threshold and tie"
    k, sel = (lab & 0x7f).astype(np.int64), lab >= 0x80
    cnt = np.stack([np.bincount(k, minlength=C), np.bincount(k[sel], minlength=C)])
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), cnt) and abs(float(share) - sel.mean()) <= 2.0 ** -24
    rel = np.abs(conf.cpu().numpy().astype(np.float64) - ref["conf"]) / ref["conf"]
    assert float(rel.max()) <= 1e-6, what
    ref_v, ref_g, scale = X.pseudo_label_elem(z, k, sel, gk)
    _value_bar(v, ref_v, what)
    _element_bar(g.cpu().numpy(), ref_g, scale, X.FACTOR, what + " gradient")
    assert torch.equal(_bits(v0), _bits(v)) and torch.equal(_bits(share0), _bits(share)) and torch.equal(counts0, counts) \
        and torch.equal(labels0, labels) and torch.equal(_bits(conf0), _bits(conf)), what + ": dlogits = NULL changes an output"
    assert torch.equal(_bits(v2), _bits(v)) and torch.equal(_bits(g2), _bits(g)) and torch.equal(labels2, labels) \
        and torch.equal(counts2, counts) and torch.equal(_bits(conf2), _bits(conf)) and torch.equal(_bits(share2), _bits(share)), what + ": two runs differ"


# ---- 1. launch geometry -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C,path,term", [(P, C, path, term) for P, C, path in X.GEOMETRY for term in TERMS],
                         ids=lambda v: str(v))
def test_launch_geometry(dev, P, C, path, term):
    """the inputs of a case are built once and shared by its terms (geometry_inputs keeps the last case)"""
    K = pkg("kernels")
    z, q = X.geometry_inputs(P, C)
    plan = X.stream_plan(P, C, path == "vector")
    _check_term(K, dev, term, z, q, path, "%s P=%d C=%d %s (%d workgroups, %d trips)" % (term, P, C, path, plan["nblk"], plan["trips"]))


def test_release_the_geometry_inputs():
    X.geometry_inputs.cache_clear()


# ---- 2. the per-element bound on the shapes of the feature tests ---------------------------------------------------------------------------
def test_the_shapes_are_those_of_the_feature_tests():
    assert X.ENTROPY_SHAPES == ENTROPY_SHAPES and X.BOUNDARY_SHAPES == BOUNDARY_SHAPES and X.PSEUDO_LABEL_SHAPES == PSEUDO_LABEL_SHAPES


@pytest.mark.parametrize("P,C,term", [(P, C, term) for term, shapes in zip(TERMS, (X.ENTROPY_SHAPES, X.BOUNDARY_SHAPES, X.PSEUDO_LABEL_SHAPES))
                                      for P, C in shapes], ids=lambda v: str(v))
def test_per_element_bound_on_the_feature_shapes(dev, P, C, term):
    K = pkg("kernels")
    z, q = X.element_inputs(P, C)
    what = "%s P=%d C=%d" % (term, P, C)
    if term == "pseudo_label":
        _check_pseudo_label(K, dev, z, torch.from_numpy(z).to(dev), what, strict_map=False)
    else:
        _check_term(K, dev, term, z, q, "aligned", what)


# ---- 3. one operand misaligned at a time -----------------------------------------------------------------------------------------------------
GUARD = 256
SENTINEL = 0x5A


class _Arena:
    """an operand of nbytes that starts `off` bytes behind a 256-byte guard inside a sentinel-filled allocation"""

    def __init__(self, dev, nbytes, off=0, src=None):
        self.n, self.lo = int(nbytes), GUARD + off
        self.base = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 16 == 0
        if src is not None:
            src = np.ascontiguousarray(src)
            assert src.nbytes == self.n
            self.base[self.lo:self.lo + self.n] = torch.from_numpy(src.view(np.uint8).reshape(-1)).to(dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.base.data_ptr() + self.lo)

    def get(self, dtype):
        return self.base[self.lo:self.lo + self.n].cpu().numpy().view(dtype)

    def guards_intact(self):
        b = self.base.cpu().numpy()
        return bool((b[:self.lo] == SENTINEL).all() and (b[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.base == SENTINEL).all())


def _raw(dev, term, z, q, tau, coef, offs=None, ws_bytes=None, grad=True, mask=None):
    """one call of the term's entry point through ctypes: every operand in an arena of its own, `offs[name]` bytes into it; the workspace
    exactly ws_bytes long (default: what the library asks for) -> (return code, {name: arena})"""
    L = pkg("_lib")
    lib = L.load()
    offs = offs or {}
    P, C = z.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = {"entropy": lib.pnp_softmax_entropy_workspace_bytes, "boundary": lib.pnp_boundary_loss_workspace_bytes,
            "pseudo_label": lib.pnp_pseudo_label_loss_workspace_bytes}[term](P, C)
    ws_bytes = need if ws_bytes is None else ws_bytes
    A = {"logits": _Arena(dev, z.nbytes, offs.get("logits", 0), z), "dlogits": _Arena(dev, z.nbytes, offs.get("dlogits", 0)),
         "out": _Arena(dev, 8), "ws": _Arena(dev, max(ws_bytes, 1))}
    dl = A["dlogits"].ptr if grad else None
    if term == "entropy":
        code = lib.pnp_softmax_entropy(A["logits"].ptr, P, C, coef, dl, A["out"].ptr, A["ws"].ptr, ws_bytes, st)
    elif term == "boundary":
        A["phi"] = _Arena(dev, q.nbytes, offs.get("phi", 0), q)
        code = lib.pnp_boundary_loss(A["logits"].ptr, A["phi"].ptr, P, C, _nsel(C), coef, dl, A["out"].ptr, A["ws"].ptr, ws_bytes, st)
    else:
        A["tau"] = _Arena(dev, 4 * C, 0, np.asarray(tau, dtype=np.float32))
        A["labels"] = _Arena(dev, P, offs.get("labels", 0))
        A["conf"] = _Arena(dev, 4 * P, offs.get("conf", 0))
        A["counts"] = _Arena(dev, 8 * C)
        code = lib.pnp_pseudo_label_loss(A["logits"].ptr, A["tau"].ptr, P, C, (1 << C) - 1 if mask is None else mask, coef, dl, A["labels"].ptr,
                                         A["conf"].ptr, A["out"].ptr, A["counts"].ptr, A["ws"].ptr, ws_bytes, st)
    torch.cuda.synchronize()
    return code, A


OUTPUTS = {"entropy": ("dlogits",), "boundary": ("dlogits",), "pseudo_label": ("dlogits", "labels", "conf", "counts")}


@pytest.mark.parametrize("P", X.MISALIGNED_P)
@pytest.mark.parametrize("term", TERMS)
def test_one_operand_misaligned_at_a_time(dev, term, P):
    """every operand whose address pixel_loss::run / pnp_pseudo_label_loss test, moved off its alignment alone: the launch takes the generic
    path, which runs the same `pixel` function (tests/test_gpu_pixel_loss.py) — gradient words, label bytes, counts and confidence words
    are those of the all-aligned launch bit for bit, the value is within 1e-6 of it, and nothing is written outside an operand"""
    L = pkg("_lib")
    z, q = X.element_inputs(P, 5)
    tau = X.tau_of(5)
    coef = X.coef_of(term, P, 5, 4)[0]
    code, ref = _raw(dev, term, z, q, tau, coef)
    L.check(code, term)
    v_ref = float(ref["out"].get(np.float32)[0])
    assert all(a.guards_intact() for a in ref.values()) and np.abs(ref["dlogits"].get(np.float32)).max() > 0
    for name, off in X.MISALIGNED[term]:
        code, got = _raw(dev, term, z, q, tau, coef, {name: off})
        L.check(code, term)
        assert got[name].ptr.value % (4 if name == "labels" else 16) != 0
        for a_name, a in got.items():
            assert a.guards_intact(), "%s P=%d, %s %d bytes in: something was written outside %s" % (term, P, name, off, a_name)
        for o in OUTPUTS[term]:
            assert np.array_equal(got[o].get(np.uint8), ref[o].get(np.uint8)), "%s P=%d, %s %d bytes in: %s differs" % (term, P, name, off, o)
        v = float(got["out"].get(np.float32)[0])
        print("%s P=%d, %s %d bytes in: value %.9g, aligned %.9g" % (term, P, name, off, v, v_ref))
        assert abs(v - v_ref) <= 1e-6 * abs(v_ref)
        if term == "pseudo_label":
            assert got["out"].get(np.float32)[1] == ref["out"].get(np.float32)[1]


# ---- 4. the selection rule on logits that are not filtered ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C,path,seed", X.SELECTION, ids=lambda v: str(v))
def test_selection_rule_on_unfiltered_logits(dev, P, C, path, seed):
    K = pkg("kernels")
    z = X.selection_logits(P, C, seed)
    zd = _place(z, dev, path)
    tau = X.tau_of(C)
    tau32 = tau.astype(np.float32)
    coef, gk = X.coef_of("pseudo_label", P, C)
    what = "unfiltered P=%d C=%d %s" % (P, C, path)
    near = X.near(z, tau)
    assert near.mean() <= X.NEAR_CAP
    ref = pseudo_label_ref(z, tau)
    for classes in (None, tuple(range(1, C))):
        v, share, counts, labels, conf, g = K.pseudo_label_loss(zd, torch.from_numpy(tau32).to(dev), classes, coef=coef, want_grad=True)
        lab, conf_dev = labels.cpu().numpy(), conf.cpu().numpy()
        k_dev, sel_dev = (lab & 0x7f).astype(np.int64), (lab >> 7).astype(bool)
        in_mask = np.ones(C, bool) if classes is None else np.isin(np.arange(C), classes)
        # (a) the rule in float32 on the device's own confidence, exactly, for every pixel
        assert k_dev.max() < C and np.array_equal(sel_dev, in_mask[k_dev] & (conf_dev >= tau32[k_dev])), what
        # (b) against float64 the map differs only where the reference itself is near a threshold or a tie
        want = (ref["labels"] & 0x7f) | ((ref["sel"] & in_mask[ref["labels"] & 0x7f]).astype(np.uint8) << 7)
        differ = lab != want
        print("%s classes %s: %d bytes differ from float64, %d pixels are near an edge; selected %d" % (what, classes, differ.sum(), near.sum(), sel_dev.sum()))
        assert not (differ & ~near).any(), what
        # (c) the counts and the share are those of the device's own bytes
        cnt = np.stack([np.bincount(k_dev, minlength=C), np.bincount(k_dev[sel_dev], minlength=C)])
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), cnt) and abs(float(share) - sel_dev.sum() / P) <= 2.0 ** -24
        # (d), (e) value and gradient against float64 under the device's own map
        ref_v, ref_g, scale = X.pseudo_label_elem(z, k_dev, sel_dev, gk)
        _value_bar(v, ref_v, what)
        gh = g.cpu().numpy()
        assert not gh[~sel_dev].any(), what + ": a gradient off the selected pixels"
        _element_bar(gh, ref_g, scale, X.FACTOR, what + " gradient")
    # the edge itself: the threshold of every class at the confidence bits of one of its pixels, then one float above them
    lab = K.pseudo_label_loss(zd, torch.zeros(C, device=dev))[3].cpu().numpy()
    pick = np.array([int(np.flatnonzero((lab & 0x7f) == k)[5 + k]) for k in range(C)])
    at = conf_dev[pick].copy()
    above = np.nextafter(at, np.float32(np.inf))
    assert (above > at).all() and at.dtype == np.float32
    lab_at = K.pseudo_label_loss(zd, torch.from_numpy(at).to(dev))[3].cpu().numpy()
    lab_above = K.pseudo_label_loss(zd, torch.from_numpy(above).to(dev))[3].cpu().numpy()
    assert [int(b) for b in lab_at[pick]] == [k | 0x80 for k in range(C)], what + ": conf == tau is not selected"
    assert [int(b) for b in lab_above[pick]] == list(range(C)), what + ": conf one float below tau is selected"
    assert np.array_equal(lab_at >> 7, conf_dev >= at[lab_at & 0x7f]) and np.array_equal(lab_above >> 7, conf_dev >= above[lab_above & 0x7f])


# ---- 5. the threshold update on maps made directly -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("portion", X.UPDATE_PORTIONS)
@pytest.mark.parametrize("P", X.UPDATE_P)
def test_update_on_maps_made_directly(dev, P, portion):
    """(negative or NaN confidences are outside the entry's contract: the loss writes 1 / s with s >= 1)"""
    K = pkg("kernels")
    C = X.UPDATE_C
    conf, lab = X.update_maps(P, P)
    keep = (lab & 0x7f) < C
    want_q = order_statistic(conf[keep], lab[keep], C, portion)
    n = np.bincount(lab[keep] & 0x7f, minlength=C)
    assert n[1] == 10 and n[6] == 25 and n[3] == 1 and n[4] == 0
    if portion == 0.28:
        assert rank_of(portion, 25) == 8 and want_q[6] == np.sort(conf[(lab & 0x7f) == 6])[::-1][7]
    if portion == 0.3:
        assert rank_of(portion, 10) == 3
    tau0 = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], dtype=np.float32)
    confd, labd = torch.from_numpy(conf).to(dev), torch.from_numpy(lab).to(dev)
    confk, labk = torch.from_numpy(conf[keep]).to(dev), torch.from_numpy(lab[keep]).to(dev)
    for beta in X.UPDATE_BETAS:
        what = "P=%d portion %g beta %g" % (P, portion, beta)
        t = torch.from_numpy(tau0).to(dev)
        q = K.pseudo_label_update(labd, confd, t, portion, beta).cpu().numpy()
        tk = torch.from_numpy(tau0).to(dev)
        qk = K.pseudo_label_update(labk, confk, tk, portion, beta).cpu().numpy()
        assert np.array_equal(q.view(np.uint32), want_q.view(np.uint32)), (what, q.tolist(), want_q.tolist())      # (the NaN of the empty class included)
        assert np.array_equal(qk.view(np.uint32), q.view(np.uint32)), what + ": the ignored bytes change q"
        th = t.cpu().numpy()
        assert np.array_equal(tk.cpu().numpy().view(np.uint32), th.view(np.uint32)), what
        assert th[4].view(np.uint32) == tau0[4].view(np.uint32)                       # the empty class keeps its threshold
        live = np.arange(C) != 4
        if beta == 0.0:
            assert np.array_equal(th[live].view(np.uint32), q[live].view(np.uint32)), what
        elif beta == 1.0:
            assert np.array_equal(th.view(np.uint32), tau0.view(np.uint32)), what
        want = update_ref(tau0, q, beta)
        assert float((np.abs(th.astype(np.float64) - want)[live] / np.maximum(np.abs(want[live]), 2.0 ** -126)).max()) <= 1e-6, what


# ---- 6. the workspace extent -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", TERMS)
def test_loss_workspace_extent(dev, term):
    """257 workgroups: with exactly the bytes the library asks for the call succeeds and writes nothing behind them; with one byte less it
    is refused and writes nothing at all"""
    L = pkg("_lib")
    P, C = X.EXTENT_P, 5
    z, q = X.geometry_inputs(P, C)
    tau = X.tau_of(C)
    coef = X.coef_of(term, P, C, 4)[0]
    need = {"entropy": X.entropy_workspace_bytes, "boundary": X.boundary_workspace_bytes, "pseudo_label": X.pseudo_label_loss_workspace_bytes}[term](P, C)
    code, A = _raw(dev, term, z, q, tau, coef, ws_bytes=need)
    L.check(code, term)
    assert all(a.guards_intact() for a in A.values()), term
    assert not (A["ws"].get(np.uint8) == SENTINEL).all() and np.abs(A["dlogits"].get(np.float32)).max() > 0
    wrapped = {"entropy": lambda K: K.softmax_entropy(torch.from_numpy(z).to(dev))[0],
               "boundary": lambda K: K.boundary_loss(torch.from_numpy(z).to(dev), torch.from_numpy(q).to(dev), 4)[0],
               "pseudo_label": lambda K: K.pseudo_label_loss(torch.from_numpy(z).to(dev), torch.from_numpy(tau.astype(np.float32)).to(dev))[0]}
    assert float(wrapped[term](pkg("kernels"))) == float(A["out"].get(np.float32)[0])
    code, A = _raw(dev, term, z, q, tau, coef, ws_bytes=need - 1)
    with pytest.raises(L.PnpError, match="workspace too small"):
        L.check(code, term)
    for name, a in A.items():
        if name not in ("logits", "phi", "tau"):
            assert a.untouched(), "%s: the refused call wrote %s" % (term, name)
    X.geometry_inputs.cache_clear()


def test_update_workspace_extent(dev):
    L = pkg("_lib")
    lib = L.load()
    P, C = 65537, X.UPDATE_C
    conf, lab = X.update_maps(P, P)
    tau0 = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], dtype=np.float32)
    need = lib.pnp_pseudo_label_update_workspace_bytes(P, C)
    assert need == X.pseudo_label_update_workspace_bytes(P, C)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nbytes in (need, need - 1):
        A = {"labels": _Arena(dev, P, 0, lab), "conf": _Arena(dev, 4 * P, 0, conf), "tau": _Arena(dev, 4 * C, 0, tau0), "q": _Arena(dev, 4 * C),
             "ws": _Arena(dev, nbytes)}
        code = lib.pnp_pseudo_label_update(A["labels"].ptr, A["conf"].ptr, P, C, 0.5, 0.0, A["tau"].ptr, A["q"].ptr, A["ws"].ptr, nbytes, st)
        torch.cuda.synchronize()
        assert all(a.guards_intact() for a in A.values())
        if nbytes == need:
            L.check(code, "pnp_pseudo_label_update")
            q = A["q"].get(np.float32)
            assert np.array_equal(q.view(np.uint32), order_statistic(conf, lab, C, 0.5).view(np.uint32))
            live = np.arange(C) != 4
            assert np.array_equal(A["tau"].get(np.uint32)[live], q.view(np.uint32)[live]) and A["tau"].get(np.uint32)[4] == tau0.view(np.uint32)[4]
            # the selection state behind the four rounds of bins: n_k of every class
            state = A["ws"].get(np.uint32)[4 * 8 * 256:].reshape(8, 3)
            assert state[:C, 2].tolist() == np.bincount(lab & 0x7f, minlength=128)[:C].tolist() and not state[C:].any()
        else:
            with pytest.raises(L.PnpError, match="workspace too small"):
                L.check(code, "pnp_pseudo_label_update")
            assert A["ws"].untouched() and A["q"].untouched() and np.array_equal(A["tau"].get(np.uint32), tau0.view(np.uint32))


# ---- 7. the signed distance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,classes", X.SDIST_PARTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "c%d" % len(v))
def test_distance_kernel_with_5_6_and_7_blocks_a_strip(dev, shape, classes):
    K = pkg("kernels")
    B, H, W, C = shape
    plan = X.col_plan(H, W, C, len(classes))
    oh = X.sdist_labels(B, H, W, C, H + W + C)
    ref_all, d2_all = phi_ref(oh, classes=range(C))
    assert d2_all.any()
    _check_phi(K, dev, oh, ref_all, d2_all, classes, "%s: %d blocks a strip of %d columns" % (shape, plan["parts"], plan["tw"]))


def test_distance_kernel_five_slices_each_with_another_class_absent_or_full(dev):
    K = pkg("kernels")
    B, H, W, C = X.SDIST_BATCH
    oh = X.sdist_labels(B, H, W, C, 11)
    lab = oh.argmax(-1)
    lab[0][lab[0] == 1] = 0                  # class 1 absent from slice 0
    lab[1][:] = 2                            # class 2 fills slice 1 (every other class absent)
    lab[2][lab[2] == 3] = 4                  # class 3 absent from slice 2
    lab[3][:] = 4                            # class 4 fills slice 3
    lab[4][lab[4] == 0] = 1                  # class 0 absent from slice 4
    oh = np.stack([(lab == c) for c in range(C)], axis=-1).astype(np.float32)
    ref_all, d2_all = phi_ref(oh, classes=range(C))
    assert not d2_all[0, :, :, 1].any() and not d2_all[1].any() and not d2_all[2, :, :, 3].any() and not d2_all[3].any() and not d2_all[4, :, :, 0].any()
    assert d2_all[0, :, :, 2].any() and d2_all[2, :, :, 1].any() and d2_all[4, :, :, 1].any()
    for classes in (list(range(C)), None, [1, 3]):
        _check_phi(K, dev, oh, ref_all, d2_all, classes, "five slices, classes %s" % (classes,))


def test_distance_kernel_inputs_that_are_not_one_hot(dev):
    """membership is `> 0.5` per class: a pixel in no class, in two classes, values of exactly 0.5, the float above it, -1 and NaN"""
    K = pkg("kernels")
    B, H, W, C = 2, 20, 70, 5
    rng = np.random.default_rng(5)
    oh = X.sdist_labels(B, H, W, C, 13)
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    rows = np.array([[0, 0, 0, 0, 0], [0, 1, 1, 0, 0], [0.5, 0.5, 0.5, 0.5, 0.5], [0.5, up, 0.5, up, 0.25], [-1, -1, 1, -1, -1],
                     [np.nan, 1, np.nan, np.nan, np.nan], [np.nan] * 5, [0.75, 0.75, 0.75, 0.75, 0.75]], dtype=np.float32)
    which = rng.integers(0, 10 * len(rows), (B, H, W))
    for r, row in enumerate(rows):
        oh[which == r] = row
    assert all((which == r).sum() > 5 for r in range(len(rows)))
    member = oh > 0.5
    assert (member.sum(-1) == 0).any() and (member.sum(-1) == 2).any() and (member.sum(-1) == 5).any() and np.isnan(oh).any()
    ref_all, d2_all = phi_ref(oh, classes=range(C))
    for classes in (list(range(C)), None, [2]):
        _check_phi(K, dev, oh, ref_all, d2_all, classes, "not one-hot, classes %s" % (classes,))
