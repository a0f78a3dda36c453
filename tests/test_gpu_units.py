"""-m gpu: the autograd Functions of functional.py and the blocks of layers.py, run through torch.autograd and held to the float64
restatement of tests/unit_ref.py — every output, every gradient that is asked for, and the BN moving statistics after the forward.

The teacher-forced files restate this glue by hand and never run it; the whole-step tests run it at 256 x 256 only, inside the band that
leaky-ReLU slope flips leave; the bit-equality tests compare it with itself.  Here the shapes are tiny and every case's seed is chosen so
that, in float64, no pre-activation is within 1e-4 of max|v| of zero and no 2x2 pool window within that of a tie (unit_ref.clearance,
asserted below on the reference each test computes and on the CPU by tests/test_units_host.py): nothing flips, no pixel is excluded,
and the Functions meet the per-kernel bar teacher_forced.TOL = 1e-4 of max|ref| (moving statistics: 1e-5).

bf16 mode has no derived bar: for every case the float64 restatement with both operands of every convolution rounded to bf16 is compared
with the un-rounded one; that difference E (of max|ref|) is the case's rounding budget and the product must be within 2 E + 1e-4 of the
un-rounded reference.  `pytest -s` prints E and every measured error.  A case whose convolutions the typed dispatch kept on float32
kernels (prof_summary names them) is held to the float32 bar instead: nothing was rounded, there is no budget to spend.

Shapes: N = 2, 8 x 8 and 7 x 9, 8 -> 16 and 5 -> 7 channels, nothing above (2, 16, 16, 32 -> 64) — but for the three resident-bf16 cases:
that kernel family serves nothing below 4096 output pixels, (4, 32, 32, 64 -> 64) is the smallest it takes.

Out of scope: sync=True (synchronised statistics need ranks; tests/test_gpu_dp.py::test_two_ranks_equal_one_gpu owns that path).
"""
import numpy as np
import pytest
import torch

import unit_ref as R
from conftest import pkg
from parity_util import rel
from teacher_forced import TOL

pytestmark = pytest.mark.gpu

MOV_TOL = 1e-5                          # BN moving mean / variance
LOSS_TOL = (2e-5, 1e-5, 1e-5)           # §4.7: segmentation loss total / cross-entropy / Dice, absolute
WGAN_TOL = 1e-6                         # §4.7: of sum|coef| * mean|x|
_REF = {}


# ---- the reference, computed once per (case, rounding, roots) and never written afterwards -----------------------------------------------
def ref_of(c, rnd=None, roots=None):
    key = (c["id"], rnd is not None, roots)
    if key not in _REF:
        r = R.run_ref(c, rnd)
        if rnd is None and c.get("clear", True):
            m = R.clearance(r["L"].rec)
            assert m >= R.MARGIN, "case %s: the float64 reference comes within %.2e of a slope flip / pool tie" % (c["id"], m)
        idx = range(len(r["outs"])) if roots is None else roots
        torch.autograd.backward([r["outs"][i] for i in idx], [r["douts"][i] for i in idx])
        _REF[key] = r
    return _REF[key]


def ref_tensors(r):
    """name -> float64 reference of every output, input gradient, parameter gradient and moving statistic"""
    out = {"out%d" % i: o.detach() for i, o in enumerate(r["outs"])}
    for k, t in r["X"].items():
        out["d_in_" + k] = t.grad
    for n, t in r["L"].V.items():
        if n.endswith("moving_mean") or n.endswith("moving_variance"):
            out[n] = t
        else:
            out["d_" + n] = t.grad if r["L"].trainable[n] else None
    return out


# ---- the product side of a program ---------------------------------------------------------------------------------------------------------
class ProductLayers(object):
    """the product's layers / ops / fan_out under the names a program uses; variables come from the active VariableStore"""

    def __init__(self, st):
        self.st, self.layers, self.ops, self.fn = st, pkg("layers"), pkg("ops"), pkg("functional")

    def var(self, name, shape, trainable=True):
        return self.st.get(name, tuple(shape), 0.0, trainable, "weight").tensor

    def __getattr__(self, name):
        if name == "PS_conv2d":
            return self.ops.PS_conv2d
        if name == "fan_out":
            return self.fn.fan_out
        return getattr(self.layers, name)


def _dev(a, dev, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad)


def run_layers(c, dev, mode="store", roots=None, overlap=False, after_forward=None, root_fn=None):
    """the case's program through layers.py.  mode 'store': a finalized VariableStore, parameter gradients go through the sinks into
    grad_arena; 'leaf': the same variables as plain leaf tensors, gradients are returned to the engine.  root_fn(outs, X) -> (roots,
    upstream gradients) replaces the random upstream gradients.  -> name -> tensor, as ref_tensors names them"""
    V, Fn = pkg("variables"), pkg("functional")
    st = V.VariableStore(dev)
    L = ProductLayers(st)
    shapes = R.input_shapes(c)
    prog = R.PROGRAMS[c["prog"]]
    with st.as_default():
        st.begin_trace()
        prog(L, {k: torch.empty(s, device="meta") for k, s in shapes.items()}, c)          # build pass: creates the variables
        if mode == "store":
            st.finalize()
        st.load_state_dict({n: R.init_value(c["seed"], n, v.shape) for n, v in st.vars.items()})
        if mode == "leaf":
            for v in st.vars.values():
                if v.trainable:
                    v.tensor.requires_grad_(True)
        else:
            st.zero_grad()
        st.begin_trace(drop_seed=c["drop_seed"])
        X = {k: _dev(R.init_value(c["seed"], "in_" + k, s), dev, True) for k, s in shapes.items()}
        outs = prog(L, X, c)
        if after_forward is not None:
            after_forward(st)
        if root_fn is not None:
            rts, ups = root_fn(outs, X)
        else:
            idx = range(len(outs)) if roots is None else roots
            rts = [outs[i] for i in idx]
            ups = [_dev(R.init_value(c["seed"], "dout%d" % i, tuple(outs[i].shape)), dev) for i in idx]
        if overlap:
            with Fn.wgrad_overlap():
                torch.autograd.backward(rts, ups)
        else:
            torch.autograd.backward(rts, ups)
    torch.cuda.synchronize()
    got = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    for k, t in X.items():
        got["d_in_" + k] = t.grad
    for n, v in st.vars.items():
        if n.endswith("moving_mean") or n.endswith("moving_variance"):
            got[n] = v.tensor.detach()
        else:
            got["d_" + n] = v.tensor.grad if v.trainable else None
    got["_store"] = st
    return got


def run_direct(c, dev, want=None, between=None):
    """one unit, functional.ConvBNActFn.apply on leaf tensors (SYMMETRIC: functional.SymPadFn in front, as layers._prepad does).
    want: which of x, w, gamma, beta, sc require a gradient (None: all, gamma / beta only when the case trains them)"""
    K, Fn = pkg("kernels"), pkg("functional")
    N, H, W, C, Kc = c["shape"]
    k = c["k"]
    if want is None:
        want = ("x", "w", "sc") + (("gamma", "beta") if c["bn_trainable"] else ())
    shapes = R.input_shapes(c)
    x = _dev(R.init_value(c["seed"], "in_x", shapes["x"]), dev, "x" in want)
    sc = _dev(R.init_value(c["seed"], "in_sc", shapes["sc"]), dev, "sc" in want) if "sc" in shapes else None
    w = _dev(R.init_value(c["seed"], "w", (k, k, C, Kc)), dev, "w" in want)
    gamma, beta = (_dev(R.init_value(c["seed"], "u/" + n, (Kc,)), dev, n in want) for n in ("gamma", "beta"))
    mm, mv = (_dev(R.init_value(c["seed"], "u/" + n, (Kc,)), dev) for n in ("moving_mean", "moving_variance"))
    xin, padding = x, c["padding"]
    if padding == "SYMMETRIC":
        xin, padding = Fn.SymPadFn.apply(x, k // 2), "VALID"
    g = K.conv_geom(tuple(xin.shape), tuple(w.shape), c["stride"], c["dil"], padding)
    out = Fn.ConvBNActFn.apply(xin, w, gamma, beta, mm, mv, sc, g, float(c["keep"]), c["drop_seed"], 0, bool(c["is_train"]),
                               float(c["alpha"]), False, None, True)
    if between is not None:
        between(dict(x=x, w=w, gamma=gamma, beta=beta, mm=mm, mv=mv, sc=sc, g=g))
    out.backward(_dev(R.init_value(c["seed"], "dout0", tuple(out.shape)), dev))
    torch.cuda.synchronize()
    return {"out0": out.detach(), "d_in_x": x.grad, "d_in_sc": sc.grad if sc is not None else None, "d_w": w.grad, "d_u/gamma": gamma.grad,
            "d_u/beta": beta.grad, "u/moving_mean": mm, "u/moving_variance": mv, "_geom": g}


# ---- comparison ------------------------------------------------------------------------------------------------------------------------------
def compare(tag, got, ref, expect_none=(), tol=TOL, budget=None):
    """every tensor of `ref` against `got`: |got - ref| <= tol * max|ref| (moving statistics: MOV_TOL); with `budget` (name -> E) the bar
    of a tensor is 2 E + tol.  A gradient the reference has and the product does not is a failure; names in expect_none must be None"""
    errs, bad = {}, []
    for n, r in ref.items():
        g = got.get(n)
        if n in expect_none:
            if g is not None:
                bad.append("%s: a gradient that was not asked for was returned" % n)
            continue
        if r is None:
            if g is not None and float(g.abs().max()) != 0.0:
                bad.append("%s: gradient for a variable the reference does not differentiate" % n)
            continue
        if g is None:
            bad.append("%s: no gradient" % n)
            continue
        assert tuple(g.shape) == tuple(r.shape), (n, g.shape, r.shape)
        e = rel(g, r)
        stat = n.endswith("moving_mean") or n.endswith("moving_variance")
        bar = (MOV_TOL if stat else tol) + (2.0 * budget[n] if budget is not None else 0.0)
        errs[n] = (e, bar)
        if not e <= bar:
            bad.append("%s: %.3e > %.3e" % (n, e, bar))
    print("units %-52s %s" % (tag, "  ".join("%s %.2e" % (n, e) for n, (e, _) in sorted(errs.items()))))
    if budget is not None:
        print("units %-52s E: %s" % (tag, "  ".join("%s %.2e" % (n, budget[n]) for n in sorted(errs))))
    assert not bad, "%s: %s" % (tag, "; ".join(bad))
    return errs


def stats_untouched(c, got, prefix="u"):
    for n in ("moving_mean", "moving_variance"):
        name = "%s/%s" % (prefix, n)
        assert torch.equal(got[name].cpu(), torch.from_numpy(R.init_value(c["seed"], name, tuple(got[name].shape)))), name


def _ids(cases):
    return [c["id"] for c in cases]


# ---- (a) one conv-BN unit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", ["direct", "layers"])
@pytest.mark.parametrize("c", R.UNIT_CASES, ids=_ids(R.UNIT_CASES))
def test_unit(dev, c, via):
    K = pkg("kernels")
    ref = ref_tensors(ref_of(c))
    got = run_direct(c, dev) if via == "direct" else run_layers(c, dev)
    if "parts" in c:
        g = got["_geom"] if via == "direct" else K.conv_geom(R.input_shapes(c)["x"], (c["k"], c["k"]) + tuple(c["shape"][3:]), c["stride"], c["dil"],
                                                            c["padding"])
        assert (K.conv_stats_parts(g) > 0) == c["parts"], "the planner no longer routes this case to the branch it is here for"
    compare("%s[%s]" % (c["id"], via), got, ref)
    if not c["is_train"]:
        stats_untouched(c, got)


# ---- (b) subsets of needs_input_grad --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", sorted(R.GRAD_SUBSETS))
@pytest.mark.parametrize("c", R.SUBSET_CASES, ids=_ids(R.SUBSET_CASES))
def test_unit_gradient_subsets(dev, c, subset):
    want = R.GRAD_SUBSETS[subset]
    ref = ref_tensors(ref_of(c))
    got = run_direct(c, dev, want=want)
    names = {"x": "d_in_x", "sc": "d_in_sc", "w": "d_w", "gamma": "d_u/gamma", "beta": "d_u/beta"}
    compare("%s[%s]" % (c["id"], subset), got, ref, expect_none=[v for k, v in names.items() if k not in want])
    if not c["is_train"]:
        stats_untouched(c, got)


# ---- (c) blocks, with the shortcut gradient added by the head's data-gradient kernel and by the engine ----------------------------------------
@pytest.mark.parametrize("res_link", [True, False], ids=["link", "nolink"])
@pytest.mark.parametrize("c", R.BLOCK_CASES, ids=_ids(R.BLOCK_CASES))
def test_blocks(dev, c, res_link):
    Fn = pkg("functional")
    ref = ref_tensors(ref_of(c))
    prev = Fn.RES_LINK
    Fn.RES_LINK = res_link
    try:
        got = run_layers(c, dev)
    finally:
        Fn.RES_LINK = prev
    compare("%s[%s]" % (c["id"], "link" if res_link else "nolink"), got, ref)


# ---- (d) fan-out and shared variables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roots", [None, (0,), (1,)], ids=["both", "first-only", "second-only"])
def test_fan_out(dev, roots):
    c = R.FAN_CASE
    ref = ref_tensors(ref_of(c, roots=roots))
    got = run_layers(c, dev, roots=roots)
    compare("fan[%s]" % (roots,), got, ref)


def test_shared_filter_gets_the_sum_of_both_uses(dev):
    c = R.SHARED_CASE
    gs = pkg("gradsink")
    seen = {}

    def after_forward(st):
        seen["pending"] = gs.lookup(st.vars["wsh"].tensor).pending

    got = run_layers(c, dev, after_forward=after_forward)
    assert seen["pending"] == 2, seen
    compare("shared", got, ref_tensors(ref_of(c)))
    got_leaf = run_layers(c, dev, mode="leaf")
    compare("shared[leaf]", got_leaf, ref_tensors(ref_of(c)))


# ---- (e) gradient destinations -------------------------------------------------------------------------------------------------------------
def test_gradient_destinations(dev):
    c = R.DEST_CASE
    ref = ref_tensors(ref_of(c))
    leaf = run_layers(c, dev, mode="leaf")
    store = run_layers(c, dev, mode="store")
    side = run_layers(c, dev, mode="store", overlap=True)
    arena = store["_store"].grad_arena
    assert float(arena.abs().max()) > 0 and store["d_w1"].data_ptr() >= arena.data_ptr()          # the sinks wrote the arena
    for tag, got in (("leaf", leaf), ("store", store), ("store+side-stream", side)):
        compare("%s[%s]" % (c["id"], tag), got, ref)
    for n in ref:
        if store[n] is not None:
            assert torch.equal(store[n], side[n]), "side stream changed %s" % n


# ---- (f) roots ---------------------------------------------------------------------------------------------------------------------------------
def _head_ref(c, extra=None, gscale=0.5, mc=1.0, md=0.5):
    r = R.run_ref(c)
    assert R.clearance(r["L"].rec) >= R.MARGIN
    logits = r["outs"][0]
    y = torch.from_numpy(R.onehot_labels(c["seed"], tuple(logits.shape[:3]), c["ncls"])).double()
    assert R.clip_margin(logits, y) > 1e-4, "a label probability sits on the cross-entropy clip"
    tot, wl, dl = R.seg_loss(logits, y, mc, md)
    obj = gscale * tot
    vals = {"seg": (float(tot.detach()), float(wl.detach()), float(dl.detach()))}
    if extra is not None:
        ev, eobj = extra(logits, y)
        vals["extra"] = float(ev.detach())
        obj = obj + eobj
    obj.backward()
    return r, y, vals


def test_seg_loss_root_with_gscale(dev):
    c, Fn = R.HEAD_CASE, pkg("functional")
    r, y, vals = _head_ref(c)
    seen = {}

    def root(outs, X):
        lv = Fn.SegLossFn.apply(outs[0], _dev(y.float().numpy(), dev), 1.0, 0.5, 0.5)
        seen["lv"] = lv.detach()
        return [lv], [torch.ones(3, device=dev)]

    got = run_layers(c, dev, root_fn=root)
    for v, rv, bar, n in zip(seen["lv"].cpu().tolist(), vals["seg"], LOSS_TOL, ("total", "xent", "dice")):
        print("units head seg loss %s: %.3e (bar %.0e)" % (n, abs(v - rv), bar))
        assert abs(v - rv) <= bar, (n, v, rv)
    compare("head[seg root, gscale 0.5]", got, ref_tensors(r))


def test_seg_and_boundary_roots_meet_in_fan_out(dev):
    import boundary_ref as BR
    c, Fn = R.HEAD_CASE, pkg("functional")
    coef, gscale = 0.3, 0.5

    def extra(logits, y):
        phi = torch.from_numpy(BR.phi_ref(y.numpy())[0])
        v = (torch.softmax(logits, -1) * phi).sum() / (phi.shape[0] * phi.shape[1] * phi.shape[2] * (c["ncls"] - 1))
        return v, coef * gscale * v

    r, y, vals = _head_ref(c, extra, gscale)
    seen = {}

    def root(outs, X):
        yd = _dev(y.float().numpy(), dev)
        a, b = Fn.fan_out(outs[0])
        lv = Fn.SegLossFn.apply(a, yd, 1.0, 0.5, gscale)
        bnd = Fn.BoundaryLossFn.apply(b, yd, None, coef, gscale)
        seen["lv"], seen["bnd"] = lv.detach(), bnd.detach()
        return [lv, bnd], [torch.ones(3, device=dev), torch.ones(1, device=dev)]

    got = run_layers(c, dev, root_fn=root)
    assert abs(float(seen["lv"][0]) - vals["seg"][0]) <= LOSS_TOL[0]
    assert abs(float(seen["bnd"]) - vals["extra"]) <= 1e-5 * max(1.0, abs(vals["extra"])), (float(seen["bnd"]), vals["extra"])
    compare("head[seg + boundary roots]", got, ref_tensors(r))


def test_wgan_root_with_a_missing_input(dev):
    Fn = pkg("functional")
    rng = np.random.default_rng(5)
    coefs, gscale = (0.7, -1.3, 0.0, 0.25), 0.5
    vals = [rng.standard_normal((6, 1)).astype(np.float32), rng.standard_normal((6, 1)).astype(np.float32), None,
            rng.standard_normal((6, 1)).astype(np.float32)]          # (the kernel takes ONE element count for all of its inputs)
    ts = [None if v is None else _dev(v, dev, True) for v in vals]
    t64 = [None if v is None else torch.from_numpy(v).double().requires_grad_(True) for v in vals]
    loss = Fn.WganLossFn.apply(ts[0], ts[1], ts[2], ts[3], coefs, gscale)
    loss.backward(torch.ones(1, device=dev))
    ref = R.wgan_loss(t64, coefs)
    (gscale * ref).backward()
    scale = sum(abs(cf) * float(t.abs().mean()) for t, cf in zip(t64, coefs) if t is not None)
    print("units wgan loss: %.3e of sum|coef| mean|x|" % (abs(float(loss) - float(ref)) / scale))
    assert abs(float(loss) - float(ref)) <= WGAN_TOL * scale
    for t, t6 in zip(ts, t64):
        if t is not None:
            assert rel(t.grad, t6.grad) <= TOL


# ---- (g) the two guards ------------------------------------------------------------------------------------------------------------------------
def test_recomputed_sign_refuses_a_weight_write_between_forward_and_backward(dev):
    K = pkg("kernels")
    c = R.UNIT_CASES[0]
    assert c["is_train"] and c["sc"] == "none" and c["alpha"] >= 0

    def step(_):
        w = torch.zeros(4096, device=dev)
        K.rmsprop_step(w, torch.ones_like(w), torch.ones_like(w), None, None, 1e-3, 0.9, 1e-10)

    with pytest.raises(RuntimeError, match="parameters were updated"):
        run_direct(c, dev, between=step)


def test_inference_backward_refuses_changed_moving_statistics(dev):
    Fn = pkg("functional")
    c = [u for u in R.UNIT_CASES if u["id"] == "infer-none-.75-unfused"][0]

    def train_forward(t):
        with torch.no_grad():
            Fn.ConvBNActFn.apply(t["x"].detach(), t["w"].detach(), t["gamma"].detach(), t["beta"].detach(), t["mm"], t["mv"], None, t["g"],
                                 1.0, 0, 0, True, 0.2, False, None, False)

    with pytest.raises(RuntimeError, match="moving statistics were updated"):
        run_direct(c, dev, between=train_forward)


# ---- (h) bf16 mode -----------------------------------------------------------------------------------------------------------------------------
def _budget(c, roots=None):
    """E per tensor: float64 restatement with bf16-rounded convolution operands against the un-rounded one, of max|ref|"""
    ref, rnd = ref_tensors(ref_of(c, roots=roots)), ref_tensors(ref_of(c, R.round_bf16, roots=roots))
    return ref, {n: rel(rnd[n], ref[n]) for n in ref if ref[n] is not None and rnd.get(n) is not None}


def _bf16_run(fn):
    Fn, L = pkg("functional"), pkg("_lib")
    Fn.set_conv_dtype("bf16")
    try:
        L.prof_summary()
        L.prof_enable(L.PROF_CONV_FWD | L.PROF_CONV_DGRAD | L.PROF_CONV_WGRAD)
        try:
            got = fn()
            torch.cuda.synchronize()
        finally:
            L.prof_enable(0)
        names = sorted({r["name"] for r in L.prof_summary()})
    finally:
        Fn.set_conv_dtype("f32")
    return got, names


BF16_SMALL = R.UNIT_CASES + [c for c in R.BLOCK_CASES if c["id"] in R.BF16_BLOCK_IDS]
assert all(c["is_train"] for c in BF16_SMALL if c["prog"] != "unit")


@pytest.mark.parametrize("c", BF16_SMALL, ids=_ids(BF16_SMALL))
def test_bf16_mode_small_cases(dev, c):
    """the cases of (a) and the two-unit blocks of (c) with functional.set_conv_dtype('bf16'): below 4096 output pixels the resident
    kernels serve nothing, the geometry-typed dispatch decides per layer which kernel family runs (printed)"""
    ref, E = _budget(c)
    got, names = _bf16_run(lambda: run_layers(c, dev))
    print("units bf16 %-40s kernels %s" % (c["id"], names))
    # where the dispatch kept every convolution of the case on float32 kernels nothing was rounded: the float32 bar, no budget
    compare("bf16 " + c["id"], got, ref, budget=E if any("bf16" in n for n in names) else None)
    if not c["is_train"]:
        stats_untouched(c, got)


@pytest.mark.parametrize("c", R.BF16_RESIDENT_CASES + [R.BF16_BLOCK_CASE], ids=_ids(R.BF16_RESIDENT_CASES + [R.BF16_BLOCK_CASE]))
def test_bf16_mode_resident(dev, c):
    K, L = pkg("kernels"), pkg("_lib")
    N, H, W, C, Kc = c["shape"]
    g = K.conv_geom((N, H, W, C), (c["k"], c["k"], C, Kc), 1, c["dil"], "SAME", dtype=L.DTYPE_BF16)
    served = tuple(K.bf16r(g, k) for k in (0, 1, 2))
    assert served == c["served"], (served, c["served"])
    ref, E = _budget(c)
    got, names = _bf16_run(lambda: run_layers(c, dev))
    print("units bf16 %-40s served %s kernels %s" % (c["id"], served, names))
    assert any("conv_bf16r_kernel" in n for n in names), names                 # a silent fp32 run must not pass
    assert any("conv_wgrad_bf16r_kernel" in n for n in names), names
    if not served[1]:          # the data gradient is off the resident family: want_h without only_h
        assert any("bf16r" not in n for n in names), names
    compare("bf16 " + c["id"], got, ref, budget=E)
