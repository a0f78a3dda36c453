"""CPU: the conditions that keep tests/test_gpu_units.py from hiding a failure.

  * every case's float64 forward is clear of zero and of pool ties (unit_ref.clearance >= unit_ref.MARGIN) — a condition of the case,
    seed included, not a measurement: no pixel is excluded on the GPU;
  * the case lists cover the matrix the GPU file states, and — asked of the planner queries that need no GPU — reach every glue branch
    of functional.ConvBNActFn they are there for, so that a planner change that re-routes a case fails here;
  * the restatement of a residual block and of a dilated residual block equals the corresponding slice of oracle.nets.segmenter_forward
    to 1e-12: the new reference is held to the existing oracle, not to itself.
"""
import itertools

import numpy as np
import pytest
import torch

import unit_ref as R
from conftest import pkg
from oracle import nets
from oracle import tf_ops as T


def _forward(c):
    with torch.no_grad():
        L = R.RefLayers(c["seed"], c["drop_seed"])
        X = {k: v.detach() for k, v in R.ref_inputs(c).items()}
        outs = R.PROGRAMS[c["prog"]](L, X, c)
    return L, outs


CLEAR_CASES = [c for c in R.ALL_CASES if c.get("clear", True)]      # (not the one bf16-only block: its bar is the rounding budget)


@pytest.mark.parametrize("c", CLEAR_CASES, ids=[c["id"] for c in CLEAR_CASES])
def test_case_is_clear_of_zero_and_of_pool_ties(c):
    L, outs = _forward(c)
    m = R.clearance(L.rec)
    assert m >= R.MARGIN, (c["id"], m)
    if c["prog"] == "head":          # the root tests: no probability on the cross-entropy clip either
        y = torch.from_numpy(R.onehot_labels(c["seed"], tuple(outs[0].shape[:3]), c["ncls"])).double()
        assert float(y.sum(-1).min()) == 1.0 == float(y.sum(-1).max()) and float(y.sum((0, 1, 2)).min()) > 0
        assert R.clip_margin(outs[0], y) > 1e-4


def test_case_ids_are_unique_and_the_seed_is_part_of_the_case():
    ids = [c["id"] for c in R.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert all(isinstance(c["seed"], int) and c["drop_seed"] != c["seed"] for c in R.ALL_CASES)


def test_unit_matrix_is_covered():
    U = R.UNIT_CASES
    vals = lambda k: {c[k] for c in U}
    assert vals("is_train") == {True, False} and vals("bn_trainable") == {True, False}
    assert vals("alpha") == {R.LEAK, 0.0, -1.0} and vals("keep") == {1.0, 0.75} and vals("sc") == {"none", "same", "half"}
    assert vals("padding") == {"SAME", "SYMMETRIC"} and 2 in vals("stride") and 2 in vals("dil")
    assert any(c["padding"] == "SYMMETRIC" and c["k"] == 5 for c in U)
    assert {c["shape"] for c in U} >= {(2, 8, 8, 8, 16), (2, 7, 9, 5, 7), (2, 16, 16, 32, 64)}
    assert max(np.prod(c["shape"][:3]) * max(c["shape"][3:]) for c in U) <= 2 * 16 * 16 * 64
    # every pair (in fact every triple) among is_train, shortcut kind and keep_prob
    seen = {(c["is_train"], c["sc"], c["keep"]) for c in U}
    assert seen == set(itertools.product((True, False), ("none", "same", "half"), (1.0, 0.75)))
    # inference with untrainable BN parameters is the fused route, with trainable ones it is not: both, and training with frozen parameters
    assert {(c["is_train"], c["bn_trainable"]) for c in U} == set(itertools.product((True, False), (True, False)))
    assert set(R.GRAD_SUBSETS) == {"all", "x-only", "params-only", "no-shortcut"} and all(c["sc"] != "none" for c in R.SUBSET_CASES)
    B = R.BLOCK_CASES
    assert {(c["prog"], c["inc_dim"]) for c in B} >= {("res", False), ("res", True), ("dr", False), ("dr", True)}
    assert any(c["prog"] == "res" and c["padding"] == "SYMMETRIC" for c in B) and any(c["prog"] == "chain" for c in B)


def _geom(K, call, dtype=None):
    x, w, padding = call["x"], call["w"], call["padding"]
    if padding == "SYMMETRIC":          # layers._prepad: the mirror pad is materialised, the convolution runs VALID
        p = w[0] // 2
        x, padding = (x[0], x[1] + 2 * p, x[2] + 2 * p, x[3]), "VALID"
    return K.conv_geom(x, w, call["stride"], call["dil"], padding, dtype=dtype)


def test_cases_reach_every_glue_branch(built):
    K, L = pkg("kernels"), pkg("_lib")
    reached = {}

    def mark(branch, cid):
        reached.setdefault(branch, []).append(cid)

    for c in R.ALL_CASES:
        RL, _ = _forward(c)
        bf16_case = "served" in c
        for call in RL.calls:
            if not call["bn"]:
                continue
            g = _geom(K, call)
            fused = (not call["is_train"]) and not call["bn_trainable"]
            if call["is_train"]:
                mark("epilogue statistics" if K.conv_stats_parts(g) > 0 else "bn_stats_update", c["id"])
            else:
                mark("fused inference" if fused else "unfused inference", c["id"])
            if not fused:
                mark("resign" if (call["sc"] is None and call["alpha"] >= 0) else "no resign", c["id"])
            if call["link"] is not None:
                mark("link " + call["link"], c["id"])
            if call["sc"] is not None:
                mark("shortcut padded" if call["sc"] != call["w"][3] else "shortcut equal", c["id"])
            gb = _geom(K, call, L.DTYPE_BF16)
            for kind, name in enumerate(("forward", "data gradient", "filter gradient")):
                if bf16_case or c in R.UNIT_CASES:
                    mark("resident %s %s" % (name, "served" if K.bf16r(gb, kind) else "not served"), c["id"])
        if "parts" in c:
            assert (K.conv_stats_parts(_geom(K, RL.calls[0])) > 0) == c["parts"], c["id"]
        if bf16_case:
            assert tuple(K.bf16r(_geom(K, RL.calls[0], L.DTYPE_BF16), k) for k in (0, 1, 2)) == c["served"], c["id"]
    want = ["epilogue statistics", "bn_stats_update", "fused inference", "unfused inference", "resign", "no resign", "link head", "link tail",
            "shortcut padded", "shortcut equal"]
    want += ["resident %s %s" % (n, s) for n in ("forward", "data gradient", "filter gradient") for s in ("served", "not served")]
    missing = [b for b in want if b not in reached]
    assert not missing, missing
    # the partly served unit: filter gradient resident, data gradient not — the BN backward writes float32 and bf16 (want_h, not only_h)
    partly = [c for c in R.BF16_RESIDENT_CASES if c["served"] == (True, False, True)]
    assert partly and partly[0]["id"] in reached["resident data gradient not served"]
    # resign in both modes of the unit cases, link roles only in SAME blocks
    assert "res-sym" not in reached["link head"] and "res" in reached["link head"] and "dr" in reached["link tail"]


def test_stream_ids_follow_the_call_order_of_a_variable_store(built):
    """RefLayers hands out the ids a VariableStore hands out: one per convolution call site, in call order, also at keep_prob 1"""
    V = pkg("variables")
    c = [b for b in R.BLOCK_CASES if b["id"] == "chain"][0]
    RL, _ = _forward(c)
    st = V.VariableStore("cpu")
    with st.as_default():
        st.begin_trace(drop_seed=c["drop_seed"])
        ids = [st.next_drop_stream() for _ in RL.calls]
    assert ids == list(range(len(RL.calls))) == list(range(RL._sid)) and st.drop_seed == c["drop_seed"]


def test_restatement_equals_the_oracle_slices():
    rng = np.random.default_rng(11)
    state = {}
    for name, shape in nets.segmenter_variable_shapes().items():
        state[name] = R.init_value(11, name, shape) if len(shape) != 4 else \
            (rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))).astype(np.float32)
    V = nets.make_variables(state, dtype=torch.float64, requires_grad=False)
    V0 = {k: v.clone() for k, v in V.items()}
    x = torch.from_numpy(rng.standard_normal((2, 16, 16, 3))).double()
    units = []
    with torch.no_grad():
        nets.segmenter_forward(V, x, keep_prob=0.75, main_bn=True, adapt_bn=True, seed=7, units=units)
    kinds = [(kind, cin, cout) for _, blocks, _ in nets.SEGMENTER_SPEC for kind, cin, cout in blocks]
    first, i = {}, 0
    for kind, cin, cout in kinds:
        if kind in ("rb", "drb"):
            first.setdefault((kind, cin != cout), i)
            i += 2
        else:
            i += 1
    for (kind, inc), i in sorted(first.items()):
        u1, u2 = units[i], units[i + 1]
        assert u2["shortcut"] is not None and (u1["dil"] == 2) == (kind == "drb")
        bn1, bn2 = ({leaf: V0[u["bn"] + "/" + leaf].clone() for leaf in ("gamma", "beta", "moving_mean", "moving_variance")} for u in (u1, u2))
        with torch.no_grad():
            if kind == "rb":
                out = R.residual_block(u1["x"], V0[u1["w"]], V0[u2["w"]], bn1, bn2, 0.75, 7, (u1["sid"], u2["sid"]), inc_dim=inc, is_train=True,
                                       leak=True)
            else:
                out = R.DR_block(u1["x"], V0[u1["w"]], V0[u2["w"]], bn1, bn2, 2, 0.75, 7, (u1["sid"], u2["sid"]), inc_dim=inc, is_train=True,
                                 leak=True)
        e = float((out - u2["out"]).abs().max() / u2["out"].abs().max())
        assert e <= 1e-12, (kind, inc, e)
        for u, bn in ((u1, bn1), (u2, bn2)):
            for leaf in ("moving_mean", "moving_variance"):
                assert float((bn[leaf] - V[u["bn"] + "/" + leaf]).abs().max()) <= 1e-12 * float(V[u["bn"] + "/" + leaf].abs().max())
    assert set(first) == {("rb", False), ("rb", True), ("drb", False)}


def test_reflayers_routes_to_the_restatement():
    """the program adapter adds nothing: RefLayers.residual_block / DR_block / PS_conv2d are the module-level restatement with the ids in
    call order"""
    c = [b for b in R.BLOCK_CASES if b["id"] == "res-inc"][0]
    RL, outs = _forward(c)
    x = R.ref_inputs(c)["x"].detach()
    fresh = R.RefLayers(c["seed"], c["drop_seed"])
    bn = [fresh._bn("b_%d" % i, 16, True) for i in (1, 2)]
    with torch.no_grad():
        out = R.residual_block(x, fresh.var("w1", (3, 3, 8, 16)), fresh.var("w2", (3, 3, 16, 16)), bn[0], bn[1], c["keep"], c["drop_seed"], (0, 1),
                               inc_dim=True, is_train=True, leak=True)
    assert torch.equal(out, outs[0])
    y = torch.arange(2 * 3 * 3 * 8, dtype=torch.float64).reshape(2, 3, 3, 8)
    w = torch.ones(5, 5, 2, 3, dtype=torch.float64)
    assert torch.equal(R.PS_conv2d(y, w, 2, 2, 1.0, 0, 0), T.conv2d(T.PS(y, 2, 2), w, 1, 1, "SYMMETRIC"))
