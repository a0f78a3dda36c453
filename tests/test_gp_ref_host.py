"""CPU: (a) tests/gp_ref.py — the references the -m gpu domain tests of csrc/critic_gp.hip compare against: the closed form of the BN
double backward equals torch autograd in float64, the eps restatement is a 24-bit uniform that follows the stream id, the penalty's adjoint is
autograd's; (b) the case lists of tests/test_gpu_gp_domain.py pinned to the branches of the launch code, restated in gp_ref.dbl_dispatch /
gp_dispatch (their workspace sizes are checked against the library's own queries): a case list that stops reaching a branch fails here,
without a GPU; (c) the hard-operand cases are well posed: the closed form run in float32 stays within 1e-4 of max|ref| of float64."""
import numpy as np
import pytest
import torch

import gp_ref as R
import test_gpu_gp_domain as GD
from conftest import pkg
from oracle import tf_ops as T

TOL = 1e-12


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _require(branches):
    missing = [k for k, v in branches.items() if not v]
    assert not missing, "no case reaches: %s" % ", ".join(missing)


# ---- (a) the references ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.2, 0.0, -1.0])
@pytest.mark.parametrize("P,C,Cs,keep", [(16, 8, 4, 0.75), (16, 8, 8, 0.5), (8, 6, 4, 1.0), (16, 5, 0, 0.75), (32, 3, 1, 0.5), (16, 4, 0, 1.0)])
def test_closed_form_equals_autograd(P, C, Cs, keep, alpha):
    """d on a grid of quarters with P a power of two: the float32 mean / var the references read are then the exact statistics, and the
    two derivations agree to float64 rounding (with rounded statistics they differ by that rounding: the closed form assumes
    mean(xhat) = 0, mean(xhat^2) = 1)"""
    rng = np.random.default_rng(P + C + Cs)
    d = torch.from_numpy(rng.integers(-8, 9, size=(P, C)) / 4.0).float()
    d64 = d.double()
    mean, var = d64.mean(0), ((d64 - d64.mean(0)) ** 2).mean(0)
    assert torch.equal(mean.float().double(), mean) and torch.equal(var.float().double(), var)
    f32 = lambda s: torch.from_numpy(rng.standard_normal(s)).float()
    gcb, gy, gamma = f32((P, C)), f32((P, C)), 1.0 + 0.3 * f32((C,))
    scb = f32((P, Cs)) if Cs else None
    y = None
    if alpha >= 0:
        y = f32((P, C))
        y.reshape(-1)[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    mask = torch.from_numpy(T.dropout_mask((P, C), keep, 3, 4)).double() if keep < 1 else None
    args = (gcb, d, y, gy, mean.float(), var.float(), gamma, scb, 1e-3, alpha, keep, mask)
    for got, ref, name in zip(R.bn_dbl_closed(*args), R.bn_dbl_autograd(*args), ("gy_bar", "xc_bar", "gamma_bar")):
        assert float(ref.abs().max()) > 0 and _rel(got, ref) < TOL, (name, _rel(got, ref))
    if mask is not None:
        assert float(R.bn_dbl_closed(*args)[1][mask == 0].abs().max()) == 0.0


def test_one_row_references_are_zero():
    o = GD.dbl_operands((1, 8, 0, 0.2, 0.75), "normal")
    for fn in (R.bn_dbl_closed, R.bn_dbl_autograd):
        for r in GD._refs(o, (1, 8, 0, 0.2, 0.75), fn):
            assert float(r.abs().max()) <= 1e-12


def test_eps_restatement():
    e = R.gp_eps(65535, 7, 123)
    assert e.dtype == np.float32 and e.shape == (65535,) and float(e.min()) >= 0.0 and float(e.max()) < 1.0
    k = e.astype(np.float64) * 16777216.0
    assert np.array_equal(k, np.round(k))                                    # multiples of 2^-24
    assert len(np.unique(e)) > 65000 and abs(float(e.mean()) - 0.5) < 0.01    # 24-bit uniform, not a few values
    e2 = R.gp_eps(65535, 7, 124)
    assert float((e == e2).mean()) < 1e-3 and not np.array_equal(R.gp_eps(1, 7, 123), R.gp_eps(1, 7, 124))
    assert not np.array_equal(e[:16], R.gp_eps(16, 8, 123)) and np.array_equal(e[:16], R.gp_eps(16, 7, 123))
    # the hash is the dropout mask's: eps_i >= 1 - keep exactly where the mask of element i is kept
    assert np.array_equal((e[:4096] * 16777216.0 >= float(T.drop_thresh(0.75))).astype(np.float32), T.dropout_mask((4096,), 0.75, 7, 123))


def test_penalty_reference():
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.standard_normal((5, 3, 7)) * 0.3)
    g[1] = 0.0
    g[2] = 0.0
    g[2, 1, 3] = -1.0
    nrm, pen, adj = R.penalty_ref(g, 10.0, 0.125)
    x = g.clone().requires_grad_(True)
    P = 10.0 * ((x.flatten(1).norm(dim=1) - 1) ** 2).mean()
    (a,) = torch.autograd.grad(P, x)
    assert _rel(nrm, g.flatten(1).norm(dim=1)) < TOL and abs(float(pen) - float(P.detach())) < TOL * float(P.detach())
    assert _rel(adj, torch.nan_to_num(a, nan=0.0).flatten(1) * 0.125) < TOL
    assert float(adj[1].abs().max()) == 0.0 and float(adj[2].abs().max()) == 0.0 and float(nrm[2]) == 1.0
    ta, tb = R.interp_terms(torch.ones(2, 3), torch.full((2, 3), 2.0), torch.tensor([0.25, 0.5]))
    assert torch.equal(ta + tb, torch.tensor([[1.75] * 3, [1.5] * 3], dtype=torch.float64))


# ---- (b) the case lists against the launch arithmetic ------------------------------------------------------------------------------------
def test_dispatch_restatements_match_the_library(built):
    lib = pkg("_lib").load()
    for P, C in sorted({c[:2] for c in GD.DBL_CASES + GD.HARD_SHAPES} | {c[:2] for c in GD.P1_CASES} | {((1 << 30) + 1, 4), (131072, 4), (131136, 8)}):
        assert int(lib.pnp_bn_dbl_bwd_workspace_bytes(P, C)) == R.dbl_dispatch(P, C)["workspace"], (P, C)
    for B, n in sorted({c[:2] for c in GD.PEN_CASES}):
        assert int(lib.pnp_gp_workspace_bytes(B, n)) == R.gp_dispatch(B, n)["workspace"], (B, n)
    assert int(lib.pnp_bn_dbl_bwd_workspace_bytes(4, 65536)) == 0 and int(lib.pnp_gp_workspace_bytes(65536, 4)) == 0
    d = R.dbl_dispatch(1000, 1200)
    assert d["vector"] and d["ny"] == 2 and d["slices"] == [{"groups": 256, "rpi": 1, "idle": 0}, {"groups": 44, "rpi": 5, "idle": 36}]
    assert (d["nblk"], d["rows_per_block"], d["nblk_capped"], d["bx"], d["apply_capped"]) == (16, 63, False, 1000, False)
    d = R.dbl_dispatch(131073, 6)
    assert not d["vector"] and d["slices"] == [{"groups": 6, "rpi": 42, "idle": 4}] and d["nblk_capped"] and d["rows_per_block"] == 65
    assert d["nblk"] == 2017 and d["apply_capped"] and d["bx"] == 2048
    assert not R.dbl_dispatch(131072, 4)["nblk_capped"] and R.dbl_dispatch(131072, 4)["nblk"] == 2048
    g = R.gp_dispatch(300, (1 << 21) + 8)
    assert g == {"vector": True, "blocks": 256, "capped": True, "norm_passes": 33, "final_loops": True, "workspace": g["workspace"]}
    assert R.gp_dispatch(2, 1 << 21)["capped"] is False and R.gp_dispatch(2, 1 << 21)["blocks"] == 256 and not R.gp_dispatch(256, 3)["final_loops"]


def test_bn_double_backward_case_list_reaches_every_branch():
    cs = GD.DBL_CASES
    assert len(set(cs)) == len(cs) and len(cs) <= 30 and all(P * C <= 5_000_000 for P, C, *_ in cs)
    assert all(Cs == 0 or (0 < Cs <= C and (C - Cs) % 2 == 0) for _, C, Cs, *_ in cs)
    D = [R.dbl_dispatch(c[0], c[1]) for c in cs]
    z = list(zip(cs, D))
    last = lambda d: d["slices"][-1]
    c0 = lambda c: (c[1] - c[2]) // 2
    crosses = lambda c, d: c[2] and any(c0(c) < s * R.NT * (4 if d["vector"] else 1) < c0(c) + c[2] for s in range(1, d["ny"]))
    _require({
        "second blockIdx.y slice, vector kernel (C > 1024)": any(d["vector"] and d["ny"] >= 2 for c, d in z),
        "second blockIdx.y slice, scalar kernel (C > 256)": any(not d["vector"] and d["ny"] >= 2 for c, d in z),
        "more than two slices": any(d["ny"] > 2 for c, d in z),
        "last slice narrower than 256, vector": any(d["vector"] and d["ny"] >= 2 and last(d)["groups"] < R.NT for c, d in z),
        "last slice narrower than 256, scalar": any(not d["vector"] and d["ny"] >= 2 and last(d)["groups"] < R.NT for c, d in z),
        "last slice one group wide (256 rows per pass beside 1)": any(d["ny"] >= 2 and last(d)["groups"] == 1 for c, d in z),
        "last slice with idle lanes": any(d["ny"] >= 2 and last(d)["idle"] > 0 for c, d in z),
        "vector kernel, group count does not divide 256 (lanes with rsub >= rpi)": any(d["vector"] and d["slices"][0]["idle"] > 0 for c, d in z),
        "scalar kernel, channel count does not divide 256": any(not d["vector"] and d["slices"][0]["idle"] > 0 for c, d in z),
        "no idle lane": any(all(s["idle"] == 0 for s in d["slices"]) for c, d in z),
        "1 < P < rpi": any(1 < c[0] < d["slices"][0]["rpi"] for c, d in z),
        "P < rpi in the last slice only": any(d["ny"] >= 2 and d["slices"][0]["rpi"] <= c[0] < last(d)["rpi"] for c, d in z),
        "P not a multiple of rpi": any(c[0] > d["slices"][0]["rpi"] > 1 and c[0] % d["slices"][0]["rpi"] for c, d in z),
        "nblk cap of 2048 (P > 131072), vector": any(d["nblk_capped"] and d["vector"] for c, d in z),
        "nblk cap of 2048 (P > 131072), scalar": any(d["nblk_capped"] and not d["vector"] for c, d in z),
        "rows per block not dividing P (a short last slab)": any(c[0] % d["rows_per_block"] for c, d in z),
        "apply grid capped at 2048 / ny, ny = 2": any(d["apply_capped"] and d["ny"] == 2 for c, d in z),
        "apply grid capped at 2048, ny = 1": any(d["apply_capped"] and d["ny"] == 1 for c, d in z),
        "apply grid uncapped with more than one workgroup": any(not d["apply_capped"] and d["bx"] > 1 for c, d in z),
        "combine with fewer than 8 slabs": any(1 < d["nblk"] < 8 for c, d in z),
        "combine with one slab": any(d["nblk"] == 1 for c, d in z),
        "combine with a slab count that is no multiple of 8": any(d["nblk"] > 8 and d["nblk"] % 8 for c, d in z),
        "combine grid with a ragged last 32 channels": any(c[1] > 32 and c[1] % 32 for c in cs),
        "no shortcut adjoint": any(c[2] == 0 for c in cs),
        "shortcut adjoint with Cs = C, vector": any(c[2] == c[1] and d["vector"] for c, d in z),
        "shortcut adjoint with Cs = C, scalar": any(c[2] == c[1] and not d["vector"] for c, d in z),
        "Cs = C - 2, vector": any(c[2] == c[1] - 2 and d["vector"] for c, d in z),
        "Cs = C - 2, scalar": any(c[2] == c[1] - 2 and not d["vector"] for c, d in z),
        "channel pad not a multiple of 4 in the vector kernel": any(d["vector"] and c[2] and c0(c) % 4 for c, d in z),
        "channel pad a multiple of 4 in the vector kernel": any(d["vector"] and 0 < c[2] < c[1] and c0(c) % 4 == 0 for c, d in z),
        "Cs = 2 inside a wide C": any(c[2] == 2 and c[1] >= 40 for c in cs),
        "shortcut crossing a slice boundary, vector": any(d["vector"] and crosses(c, d) for c, d in z),
        "shortcut crossing a slice boundary, scalar": any(not d["vector"] and crosses(c, d) for c, d in z),
        "alpha < 0 with y null, vector": any(c[3] < 0 and d["vector"] for c, d in z),
        "alpha < 0 with y null, scalar": any(c[3] < 0 and not d["vector"] for c, d in z),
        "alpha = 0": any(c[3] == 0.0 for c in cs), "alpha = 0.2": any(c[3] == 0.2 for c in cs),
        "keep = 0.5": any(c[4] == 0.5 for c in cs), "keep = 0.75": any(c[4] == 0.75 for c in cs), "keep = 1": any(c[4] == 1.0 for c in cs),
        "dropout mask in the scalar kernel": any(c[4] < 1 and not d["vector"] for c, d in z),
        "dropout mask past the first slice": any(c[4] < 1 and d["ny"] >= 2 for c, d in z),
        "P = 1": any(c[0] == 1 for c in GD.P1_CASES), "P = 1 with a shortcut adjoint, Cs = C": any(c[0] == 1 and c[2] == c[1] for c in GD.P1_CASES),
        "P = 1 with a padded shortcut adjoint": any(c[0] == 1 and 0 < c[2] < c[1] for c in GD.P1_CASES),
    })
    assert {c[0] for c in cs} | {c[0] for c in GD.P1_CASES} >= {1, 3, 63, 64, 1000, 3000, 131073}
    assert {c[1] for c in cs} >= {1, 3, 4, 5, 6, 8, 20, 24, 40, 64, 257, 1028, 1030, 1200}
    # operands: signed zeros of y under a non-zero g_y, a channel constant over the rows
    case = (63, 20, 18, 0.2, 0.75)
    o = GD.dbl_operands(case)
    yz = o["y"] == 0
    assert int(yz.sum()) >= 2 and bool(torch.signbit(o["y"][yz]).any()) and not bool(torch.signbit(o["y"][yz]).all())
    assert bool((o["gy"][yz] != 0).all()) and float(o["var"][10]) == 0.0 and float(o["var"].min()) == 0.0 and int((o["var"] == 0).sum()) == 1
    assert o["mask"] is not None and 0.6 < float(o["mask"].mean()) < 0.9 and GD.dbl_operands((64, 24, 0, -1.0, 1.0))["y"] is None
    # the other lists
    assert all(P == 1 and R.dbl_dispatch(P, C)["nblk"] == 1 for P, C, _ in GD.P1_CASES) and {C for _, C, _ in GD.P1_CASES} >= {1, 5, 8, 257, 1028}
    dd = [R.dbl_dispatch(c[0], c[1]) for c in GD.DET_CASES]
    _require({"determinism, scalar kernel": any(not d["vector"] for d in dd), "determinism, vector kernel": any(d["vector"] and d["ny"] == 1 for d in dd),
              "determinism, two slices": any(d["ny"] == 2 for d in dd), "determinism over more than 8 slabs": all(d["nblk"] > 8 for d in dd)})
    _require({"gamma_bar, scalar kernel": any(not R.dbl_dispatch(c[0], c[1])["vector"] for c in GD.GBAR_CASES),
              "gamma_bar, vector kernel": any(R.dbl_dispatch(c[0], c[1])["vector"] for c in GD.GBAR_CASES),
              "gamma_bar past the first 32 channels": any(c[1] > 32 for c in GD.GBAR_CASES)})
    hd = [R.dbl_dispatch(c[0], c[1]) for c in GD.HARD_SHAPES]
    assert 3 <= len(GD.HARD_SHAPES) <= 4 and set(GD.HARD_KINDS) >= {"d100", "d5", "gc_off", "gy_off", "both_off", "wide"}
    _require({"hard operands, scalar": any(not d["vector"] for d in hd), "hard operands, two slices": any(d["ny"] == 2 for d in hd),
              "hard operands, slab cap": any(d["nblk_capped"] for d in hd), "hard operands with a shortcut": any(c[2] for c in GD.HARD_SHAPES)})
    what = [w for w, _ in GD.DBL_REFUSALS]
    assert len(set(what)) == len(what) == 11


def test_interpolation_and_penalty_case_lists_reach_every_branch():
    ic = GD.INTERP_CASES
    di = [R.gp_dispatch(B, n) for B, n, _ in ic]
    assert {n for _, n, _ in ic} >= {1, 3, 4, 105, 8188, (1 << 21) + 8, (1 << 21) + 3} and {B for B, _, _ in ic} >= {1, 2, 300, 65535}
    assert (65535, 3, False) in ic and all(B * n <= 5_000_000 for B, n, _ in ic)
    _require({"interpolation, 16 bytes per lane": any(d["vector"] for d in di), "interpolation, one element per lane": any(not d["vector"] for d in di),
              "interpolation grid capped, vector": any(d["vector"] and d["capped"] for d in di),
              "interpolation grid capped, scalar": any(not d["vector"] and d["capped"] for d in di),
              "interpolation, more than one workgroup per sample, uncapped": any(1 < d["blocks"] and not d["capped"] for d in di),
              "interpolation, n below one quad": any(n < 4 for _, n, _ in ic),
              "interpolation with a = -b": any(neg for _, _, neg in ic)})
    pc = GD.PEN_CASES
    dp = [R.gp_dispatch(c[0], c[1]) for c in pc]
    z = list(zip(pc, dp))
    has = lambda c, k: k in c[4][:c[0]]
    assert all(c[0] * c[1] <= 10_000_000 for c in pc)
    _require({"penalty, 16 bytes per lane": any(d["vector"] for d in dp), "penalty, one element per lane": any(not d["vector"] for d in dp),
              "n = 64 * 256 * 4 + 4 (a second pass of one lane of the norm kernel)": any(c[1] == 64 * 256 * 4 + 4 and d["norm_passes"] == 2 for c, d in z),
              "a second pass in the scalar form": any(not d["vector"] and d["norm_passes"] == 2 for c, d in z),
              "scale kernel's cap of 256 workgroups, vector": any(d["vector"] and d["capped"] for c, d in z),
              "scale kernel's cap of 256 workgroups, scalar": any(not d["vector"] and d["capped"] for c, d in z),
              "B > 256 (the loop of gp_final_kernel)": any(d["final_loops"] for d in dp), "B = 1": any(c[0] == 1 for c in pc),
              "an all-zero sample": any(has(c, "zero") for c in pc), "a one-hot sample": any(has(c, "onehot") for c in pc),
              "elements of 1e20": any(has(c, "huge") for c in pc), "elements of 1e-25": any(has(c, "tiny") for c in pc),
              "1e20 on both load widths": {d["vector"] for c, d in z if has(c, "huge")} == {True, False},
              "1e-25 on both load widths": {d["vector"] for c, d in z if has(c, "tiny")} == {True, False},
              "a batch of one-hots": any(c[4] and set(c[4][:c[0]]) == {"onehot"} and len(c[4]) >= c[0] > 1 for c in pc),
              "coef 0": any(c[2] == 0.0 for c in pc), "coef 10": any(c[2] == 10.0 for c in pc),
              "coef 0 with elements of 1e20": any(c[2] == 0.0 and has(c, "huge") for c in pc),
              "gscale 1": any(c[3] == 1.0 for c in pc), "gscale 1/8": any(c[3] == 0.125 for c in pc)})
    x = GD._pen_operand((5, 105, 10.0, 1.0, GD.PLANTS_HUGE), torch.device("cpu"))
    assert float(x[0].abs().max()) == 0.0 and float(x[1].abs().sum()) == 1.0 and 0 < float(x[2].abs().max()) < 1e-23 and float(x[3].abs().max()) > 1e20
    assert not bool(torch.isfinite((x[3] * x[3]).sum())) and float((x[2] * x[2]).sum()) == 0.0       # what a float32 accumulator makes of them


# ---- (c) the hard-operand cases are well posed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GD.HARD_CASES, ids=lambda c: "P%d-C%d-Cs%d-a%g-k%g-%s" % c)
def test_hard_operands_are_within_reach_of_float32(case):
    shape, kind = case[:5], case[5]
    o = GD.dbl_operands(shape, kind)
    ref = GD._refs(o, shape)
    e = GD._errs(GD._refs(o, shape, R.bn_dbl_closed_f32), ref)
    print("hard %s: float32 restatement %.2e %.2e %.2e of max|ref| (gy_bar, xc_bar, gamma_bar)" % ((case,) + tuple(e)))
    assert all(float(r.abs().max()) > 0 for r in ref) and max(e) < 1e-4, e
