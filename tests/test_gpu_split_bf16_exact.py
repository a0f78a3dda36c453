"""-m gpu: the split-bf16 convolution kernels (csrc/conv_x3_direct.hip stride-1 and strided, csrc/conv_x3_wgrad.hip, csrc/conv_x3_narrow.hip)
held PER ELEMENT.  Every output of every case is ONE product of two fp32 values (tests/split_bf16_ref.py: one operand is nonzero only on a
lattice of pixels whose pitch is the filter's reach, one channel per lattice pixel; for the filter gradient one impulse per channel), so
the result shows the six kept plane products of the kernels bare — no chain of 576 .. 1600 terms whose rounding a lost product, a wrong
LDS offset on one tap, a stale filter stage behind an item boundary or a patch row of the previous tile could hide in:

  * where the float64 reference is 0 (the zero-padded borders: windows without a lattice point) the result is 0 by value;
  * elsewhere |got - ref| <= BOUND * |ref|, BOUND = 4 * 2^-24.  Where BOUND comes from, and that every five-term variant of the arithmetic
    fails this very assertion on these very operands: the host emulation, tests/test_split_bf16_host.py (six terms: at most 1.87 * 2^-24;
    a dropped term: further than 2^-21 on 75 .. 100 % of the outputs);
  * with a signed power of two as the dense operand the result is the float64 reference rounded to fp32, bit for bit.

Every case checks which symbols ran (x3d_expected / x3s_expected of test_gpu_x3_domain.py, FWD / DGRAD of test_gpu_x3_narrow.py): an fp32
hand-back would pass trivially.  Reference: the float64 convolution (oracle.tf_ops.conv2d + autograd) of the same float32 arrays.  The
multi-item layers have more items than persistent workgroups and a partial last round.  Epilogues (dropout, residual, BN statistics) are
the neighbouring tests'.

Measured on MI355X: see DESIGN §25."""
import numpy as np
import pytest
import torch

import split_bf16_ref as R
from conftest import pkg
from test_gpu_x3_domain import DGRAD as S_DGRAD, FWD as S_FWD, _ran, x3d_expected, x3s_expected
from test_gpu_x3_narrow import DGRAD as N_DGRAD, FWD as N_FWD

pytestmark = pytest.mark.gpu


@pytest.fixture
def route():
    """mode 2 of the family and of the logits kernels, the strided and filter-gradient members on; the Winograd filter-gradient planner,
    which is asked before the split-bf16 one, off; restores what was in force"""
    K = pkg("kernels")
    prev = (K.x3_direct(-1), K.x3_strided(-1), K.x3_wgrad(-1), K.x3_narrow(-1), K.wino_mode(-1), K.wino_wgrad_mode(0))
    K.x3_direct(2); K.x3_strided(1); K.x3_wgrad(1); K.x3_narrow(2)
    yield K
    K.x3_direct(prev[0]); K.x3_strided(prev[1]); K.x3_wgrad(prev[2]); K.x3_narrow(prev[3]); K.wino_mode(prev[4]); K.wino_wgrad_mode(prev[5])


def expected_symbols(case):
    """the symbols of the case's launch in mode 2, from the planners' predicates as the neighbouring tests restate them"""
    if case.family == "x3d" or case.family == "x3w":
        return x3d_expected(case.layer[:5], case.kind)
    if case.family == "x3s":
        assert x3s_expected(case.layer, case.kind) > 0, case.id
        return [["x3s_filter_kernel<false>", S_FWD], ["x3s_filter_kernel<true>", S_DGRAD]][case.kind]
    return [N_FWD, N_DGRAD][case.kind]


def launch(case, ops, K, L, dev):
    """-> (result on the host, symbols that ran); the route the library reports is the family of those symbols (_ran)"""
    N, H, W, C, Kf, R_, S, s, padding = case.layer
    x, w, dy = (None if a is None else torch.from_numpy(np.array(a)).to(dev) for a in ops)
    g = K.conv_geom((N, H, W, C), (R_, S, C, Kf), s, 1, padding)
    if case.family == "x3d":
        K.wino_mode(2)               # (as test_gpu_x3_direct.py: the narrow layers are the Winograd route's, which hands them over)
    if case.kind == 0:
        out, names = _ran(L, lambda: K.conv2d_fwd(x, w, g), L.PROF_CONV_FWD, g)
    elif case.kind == 1:
        out, names = _ran(L, lambda: K.conv2d_dgrad(dy, w, g), L.PROF_CONV_DGRAD, g)
    else:
        out, names = _ran(L, lambda: K.conv2d_wgrad(x, dy, g), L.PROF_CONV_WGRAD, g)
    return out.cpu(), names


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_every_output_is_one_product(dev, route, case):
    """BOUND: tests/test_split_bf16_host.py (the host emulation of the six kept products on these operands)"""
    K, L = route, pkg("_lib")
    ops = case.operands()
    ref = case.reference(ops)
    got, names = launch(case, ops, K, L, dev)
    want = expected_symbols(case)
    assert want is not None and names == sorted(want), (names, want)
    assert tuple(got.shape) == tuple(ref.shape)
    worst, n = R.check_per_element(got.numpy(), ref.numpy())
    print("split-bf16 exact %s: max %.2f * 2^-24 over %d nonzero of %d outputs; ran %s" % (case.id, worst, n, ref.numel(), names))
    if case.dense == "pow2":
        # (the zeros are held by value above: the sign of a sum of zero products is not the arithmetic under test)
        differ = (R.fp32_bits(got.numpy()) != R.fp32_bits(ref.float().numpy())) & (ref.numpy() != 0)
        assert not differ.any(), "%d of %d outputs are not the reference rounded to fp32, bit for bit" % (int(differ.sum()), differ.size)
