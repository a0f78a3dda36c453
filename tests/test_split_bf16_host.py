"""No GPU: the host emulation of the split-bf16 arithmetic (tests/split_bf16_ref.py) on EXACTLY the operands of every case of
tests/test_gpu_split_bf16_exact.py.  This is where that test's BOUND comes from and where its sharpness can be checked without a device:

  (a) the split is exact: h + m + l == v for every value of every operand;
  (b) the six-term product of every nonzero output is within BOUND = 4 * 2^-24 of the float64 product (measured: at most 1.87 * 2^-24);
  (c) each of the six terms, dropped in turn, moves at least a quarter of the case's nonzero outputs further than 2^-21 — a condition on
      the INPUTS (measured share: 0.76 .. 1.0) — and the five-term result fails the assertion the GPU test makes (check_per_element);
  (d) with a power-of-two dense operand the six-term result is bit-equal to the fp32 product, and each term that the one nonzero plane of
      the power-of-two side is in, dropped in turn, changes at least half of the outputs;
  (e) every output of every sparse case is at most one product: the convolution of the operands' nonzero indicators, in float64, in the
      direction under test, has maximum 1 — and as many ones as Case.pairs() found products."""
import numpy as np
import pytest

import split_bf16_ref as R


def test_two_to_the_twenty_random_pairs():
    """the figures of the module's docstring.  Six terms: the last fp32 addition rounds by at most 2^-24 of the result, the three dropped
    products are at most 2 * 2^-26 + 2^-34 of it for significands at the unfavourable ends of their binades, the earlier additions round
    sums of 2^-8 of the result: under 2 * 2^-24 = BOUND / 2 in all (measured 1.71).  Any five: outside 2^-21 on >= 3/4 of the pairs (a small term) or
    on all but a few in ten thousand (a large one: a middle plane is now and then zero)"""
    rng = np.random.default_rng(0)
    a, b = R.values(rng, 1 << 20), R.values(rng, 1 << 20)
    exact = a.astype(np.float64) * b.astype(np.float64)
    e6 = float(R.rel_err(R.product6(a, b), exact).max())
    shares = [float((R.rel_err(R.product6(a, b, drop=d), exact) > R.VISIBLE).mean()) for d in range(6)]
    print("2^20 pairs: six terms %s; share outside 2^-21 with term i dropped: %s" % (R.units(e6), ["%.3f" % s for s in shares]))
    assert e6 <= R.BOUND / 2
    assert min(shares) >= 0.75 and min(shares[3:]) >= 0.999, shares


def test_check_per_element_is_strict():
    """the shared assertion: a nonzero where the reference is zero, and one element outside the bound, each fail"""
    ref = np.array([0.0, 1.0, -3.0, 0.0])
    assert R.check_per_element(ref.astype(np.float32), ref) == (0.0, 2)
    R.check_per_element(np.array([-0.0, 1.0, -3.0, 0.0], np.float32), ref)          # zero by value
    for bad in ([1e-30, 1.0, -3.0, 0.0], [0.0, 1.0 + 5 * 2.0 ** -24, -3.0, 0.0], [0.0, 1.0, 3.0, 0.0], [0.0, 0.0, -3.0, 0.0]):
        with pytest.raises(AssertionError):
            R.check_per_element(np.array(bad, np.float64), ref)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_case_operands(case):
    ops = case.operands()
    x, w, dy = ops
    again = case.operands()
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(ops, again)), "operands() is not reproducible"
    # (a) the split is exact, and no plane is near the denormals
    for v in ops:
        if v is None:
            continue
        h, m, l = R.split3(v)
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), v.astype(np.float64))
        nz = v[v != 0]
        assert nz.size and np.abs(nz).min() >= 2.0 ** -10 and np.abs(nz).max() <= 2.0 ** 10
    # (e) at most one product per output, and pairs() found all of them
    cnt = case.products_per_output(ops)
    assert cnt.max() == 1.0, cnt.max()
    a, b = case.pairs(ops)
    assert a.size == b.size == int(cnt.sum()) * case.collapsed(), (a.size, cnt.sum(), case.collapsed())
    # (only an unpadded forward has a product in every output)
    assert (cnt == 0).any() or (case.kind == 0 and case.layer[8] == "VALID"), "no output without a product: the exact zeros go unchecked"
    exact = a.astype(np.float64) * b.astype(np.float64)
    assert (exact != 0).all()
    # ... and they are the nonzero values of the float64 reference the GPU test compares with (a float64 product of two fp32 values is exact)
    ref = case.reference(ops).numpy()
    assert np.array_equal(np.sort(ref[ref != 0]), np.sort(exact))
    assert np.array_equal(ref != 0, np.broadcast_to(cnt == 1, ref.shape))
    pa, pb = R.split3(a), R.split3(b)
    six = R.product6(pa, pb)
    if case.dense == "values":
        # (b) the reference arithmetic is inside the bound
        e6, n = R.check_per_element(six, exact)
        # (c) every dropped term is visible
        shares = []
        for d in range(6):
            five = R.product6(pa, pb, drop=d)
            shares.append(float((R.rel_err(five, exact) > R.VISIBLE).mean()))
            with pytest.raises(AssertionError):
                R.check_per_element(five, exact)
        print("%s: %d products, six terms %.2f * 2^-24, share outside 2^-21 per dropped term %s" % (case.id, n, e6, ["%.3f" % s for s in shares]))
        assert min(shares) >= 0.25, shares
    else:
        # (d) bit-equal to the fp32 product (which is the exact one: the power of two only moves the exponent)
        prod = a * b
        assert np.array_equal(prod.astype(np.float64), exact)
        assert np.array_equal(R.fp32_bits(six), R.fp32_bits(prod))
        shares = {}
        for d in R.TERMS_OF_PLANE0[case.pow2_side()]:
            shares[d] = float((R.fp32_bits(R.product6(pa, pb, drop=d)) != R.fp32_bits(prod)).mean())
        print("%s: %d products bit-equal, share changed per dropped term %s" % (case.id, a.size, shares))
        assert min(shares.values()) >= 0.5, shares


def test_the_cases_cover_what_the_gpu_test_promises():
    """every kernel family in both directions with random and with power-of-two operands; the multi-item layers have more items than
    workgroups and a partial last round"""
    have = {(c.family, c.kind, c.dense) for c in R.CASES}
    for fam, kinds in (("x3d", (0, 1)), ("x3s", (0, 1)), ("x3n", (0, 1)), ("x3w", (2,))):
        for k in kinds:
            assert (fam, k, "values") in have and (fam, k, "pow2") in have, (fam, k)
    assert {(c.sparse, c.dense) for c in R.CASES if c.family == "x3w"} == {("x", "values"), ("dy", "values"), ("x", "pow2"), ("dy", "pow2")}
    for c in R.CASES:
        N, H, W, C, K = c.layer[:5]
        if c.family == "x3d" and H > 16:
            cin, kout = (C, K) if c.kind == 0 else (K, C)
            items = N * (H // 16) * (W // 16) * (kout // (32 if kout == 32 else 64))
            assert items > 256 and items % 256, (c.id, items)
        if c.family == "x3w":
            tiles = N * (H // 16) * (W // 16)
            assert tiles > 256 and tiles % 256, (c.id, tiles)
        if c.family == "x3n":
            items = N * (c.OH // 8) * (c.OW // 16) if c.kind == 0 else N * -(-H // 16) * -(-W // 16)
            assert items > 512 and items % 512, (c.id, items)
