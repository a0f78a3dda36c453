"""not gpu: the case list of tests/test_gpu_fda_domain.py (tests/fda_domain_cases.py) against the reference alone.  Every case meets the
input condition (band_ratio >= 1e-6) and its fp32 route (fda_ref.fda_route32) lies within FDA's kernel bar (1e-5 of max|ref|), so that
the GPU test's bar 2 x max(route error, 1e-6) is never looser than 2e-5.  The condition alone bounds nothing: the error follows the phase
sensitivity |T| / |S| over the band.  Also: spectral is exactly Hermitian, the route equals the reference on small images,
and the list reaches the edges of csrc/fda.hip's launch geometry."""
import numpy as np
import pytest

import fda_domain_cases as FD
import fda_ref as R


@pytest.mark.parametrize("name", [c[0] for c in FD.CASES])
def test_case_meets_the_condition_and_its_route_the_bar(name):
    _, shape, band, pair, gen, _ = FD.BY_NAME[name]
    src, _ = FD.inputs(name)
    ratio = R.band_ratio(src, band)
    ref, route, err, bar = FD.reference(name)
    scale = np.abs(ref).max()
    print("%s %s (%s): smallest band |S| / max|S| %.2e, route error %.3e, bar %.3e of max|ref|" % (name, shape, gen, ratio, err, bar / scale))
    assert ratio >= 1e-6, "input condition"
    assert err <= 1e-5, "the fp32 route misses FDA's kernel bar"
    assert bar <= 2e-5 * scale * (1 + 1e-12)


@pytest.mark.parametrize("H,W,C", [(8, 8, 1), (7, 9, 3), (16, 12, 2)])
def test_spectral_is_exactly_hermitian(H, W, C):
    x, X = R.spectral(np.random.default_rng(3), 2, H, W, C, FD.SPECTRAL_FLOOR, return_spectrum=True)
    assert x.dtype == np.float32 and x.shape == (2, H, W, C)
    assert np.array_equal(X, np.conj(R._mirror(X)))                          # X(-k) = conj X(k) bit for bit
    fu, fv = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    env = np.exp(-(fu * fu + fv * fv) / (2.0 * R.SPECTRAL_SIGMA ** 2))
    assert (np.abs(X) >= FD.SPECTRAL_FLOOR * env * (1 - 1e-12)).all() and (np.abs(X) <= env * (1 + 1e-12)).all()
    for i in range(2):
        for c in range(C):
            z = np.fft.ifft2(X[i, c])
            print("max |Im| %.3e of max |Re| %.3e" % (np.abs(z.imag).max(), np.abs(z.real).max()))
            assert np.abs(z.imag).max() <= 1e-12 * np.abs(z.real).max()
            y = z.real / np.sqrt(np.mean(z.real ** 2))
            assert np.array_equal(x[i, :, :, c], y.astype(np.float32))


def test_spectral_at_full_size_is_hermitian():
    _, X = R.spectral(np.random.default_rng(4), 1, 1024, 1023, 1, FD.SPECTRAL_FLOOR, return_spectrum=True)
    z = np.fft.ifft2(X[0, 0])
    assert np.array_equal(X, np.conj(R._mirror(X)))
    assert np.abs(z.imag).max() <= 1e-12 * np.abs(z.real).max()


@pytest.mark.parametrize("H,W", [(5, 6), (8, 8)])
def test_route_agrees_with_the_reference(H, W):
    rng = np.random.default_rng(1)
    src, tgt = R.blobs(rng, 2, H, W, 2), (1.5 * R.blobs(rng, 3, H, W, 2) + 0.4).astype(np.float32)
    for band, pair in [([b, b], [2, 0]) for b in range(0, (min(H, W) - 1) // 2 + 1)] + [([-1, 1], [1, 1])]:
        ref = R.fda_ref(src, tgt, band, pair)
        route = R.fda_route32(src, tgt, band, pair)
        err = np.abs(route - ref).max() / np.abs(ref).max()
        print("%dx%d band %s: route error %.3e of max|ref|" % (H, W, band, err))
        assert err <= 1e-5, (H, W, band)
        for i, b in enumerate(band):
            if b < 0:
                assert np.array_equal(route[i], src[i].astype(np.float64))


def test_route_takes_the_target_amplitude_where_the_source_is_zero():
    rng = np.random.default_rng(2)
    src, tgt = R.blobs(rng, 1, 8, 8, 2), R.blobs(rng, 1, 8, 8, 2)
    src[0, :, :, 1] = 0.0
    ref, route = R.fda_ref(src, tgt, [2], [0]), R.fda_route32(src, tgt, [2], [0])
    assert np.abs(route - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.abs(route[0, :, :, 1] - ref[0, :, :, 1]).max() <= 1e-5 * np.abs(ref[0, :, :, 1]).max()


def test_route_bar():
    ref = np.array([1.0, -4.0, 2.0])
    assert R.route_bar(ref, ref + [0.0, 1e-4, 0.0]) == pytest.approx(2 * 1e-4)
    assert R.route_bar(ref, ref) == pytest.approx(2 * 1e-6 * 4.0)


def test_the_list_reaches_every_edge():
    shapes = [c[1] for c in FD.CASES]
    assert {s[4] for s in shapes} == {1, 2, 3, 4}
    for C in (1, 2, 3, 4):
        assert any(c[1][4] == C and c[1][2:4] == (16, 16) and sorted(c[2]) == [0, 7] for c in FD.CASES), C
    assert any(s[2:4] == (1024, 1024) for s in shapes) and any(s[2] == 1 and s[3] == 1 for s in shapes)
    for B, Bt, H, W, C in shapes:
        assert 1 <= B <= FD.MAX_BATCH and 1 <= Bt <= FD.MAX_BATCH and 1 <= H <= FD.MAX_EXTENT and 1 <= W <= FD.MAX_EXTENT
        assert 1 <= C <= FD.MAX_CH
    for name, (B, Bt, H, W, C), band, pair, gen, _ in FD.CASES:
        assert len(band) == len(pair) == B and gen in ("blobs", "spectral")
        assert all(-1 <= b <= (min(H, W) - 1) // 2 for b in band) and all(0 <= p < Bt for p in pair), name

    # the split sums on either side of their switch, with extents that end segments unevenly
    row = {(n, c[1][3]) for c in FD.CASES for _, n, _ in FD.analyses(c)}
    col = {(n, c[1][2]) for c in FD.CASES for _, _, n in FD.analyses(c)}
    assert FD.segments(128) == 2 and FD.segments(132) == 1 and FD.segments(127) == 2 and FD.segments(129) == 1
    assert any(n == 128 and W % 2 for n, W in row) and any(n == 132 for n, _ in row)
    assert any(n == 127 and H % 2 for n, H in col) and any(n == 129 for n, _ in col)
    assert FD.segments(1) == 256 and any(n == 1 and W >= 1000 and W % 256 for n, W in row)
    assert any(n == 1 and H >= 1000 and H % 256 for n, H in col)

    # the NT-strided loops run more than once, and the synthesis kernels' shared arrays fill up
    assert any(s[2] > FD.NT for s in shapes) and any(s[3] * s[4] > FD.NT for s in shapes)
    assert max(2 * b + 1 for c in FD.CASES for b in c[2]) == 2 * FD.MAX_BAND + 1
    assert max(c[1][4] * (b + 1) for c in FD.CASES for b in c[2]) == (FD.MAX_BAND + 1) * FD.MAX_CH

    # the batch: 256 samples, pair 255, shared targets with unequal bands, unused targets, targets paired only with band -1
    assert max(s[0] for s in shapes) == FD.MAX_BATCH and max(s[1] for s in shapes) == FD.MAX_BATCH
    assert max(p for c in FD.CASES for p in c[3]) == FD.MAX_BATCH - 1
    shared_unequal = unused = only_minus_one = 0
    for _, (B, Bt, H, W, C), band, pair, _, _ in FD.CASES:
        for j in range(Bt):
            mine = [b for b, p in zip(band, pair) if p == j]
            shared_unequal += len(set(mine)) > 1 and max(mine) >= 0
            unused += not mine
            only_minus_one += bool(mine) and max(mine) == -1
    assert shared_unequal and unused and only_minus_one, (shared_unequal, unused, only_minus_one)
    tb = FD.target_bands(*FD.BY_NAME["batch256_shared"][2:4], FD.MAX_BATCH)
    assert tb[128:] == [-1] * 128 and tb[0] == -1 and tb[3] == 2 and tb[4] == 3           # j = 3: bands 2 and -1; j = 4: 3 and 0
