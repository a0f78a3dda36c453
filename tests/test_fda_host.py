"""not gpu: Fourier domain adaptation on the host — the float64 reference against a direct DFT, its properties, the
stylizer's draws, the train_segmenter flags, and the wrapper's refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from conftest import pkg
from fda_ref import blobs, fda_ref, swap_channel

F = pkg("fda")          # the module under test; the reference's own tests below share the file


def _direct(s, t, b):
    """the definition with O(H^2 W^2) DFT matrices and signed frequencies: |u| <= b, |v| <= b take |T|, the rest stays S"""
    H, W = s.shape
    Fh = np.exp(-2j * np.pi * np.outer(np.arange(H), np.arange(H)) / H)
    Fw = np.exp(-2j * np.pi * np.outer(np.arange(W), np.arange(W)) / W)
    S, T = Fh @ s @ Fw.T, Fh @ t @ Fw.T
    su = np.array([k if k <= H // 2 else k - H for k in range(H)])
    sv = np.array([k if k <= W // 2 else k - W for k in range(W)])
    band = (np.abs(su)[:, None] <= b) & (np.abs(sv)[None, :] <= b)
    out = S.copy()
    out[band] = np.abs(T[band]) * np.exp(1j * np.angle(S[band]))
    return np.real(np.conj(Fh) @ out @ np.conj(Fw).T / (H * W))


@pytest.mark.parametrize("H,W", [(5, 6), (8, 8)])
def test_reference_against_a_direct_dft(H, W):
    rng = np.random.default_rng(1)
    src, tgt = blobs(rng, 2, H, W, 2).astype(np.float64), blobs(rng, 3, H, W, 2).astype(np.float64)
    for b in range(0, (min(H, W) - 1) // 2 + 1):
        band, pair = [b, b], [2, 0]
        ref = fda_ref(src, tgt, band, pair)
        for i in range(2):
            for c in range(2):
                d = _direct(src[i, :, :, c], tgt[pair[i], :, :, c], b)
                assert np.abs(ref[i, :, :, c] - d).max() <= 1e-12 * np.abs(d).max(), (H, W, b, i, c)


@pytest.mark.parametrize("H,W,b", [(5, 6, 2), (7, 9, 3), (16, 12, 5), (64, 64, 31)])
def test_inverse_is_real(H, W, b):
    rng = np.random.default_rng(2)
    src, tgt = blobs(rng, 2, H, W, 3), 1.5 * blobs(rng, 2, H, W, 3) + 0.4
    z = fda_ref(src, tgt, [b, b], [1, 0], return_complex=True)
    print("max |Im| %.3e of max |out| %.3e" % (np.abs(z.imag).max(), np.abs(z.real).max()))
    assert np.abs(z.imag).max() <= 1e-12 * np.abs(z.real).max()


def test_target_equal_to_source_returns_source():
    rng = np.random.default_rng(3)
    src = blobs(rng, 3, 16, 12, 3)
    out = fda_ref(src, src, [0, 3, 5], [0, 1, 2])
    assert np.abs(out - src).max() <= 1e-12 * np.abs(src).max()


def test_band_zero_swaps_the_dc_term_only():
    rng = np.random.default_rng(4)
    src, tgt = blobs(rng, 1, 7, 9, 3), blobs(rng, 1, 7, 9, 3) - 0.7
    out = fda_ref(src, tgt, [0], [0])
    for c in range(3):
        s, t, o = src[0, :, :, c].astype(np.float64), tgt[0, :, :, c].astype(np.float64), out[0, :, :, c]
        want = np.sign(s.mean()) * abs(t.mean())
        assert abs(o.mean() - want) <= 1e-12 * abs(want)
        assert np.abs((o - o.mean()) - (s - s.mean())).max() <= 1e-12 * np.abs(s).max()      # everything but the mean is kept


def test_band_minus_one_and_zero_channels():
    rng = np.random.default_rng(5)
    src, tgt = blobs(rng, 2, 8, 8, 1), blobs(rng, 1, 8, 8, 1)
    out = fda_ref(src, tgt, [-1, 2], [0, 0])
    assert np.array_equal(out[0], src[0].astype(np.float64))
    z = np.zeros((8, 8))
    # |S| = 0: the phase is 0 (numpy's angle(0)), so the band carries |T| itself
    T = np.fft.fftshift(np.fft.fft2(tgt[0, :, :, 0].astype(np.float64)))
    keep = np.zeros_like(T)
    keep[4 - 2:4 + 3, 4 - 2:4 + 3] = np.abs(T)[4 - 2:4 + 3, 4 - 2:4 + 3]
    assert np.abs(np.real(swap_channel(z, tgt[0, :, :, 0], 2)) - np.real(np.fft.ifft2(np.fft.ifftshift(keep)))).max() < 1e-12


def test_beta_to_band_is_floor():
    assert [F.beta_to_band(b, 256, 256) for b in (0.0, 0.01, 0.05, 0.09, 0.4999)] == [0, 2, 12, 23, 127]
    assert F.beta_to_band(0.09, 256, 200) == 18 and F.beta_to_band(0.49, 7, 9) == 3 and F.beta_to_band(0.49, 8, 8) == 3
    for n in (1, 2, 7, 8, 255, 256, 1024):
        for beta in (0.0, 0.1, 0.25, 0.4, 0.49999999999999994):
            assert 0 <= F.beta_to_band(beta, n, n + 3) == min(int(np.floor(beta * n)), (n - 1) // 2) <= (n - 1) // 2


def test_stylizer_draws():
    P = pkg("parallel")
    s = F.FdaStylizer(["unused"], beta=(0.01, 0.09), prob=0.3, seed=5, shard=(2, 4))
    ref = np.random.default_rng(5 + P.rank_seed(2))
    band, pair = s.draw(4000, 7, 256, 256)
    u, beta, p = ref.random(4000), ref.uniform(0.01, 0.09, 4000), ref.integers(0, 7, 4000)
    assert np.array_equal(pair, p) and pair.dtype == np.int32 and band.dtype == np.int32
    assert pair.min() == 0 and pair.max() == 6
    want = np.where(u < 0.3, np.floor(beta * 256).astype(np.int64), -1)
    assert np.array_equal(band, want)
    share = float((band >= 0).mean())
    assert abs(share - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / 4000), share           # five standard deviations of the binomial share
    assert band[band >= 0].min() >= 2 and band.max() <= 23
    # reproducible from the seed and the rank, and ranks differ
    b2, p2 = F.FdaStylizer(["unused"], beta=(0.01, 0.09), prob=0.3, seed=5, shard=(2, 4)).draw(4000, 7, 256, 256)
    assert np.array_equal(b2, band) and np.array_equal(p2, pair)
    b3, p3 = F.FdaStylizer(["unused"], beta=(0.01, 0.09), prob=0.3, seed=5, shard=(1, 4)).draw(4000, 7, 256, 256)
    assert not np.array_equal(p3, pair)
    assert (F.FdaStylizer(["unused"], prob=0.0).draw(64, 3, 64, 64)[0] == -1).all()
    b1 = F.FdaStylizer(["unused"], beta=0.05, prob=1.0).draw(64, 3, 64, 64)[0]
    assert (b1 == 3).all()


def test_stylizer_refusals():
    for beta in (0.5, -0.01, (0.2, 0.1), (0.1, 0.5), (0.1, 0.2, 0.3), float("nan"), "x"):
        with pytest.raises(ValueError):
            F.FdaStylizer(["unused"], beta=beta)
    for prob in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError):
            F.FdaStylizer(["unused"], prob=prob)


def test_train_segmenter_flags():
    ts = pkg("train_segmenter")
    _, a = ts.parse_args([])
    assert a.fda_target is None and a.fda_beta is None and a.fda_prob is None
    _, a = ts.parse_args(["--fda-target", "L"])
    assert (a.fda_target, a.fda_beta, a.fda_prob) == ("L", 0.01, 1.0)
    _, a = ts.parse_args(["--fda-target", "L", "--fda-beta", "0.01,0.09", "--fda-prob", "0.5"])
    assert (a.fda_beta, a.fda_prob) == ((0.01, 0.09), 0.5)
    _, a = ts.parse_args(["--fda-target", "L", "--fda-beta", "0.05", "--fda-prob", "0"])
    assert (a.fda_beta, a.fda_prob) == (0.05, 0.0)
    for bad in (["--fda-target", "L", "--fda-beta", "0.5"], ["--fda-target", "L", "--fda-beta", "-0.1"],
                ["--fda-target", "L", "--fda-beta", "0.09,0.01"], ["--fda-target", "L", "--fda-beta", "0.1,0.6"],
                ["--fda-target", "L", "--fda-beta", "0.1,0.2,0.3"], ["--fda-target", "L", "--fda-beta", "abc"],
                ["--fda-target", "L", "--fda-prob", "1.5"], ["--fda-target", "L", "--fda-prob", "-0.1"],
                ["--fda-beta", "0.01"], ["--fda-prob", "0.5"]):
        with pytest.raises(SystemExit):
            ts.parse_args(bad)


def test_wrapper_refuses_cpu_tensors(built):
    K, L = pkg("kernels"), pkg("_lib")
    x, t = torch.zeros((2, 8, 8, 3)), torch.zeros((1, 8, 8, 3))
    with pytest.raises(L.PnpError):
        K.fda_amplitude_swap(x, t, [1, 1], [0, 0])
    with pytest.raises(L.PnpError):
        K.fda_amplitude_swap(x, t, [-1, -1], [0, 0], out=x)


def test_workspace_query(built):
    lib = built._lib.load()
    need = lib.pnp_fda_workspace_bytes(16, 16, 256, 256, 3, 23)
    assert need == 32 * 3 * 24 * (256 + 47) * 8
    assert lib.pnp_fda_workspace_bytes(16, 16, 256, 256, 3, -1) == 0
    assert lib.pnp_fda_workspace_bytes(16, 16, 256, 256, 3, 128) == 0          # beyond (min(H, W) - 1) // 2: no valid call
    assert lib.pnp_fda_workspace_bytes(0, 16, 256, 256, 3, 2) == 0
