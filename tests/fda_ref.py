"""float64 restatement of Fourier domain adaptation with np.fft, in the FDA authors' form (FDA_source_to_target_np:
fftshift, swap the centred (2b+1)^2 block of the amplitude, keep the phase, inverse): the definition the kernel is held to.  Per sample a
band (-1: unchanged) and the index of its target."""
import numpy as np


def swap_channel(s, t, b):
    """one channel: s, t [H, W] real -> Re IDFT2 of s's spectrum with |T| on |u|, |v| <= b (float64)"""
    if b < 0:
        return np.array(s, dtype=np.float64)
    H, W = s.shape
    S = np.fft.fftshift(np.fft.fft2(np.asarray(s, np.float64)))
    T = np.fft.fftshift(np.fft.fft2(np.asarray(t, np.float64)))
    amp, pha = np.abs(S), np.angle(S)
    ch, cw = H // 2, W // 2          # the zero frequency after fftshift
    amp[ch - b:ch + b + 1, cw - b:cw + b + 1] = np.abs(T)[ch - b:ch + b + 1, cw - b:cw + b + 1]
    return np.fft.ifft2(np.fft.ifftshift(amp * np.exp(1j * pha)))


def fda_ref(src, tgt, band, pair, return_complex=False):
    """src [B, H, W, C], tgt [Bt, H, W, C] -> [B, H, W, C] float64 (complex with return_complex: the inverse before Re)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    out = np.zeros(src.shape, np.complex128 if return_complex else np.float64)
    for i in range(src.shape[0]):
        for c in range(src.shape[3]):
            r = swap_channel(src[i, :, :, c], tgt[int(pair[i]), :, :, c], int(band[i]))
            out[i, :, :, c] = r if return_complex else np.real(r)
    return out


def blobs(rng, B, H, W, C):
    """the test generator: per channel four Gaussian blobs (centres U(0.2, 0.8), radii U(0.05, 0.3) of max(H, W), amplitudes U(-2, 2))
    plus N(0, 0.3) noise"""
    yy, xx = np.meshgrid(np.arange(H) / max(H, W), np.arange(W) / max(H, W), indexing="ij")
    out = np.zeros((B, H, W, C))
    for i in range(B):
        for c in range(C):
            img = rng.normal(0.0, 0.3, (H, W))
            for _ in range(4):
                cy, cx = rng.uniform(0.2, 0.8, 2) * np.array([H, W]) / max(H, W)
                r, a = rng.uniform(0.05, 0.3), rng.uniform(-2.0, 2.0)
                img += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
            out[i, :, :, c] = img
    return out.astype(np.float32)


def band_ratio(src, band):
    """min over stylised samples and channels, over the band's coefficients, of |S(k)| / max |S| of that image (inf if there are none;
    all-zero channels are skipped)"""
    worst = np.inf
    for i in range(src.shape[0]):
        b = int(band[i])
        if b < 0:
            continue
        for c in range(src.shape[3]):
            x = np.asarray(src[i, :, :, c], np.float64)
            if not np.any(x):
                continue
            A = np.abs(np.fft.fftshift(np.fft.fft2(x)))
            ch, cw = x.shape[0] // 2, x.shape[1] // 2
            worst = min(worst, A[ch - b:ch + b + 1, cw - b:cw + b + 1].min() / A.max())
    return worst
