"""float64 restatement of Fourier domain adaptation with np.fft, in the FDA authors' form (FDA_source_to_target_np:
fftshift, swap the centred (2b+1)^2 block of the amplitude, keep the phase, inverse): the definition the kernel is held to.  Per sample a
band (-1: unchanged) and the index of its target.

The error of any fp32 evaluation is driven by the phase sensitivity |T| / |S| over the band, not by band_ratio alone: band_ratio >= 1e-6
is the input condition, not a bound.  fda_route32 is the fp32 yardstick (the kernel's separable method in float32 matmuls) and
route_bar the per-case bar built on it."""
import numpy as np
import torch


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


SPECTRAL_SIGMA = 0.5          # the envelope's width in cycles per sample


def _mirror(a):
    """a(-k mod N) over the last two axes"""
    return np.roll(np.flip(a, (-2, -1)), 1, (-2, -1))


def spectral(rng, B, H, W, C, floor, return_spectrum=False):
    """the source generator for sizes where blobs misses the input condition: per channel an exactly Hermitian spectrum X (X(-k) =
    conj X(k) bit for bit, the self-conjugate bins real) with floor * env(k) <= |X(k)| <= env(k), env = exp(-|f|^2 / (2 sigma^2)) over
    the signed frequencies f = k / N (peak 1 at DC); the image is Re IDFT2(X) scaled to unit rms and rounded to float32.  Draws per
    channel: the amplitude's uniforms, then the phase's.  -> [B, H, W, C] float32 (and X [B, C, H, W] complex128 with
    return_spectrum)"""
    fu, fv = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    env = np.exp(-(fu * fu + fv * fv) / (2.0 * SPECTRAL_SIGMA ** 2))          # even in k exactly: (-f)^2 == f^2
    out = np.zeros((B, H, W, C), np.float32)
    spec = np.zeros((B, C, H, W), np.complex128)
    for i in range(B):
        for c in range(C):
            a = floor + (1.0 - floor) * rng.random((H, W))
            amp = env * (0.5 * (a + _mirror(a)))                                 # a + a(-k) is symmetric bit for bit
            p = rng.uniform(-np.pi, np.pi, (H, W))
            phi = 0.5 * (p - _mirror(p))                                         # odd bit for bit, 0 on the self-conjugate bins
            m = np.abs(phi)
            X = amp * (np.cos(m) + 1j * (np.sign(phi) * np.sin(m)))
            x = np.fft.ifft2(X).real
            x /= np.sqrt(np.mean(x * x))
            out[i, :, :, c] = x
            spec[i, c] = X
    return (out, spec) if return_spectrum else out


def _twiddles(n, k, x, sign):
    """[len(k), len(x)] of exp(sign 2 pi i k x / n): (k x) mod n in exact integers, the angle in float64, rounded to complex64"""
    m = np.mod(np.outer(np.asarray(k, np.int64), np.asarray(x, np.int64)), n)
    return torch.from_numpy(np.exp(sign * 2j * np.pi * m / n).astype(np.complex64))


def fda_route32(src, tgt, band, pair):
    """the fp32 route: the kernel's separable truncated DFT written in float32 with torch complex64 matmuls on the CPU (no FFT):
    R = x Aw (band-only row DFT, v in [0, b]), F = Ah R (column DFT, u in [-b, b]), D = (|T| - |S|) S / |S| (|T| where |S| = 0),
    G = Gh D (column synthesis), out = src + Re(G Bw) / (H W) (real row synthesis, v > 0 weighted 2).  -> [B, H, W, C] float64 holding
    float32 values"""
    s32 = torch.from_numpy(np.array(src, np.float32))
    t32 = torch.from_numpy(np.array(tgt, np.float32))
    B, H, W, C = s32.shape
    inv_hw = torch.tensor(1.0 / (H * W), dtype=torch.float32)
    out = s32.clone()
    mats = {}
    for i in range(B):
        b = int(band[i])
        if b < 0:
            continue
        if b not in mats:
            v, u, h, w = np.arange(b + 1), np.arange(-b, b + 1), np.arange(H), np.arange(W)
            weight = torch.from_numpy(np.where(v > 0, 2.0, 1.0).astype(np.float32))[:, None]
            mats[b] = (_twiddles(W, w, v, -1), _twiddles(H, u, h, -1), _twiddles(H, h, u, 1), _twiddles(W, v, w, 1) * weight)
        Aw, Ah, Gh, Bw = mats[b]

        def analyse(x):                                             # [H, W, C] float32 -> [C, 2b + 1, b + 1]
            return Ah @ (x.permute(2, 0, 1).to(torch.complex64) @ Aw)

        S, T = analyse(s32[i]), analyse(t32[int(pair[i])])
        r, t = S.abs(), T.abs()
        D = torch.where(r > 0, S * ((t - r) / torch.where(r > 0, r, torch.ones_like(r))), t.to(torch.complex64))
        y = (Gh @ D @ Bw).real * inv_hw                             # [C, H, W]
        out[i] = s32[i] + y.permute(1, 2, 0)
    return out.numpy().astype(np.float64)


def route_bar(ref, route):
    """the bar built on the fp32 route: 2 x max(max|route - ref| / max|ref|, 1e-6) x max|ref| (absolute)"""
    scale = float(np.abs(ref).max())
    return 2.0 * max(float(np.abs(np.asarray(route) - ref).max()) / scale, 1e-6) * scale
