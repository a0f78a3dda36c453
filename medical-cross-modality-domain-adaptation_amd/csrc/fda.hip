// fda.hip — Fourier domain adaptation (Yang & Soatto, CVPR 2020; not in the reference): every source image keeps the
// phase of its 2-D spectrum and takes a target image's amplitude on the low-frequency square |u| <= b, |v| <= b.
//
//   S = DFT2(src[i, :, :, c]),  T = DFT2(tgt[pair[i], :, :, c]),  b = band[i]
//   D(u, v) = (|T| - |S|) S / |S|   (|S| = 0 exactly: |T|)   on the band, 0 elsewhere
//   out[i, :, :, c] = src[i, :, :, c] + Re IDFT2(D)          (b = -1: the sample is copied bit for bit)
//
// A separable truncated DFT: only the band is ever formed.  src and tgt are real, so D is Hermitian and only v in [0, b] is kept; the
// row synthesis weighs v > 0 twice.
//   1 row analysis       R(h, v) = sum_w x(h, w) e^{-2 pi i v w / W}, v in [0, b]: every row of every source and of every target in use
//   2 column analysis    F(u, v) = sum_h R(h, v) e^{-2 pi i u h / H},  u in [-b, b]
//   3 column synthesis   G(h, v) = sum_u D(u, v) e^{+2 pi i u h / H}, D formed from the source's and the target's F with hypotf
//   4 row synthesis      out(h, w) = src(h, w) + 1 / (H W) sum_v m_v Re(G(h, v) e^{+2 pi i v w / W}),  m_0 = 1, m_v>0 = 2
// Twiddles: (k x) mod N is kept exactly in integers and indexes a table that each block fills with sincospi in double, rounded to fp32;
// no angle is accumulated.
// Plain fp32 FMAs, no atomics, one fixed summation order: bit-identical from run to run.  band and pair travel in the argument block
// (checked on the host, no copy, no host read); a target's band is the largest band of the samples paired with it.
#include "pnp_common.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int NT = 256;
constexpr int MAX_BATCH = 256;
constexpr int MAX_EXTENT = 1024;
constexpr int MAX_CH = 4;
constexpr int MAX_BAND = (MAX_EXTENT - 1) / 2;

struct FdaArgs {
    int16_t band[MAX_BATCH];      // per source sample; -1: copied
    int16_t tband[MAX_BATCH];     // per target image: the largest band of the samples paired with it; -1: not in use
    uint8_t pair[MAX_BATCH];
};

// tw[k] = (cos, sin)(2 pi k / N), the angle taken in (-pi, pi], evaluated in double and rounded once to fp32.  An fp32 argument 2 kk / N
// is itself off by up to 2^-24 of its value; such a table nearly doubled the error of a phase-sensitive case.
__device__ __forceinline__ void fill_twiddles(float2* tw, int N) {
    for (int k = threadIdx.x; k < N; k += NT) {
        const int kk = 2 * k <= N ? k : k - N;
        double s, c;
        sincospi((double)(2 * kk) / (double)N, &s, &c);
        tw[k] = make_float2((float)c, (float)s);
    }
}

// threads that share one output's sum when a block has fewer outputs than threads (a power of two, contiguous segments)
__device__ __forceinline__ int segments(int nout) {
    int nseg = 1;
    while (nseg * 2 * nout <= NT) nseg *= 2;
    return nseg;
}

// the per-segment partial sums of thread t's output, added in segment order by the output's first thread
__device__ __forceinline__ float2 combine(float2* part, float2 mine, int nseg) {
    part[threadIdx.x] = mine;
    __syncthreads();
    float2 acc = part[threadIdx.x];
    if (threadIdx.x % nseg == 0)
        for (int k = 1; k < nseg; ++k) {
            acc.x += part[threadIdx.x + k].x;
            acc.y += part[threadIdx.x + k].y;
        }
    return acc;
}

__device__ __forceinline__ int img_band(const FdaArgs& a, int img, int B) { return img < B ? a.band[img] : a.tband[img - B]; }

// ---- 1 row analysis: one block per (image, row); images 0..B-1 are the sources, B..B+Bt-1 the targets ---------------------------------
__global__ void __launch_bounds__(NT) fda_row_analysis(const float* __restrict__ src, const float* __restrict__ tgt, float2* __restrict__ R,
                                                        int B, int H, int W, int C, int bmax, FdaArgs a) {
    __shared__ float xs[MAX_EXTENT * MAX_CH];
    __shared__ float2 tw[MAX_EXTENT];
    __shared__ float2 part[NT];
    const int img = blockIdx.x / H, h = blockIdx.x % H;
    const int b = img_band(a, img, B);
    if (b < 0) return;
    const float* __restrict__ row = (img < B ? src + (size_t)img * H * W * C : tgt + (size_t)(img - B) * H * W * C) + (size_t)h * W * C;
    for (int e = threadIdx.x; e < W * C; e += NT) xs[e] = row[e];
    fill_twiddles(tw, W);
    __syncthreads();
    const int nout = C * (b + 1), nseg = segments(nout), seg = (W + nseg - 1) / nseg;
    for (int o0 = 0; o0 < nout; o0 += NT / nseg) {      // nseg > 1: a single pass
        const int o = o0 + (int)threadIdx.x / nseg, s = (int)threadIdx.x % nseg;
        float2 acc = make_float2(0.f, 0.f);
        if (o < nout) {
            const int v = o / C, c = o % C;
            const int w0 = std::min(W, s * seg), w1 = std::min(W, w0 + seg);
            int idx = (v * w0) % W;
            for (int w = w0; w < w1; ++w) {
                const float x = xs[w * C + c];
                const float2 t = tw[idx];
                acc.x = fmaf(x, t.x, acc.x);
                acc.y = fmaf(-x, t.y, acc.y);
                idx += v;
                if (idx >= W) idx -= W;
            }
        }
        if (nseg > 1) acc = combine(part, acc, nseg);
        if (o < nout && s == 0) {
            const int v = o / C, c = o % C;
            R[(((size_t)img * C + c) * (bmax + 1) + v) * H + h] = acc;
        }
    }
}

// ---- 2 column analysis: one block per (image, channel, v) ------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) fda_col_analysis(const float2* __restrict__ R, float2* __restrict__ F, int B, int H, int C, int bmax,
                                                        FdaArgs a) {
    __shared__ float2 col[MAX_EXTENT];
    __shared__ float2 tw[MAX_EXTENT];
    __shared__ float2 part[NT];
    const int nb = bmax + 1;
    const int img = blockIdx.x / (C * nb), c = (blockIdx.x / nb) % C, v = blockIdx.x % nb;
    const int b = img_band(a, img, B);
    if (v > b) return;
    const size_t line = ((size_t)img * C + c) * nb + v;
    for (int h = threadIdx.x; h < H; h += NT) col[h] = R[line * H + h];
    fill_twiddles(tw, H);
    __syncthreads();
    const int nout = 2 * b + 1, nseg = segments(nout), seg = (H + nseg - 1) / nseg;
    for (int o0 = 0; o0 < nout; o0 += NT / nseg) {
        const int o = o0 + (int)threadIdx.x / nseg, s = (int)threadIdx.x % nseg;
        float2 acc = make_float2(0.f, 0.f);
        if (o < nout) {
            const int um = o - b < 0 ? o - b + H : o - b;      // u mod H
            const int h0 = std::min(H, s * seg), h1 = std::min(H, h0 + seg);
            int idx = (um * h0) % H;
            for (int h = h0; h < h1; ++h) {
                const float2 x = col[h], t = tw[idx];      // x * conj(t)
                acc.x = fmaf(x.x, t.x, fmaf(x.y, t.y, acc.x));
                acc.y = fmaf(x.y, t.x, fmaf(-x.x, t.y, acc.y));
                idx += um;
                if (idx >= H) idx -= H;
            }
        }
        if (nseg > 1) acc = combine(part, acc, nseg);
        if (o < nout && s == 0) F[line * (2 * bmax + 1) + (o - b + bmax)] = acc;
    }
}

// ---- 3 column synthesis of D: one block per (source, channel, v); G overwrites the source's R ------------------------------------------
__global__ void __launch_bounds__(NT) fda_col_synthesis(const float2* __restrict__ F, float2* __restrict__ G, int B, int H, int C, int bmax,
                                                         FdaArgs a) {
    __shared__ float2 d[2 * MAX_BAND + 1];
    __shared__ float2 tw[MAX_EXTENT];
    const int nb = bmax + 1;
    const int i = blockIdx.x / (C * nb), c = (blockIdx.x / nb) % C, v = blockIdx.x % nb;
    const int b = a.band[i];
    if (v > b) return;
    const size_t ls = ((size_t)i * C + c) * nb + v, lt = ((size_t)(B + a.pair[i]) * C + c) * nb + v;
    for (int o = threadIdx.x; o < 2 * b + 1; o += NT) {
        const int k = o - b + bmax;
        const float2 S = F[ls * (2 * bmax + 1) + k], T = F[lt * (2 * bmax + 1) + k];
        const float r = hypotf(S.x, S.y), t = hypotf(T.x, T.y);
        if (r > 0.f) {
            const float g = (t - r) / r;
            d[o] = make_float2(S.x * g, S.y * g);
        } else {
            d[o] = make_float2(t, 0.f);      // numpy's angle(0) = 0
        }
    }
    fill_twiddles(tw, H);
    __syncthreads();
    for (int h = threadIdx.x; h < H; h += NT) {
        int idx = (H - (b * h) % H) % H;            // (-b h) mod H
        float2 acc = make_float2(0.f, 0.f);
        for (int o = 0; o < 2 * b + 1; ++o) {
            const float2 x = d[o], t = tw[idx];     // x * t
            acc.x = fmaf(x.x, t.x, fmaf(-x.y, t.y, acc.x));
            acc.y = fmaf(x.y, t.x, fmaf(x.x, t.y, acc.y));
            idx += h;
            if (idx >= H) idx -= H;
        }
        G[ls * H + h] = acc;
    }
}

// ---- 4 real row synthesis added onto src: one block per (source, row) ------------------------------------------------------------------
__global__ void __launch_bounds__(NT) fda_row_synthesis(const float* src, const float2* __restrict__ G, float* out, int H, int W, int C,
                                                         int bmax, float inv_hw, FdaArgs a) {
    __shared__ float2 g[(MAX_BAND + 1) * MAX_CH];
    __shared__ float2 tw[MAX_EXTENT];
    const int i = blockIdx.x / H, h = blockIdx.x % H;
    const int b = a.band[i];
    const size_t base = ((size_t)i * H + h) * W * C;      // src and out may be one buffer: each element is read, then written, by one thread
    if (b < 0) {
        if (out != src)
            for (int e = threadIdx.x; e < W * C; e += NT) out[base + e] = src[base + e];
        return;
    }
    const int nb = bmax + 1;
    for (int o = threadIdx.x; o < C * (b + 1); o += NT) {
        const int c = o / (b + 1), v = o % (b + 1);
        g[o] = G[(((size_t)i * C + c) * nb + v) * H + h];
    }
    fill_twiddles(tw, W);
    __syncthreads();
    for (int e = threadIdx.x; e < W * C; e += NT) {
        const int w = e / C, c = e % C;
        const float2* gc = g + c * (b + 1);
        const float dc = gc[0].x;                   // v = 0: Im G(h, 0) cancels against u -> -u
        float ac = 0.f;
        int idx = w;
        for (int v = 1; v <= b; ++v) {
            const float2 t = tw[idx];
            ac = fmaf(gc[v].x, t.x, fmaf(-gc[v].y, t.y, ac));
            idx += w;
            if (idx >= W) idx -= W;
        }
        out[base + e] = fmaf(fmaf(2.f, ac, dc), inv_hw, src[base + e]);
    }
}

inline bool in_range(long long v, long long lo, long long hi) { return v >= lo && v <= hi; }

inline bool overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" {

size_t pnp_fda_workspace_bytes(int32_t B, int32_t Bt, int32_t H, int32_t W, int32_t C, int32_t max_band) {
    if (!in_range(B, 1, MAX_BATCH) || !in_range(Bt, 1, MAX_BATCH) || !in_range(H, 1, MAX_EXTENT) || !in_range(W, 1, MAX_EXTENT) ||
        !in_range(C, 1, MAX_CH) || !in_range(max_band, -1, (std::min(H, W) - 1) / 2) || max_band < 0)
        return 0;
    // R (then G) [B + Bt][C][b + 1][H] and F [B + Bt][C][b + 1][2 b + 1], complex fp32
    return (size_t)(B + Bt) * C * (max_band + 1) * ((size_t)H + 2 * max_band + 1) * sizeof(float2);
}

int pnp_fda_amplitude_swap(const float* src, int32_t B, const float* tgt, int32_t Bt, int32_t H, int32_t W, int32_t C, const int32_t* band,
                           const int32_t* pair, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(src && tgt && band && pair && out, "pnp_fda_amplitude_swap: bad argument (null pointer)");
    PNP_REQUIRE(in_range(B, 1, MAX_BATCH) && in_range(Bt, 1, MAX_BATCH), "pnp_fda_amplitude_swap: B = %d, Bt = %d, each must lie in [1, %d]",
                (int)B, (int)Bt, MAX_BATCH);
    PNP_REQUIRE(in_range(H, 1, MAX_EXTENT) && in_range(W, 1, MAX_EXTENT), "pnp_fda_amplitude_swap: H = %d, W = %d, each must lie in [1, %d]",
                (int)H, (int)W, MAX_EXTENT);
    PNP_REQUIRE(in_range(C, 1, MAX_CH), "pnp_fda_amplitude_swap: C = %d, must lie in [1, %d]", (int)C, MAX_CH);
    const int bcap = (std::min(H, W) - 1) / 2;
    FdaArgs a = {};
    int bmax = -1;
    for (int j = 0; j < Bt; ++j) a.tband[j] = -1;
    for (int i = 0; i < B; ++i) {
        PNP_REQUIRE(in_range(band[i], -1, bcap), "pnp_fda_amplitude_swap: band[%d] = %d, must lie in [-1, %d] for %d x %d", i, (int)band[i], bcap,
                    (int)H, (int)W);
        PNP_REQUIRE(in_range(pair[i], 0, Bt - 1), "pnp_fda_amplitude_swap: pair[%d] = %d, must lie in [0, %d)", i, (int)pair[i], (int)Bt);
        a.band[i] = (int16_t)band[i];
        a.pair[i] = (uint8_t)pair[i];
        a.tband[pair[i]] = (int16_t)std::max<int>(a.tband[pair[i]], band[i]);
        bmax = std::max<int>(bmax, band[i]);
    }
    const size_t ns = (size_t)B * H * W * C * sizeof(float), nt = (size_t)Bt * H * W * C * sizeof(float);
    PNP_REQUIRE(!overlap(out, ns, tgt, nt), "pnp_fda_amplitude_swap: out overlaps tgt");
    PNP_REQUIRE(out == src || !overlap(out, ns, src, ns), "pnp_fda_amplitude_swap: out overlaps src in part (in place means out == src)");
    const size_t need = pnp_fda_workspace_bytes(B, Bt, H, W, C, bmax);
    PNP_REQUIRE(workspace || need == 0, "pnp_fda_amplitude_swap: bad argument (null workspace)");
    PNP_REQUIRE(workspace_bytes >= need, "pnp_fda_amplitude_swap: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int nb = bmax + 1;
    float2* R = (float2*)workspace;
    float2* F = R + (size_t)(B + Bt) * C * nb * H;
    if (bmax >= 0) {
        hipLaunchKernelGGL(fda_row_analysis, dim3((unsigned)((B + Bt) * H)), dim3(NT), 0, st, src, tgt, R, (int)B, (int)H, (int)W, (int)C, bmax, a);
        PNP_CHECK_LAUNCH("fda_row_analysis");
        hipLaunchKernelGGL(fda_col_analysis, dim3((unsigned)((B + Bt) * C * nb)), dim3(NT), 0, st, (const float2*)R, F, (int)B, (int)H, (int)C,
                           bmax, a);
        PNP_CHECK_LAUNCH("fda_col_analysis");
        hipLaunchKernelGGL(fda_col_synthesis, dim3((unsigned)(B * C * nb)), dim3(NT), 0, st, (const float2*)F, R, (int)B, (int)H, (int)C, bmax, a);
        PNP_CHECK_LAUNCH("fda_col_synthesis");
    } else if (out == src) {
        return PNP_OK;      // every sample keeps its values, in place
    }
    const float inv_hw = (float)(1.0 / ((double)H * (double)W));
    hipLaunchKernelGGL(fda_row_synthesis, dim3((unsigned)(B * H)), dim3(NT), 0, st, src, (const float2*)R, out, (int)H, (int)W, (int)C, bmax,
                       inv_hw, a);
    PNP_CHECK_LAUNCH("fda_row_synthesis");
    return PNP_OK;
}

}  // extern "C"
