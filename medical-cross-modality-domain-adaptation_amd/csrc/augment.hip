// Training input from resident volumes: per-volume preprocessing (clip at an exact order statistic, z-score) and the
// augmented slice gather (affine-warped 3-frame slices, bilinear image / nearest label / one-hot, one pass).
//
//   preprocess   init          zero the 4 histograms, the selection state {prefix, k}
//                hist x 4      per block: LDS histogram of the round's 8-bit digit over the keys that share the prefix found so far, then
//                              integer atomics of the non-empty bins into the round's global histogram
//                pick  x 4     one wave walks the 256 bins: the digit whose bin holds rank k; prefix |= digit << shift, k -= bins below
//                sum           per-block float64 partial sums of min(v, clip) and partial minima of v (fixed grid, fixed tree)
//                dev           every block re-adds the partial sums in the same fixed order -> mean; partial sums of squared deviations
//                normalize     every block re-adds both partial lists -> mean, std; out = (min(v, clip) - mean) / std; block 0 writes stats
//   gather       one launch: a lane owns 4 consecutive output pixels = three float4 of image, one float4 of label, ncls float4 of one-hot
//   warped gather: the same launch shape; a cubic B-spline displacement from a per-sample control table joins the
//                coordinate, gain / bias / hashed Gaussian noise act on the image values on the way out
//
// Every sum is a fixed-order tree over a grid that depends on n alone, every atomic is an integer atomic: results are bit-identical
// from run to run.
#include <algorithm>
#include <math.h>
#include <type_traits>

#include "block_sum.h"
#include "pnp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;        // grid of the reductions: the partial lists have at most this many entries
constexpr int kMaxExtentXY = 4096;
constexpr int kMaxCls = 32;
constexpr int kMaxWarpGrid = 16;          // cells per axis of a warp's control lattice

struct SelState {
    uint32_t prefix;    // the key bits fixed by the rounds done so far
    uint32_t k;         // rank of the wanted element among the keys that share the prefix (n < 2^31)
};

// order-preserving key of a finite float: negative values flip all bits, the others set the sign bit (-0.0 sorts just below +0.0: the
// two are equal by value, which is all the clip needs)
__device__ __forceinline__ uint32_t key_of(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__global__ void __launch_bounds__(kThreads) pre_init_kernel(unsigned int* __restrict__ hist, SelState* __restrict__ st, uint32_t k) {
    for (int i = threadIdx.x; i < 4 * 256; i += kThreads) hist[i] = 0u;
    if (threadIdx.x == 0) {
        st->prefix = 0u;
        st->k = k;
    }
}

__global__ void __launch_bounds__(kThreads) pre_hist_kernel(const float* __restrict__ v, long long n, int shift, uint32_t mask,
                                                            const SelState* __restrict__ st, unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t prefix = st->prefix;
    const long long gs = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += gs) {
        const uint32_t key = key_of(v[i]);
        if ((key & mask) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned int c = h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

__global__ void __launch_bounds__(64) pre_pick_kernel(const unsigned int* __restrict__ hist, int shift, SelState* __restrict__ st) {
    if (threadIdx.x != 0) return;
    uint32_t k = st->k;
    int b = 0;
    for (; b < 255; ++b) {
        const unsigned int c = hist[b];
        if (k < c) break;
        k -= c;
    }
    st->prefix |= (uint32_t)b << shift;
    st->k = k;
}

__global__ void __launch_bounds__(kThreads) pre_sum_kernel(const float* __restrict__ v, long long n, const SelState* __restrict__ st,
                                                           double* __restrict__ psum, float* __restrict__ pmin) {
    __shared__ double sh[kThreads];
    __shared__ float shm[kThreads];
    const float clip = float_of(st->prefix);
    const long long gs = (long long)gridDim.x * kThreads;
    double a = 0.0;
    float m = INFINITY;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += gs) {
        const float x = v[i];
        a += (double)fminf(x, clip);
        m = fminf(m, x);
    }
    shm[threadIdx.x] = m;
    const double s = block_tree<kThreads>(a, sh);
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) shm[threadIdx.x] = fminf(shm[threadIdx.x], shm[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = s;
        pmin[blockIdx.x] = shm[0];
    }
}

__global__ void __launch_bounds__(kThreads) pre_dev_kernel(const float* __restrict__ v, long long n, const SelState* __restrict__ st,
                                                           const double* __restrict__ psum, double* __restrict__ pdev) {
    __shared__ double sh[kThreads];
    const float clip = float_of(st->prefix);
    const double mean = block_sum_of_list<kThreads>(psum, gridDim.x, sh) / (double)n;
    const long long gs = (long long)gridDim.x * kThreads;
    double a = 0.0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += gs) {
        const double d = (double)fminf(v[i], clip) - mean;
        a = fma(d, d, a);
    }
    const double s = block_tree<kThreads>(a, sh);
    if (threadIdx.x == 0) pdev[blockIdx.x] = s;
}

__device__ __forceinline__ float normalized(float x, float clip, double mean, double inv_std) {
    return (float)(((double)fminf(x, clip) - mean) * inv_std);
}

__global__ void __launch_bounds__(kThreads) pre_normalize_kernel(const float* v, float* out, long long n, const SelState* __restrict__ st,
                                                                 const double* __restrict__ psum, const double* __restrict__ pdev,
                                                                 const float* __restrict__ pmin, double* __restrict__ stats) {
    __shared__ double sh[kThreads];
    __shared__ float shm[kThreads];
    const float clip = float_of(st->prefix);
    const double mean = block_sum_of_list<kThreads>(psum, gridDim.x, sh) / (double)n;
    const double std_ = sqrt(block_sum_of_list<kThreads>(pdev, gridDim.x, sh) / (double)n);
    const double inv_std = std_ > 0.0 ? 1.0 / std_ : 0.0;          // std == 0: every output is 0
    if (blockIdx.x == 0) {
        float m = INFINITY;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += kThreads) m = fminf(m, pmin[i]);
        shm[threadIdx.x] = m;
        __syncthreads();
        for (int h = kThreads / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) shm[threadIdx.x] = fminf(shm[threadIdx.x], shm[threadIdx.x + h]);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            stats[0] = (double)clip;
            stats[1] = mean;
            stats[2] = std_;
            stats[3] = (double)normalized(shm[0], clip, mean, inv_std);
        }
    }
    const long long gs = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += gs) out[i] = normalized(v[i], clip, mean, inv_std);
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------------
struct Px {
    float c[3];
    float lab;
};

// FRAC (pnp_aug_slices_z): channels 0 / 2 sit at the fractional frames zlo / zhi (clamped into [0, Z - 1] by the caller);
// a corner's value there is the lerp between the two frames around it, taken BEFORE the bilinear chain (z is the fastest axis: the two
// reads are adjacent).  Without FRAC the three channels are the frames z - 1, z, z + 1 and (zlo, zhi) are not read.
// sample_at: the sample at source coordinates (sx, sy) — what the affine gathers and the warped one share.
template <bool FRAC>
__device__ __forceinline__ Px sample_at(const pnp_aug_volume& vol, int z, float zlo, float zhi, float sx, float sy) {
    Px r;
    const float fill = vol.fill;
    r.c[0] = r.c[1] = r.c[2] = fill;
    r.lab = 0.f;
    const int X = vol.X, Y = vol.Y, Z = vol.Z;
    // outside (-1, X) x (-1, Y) all four corners are outside the slice (a NaN coordinate fails the comparisons too)
    if (!(sx > -1.f && sx < (float)X && sy > -1.f && sy < (float)Y)) return r;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;             // in [-1, X - 1] x [-1, Y - 1]
    const float tx = sx - fx0, ty = sy - fy0;           // exact (Sterbenz / small magnitudes)
    const float ux = 1.f - tx, uy = 1.f - ty;
    const bool xin0 = x0 >= 0, xin1 = x0 + 1 < X, yin0 = y0 >= 0, yin1 = y0 + 1 < Y;
    const float* img = vol.image;
    const long long rowY = (long long)Y * Z;
    float v00[3], v01[3], v10[3], v11[3];
    if constexpr (FRAC) {
        const long long o00 = (long long)x0 * rowY + (long long)y0 * Z;      // frame 0 of corner (x0, y0)
        const float flo = floorf(zlo), fhi = floorf(zhi);                   // zlo, zhi in [0, Z - 1]: the conversions are safe
        const float tz[2] = {zlo - flo, zhi - fhi};                         // exact
        const int za[2] = {(int)flo, (int)fhi};
        const int zb[2] = {min(za[0] + 1, Z - 1), min(za[1] + 1, Z - 1)};
        // one corner: in-slice ? lerp along z (outer channels) / the centre frame : fill
        auto corner = [&](bool in, long long o, float* v) {
            v[0] = v[1] = v[2] = fill;
            if (in) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float a = img[o + za[e]], b = img[o + zb[e]];
                    v[2 * e] = fmaf(tz[e], b - a, a);
                }
                v[1] = img[o + z];
            }
        };
        corner(xin0 && yin0, o00, v00);
        corner(xin0 && yin1, o00 + Z, v01);
        corner(xin1 && yin0, o00 + rowY, v10);
        corner(xin1 && yin1, o00 + rowY + Z, v11);
    } else {
        const long long o00 = (long long)x0 * rowY + (long long)y0 * Z + (z - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v00[c] = (xin0 && yin0) ? img[o00 + c] : fill;
            v01[c] = (xin0 && yin1) ? img[o00 + Z + c] : fill;
            v10[c] = (xin1 && yin0) ? img[o00 + rowY + c] : fill;
            v11[c] = (xin1 && yin1) ? img[o00 + rowY + Z + c] : fill;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = fmaf(v01[c], ty, v00[c] * uy);          // along y at x0
        const float b = fmaf(v11[c], ty, v10[c] * uy);          // along y at x0 + 1
        r.c[c] = fmaf(b, tx, a * ux);
    }
    const float lxf = floorf(sx + 0.5f), lyf = floorf(sy + 0.5f);
    if (lxf >= 0.f && lxf < (float)X && lyf >= 0.f && lyf < (float)Y)
        r.lab = (float)vol.label[(long long)(int)lxf * rowY + (long long)(int)lyf * Z + z];
    return r;
}

template <bool FRAC>
__device__ __forceinline__ Px sample_pixel(const pnp_aug_volume& vol, bool ok, int z, float zlo, float zhi, const float* m, int i, int j) {
    if (!ok) {
        Px r;
        r.c[0] = r.c[1] = r.c[2] = vol.fill;
        r.lab = 0.f;
        return r;
    }
    const float sx = fmaf(m[0], (float)i, fmaf(m[1], (float)j, m[2]));
    const float sy = fmaf(m[3], (float)i, fmaf(m[4], (float)j, m[5]));
    return sample_at<FRAC>(vol, z, zlo, zhi, sx, sy);
}

// the stores of one lane's group of 4 consecutive pixels, handed over by value as the vectors that are stored: xa, xb, xc = the 12 image
// floats, lab = the 4 labels (cnt < 4: the scalar tail of the batch)
__device__ __forceinline__ void store_group(f32x4 xa, f32x4 xb, f32x4 xc, f32x4 lab4, int cnt, long long p0, float* __restrict__ x,
                                            float* __restrict__ label, float* __restrict__ onehot, int ncls) {
    if (cnt == 4) {
        f32x4* xo = (f32x4*)(x + p0 * 3);
        xo[0] = xa;
        xo[1] = xb;
        xo[2] = xc;
        *(f32x4*)(label + p0) = lab4;
        if (onehot) {
            f32x4* oo = (f32x4*)(onehot + p0 * ncls);
            int t = 0, c = 0;                                // element e = 4 * w + u of the group's 4 * ncls floats: pixel t, class c
            for (int w = 0; w < ncls; ++w) {
                f32x4 o;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float lab = t == 0 ? lab4[0] : t == 1 ? lab4[1] : t == 2 ? lab4[2] : lab4[3];
                    o[u] = lab == (float)c ? 1.f : 0.f;
                    if (++c == ncls) {
                        c = 0;
                        ++t;
                    }
                }
                oo[w] = o;
            }
        }
    } else {
        for (int t = 0; t < cnt; ++t) {
            const float lab = t == 0 ? lab4[0] : t == 1 ? lab4[1] : lab4[2];
            const float c0 = t == 0 ? xa[0] : t == 1 ? xa[3] : xb[2];
            const float c1 = t == 0 ? xa[1] : t == 1 ? xb[0] : xb[3];
            const float c2 = t == 0 ? xa[2] : t == 1 ? xb[1] : xc[0];
            x[(p0 + t) * 3 + 0] = c0;
            x[(p0 + t) * 3 + 1] = c1;
            x[(p0 + t) * 3 + 2] = c2;
            label[p0 + t] = lab;
            if (onehot)
                for (int c = 0; c < ncls; ++c) onehot[(p0 + t) * ncls + c] = lab == (float)c ? 1.f : 0.f;
        }
    }
}

__device__ __forceinline__ void store_group(const Px* px, int cnt, long long p0, float* __restrict__ x, float* __restrict__ label,
                                            float* __restrict__ onehot, int ncls) {
    store_group(f32x4{px[0].c[0], px[0].c[1], px[0].c[2], px[1].c[0]}, f32x4{px[1].c[1], px[1].c[2], px[2].c[0], px[2].c[1]},
                f32x4{px[2].c[2], px[3].c[0], px[3].c[1], px[3].c[2]}, f32x4{px[0].lab, px[1].lab, px[2].lab, px[3].lab}, cnt, p0, x, label,
                onehot, ncls);
}

// one kernel, two records: FRAC = false is pnp_aug_slices (pnp_aug_sample, frames z - 1, z, z + 1), FRAC = true pnp_aug_slices_z
// (pnp_aug_sample_z: any centre frame, the outer channels at frame -+ dz, clamped)
template <bool FRAC>
__global__ void __launch_bounds__(kThreads) aug_slices_kernel(const pnp_aug_volume* __restrict__ vols, int nvol,
                                                              const std::conditional_t<FRAC, pnp_aug_sample_z, pnp_aug_sample>* __restrict__ samples,
                                                              int H, int W, long long P, float* __restrict__ x, float* __restrict__ label,
                                                              float* __restrict__ onehot, int ncls, unsigned int* __restrict__ errors) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;      // group of 4 consecutive pixels of the flat [B*H*W] index
    const long long p0 = g * 4;
    if (p0 >= P) return;
    const long long HW = (long long)H * W;
    int b = (int)(p0 / HW);
    const long long q = p0 - (long long)b * HW;
    int i = (int)(q / W), j = (int)(q - (long long)i * W);
    const int cnt = (int)((P - p0 < 4) ? (P - p0) : 4);
    Px px[4];
    int cur = -1;
    pnp_aug_volume vol;
    std::conditional_t<FRAC, pnp_aug_sample_z, pnp_aug_sample> s;
    bool ok = false;
    float zlo = 0.f, zhi = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < cnt) {
            if (b != cur) {
                cur = b;
                s = samples[b];
                const bool vok = s.volume >= 0 && s.volume < nvol;
                if (vok) {
                    vol = vols[s.volume];
                } else {
                    vol.image = nullptr; vol.label = nullptr; vol.X = vol.Y = vol.Z = 0; vol.fill = 0.f;
                }
                if constexpr (FRAC) {
                    // dz: finite and >= 0 (NaN fails both comparisons); the clamp replicates the edge frames
                    ok = vok && s.frame >= 0 && s.frame <= vol.Z - 1 && s.dz >= 0.f && s.dz < INFINITY;
                    if (ok) {
                        const float top = (float)(vol.Z - 1);
                        zlo = fminf(fmaxf((float)s.frame - s.dz, 0.f), top);
                        zhi = fminf(fmaxf((float)s.frame + s.dz, 0.f), top);
                    }
                } else {
                    ok = vok && s.frame >= 1 && s.frame <= vol.Z - 2;
                }
                if (!ok && i == 0 && j == 0) atomicAdd(errors, 1u);       // once per refused sample: by the lane that owns its first pixel
            }
            px[t] = sample_pixel<FRAC>(vol, ok, s.frame, zlo, zhi, s.m, i, j);
            if (++j == W) {
                j = 0;
                if (++i == H) {
                    i = 0;
                    ++b;
                }
            }
        } else {
            px[t].c[0] = px[t].c[1] = px[t].c[2] = px[t].lab = 0.f;
        }
    }
    store_group(px, cnt, p0, x, label, onehot, ncls);
}

// ---- the warped gather (pnp_aug_slices_warp) ----------------------------------------------------------------------------
// the four uniform cubic B-spline weights at t in [0, 1].  No product feeds an addition outside an fmaf: the compiler has nothing to
// contract, the order below is the contract (include/pnp_hip.h).
__device__ __forceinline__ void bspline_weights(float t, float* w) {
#pragma clang fp contract(off)
    const float k6 = 1.f / 6.f;
    const float u = 1.f - t;
    w[0] = ((u * u) * u) * k6;
    w[1] = fmaf(t * t, fmaf(3.f, t, -6.f), 4.f) * k6;
    w[2] = fmaf(t, fmaf(t, fmaf(-3.f, t, 3.f), 3.f), 1.f) * k6;
    w[3] = ((t * t) * t) * k6;
}

// the standard normal of counter e under `seed`: Box-Muller over two draws of the dropout counter hash (pnp_common.h)
__device__ __forceinline__ float normal_of(uint32_t e, uint32_t seed) {
#pragma clang fp contract(off)
    const uint32_t h1 = pnp_fmix32(((2u * e) * 0xCC9E2D51u) ^ seed);
    const uint32_t h2 = pnp_fmix32(((2u * e + 1u) * 0xCC9E2D51u) ^ seed);
    const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f;            // (0, 1], exact
    const float u2 = (float)(h2 >> 8) * 0x1p-24f;                   // [0, 1), exact
    return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// aug_slices_kernel<true> with pnp_aug_sample_w records: WARP (G >= 1) adds the B-spline displacement of the sample's control table to
// the coordinates of the samples that ask for it; gain / bias / noise act on the image channels of every accepted sample.  A lane keeps
// the row weights of its current output row and the four row-contracted control values of its current cell column: its 4 pixels share
// them unless the group crosses a row, a sample or a cell border.
template <bool WARP>
__global__ void __launch_bounds__(kThreads) aug_slices_warp_kernel(const pnp_aug_volume* __restrict__ vols, int nvol,
                                                                   const pnp_aug_sample_w* __restrict__ samples,
                                                                   const float2* __restrict__ ctrl, int G, int H, int W, long long P,
                                                                   float* __restrict__ x, float* __restrict__ label, float* __restrict__ onehot,
                                                                   int ncls, unsigned int* __restrict__ errors) {
#pragma clang fp contract(off)                                               // every fused operation below is an explicit fmaf
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;      // group of 4 consecutive pixels of the flat [B*H*W] index
    const long long p0 = g * 4;
    if (p0 >= P) return;
    const long long HW = (long long)H * W;
    int b = (int)(p0 / HW);
    const long long q = p0 - (long long)b * HW;
    int i = (int)(q / W), j = (int)(q - (long long)i * W);
    const int cnt = (int)((P - p0 < 4) ? (P - p0) : 4);
    const int GP = G + 3;                                                     // control points per axis
    const float rh = WARP ? (float)G / (float)H : 0.f, rw = WARP ? (float)G / (float)W : 0.f;
    Px px[4];
    int cur = -1;
    pnp_aug_volume vol;
    pnp_aug_sample_w s;
    bool ok = false;
    float zlo = 0.f, zhi = 0.f;
    int row_i = -1, ci = 0, col = -1;                                         // the cached row (of sample `cur`) and cell column
    float bi[4] = {0.f, 0.f, 0.f, 0.f};
    float2 rc[4] = {};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < cnt) {
            if (b != cur) {
                cur = b;
                row_i = -1;
                s = samples[b];
                const bool vok = s.volume >= 0 && s.volume < nvol;
                if (vok) {
                    vol = vols[s.volume];
                } else {
                    vol.image = nullptr; vol.label = nullptr; vol.X = vol.Y = vol.Z = 0; vol.fill = 0.f;
                }
                ok = vok && s.frame >= 0 && s.frame <= vol.Z - 1 && s.dz >= 0.f && s.dz < INFINITY && (WARP || s.warp == 0);
                if (ok) {
                    const float top = (float)(vol.Z - 1);
                    zlo = fminf(fmaxf((float)s.frame - s.dz, 0.f), top);
                    zhi = fminf(fmaxf((float)s.frame + s.dz, 0.f), top);
                }
                if (!ok && i == 0 && j == 0) atomicAdd(errors, 1u);       // once per refused sample: by the lane that owns its first pixel
            }
            if (ok) {
                float sx = fmaf(s.m[0], (float)i, fmaf(s.m[1], (float)j, s.m[2]));
                float sy = fmaf(s.m[3], (float)i, fmaf(s.m[4], (float)j, s.m[5]));
                if constexpr (WARP) {
                    if (s.warp != 0) {
                        if (i != row_i) {
                            row_i = i;
                            col = -1;
                            const float gi = ((float)i + 0.5f) * rh;          // in [0, G] (+ rounding): the conversion is safe
                            ci = max(min((int)floorf(gi), G - 1), 0);
                            bspline_weights(gi - (float)ci, bi);
                        }
                        const float gj = ((float)j + 0.5f) * rw;
                        const int cj = max(min((int)floorf(gj), G - 1), 0);
                        if (cj != col) {
                            col = cj;
                            const float2* c0 = ctrl + ((long long)b * GP + ci) * GP + cj;       // rows ci .. ci + 3 <= G + 2, columns likewise
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const float2 a0 = c0[k], a1 = c0[GP + k], a2 = c0[2 * GP + k], a3 = c0[3 * GP + k];
                                rc[k].x = fmaf(bi[3], a3.x, fmaf(bi[2], a2.x, fmaf(bi[1], a1.x, bi[0] * a0.x)));
                                rc[k].y = fmaf(bi[3], a3.y, fmaf(bi[2], a2.y, fmaf(bi[1], a1.y, bi[0] * a0.y)));
                            }
                        }
                        float bj[4];
                        bspline_weights(gj - (float)cj, bj);
                        const float dx = fmaf(bj[3], rc[3].x, fmaf(bj[2], rc[2].x, fmaf(bj[1], rc[1].x, bj[0] * rc[0].x)));
                        const float dy = fmaf(bj[3], rc[3].y, fmaf(bj[2], rc[2].y, fmaf(bj[1], rc[1].y, bj[0] * rc[0].y)));
                        sx += dx;               // a non-finite or huge displacement fails sample_at's comparison, before any conversion
                        sy += dy;
                    }
                }
                Px r = sample_at<true>(vol, s.frame, zlo, zhi, sx, sy);
                if (!(s.gain == 1.f && s.bias == 0.f)) {                  // (the fmaf would turn a -0 into +0: the identity returns the value)
#pragma unroll
                    for (int c = 0; c < 3; ++c) r.c[c] = fmaf(s.gain, r.c[c], s.bias);
                }
                if (s.noise != 0.f) {
                    const uint32_t e = 3u * ((uint32_t)i * (uint32_t)W + (uint32_t)j);         // 6 H W < 2^32 (checked on the host)
#pragma unroll
                    for (int c = 0; c < 3; ++c) r.c[c] = fmaf(s.noise, normal_of(e + (uint32_t)c, s.seed), r.c[c]);
                }
                px[t] = r;
            } else {
                px[t].c[0] = px[t].c[1] = px[t].c[2] = vol.fill;
                px[t].lab = 0.f;
            }
            if (++j == W) {
                j = 0;
                if (++i == H) {
                    i = 0;
                    ++b;
                }
            }
        } else {
            px[t].c[0] = px[t].c[1] = px[t].c[2] = px[t].lab = 0.f;
        }
    }
    store_group(px, cnt, p0, x, label, onehot, ncls);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct PreLayout {
    size_t hist, state, psum, pdev, pmin, total;
};

PreLayout pre_layout() {
    PreLayout L;
    size_t o = 0;
    L.hist = o;  o += 4 * 256 * sizeof(unsigned int);
    L.state = o; o += 256;
    L.psum = o;  o += kMaxBlocks * sizeof(double);
    L.pdev = o;  o += kMaxBlocks * sizeof(double);
    L.pmin = o;  o += kMaxBlocks * sizeof(float);
    L.total = o;
    return L;
}

bool pre_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }

// the argument checks every gather entry point shares; `who` names the caller in the messages
int aug_slices_check(const char* who, int min_z, const pnp_aug_volume* vols_host, const void* vols_dev, int32_t nvol, const void* samples_dev,
                     int32_t B, int32_t H, int32_t W, float* x, float* label, float* onehot, int32_t ncls, uint32_t* errors) {
    PNP_REQUIRE(B >= 1, "%s: B = %d, at least one sample is needed", who, (int)B);
    PNP_REQUIRE(H >= 1 && W >= 1, "%s: output size %d x %d must be at least 1 x 1", who, (int)H, (int)W);
    PNP_REQUIRE(vols_host && vols_dev && samples_dev, "%s: null table", who);
    PNP_REQUIRE(nvol >= 1, "%s: nvol = %d, at least one volume is needed", who, (int)nvol);
    PNP_REQUIRE(x && label && errors, "%s: null output pointer", who);
    PNP_REQUIRE(!onehot || (ncls >= 1 && ncls <= kMaxCls), "%s: ncls %d outside [1, %d]", who, (int)ncls, kMaxCls);
    PNP_REQUIRE(((uintptr_t)x | (uintptr_t)label | (uintptr_t)onehot) % 16 == 0, "%s: outputs must be 16-byte aligned", who);
    const long long P = (long long)B * H * W;
    PNP_REQUIRE(P < ((long long)1 << 31), "%s: B * H * W = %lld is not below 2^31", who, P);
    for (int i = 0; i < nvol; ++i) {
        const pnp_aug_volume& v = vols_host[i];
        PNP_REQUIRE(v.image && v.label, "%s: volume %d: null pointer", who, i);
        PNP_REQUIRE(v.X >= 1 && v.Y >= 1 && v.X <= kMaxExtentXY && v.Y <= kMaxExtentXY,
                    "%s: volume %d: extents %d x %d outside [1, %d]", who, i, (int)v.X, (int)v.Y, kMaxExtentXY);
        PNP_REQUIRE(v.Z >= min_z, "%s: volume %d: Z = %d, at least %d frames are needed", who, i, (int)v.Z, min_z);
        PNP_REQUIRE((long long)v.X * v.Y * v.Z < ((long long)1 << 40), "%s: volume %d is too large", who, i);
    }
    return PNP_OK;
}

unsigned aug_slices_blocks(int32_t B, int32_t H, int32_t W) {
    const long long groups = ((long long)B * H * W + 3) / 4;
    return (unsigned)((groups + kThreads - 1) / kThreads);
}

// the checks and the launch of the two affine entry points.  FRAC needs Z >= 1, the other Z >= 3.
template <bool FRAC>
int aug_slices_launch(const char* who, const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol,
                      const std::conditional_t<FRAC, pnp_aug_sample_z, pnp_aug_sample>* samples_dev, int32_t B, int32_t H, int32_t W, float* x,
                      float* label, float* onehot, int32_t ncls, uint32_t* errors, void* stream) {
    const int rc = aug_slices_check(who, FRAC ? 1 : 3, vols_host, vols_dev, nvol, samples_dev, B, H, W, x, label, onehot, ncls, errors);
    if (rc != PNP_OK) return rc;
    hipLaunchKernelGGL(aug_slices_kernel<FRAC>, dim3(aug_slices_blocks(B, H, W)), dim3(kThreads), 0, (hipStream_t)stream, vols_dev, (int)nvol,
                       samples_dev, (int)H, (int)W, (long long)B * H * W, x, label, onehot, (int)(onehot ? ncls : 0), errors);
    PNP_CHECK_LAUNCH("aug_slices_kernel");
    return PNP_OK;
}

}  // namespace

extern "C" {

size_t pnp_volume_preprocess_workspace_bytes(int64_t n) {
    if (!pre_n_ok(n)) return 0;
    return pre_layout().total;
}

int pnp_volume_preprocess(const float* v, float* out, int64_t n, int32_t percentile, double* stats, void* workspace,
                          size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(n >= 1, "pnp_volume_preprocess: n = %lld, at least one voxel is needed", (long long)n);
    PNP_REQUIRE(pre_n_ok(n), "pnp_volume_preprocess: n = %lld is not below 2^31", (long long)n);
    PNP_REQUIRE(percentile >= 0 && percentile <= 100, "pnp_volume_preprocess: percentile %d outside [0, 100]", (int)percentile);
    PNP_REQUIRE(v && out && stats && workspace, "pnp_volume_preprocess: null pointer");
    const PreLayout L = pre_layout();
    PNP_REQUIRE(workspace_bytes >= L.total, "pnp_volume_preprocess: workspace too small: %zu bytes < %zu (pnp_volume_preprocess_workspace_bytes)",
                workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned int* hist = (unsigned int*)(ws + L.hist);
    SelState* state = (SelState*)(ws + L.state);
    double* psum = (double*)(ws + L.psum);
    double* pdev = (double*)(ws + L.pdev);
    float* pmin = (float*)(ws + L.pmin);
    const uint32_t k = (uint32_t)(((long long)percentile * (n - 1) + 99) / 100);        // <= n - 1 for every percentile in [0, 100]
    const unsigned nb = (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, kMaxBlocks);

    hipLaunchKernelGGL(pre_init_kernel, dim3(1), dim3(kThreads), 0, st, hist, state, k);
    PNP_CHECK_LAUNCH("pre_init_kernel");
    uint32_t mask = 0u;
    for (int r = 0; r < 4; ++r) {
        const int shift = 24 - 8 * r;
        hipLaunchKernelGGL(pre_hist_kernel, dim3(nb), dim3(kThreads), 0, st, v, (long long)n, shift, mask, state, hist + r * 256);
        PNP_CHECK_LAUNCH("pre_hist_kernel");
        hipLaunchKernelGGL(pre_pick_kernel, dim3(1), dim3(64), 0, st, hist + r * 256, shift, state);
        PNP_CHECK_LAUNCH("pre_pick_kernel");
        mask |= 255u << shift;
    }
    hipLaunchKernelGGL(pre_sum_kernel, dim3(nb), dim3(kThreads), 0, st, v, (long long)n, state, psum, pmin);
    PNP_CHECK_LAUNCH("pre_sum_kernel");
    hipLaunchKernelGGL(pre_dev_kernel, dim3(nb), dim3(kThreads), 0, st, v, (long long)n, state, psum, pdev);
    PNP_CHECK_LAUNCH("pre_dev_kernel");
    hipLaunchKernelGGL(pre_normalize_kernel, dim3(nb), dim3(kThreads), 0, st, v, out, (long long)n, state, psum, pdev, pmin, stats);
    PNP_CHECK_LAUNCH("pre_normalize_kernel");
    return PNP_OK;
}

int pnp_aug_slices(const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol, const pnp_aug_sample* samples_dev,
                   int32_t B, int32_t H, int32_t W, float* x, float* label, float* onehot, int32_t ncls, uint32_t* errors,
                   void* stream) {
    return aug_slices_launch<false>("pnp_aug_slices", vols_host, vols_dev, nvol, samples_dev, B, H, W, x, label, onehot, ncls, errors, stream);
}

int pnp_aug_slices_z(const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol, const pnp_aug_sample_z* samples_dev,
                     int32_t B, int32_t H, int32_t W, float* x, float* label, float* onehot, int32_t ncls, uint32_t* errors,
                     void* stream) {
    return aug_slices_launch<true>("pnp_aug_slices_z", vols_host, vols_dev, nvol, samples_dev, B, H, W, x, label, onehot, ncls, errors, stream);
}

int pnp_aug_slices_warp(const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol, const pnp_aug_sample_w* samples_dev,
                        const float* ctrl_dev, int32_t G, int32_t B, int32_t H, int32_t W, float* x, float* label, float* onehot, int32_t ncls,
                        uint32_t* errors, void* stream) {
    const char* who = "pnp_aug_slices_warp";
    const int rc = aug_slices_check(who, 1, vols_host, vols_dev, nvol, samples_dev, B, H, W, x, label, onehot, ncls, errors);
    if (rc != PNP_OK) return rc;
    PNP_REQUIRE(G >= 0 && G <= kMaxWarpGrid, "%s: G = %d outside [0, %d]", who, (int)G, kMaxWarpGrid);
    PNP_REQUIRE((G == 0) == (ctrl_dev == nullptr), "%s: the control table must be null exactly when G == 0 (G = %d)", who, (int)G);
    PNP_REQUIRE((uintptr_t)ctrl_dev % 8 == 0, "%s: the control table must be 8-byte aligned", who);
    PNP_REQUIRE(6ll * H * W < (1ll << 32), "%s: 6 * H * W = %lld is not below 2^32 (the noise counter)", who, 6ll * H * W);
    const dim3 grid(aug_slices_blocks(B, H, W)), block(kThreads);
    const long long P = (long long)B * H * W;
    if (G == 0)
        hipLaunchKernelGGL(aug_slices_warp_kernel<false>, grid, block, 0, (hipStream_t)stream, vols_dev, (int)nvol, samples_dev, (const float2*)nullptr,
                           0, (int)H, (int)W, P, x, label, onehot, (int)(onehot ? ncls : 0), errors);
    else
        hipLaunchKernelGGL(aug_slices_warp_kernel<true>, grid, block, 0, (hipStream_t)stream, vols_dev, (int)nvol, samples_dev,
                           (const float2*)ctrl_dev, (int)G, (int)H, (int)W, P, x, label, onehot, (int)(onehot ? ncls : 0), errors);
    PNP_CHECK_LAUNCH("aug_slices_warp_kernel");
    return PNP_OK;
}

}  // extern "C"
