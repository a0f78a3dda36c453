// elementwise.hip — the HBM-bound kernels of the hot path: batch-norm (+dropout-mask, +residual, +leaky-ReLU),
// 2x2 max-pool, phase-shift (PS) upsampling, critic-input assembly, dropout, axpby.
// Reference call sites: layers.py:95-100 (batch_norm), 145-189 (residual_block / DR_block tails),
// 102-103 (max_pool2d), ops.py:3-27 (PS), adversarial.py:325-335 (critic input), layers.py:25,74,93 (dropout).
// All tensors are [P][C] fp32 with C contiguous; every kernel moves 16 B per lane where C % 4 == 0.
#include "pnp_common.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
// four values rounded to bf16 (nearest-even), one 8-byte store: the bf16 copies the resident convolutions read (conv_bf16r.hip)
__device__ __forceinline__ void st4h(__bf16* p, f32x4 v) {
    bf16x4_t h;
    h[0] = (__bf16)v[0]; h[1] = (__bf16)v[1]; h[2] = (__bf16)v[2]; h[3] = (__bf16)v[3];
    *reinterpret_cast<bf16x4_t*>(p) = h;
}

// grid of the thread-owns-a-channel-quad kernels: x = row slabs (rpi rows per pass, <= cap workgroups over all channel slices), y = slices of 256 quads
inline dim3 grid_rows(long long P, int C4, int cap = 256 * 8) {
    const int ny = (C4 + NT - 1) / NT;
    const int c4s = C4 < NT ? C4 : NT;
    const int rpi = NT / c4s;
    long long bx = (P + rpi - 1) / rpi;
    const long long cx = cap / ny > 0 ? cap / ny : 1;
    if (bx > cx) bx = cx;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)ny);
}

inline int grid_for(size_t nvec, int cap = 256 * 8) {
    long long b = (long long)((nvec + NT - 1) / NT);
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// ------------------------------------------------------------------------------------------------
// Column reductions over [P][C]: each block reduces a slab of rows for every channel.
// partial layout: ws[(blk * 2 + q) * C + c], q in {0,1}
// KIND 0: BN statistics  q0 = sum(x - s), q1 = sum((x-s)^2) with shift s = x[0][c]
// KIND 1: BN backward    q0 = sum(dz),    q1 = sum(dz * xhat)
struct ColArgs {
    const float* x;      // KIND0: x ; KIND1: x (pre-BN input)
    const float* dout;   // KIND1
    const float* out;    // KIND1 (post activation), may be null when alpha<0
    const float* mean;   // KIND1
    const float* var;    // KIND1
    const float* gamma;  // KIND1, out == null: the activation's sign is recomputed from x (needs gamma, beta)
    const float* beta;
    float* ws;
    long long P;
    int C;
    int rows_per_block;
    float eps, alpha;
};

constexpr int COLRED_SLAB = 128;

// The arithmetic every BN kernel shares, written once: the vector kernels call it per lane of a channel quad, the scalar kernels per element,
// so "the same expressions in the same order" (tests/test_gpu_elementwise_domain.py holds the two forms to the same bits) is one text.
// The pre-activation value.  The fused multiply-add is explicit: the backward kernels recompute this value bit for bit when they are not
// handed `out`.
__device__ __forceinline__ float bn_pre(float x, float m, float gsc, float b) { return fmaf(x - m, gsc, b); }

// g through a leaky ReLU whose deciding value (the activation's output, or its input: they have the same sign) is o
__device__ __forceinline__ float leaky_gate(float g, float o, float alpha) { return o > 0.f ? g : g * alpha; }

// Per-channel coefficients of channels c .. c + 3 (quad) or of channel c alone, in lane 0 (!quad): 1 / sqrt(var + eps) — a square root and
// a correctly rounded division, formed once per thread where the thread owns its channels — gamma times it, and for the backward the two
// sums over the rows behind them.  bn_coef gives m and rs and leaves the rest zero: a kernel adds what it reads (bn_coef_scale, b = ldc(beta),
// bn_coef_sums) under its own conditions, since gamma, beta and the sums may each be absent.
struct BnCoef {
    f32x4 m, rs, gsc, b, dgp, dbp;       // mean, 1 / sqrt(var + eps), gamma * rs, beta, dgamma * invP, dbeta * invP
};
__device__ __forceinline__ f32x4 ldc(const float* p, int c, bool quad) { return quad ? ld4(p + c) : f32x4{p[c], 0.f, 0.f, 0.f}; }
__device__ __forceinline__ BnCoef bn_coef(const float* mean, const float* var, float eps, int c, bool quad) {
    BnCoef k{};
    k.m = ldc(mean, c, quad);
    const f32x4 v = ldc(var, c, quad);
#pragma unroll
    for (int e = 0; e < (quad ? 4 : 1); ++e) k.rs[e] = 1.0f / sqrtf(v[e] + eps);
    return k;
}
__device__ __forceinline__ void bn_coef_scale(BnCoef& k, const float* gamma, int c, bool quad) {
    const f32x4 ga = ldc(gamma, c, quad);
#pragma unroll
    for (int e = 0; e < (quad ? 4 : 1); ++e) k.gsc[e] = ga[e] * k.rs[e];
}
__device__ __forceinline__ void bn_coef_sums(BnCoef& k, const float* dgamma, const float* dbeta, float invP, int c, bool quad) {
    const f32x4 dg = ldc(dgamma, c, quad), db = ldc(dbeta, c, quad);
#pragma unroll
    for (int e = 0; e < (quad ? 4 : 1); ++e) {
        k.dgp[e] = dg[e] * invP;
        k.dbp[e] = db[e] * invP;
    }
}

// The gradient behind the fused activation (alpha < 0: none): its sign is read from `out` (o) where the caller has it, otherwise it is that
// of the pre-activation value exactly as bn_apply_kernel formed it, recomputed from x.
__device__ __forceinline__ float bn_gated(float g, bool has_out, float o, float x, const BnCoef& k, int e, float alpha) {
    if (alpha < 0.f) return g;
    return leaky_gate(g, has_out ? o : bn_pre(x, k.m[e], k.gsc[e], k.b[e]), alpha);
}

// the normalised input: what dgamma sums against the gated gradient, and what the training-mode dx subtracts
__device__ __forceinline__ float bn_xhat(float x, const BnCoef& k, int e) { return (x - k.m[e]) * k.rs[e]; }

template <int KIND>
__global__ void __launch_bounds__(NT) colreduce_kernel(ColArgs a) {
    __shared__ float red[NT * 8];
    const int C4 = a.C >> 2;
    const int rpi = NT / C4;                 // rows per iteration (C4 <= 256 guaranteed by the host)
    const int t = threadIdx.x;
    const int cg = t % C4, rsub = t / C4;
    const bool active = rsub < rpi;
    const long long r0 = (long long)blockIdx.x * a.rows_per_block;
    long long r1 = r0 + a.rows_per_block;
    if (r1 > a.P) r1 = a.P;
    f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    if (active) {
        const int c = cg * 4;
        BnCoef k{};
        if constexpr (KIND == 0) {
            k.m = ld4(a.x + c);   // shift
        } else {
            k = bn_coef(a.mean, a.var, a.eps, c, true);
            if (!a.out && a.alpha >= 0.f) {
                bn_coef_scale(k, a.gamma, c, true);
                k.b = ld4(a.beta + c);
            }
        }
        for (long long r = r0 + rsub; r < r1; r += rpi) {
            const size_t off = (size_t)r * a.C + c;
            f32x4 xv = ld4(a.x + off);
            if constexpr (KIND == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float d = xv[e] - k.m[e];
                    s0[e] += d;
                    s1[e] = fmaf(d, d, s1[e]);
                }
            } else {
                f32x4 g = ld4(a.dout + off), o = {0, 0, 0, 0};
                if (a.alpha >= 0.f && a.out) o = ld4(a.out + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    g[e] = bn_gated(g[e], a.out, o[e], xv[e], k, e, a.alpha);
                    s0[e] += g[e];
                    s1[e] = fmaf(g[e], bn_xhat(xv[e], k, e), s1[e]);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[t * 8 + e] = s0[e];
        red[t * 8 + 4 + e] = s1[e];
    }
    __syncthreads();
    if (t < C4) {
        f32x4 a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
        for (int j = 0; j < rpi; ++j) {
            const int tt = j * C4 + t;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[e] += red[tt * 8 + e];
                a1[e] += red[tt * 8 + 4 + e];
            }
        }
        float* w0 = a.ws + ((size_t)blockIdx.x * 2 + 0) * a.C + t * 4;
        float* w1 = a.ws + ((size_t)blockIdx.x * 2 + 1) * a.C + t * 4;
        st4(w0, a0);
        st4(w1, a1);
    }
}

// scalar fallback for C % 4 != 0 or C > 1024: one thread per channel per block-slab.  The thread walks ALL rows of its slab (P below 64 rows, 64 or more otherwise) in
// one chain, where a thread of colreduce_kernel walks rows_per_block / rpi of them: the chain is summed in double (a float32 chain of 63
// rows missed the statistics' 1e-6 / 1e-5 bars at C = 1028: tests/test_gpu_elementwise_domain.py), the partial is rounded to float once
template <int KIND>
__global__ void colreduce_scalar_kernel(ColArgs a) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    const long long r0 = (long long)blockIdx.x * a.rows_per_block;
    long long r1 = r0 + a.rows_per_block;
    if (r1 > a.P) r1 = a.P;
    double s0 = 0.0, s1 = 0.0;
    BnCoef k{};
    if constexpr (KIND == 0) {
        k.m[0] = a.x[c];
    } else {
        k = bn_coef(a.mean, a.var, a.eps, c, false);
        if (!a.out && a.alpha >= 0.f) {
            bn_coef_scale(k, a.gamma, c, false);
            k.b[0] = a.beta[c];
        }
    }
    for (long long r = r0; r < r1; ++r) {
        const size_t off = (size_t)r * a.C + c;
        float xv = a.x[off];
        if constexpr (KIND == 0) {
            const float d = xv - k.m[0];
            s0 += (double)d;
            s1 += (double)d * (double)d;
        } else {
            const float g = bn_gated(a.dout[off], a.out, (a.alpha >= 0.f && a.out) ? a.out[off] : 0.f, xv, k, 0, a.alpha);
            s0 += (double)g;
            s1 += (double)g * (double)bn_xhat(xv, k, 0);
        }
    }
    a.ws[((size_t)blockIdx.x * 2 + 0) * a.C + c] = (float)s0;
    a.ws[((size_t)blockIdx.x * 2 + 1) * a.C + c] = (float)s1;
}

// The sum of a list of partials by one workgroup of 1024 threads = 32 channels x 32 slices of the list: entries b0 .. b1 - 1 of channel c,
// slice sl taking every 32nd, in double; then the 32 slices in order.  Fixed summation order => deterministic.  slab > 0: the list was
// compacted; entry b is partial (b >> 1) * slab + (b & 1).  `mine` for the threads (slice 0 of a channel below C) that hold the sums.
struct SlabSum {
    double s0, s1;
    bool mine;
};
__device__ __forceinline__ SlabSum slab_sum(double (&red)[2][32][33], const float* ws, int b0, int b1, int slab, int C, int c) {
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    double s0 = 0.0, s1 = 0.0;
    if (c < C) {
        for (int b = b0 + sl; b < b1; b += 32) {
            const int row = slab > 0 ? (b >> 1) * slab + (b & 1) : b;
            s0 += (double)ws[((size_t)row * 2 + 0) * C + c];
            s1 += (double)ws[((size_t)row * 2 + 1) * C + c];
        }
    }
    red[0][sl][cl] = s0;
    red[1][sl][cl] = s1;
    __syncthreads();
    if (sl != 0 || c >= C) return {0.0, 0.0, false};
    s0 = 0.0;
    s1 = 0.0;
    for (int j = 0; j < 32; ++j) {
        s0 += red[0][j][cl];
        s1 += red[1][j][cl];
    }
    return {s0, s1, true};
}

// what the float hi = (float)s leaves of a double sum s, as a float: (hi, low) carry s to 48 bits.  An overflowed sum stays +-inf with a
// zero low part: inf - inf would turn it into NaN
__device__ __forceinline__ float low_part(double s, float hi) { return (fabsf(hi) <= 3.4e38f) ? (float)(s - (double)hi) : 0.f; }

// Long partial lists (the convolution epilogue leaves one partial per 64 output rows: 16 384 of them for a 64-channel layer at 256^2,
// which the C/32 = 2 workgroups of the final kernel walked alone: 240 us) are first compacted IN PLACE by (C/32) x nslab workgroups:
// slab s = partials [s*SLAB, (s+1)*SLAB) (the last slab takes the remainder) is summed in double and written back over its own first two
// partials as a (high, low) pair of floats, which together carry the double sum to 48 bits.  Only this workgroup ever reads those two
// rows of its 32 channels, so there is no race; the summation order is fixed => deterministic.  The partial list is consumed.
__global__ void __launch_bounds__(1024) colreduce_compact_kernel(float* __restrict__ ws, int nblk, int nslab, int C) {
    __shared__ double red[2][32][33];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const int s = blockIdx.y;
    const int b0 = s * COLRED_SLAB;
    const int b1 = (s == nslab - 1) ? nblk : b0 + COLRED_SLAB;
    const SlabSum t = slab_sum(red, ws, b0, b1, 0, C, c);
    if (!t.mine) return;
    const float h0 = (float)t.s0, h1 = (float)t.s1;
    ws[((size_t)b0 * 2 + 0) * C + c] = h0;
    ws[((size_t)b0 * 2 + 1) * C + c] = h1;
    ws[((size_t)(b0 + 1) * 2 + 0) * C + c] = low_part(t.s0, h0);
    ws[((size_t)(b0 + 1) * 2 + 1) * C + c] = low_part(t.s1, h1);
}

// tf.contrib.layers.batch_norm(updates_collections=None): the moving averages move with every training-mode forward (the variance that
// goes in is the unbiased one)
__device__ __forceinline__ float bn_bessel(long long P) { return P > 1 ? (float)((double)P / (double)(P - 1)) : 1.0f; }
__device__ __forceinline__ void bn_move(float* avg, float v, float one_minus_decay) { *avg -= (*avg - v) * one_minus_decay; }

// final combine over blocks in double. KIND 0 -> mean,var ; KIND 1 -> dbeta (o0), dgamma (o1)
template <int KIND>
__global__ void __launch_bounds__(1024) colreduce_final_kernel(const float* __restrict__ ws, const float* __restrict__ x0,
                                                               float* o0, float* o1, int nblk, int C, long long P, float* mm, float* mv,
                                                               float decay, int slab, float* acc0, float* acc1) {
    __shared__ double red[2][32][33];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const SlabSum t = slab_sum(red, ws, 0, nblk, slab, C, c);
    if (!t.mine) return;
    const double s0 = t.s0, s1 = t.s1;
    if constexpr (KIND == 0) {
        const double inv = 1.0 / (double)P;
        const double md = s0 * inv;                 // mean of (x - shift)
        double var = s1 * inv - md * md;
        if (var < 0.0) var = 0.0;
        const float meanf = (float)((double)x0[c] + md), varf = (float)var;
        o0[c] = meanf;
        o1[c] = varf;
        if (mm) {
            const float one_minus = 1.0f - decay, bessel = bn_bessel(P);
            bn_move(mm + c, meanf, one_minus);
            bn_move(mv + c, varf * bessel, one_minus);
        }
    } else {
        o0[c] = (float)s0;
        o1[c] = (float)s1;
        if (acc0) {         // the parameter gradients straight into the gradient arena (which may already hold another use's share)
            acc0[c] += (float)s0;
            acc1[c] += (float)s1;
        }
    }
}

// the final combine, in two launches when the list is long (>= 4 slabs)
template <int KIND>
int launch_colreduce_final(float* ws, const float* x0, float* o0, float* o1, int nblk, int C, long long P, float* mm, float* mv, float decay,
                           hipStream_t st, const char* who, float* acc0 = nullptr, float* acc1 = nullptr) {
    int slab = 0, n = nblk;
    if (nblk >= 4 * COLRED_SLAB) {
        const int nslab = nblk / COLRED_SLAB;
        hipLaunchKernelGGL(colreduce_compact_kernel, dim3(pnp_cdiv(C, 32), nslab), dim3(1024), 0, st, ws, nblk, nslab, C);
        PNP_CHECK_LAUNCH(who);
        slab = COLRED_SLAB;
        n = 2 * nslab;
    }
    hipLaunchKernelGGL(colreduce_final_kernel<KIND>, dim3(pnp_cdiv(C, 32)), dim3(1024), 0, st, (const float*)ws, x0, o0, o1, n, C, P, mm, mv,
                       decay, slab, acc0, acc1);
    PNP_CHECK_LAUNCH(who);
    return PNP_OK;
}

int colreduce_plan(long long P, int* nblk, int* rpb) {
    // ~2048 blocks max, at least 64 rows per block
    static const int cap = getenv("PNP_BN_NBLK") ? atoi(getenv("PNP_BN_NBLK")) : 2048;
    long long b = (P + 63) / 64;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    long long r = (P + b - 1) / b;
    b = (P + r - 1) / r;
    *nblk = (int)b;
    *rpb = (int)r;
    return 0;
}

// A column reduction is the reduction launch (one partial row per workgroup) and then the final combine of launch_colreduce_final: one
// launch, or two for a list of >= 4 slabs.  Combining inside the reduction launch (the last workgroup to take a ticket sums the list) was
// built, measured and removed: the device-scope release / acquire around every workgroup's ticket cost far more than the two ~8 us launches
// it saved (242.4 -> 208.3 slices/s: profiles/r05_bn_one_launch_ab.txt, tools/experiments/README.md row 5).
template <int KIND>
int run_colreduce(ColArgs a, float* o0, float* o1, void* ws, size_t ws_bytes, hipStream_t st, const char* who, float* mm = nullptr,
                  float* mv = nullptr, float decay = 0.f, float* acc0 = nullptr, float* acc1 = nullptr) {
    int nblk, rpb;
    colreduce_plan(a.P, &nblk, &rpb);
    const size_t need = (size_t)nblk * 2 * a.C * sizeof(float);
    if (ws_bytes < need || !ws) {
        pnp_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
        return PNP_EWORKSPACE;
    }
    a.ws = (float*)ws;
    a.rows_per_block = rpb;
    if ((a.C & 3) == 0 && a.C <= 1024) hipLaunchKernelGGL(colreduce_kernel<KIND>, dim3(nblk), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(colreduce_scalar_kernel<KIND>, dim3(nblk, pnp_cdiv(a.C, 64)), dim3(64), 0, st, a);
    PNP_CHECK_LAUNCH(who);
    return launch_colreduce_final<KIND>((float*)ws, a.x, o0, o1, nblk, a.C, a.P, mm, mv, decay, st, who, acc0, acc1);
}

__global__ void bn_update_moving_kernel(float* mm, float* mv, const float* mean, const float* var, long long P, int C,
                                        float decay) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float one_minus = 1.0f - decay, bessel = bn_bessel(P);
    bn_move(mm + c, mean[c], one_minus);
    bn_move(mv + c, var[c] * bessel, one_minus);
}

struct BnApplyArgs {
    const float *x, *mean, *var, *gamma, *beta, *shortcut;
    float* y;
    long long P;
    int C, Cs;
    float eps, alpha;
    __bf16* yh;      // bf16 copy of y (the next convolution's operand on the bf16-resident path); null: none
};

// VEC: a thread owns ONE channel quad and walks rows (block = rpi rows x C4s quads, blockIdx.y = slice of 256 quads): the per-channel
// coefficients — 1 / sqrt(var + eps) is a square root and a correctly rounded division — are formed once per thread, and no index needs a
// 64-bit division (round 6: the element-at-a-time form re-did both for every vector and ran VALU-bound at 1.8-2.4 TB/s on the critics'
// 537 MB maps).  Both forms run bn_apply_elem on every element and differ only in how they walk memory: bit-identical results.
// one element of the forward: BN, + the shortcut's element s where the channel has one, leaky ReLU (alpha < 0: none)
__device__ __forceinline__ float bn_apply_elem(float x, const BnCoef& k, int e, bool has_s, float s, float alpha) {
    float r = bn_pre(x, k.m[e], k.gsc[e], k.b[e]);
    if (has_s) r += s;
    if (alpha >= 0.f) r = leaky_gate(r, r, alpha);
    return r;
}

template <bool VEC>
__global__ void __launch_bounds__(NT) bn_apply_kernel(BnApplyArgs a) {
    const int cpad = (a.C - a.Cs) / 2;
    if constexpr (VEC) {
        const int C4 = a.C >> 2;
        const int kq0 = blockIdx.y * NT;
        const int C4s = (C4 - kq0) < NT ? (C4 - kq0) : NT;
        const int rpi = NT / C4s;
        const int cg = threadIdx.x % C4s, rsub = threadIdx.x / C4s;
        if (rsub >= rpi) return;
        const int c = (kq0 + cg) * 4;
        BnCoef k = bn_coef(a.mean, a.var, a.eps, c, true);
        bn_coef_scale(k, a.gamma, c, true);
        k.b = ld4(a.beta + c);
        const int cs = c - cpad;
        const bool has_s = a.shortcut && cs >= 0 && cs < a.Cs;
        // a workgroup streams ONE contiguous slab of rows (like colreduce_kernel, which reads the same tensors at 6 TB/s; strided passes of
        // 16 rows per workgroup ran at 2.7-3.6 TB/s on the 537 MB maps)
        const long long per = ((a.P + gridDim.x - 1) / gridDim.x + rpi - 1) / rpi * rpi;
        const long long rend = ((long long)blockIdx.x + 1) * per < a.P ? ((long long)blockIdx.x + 1) * per : a.P;
        for (long long row = (long long)blockIdx.x * per + rsub; row < rend; row += rpi) {
            const size_t i = (size_t)row * C4 + kq0 + cg;
            const f32x4 xv = ld4(a.x + i * 4);
            f32x4 r, sv = {0, 0, 0, 0};
            if (has_s) sv = ld4(a.shortcut + (size_t)row * a.Cs + cs);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = bn_apply_elem(xv[e], k, e, has_s, sv[e], a.alpha);
            st4(a.y + i * 4, r);
            if (a.yh) st4h(a.yh + i * 4, r);
        }
    } else {
        const int CV = a.C;
        const size_t nvec = (size_t)a.P * CV;
        const size_t gs = (size_t)gridDim.x * NT;
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += gs) {
            const size_t row = i / CV;
            const int c = (int)(i - row * CV);
            BnCoef k = bn_coef(a.mean, a.var, a.eps, c, false);
            bn_coef_scale(k, a.gamma, c, false);
            k.b[0] = a.beta[c];
            const int cs = c - cpad;
            const bool has_s = a.shortcut && cs >= 0 && cs < a.Cs;
            const float r = bn_apply_elem(a.x[i], k, 0, has_s, has_s ? a.shortcut[row * a.Cs + cs] : 0.f, a.alpha);
            a.y[i] = r;
            if (a.yh) a.yh[i] = (__bf16)r;
        }
    }
}

struct BnBwdArgs {
    const float *dout, *out, *x, *mean, *var, *gamma, *beta, *dgamma, *dbeta;      // out == null: sign recomputed from x (needs beta)
    float *dx, *dshortcut;
    long long P;
    long long P_norm;    // rows behind dgamma / dbeta: P, or the global row count when the sums were all-reduced (SyncBN)
    int C, Cs;
    float eps, alpha;
    int training;
    int do_drop;
    uint32_t drop_key, drop_thresh;
    float drop_keep;
    const pnp_step_params* sp;       // step capture: dropout seed from device memory (pnp_common.h)
    uint32_t drop_sid;
    __bf16* dxh;     // bf16 copy of dx (operand of the bf16-resident data / filter gradient kernels); null: none
};

// One element of dx from g, the gradient behind the activation (bn_gated: what the shortcut receives); idx is the element's flat index (the
// dropout mask's).
// Which products are fused into an FMA is written out and not left to the compiler: it once fused g - dbeta * invP in the scalar kernel,
// where the vector kernel held the rounded product in a register, and the two differed in the last bit of a training-mode dx
// (tests/test_gpu_elementwise_domain.py).
__device__ __forceinline__ float bn_bwd_elem(const BnBwdArgs& a, const BnCoef& k, int e, float x, float g, uint32_t idx, uint32_t dkey) {
#pragma clang fp contract(off)
    float r = a.training ? k.gsc[e] * fmaf(-bn_xhat(x, k, e), k.dgp[e], g - k.dbp[e]) : k.gsc[e] * g;
    if (a.do_drop) r = pnp_drop_keep(idx, dkey, a.drop_thresh) ? r / a.drop_keep : 0.f;
    return r;
}

// VEC: the thread-owns-a-channel-quad mapping of bn_apply_kernel.  This branch keeps its own staged text (gate, store, dx, dropout, each
// over the quad): the same expressions in the same order as bn_gated + bn_bwd_elem, which the scalar branch calls.  Built on the helpers it
// gave the same bits but lost packed multiplies and ran 44 -> 47-49 us per launch in the joint step (profiles/bn_once_ab.txt).
template <bool VEC>
__global__ void __launch_bounds__(NT) bn_bwd_apply_kernel(BnBwdArgs a) {
#pragma clang fp contract(off)
    const int cpad = (a.C - a.Cs) / 2;
    const float invP = (float)(1.0 / (double)a.P_norm);
    const uint32_t dkey = a.do_drop ? pnp_eff_drop_key(a.drop_key, a.sp, a.drop_sid) : 0u;
    const bool resign = a.alpha >= 0.f && !a.out;
    if constexpr (VEC) {
        const int C4 = a.C >> 2;
        const int kq0 = blockIdx.y * NT;
        const int C4s = (C4 - kq0) < NT ? (C4 - kq0) : NT;
        const int rpi = NT / C4s;
        const int cg = threadIdx.x % C4s, rsub = threadIdx.x / C4s;
        if (rsub >= rpi) return;
        const int c = (kq0 + cg) * 4;
        const f32x4 m = ld4(a.mean + c), v = ld4(a.var + c), ga = ld4(a.gamma + c);
        f32x4 rs, gsc, b = {0, 0, 0, 0}, dgp = {0, 0, 0, 0}, dbp = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            rs[e] = 1.0f / sqrtf(v[e] + a.eps);
            gsc[e] = ga[e] * rs[e];
        }
        if (a.alpha >= 0.f && !a.out) b = ld4(a.beta + c);
        if (a.training) {
            const f32x4 dg = ld4(a.dgamma + c), db = ld4(a.dbeta + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dgp[e] = dg[e] * invP;
                dbp[e] = db[e] * invP;
            }
        }
        const int cs = c - cpad;
        const bool has_s = a.dshortcut && cs >= 0 && cs < a.Cs;
        // a workgroup streams ONE contiguous slab of rows (like colreduce_kernel, which reads the same tensors at 6 TB/s; strided passes of
        // 16 rows per workgroup ran at 2.7-3.6 TB/s on the 537 MB maps)
        const long long per = ((a.P + gridDim.x - 1) / gridDim.x + rpi - 1) / rpi * rpi;
        const long long rend = ((long long)blockIdx.x + 1) * per < a.P ? ((long long)blockIdx.x + 1) * per : a.P;
        for (long long row = (long long)blockIdx.x * per + rsub; row < rend; row += rpi) {
            const size_t i = (size_t)row * C4 + kq0 + cg;
            f32x4 g = ld4(a.dout + i * 4);
            const f32x4 xv = ld4(a.x + i * 4);
            if (a.alpha >= 0.f) {
                if (a.out) {
                    const f32x4 o = ld4(a.out + i * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[e] = o[e] > 0.f ? g[e] : g[e] * a.alpha;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[e] = fmaf(xv[e] - m[e], gsc[e], b[e]) > 0.f ? g[e] : g[e] * a.alpha;
                }
            }
            if (has_s) st4(a.dshortcut + (size_t)row * a.Cs + cs, g);
            f32x4 r;
            if (a.training) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (xv[e] - m[e]) * rs[e];
                    r[e] = gsc[e] * fmaf(-xh, dgp[e], g[e] - dbp[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = gsc[e] * g[e];
            }
            if (a.do_drop) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    r[e] = pnp_drop_keep((uint32_t)(i * 4 + e), dkey, a.drop_thresh) ? r[e] / a.drop_keep : 0.f;
            }
            if (a.dx) st4(a.dx + i * 4, r);       // (null: only the bf16 copy is wanted — dx feeds nothing but resident convolutions)
            if (a.dxh) st4h(a.dxh + i * 4, r);
        }
    } else {
        const int CV = a.C;
        const size_t nvec = (size_t)a.P * CV;
        const size_t gs = (size_t)gridDim.x * NT;
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < nvec; i += gs) {
            const size_t row = i / CV;
            const int c = (int)(i - row * CV);
            BnCoef k = bn_coef(a.mean, a.var, a.eps, c, false);
            bn_coef_scale(k, a.gamma, c, false);
            if (resign) k.b[0] = a.beta[c];
            if (a.training) bn_coef_sums(k, a.dgamma, a.dbeta, invP, c, false);
            const float g = bn_gated(a.dout[i], a.out, (a.alpha >= 0.f && a.out) ? a.out[i] : 0.f, a.x[i], k, 0, a.alpha);
            const float r = bn_bwd_elem(a, k, 0, a.x[i], g, (uint32_t)i, dkey);
            if (a.dshortcut) {
                const int cs = c - cpad;
                if (cs >= 0 && cs < a.Cs) a.dshortcut[row * a.Cs + cs] = g;
            }
            if (a.dx) a.dx[i] = r;
            if (a.dxh) a.dxh[i] = (__bf16)r;
        }
    }
}

__global__ void __launch_bounds__(NT) dropout_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n,
                                                     uint32_t key, uint32_t thresh, float keep, __bf16* __restrict__ yh,
                                                     const pnp_step_params* sp, uint32_t sid) {
    key = pnp_eff_drop_key(key, sp, sid);
    const size_t gs = (size_t)gridDim.x * NT;
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += gs) {
        f32x4 v = ld4(x + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pnp_drop_keep((uint32_t)(i * 4 + e), key, thresh) ? v[e] / keep : 0.f;
        if (y) st4(y + i * 4, v);
        if (yh) st4h(yh + i * 4, v);
    }
    for (size_t i = (n4 << 2) + (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += gs) {
        const float v = pnp_drop_keep((uint32_t)i, key, thresh) ? x[i] / keep : 0.f;
        if (y) y[i] = v;
        if (yh) yh[i] = (__bf16)v;
    }
}

__global__ void __launch_bounds__(NT) axpby_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, float a,
                                                   float b) {
    const size_t gs = (size_t)gridDim.x * NT;
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += gs) {
        f32x4 xv = ld4(x + i * 4), yv = ld4(y + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[e] = a * xv[e] + b * yv[e];
        st4(y + i * 4, yv);
    }
    for (size_t i = (n4 << 2) + (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += gs) y[i] = a * x[i] + b * y[i];
}

// out = x + y: the sum TF's autodiff emits as AddN where a tensor feeds two branches (functional.FanOutFn)
__global__ void __launch_bounds__(NT) add_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, size_t n) {
    const size_t gs = (size_t)gridDim.x * NT;
    const size_t n4 = n >> 2;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += gs) {
        const f32x4 xv = ld4(x + i * 4), yv = ld4(y + i * 4);
        st4(out + i * 4, xv + yv);
    }
    for (size_t i = (n4 << 2) + (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += gs) out[i] = x[i] + y[i];
}

// ---- 2x2/2 max-pool -----------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(NT) maxpool2_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ out, int N, int H, int W, int C) {
    const int OH = H >> 1, OW = W >> 1;
    const int CV = ((C & 3) == 0) ? (C >> 2) : C;
    const bool vec = (C & 3) == 0;
    const size_t total = (size_t)N * OH * OW * CV;
    const size_t gs = (size_t)gridDim.x * NT;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += gs) {
        const int cv = (int)(i % CV);
        size_t q = i / CV;
        const int ow = (int)(q % OW);
        q /= OW;
        const int oh = (int)(q % OH);
        const int n = (int)(q / OH);
        const size_t base = (((size_t)n * H + 2 * oh) * W + 2 * ow) * C;
        const size_t o01 = (size_t)C, o10 = (size_t)W * C, o11 = (size_t)W * C + C;
        if (vec) {
            const int c = cv * 4;
            f32x4 v00 = ld4(x + base + c), v01 = ld4(x + base + o01 + c), v10 = ld4(x + base + o10 + c),
                  v11 = ld4(x + base + o11 + c);
            if constexpr (!BWD) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = fmaxf(fmaxf(v00[e], v01[e]), fmaxf(v10[e], v11[e]));
                st4(out + i * 4, r);
            } else {
                f32x4 g = ld4(dy + i * 4);
                f32x4 d00, d01, d10, d11;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // first maximal element in window scan order (row-major) gets the gradient
                    float m = v00[e];
                    int am = 0;
                    if (v01[e] > m) { m = v01[e]; am = 1; }
                    if (v10[e] > m) { m = v10[e]; am = 2; }
                    if (v11[e] > m) { m = v11[e]; am = 3; }
                    d00[e] = am == 0 ? g[e] : 0.f;
                    d01[e] = am == 1 ? g[e] : 0.f;
                    d10[e] = am == 2 ? g[e] : 0.f;
                    d11[e] = am == 3 ? g[e] : 0.f;
                }
                st4(out + base + c, d00);
                st4(out + base + o01 + c, d01);
                st4(out + base + o10 + c, d10);
                st4(out + base + o11 + c, d11);
            }
        } else {
            const int c = cv;
            float v00 = x[base + c], v01 = x[base + o01 + c], v10 = x[base + o10 + c], v11 = x[base + o11 + c];
            if constexpr (!BWD) {
                out[i] = fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
            } else {
                float g = dy[i];
                float m = v00;
                int am = 0;
                if (v01 > m) { m = v01; am = 1; }
                if (v10 > m) { m = v10; am = 2; }
                if (v11 > m) { m = v11; am = 3; }
                out[base + c] = am == 0 ? g : 0.f;
                out[base + o01 + c] = am == 1 ? g : 0.f;
                out[base + o10 + c] = am == 2 ? g : 0.f;
                out[base + o11 + c] = am == 3 ? g : 0.f;
            }
        }
    }
}

// ---- PS (phase shift): out[n, i*r+u, j*r+v, c] = x[n,i,j, c*r*r + v*r + u] ----------------------
// One thread per OUTPUT element (fwd) / per INPUT-GRAD element (bwd); the thread index runs over the
// output layout so stores are coalesced; loads hit the same 10 KB input pixel row (L1/L2 resident).
template <bool BWD>
__global__ void __launch_bounds__(NT) ps_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int A, int B,
                                                int r, int nc) {
    const int Cin = nc * r * r;
    const size_t total = (size_t)N * A * B * Cin;
    const size_t gs = (size_t)gridDim.x * NT;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += gs) {
        if constexpr (!BWD) {
            // decode i in the fine (output) layout [N][A*r][B*r][nc]
            const int c = (int)(i % nc);
            size_t q = i / nc;
            const int wo = (int)(q % (B * r));
            q /= (B * r);
            const int ho = (int)(q % (A * r));
            const int n = (int)(q / (A * r));
            const int ii = ho / r, u = ho - ii * r;
            const int jj = wo / r, v = wo - jj * r;
            const size_t coarse = (((size_t)n * A + ii) * B + jj) * Cin + (size_t)c * r * r + v * r + u;
            dst[i] = src[coarse];
        } else {
            // decode i in the coarse (input-gradient) layout [N][A][B][nc*r*r]: coalesced stores, gathered loads
            const int cc = (int)(i % Cin);
            size_t q = i / Cin;
            const int jj = (int)(q % B);
            q /= B;
            const int ii = (int)(q % A);
            const int n = (int)(q / A);
            const int c = cc / (r * r);
            const int vu = cc - c * r * r;
            const int v = vu / r, u = vu - v * r;
            const size_t fine = (((size_t)n * A * r + ii * r + u) * (B * r) + jj * r + v) * nc + c;
            dst[i] = src[fine];
        }
    }
}

// LDS-transposing version: the permutation is contiguous in the COARSE layout per pixel (all nc*r*r channels) and in the FINE layout per
// (pixel row u: r*nc floats, and consecutive coarse pixels jj continue the same fine row), but a thread-per-element copy is 4-byte
// scattered on one side (173 / 262 us for the 168 MB of g10's output at B=16, 2-4x the HBM time).  A workgroup takes T coarse pixels of
// one row (T*Cin <= 4096 floats), moves them through LDS and is coalesced on both sides.  LDS slot of coarse element x: x + x/64 — the
// fine order walks channels first (stride r*r = 64 floats in x), 65 makes that walk conflict-free.
template <bool BWD>
__global__ void __launch_bounds__(NT) ps_tile_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int A, int B, int r,
                                                     int nc, int T) {
    __shared__ float tile[4096 + 64];
    const int t = threadIdx.x;
    const int rr = r * r, Cin = nc * rr, X = T * Cin, rn = r * nc, run = T * rn;
    const int bpr = B / T;
    int b = blockIdx.x;
    const int jb = b % bpr;
    b /= bpr;
    const int ii = b % A, n = b / A;
    const int jj0 = jb * T;
    const size_t base_c = (((size_t)n * A + ii) * B + jj0) * Cin;
    const size_t fine0 = (((size_t)n * A * r + (size_t)ii * r) * (size_t)(B * r) + (size_t)jj0 * r) * nc;
    const size_t row_stride = (size_t)(B * r) * nc;
    const float inv_run = 1.0f / (float)run, inv_rn = 1.0f / (float)rn, inv_nc = 1.0f / (float)nc;
    // exact for these small integers: (f + 0.5) / d is at least 0.5/d away from an integer
    auto fdiv = [](int f, float inv) { return (int)(((float)f + 0.5f) * inv); };
    auto decode = [&](int f, int& u, int& rem) {      // fine-order index -> coarse-order index x
        u = fdiv(f, inv_run);
        rem = f - u * run;
        const int tj = fdiv(rem, inv_rn);
        const int q = rem - tj * rn;
        const int v = fdiv(q, inv_nc);
        const int c = q - v * nc;
        return tj * Cin + c * rr + v * r + u;
    };
    if constexpr (!BWD) {
        for (int x = t; x < X; x += NT) tile[x + (x >> 6)] = src[base_c + x];
        __syncthreads();
        for (int f = t; f < X; f += NT) {
            int u, rem;
            const int x = decode(f, u, rem);
            dst[fine0 + (size_t)u * row_stride + rem] = tile[x + (x >> 6)];
        }
    } else {
        for (int f = t; f < X; f += NT) {
            int u, rem;
            const int x = decode(f, u, rem);
            tile[x + (x >> 6)] = src[fine0 + (size_t)u * row_stride + rem];
        }
        __syncthreads();
        for (int x = t; x < X; x += NT) dst[base_c + x] = tile[x + (x >> 6)];
    }
}

// coarse pixels per workgroup of ps_tile_kernel: the largest divisor of B with T*Cin <= 4096 (0: use the per-element kernel)
inline int ps_tile_T(int B, int Cin) {
    static const int off = getenv("PNP_PS_NOTILE") ? 1 : 0;
    if (off || Cin > 4096) return 0;
    int T = 4096 / Cin;
    if (T > B) T = B;
    while (T > 1 && (B % T) != 0) --T;
    return T;
}

// ---- critic input assembly (adversarial.py:325-335) ---------------------------------------------
struct CriticArgs {
    const float *a, *b, *c, *d, *logits;
    float* out;
    long long P;
    int Ca, tile_a, Cb, Cc, Cd, ncls, Ctot;
};
__device__ __forceinline__ float critic_channel(const CriticArgs& k, size_t p, int ch, int o1, int o2, int o3, int o4, int o5) {
    if (ch < o1) return k.a[p * k.Ca + (ch % k.Ca)];
    if (ch < o2) return k.b[p * k.Cb + (ch - o1)];
    if (ch < o3) return k.c[p * k.Cc + (ch - o2)];
    if (ch < o4) return k.d[p * k.Cd + (ch - o3)];
    if (ch < o5) return k.logits[p * k.ncls + (ch - o4)];
    const float* z = k.logits + p * k.ncls;
    int am = 0;
    float m = z[0];
    for (int j = 1; j < k.ncls; ++j)
        if (z[j] > m) { m = z[j]; am = j; }
    return (float)am;
}
// VEC: one 16-byte store per thread (Ctot % 4 == 0: the reference's 32 channels), i.e. 8 lanes cover one pixel's 128 contiguous bytes
template <bool VEC>
__global__ void __launch_bounds__(NT) critic_input_fwd_kernel(CriticArgs k) {
    const int CV = VEC ? (k.Ctot >> 2) : k.Ctot;
    const size_t total = (size_t)k.P * CV;
    const size_t gs = (size_t)gridDim.x * NT;
    const int o1 = k.Ca * k.tile_a, o2 = o1 + k.Cb, o3 = o2 + k.Cc, o4 = o3 + k.Cd, o5 = o4 + k.ncls;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += gs) {
        const size_t p = i / CV;
        const int cv = (int)(i - p * CV);
        if constexpr (VEC) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = critic_channel(k, p, 4 * cv + e, o1, o2, o3, o4, o5);
            st4(k.out + i * 4, v);
        } else {
            k.out[i] = critic_channel(k, p, cv, o1, o2, o3, o4, o5);
        }
    }
}
struct CriticBwdArgs {
    const float* dout;
    float *da, *db, *dc, *dd, *dlogits;
    long long P;
    int Ca, tile_a, Cb, Cc, Cd, ncls, Ctot;
};
// one thread per (pixel, source channel) over the concatenated *source* channel space Ca+Cb+Cc+Cd+ncls
__global__ void __launch_bounds__(NT) critic_input_bwd_kernel(CriticBwdArgs k) {
    const int Csrc = k.Ca + k.Cb + k.Cc + k.Cd + k.ncls;
    const size_t total = (size_t)k.P * Csrc;
    const size_t gs = (size_t)gridDim.x * NT;
    const int o1 = k.Ca * k.tile_a, o2 = o1 + k.Cb, o3 = o2 + k.Cc, o4 = o3 + k.Cd;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += gs) {
        const size_t p = i / Csrc;
        int ch = (int)(i - p * Csrc);
        const float* g = k.dout + p * k.Ctot;
        if (ch < k.Ca) {
            float s = 0.f;
            for (int t = 0; t < k.tile_a; ++t) s += g[t * k.Ca + ch];
            if (k.da) k.da[p * k.Ca + ch] = s;
            continue;
        }
        ch -= k.Ca;
        if (ch < k.Cb) { if (k.db) k.db[p * k.Cb + ch] = g[o1 + ch]; continue; }
        ch -= k.Cb;
        if (ch < k.Cc) { if (k.dc) k.dc[p * k.Cc + ch] = g[o2 + ch]; continue; }
        ch -= k.Cc;
        if (ch < k.Cd) { if (k.dd) k.dd[p * k.Cd + ch] = g[o3 + ch]; continue; }
        ch -= k.Cd;
        if (k.dlogits) k.dlogits[p * k.ncls + ch] = g[o4 + ch];   // argmax channel has zero gradient
    }
}

// ---- PS fused into its consumers ----------------------------------------------------------------
// The two places where the model leaves the 32 x 32 grid through PS(r = 8) — the segmenter head (PS, mirror pad, 5x5 logits convolution)
// and the feature critic's input (four PS, then critic_input) — wrote the fine tensors only for the next kernel to read them again.  These
// kernels keep ps_tile_kernel's shape (a workgroup owns T coarse pixels jj0 .. jj0+T-1 of coarse row ii, moves them through LDS at slot
// x + x/64 and is coalesced on both sides) and do the consumer's work on the way.  They move values and, where they sum, keep the order of
// the kernel they replace: every result is bit-identical to the unfused sequence.

// f / d for the small non-negative integers of a tile (f < 2^14, quotient x divisor far below 2^21): (f + 0.5) / d is at least 0.5 / d
// away from an integer, the float product is not
__device__ __forceinline__ int tdiv(int f, float inv) { return (int)(((float)f + 0.5f) * inv); }
__device__ __forceinline__ int mirror(int h, int H) { return h < 0 ? -1 - h : (h >= H ? 2 * H - 1 - h : h); }

struct PsTile {
    int n, ii, jb, bpr;
};
__device__ __forceinline__ PsTile ps_tile_of(int b, int A, int B, int T) {
    PsTile q;
    q.bpr = B / T;
    q.jb = b % q.bpr;
    b /= q.bpr;
    q.ii = b % A;
    q.n = b / A;
    return q;
}
// cnt contiguous floats (a multiple of 4 when VEC) from src into the LDS image at coarse index x0 ..
template <bool VEC>
__device__ __forceinline__ void ps_stage_in(float* tile, int x0, const float* __restrict__ src, int cnt) {
    if constexpr (VEC) {
        for (int i = threadIdx.x; i < (cnt >> 2); i += NT) {
            const f32x4 v = ld4(src + 4 * i);
            const int x = x0 + 4 * i;
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[x + e + ((x + e) >> 6)] = v[e];
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += NT) tile[x0 + i + ((x0 + i) >> 6)] = src[i];
    }
}

// PS + mirror pad: the workgroup writes the part of the padded image whose source pixels it holds — its r x T*r fine pixels, plus the
// border rows / columns that mirror onto them when it sits at an edge (p <= r: only the first and last tile of a row or column do).
// VW = 4: one 16-byte store per thread (nc % 4 == 0)
template <int VW>
__global__ void __launch_bounds__(NT) ps_pad_fwd_kernel(const float* __restrict__ src, float* __restrict__ dst, int A, int B, int r, int nc,
                                                        int p, int T) {
    __shared__ float tile[4096 + 64];
    const PsTile q = ps_tile_of(blockIdx.x, A, B, T);
    const int rr = r * r, Cin = nc * rr;
    const int H = A * r, W = B * r, Wp = W + 2 * p;
    const int h0 = q.ii * r, w0 = q.jb * T * r;
    const float* in = src + (((size_t)q.n * A + q.ii) * B + (size_t)q.jb * T) * Cin;
    if ((Cin & 3) == 0) ps_stage_in<true>(tile, 0, in, T * Cin);
    else ps_stage_in<false>(tile, 0, in, T * Cin);
    __syncthreads();
    // the region in padded coordinates: rows [rlo, rhi), columns [clo, chi)
    const int rlo = h0 + (q.ii == 0 ? 0 : p), rhi = h0 + r + p + (q.ii == A - 1 ? p : 0);
    const int clo = w0 + (q.jb == 0 ? 0 : p), chi = w0 + T * r + p + (q.jb == q.bpr - 1 ? p : 0);
    const int ncv = nc / VW, rowv = (chi - clo) * ncv, total = (rhi - rlo) * rowv;
    const float inv_rowv = 1.0f / (float)rowv, inv_ncv = 1.0f / (float)ncv, inv_r = 1.0f / (float)r;
    float* out = dst + ((size_t)q.n * (H + 2 * p) * Wp) * nc;
    for (int f = threadIdx.x; f < total; f += NT) {
        const int ro = tdiv(f, inv_rowv), rem = f - ro * rowv;
        const int co = tdiv(rem, inv_ncv), cv = rem - co * ncv;
        const int u = mirror(rlo + ro - p, H) - h0, lc = mirror(clo + co - p, W) - w0;
        const int tj = tdiv(lc, inv_r), v = lc - tj * r;
        const int x = tj * Cin + cv * VW * rr + v * r + u;
        float* o = out + ((size_t)(rlo + ro) * Wp + (clo + co)) * nc + cv * VW;
        if constexpr (VW == 4) {
            f32x4 val;
#pragma unroll
            for (int e = 0; e < 4; ++e) val[e] = tile[x + e * rr + ((x + e * rr) >> 6)];
            st4(o, val);
        } else {
            *o = tile[x + (x >> 6)];
        }
    }
}

// backward: every fine pixel of the tile sums the padded positions that mirror onto it in sympad_bwd_kernel's order (rows h+p, the top
// mirror, the bottom mirror; inside each, the columns likewise) and lands in the coarse layout through LDS
template <int VW>
__global__ void __launch_bounds__(NT) ps_pad_bwd_kernel(const float* __restrict__ dxp, float* __restrict__ dx, int A, int B, int r, int nc,
                                                        int p, int T) {
    __shared__ float tile[4096 + 64];
    const PsTile q = ps_tile_of(blockIdx.x, A, B, T);
    const int rr = r * r, Cin = nc * rr;
    const int H = A * r, W = B * r, Wp = W + 2 * p;
    const int h0 = q.ii * r, w0 = q.jb * T * r;
    const int ncv = nc / VW, rowv = T * r * ncv, total = r * rowv;
    const float inv_rowv = 1.0f / (float)rowv, inv_ncv = 1.0f / (float)ncv, inv_r = 1.0f / (float)r;
    const float* in = dxp + ((size_t)q.n * (H + 2 * p) * Wp) * nc;
    for (int f = threadIdx.x; f < total; f += NT) {
        const int u = tdiv(f, inv_rowv), rem = f - u * rowv;
        const int lc = tdiv(rem, inv_ncv), cv = rem - lc * ncv;
        const int h = h0 + u, w = w0 + lc;
        float s[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e] = 0.f;
        for (int i = 0; i < 3; ++i) {
            if ((i == 1 && h >= p) || (i == 2 && h < H - p)) continue;
            const int hs = i == 0 ? h + p : (i == 1 ? p - 1 - h : 2 * H - 1 - h + p);
            for (int j = 0; j < 3; ++j) {
                if ((j == 1 && w >= p) || (j == 2 && w < W - p)) continue;
                const int ws = j == 0 ? w + p : (j == 1 ? p - 1 - w : 2 * W - 1 - w + p);
                const float* g = in + ((size_t)hs * Wp + ws) * nc + cv * VW;
                if constexpr (VW == 4) {
                    const f32x4 gv = ld4(g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += gv[e];
                } else {
                    s[0] += *g;
                }
            }
        }
        const int tj = tdiv(lc, inv_r), v = lc - tj * r;
        const int x = tj * Cin + cv * VW * rr + v * r + u;
#pragma unroll
        for (int e = 0; e < VW; ++e) tile[x + e * rr + ((x + e * rr) >> 6)] = s[e];
    }
    __syncthreads();
    float* out = dx + (((size_t)q.n * A + q.ii) * B + (size_t)q.jb * T) * Cin;
    for (int x = threadIdx.x; x < T * Cin; x += NT) out[x] = tile[x + (x >> 6)];
}

// largest divisor T of B with T <= cap (cap >= 1)
inline int ps_fused_T(int B, int cap) {
    int T = cap < B ? cap : B;
    while (T > 1 && (B % T) != 0) --T;
    return T;
}

// critic input from the coarse tensors.  C[s]: channels of source s AFTER PS; the LDS image holds, per coarse pixel, the sources' coarse
// channels back to back (Cs = sum C[s] fine channels, Cs * r * r floats: 1408 at the model's sizes)
struct CriticPsArgs {
    const float* src[4];
    const float* logits;
    float* out;
    int A, B, r, T, C[4], tile_a, ncls, Ctot;
};
constexpr int CRITIC_PS_RAW = 6144;     // floats of the backward's LDS image of dout
// VEC: one 16-byte store per thread (Ctot % 4 == 0: the reference's 32 channels), a fine row of the tile = T * r * Ctot contiguous floats.
// The argmax is taken by the one thread of a pixel that stores the last channel
template <bool VEC>
__global__ void __launch_bounds__(NT) critic_ps_fwd_kernel(CriticPsArgs k) {
    __shared__ float tile[4096 + 64];
    const PsTile q = ps_tile_of(blockIdx.x, k.A, k.B, k.T);
    const int r = k.r, rr = r * r, T = k.T;
    const int Cs = k.C[0] + k.C[1] + k.C[2] + k.C[3], Xp = Cs * rr;
    const size_t cpix = ((size_t)q.n * k.A + q.ii) * k.B + (size_t)q.jb * T;
    int off = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int cnt = k.C[s] * rr;
        for (int tj = 0; tj < T; ++tj) {
            const float* in = k.src[s] + (cpix + tj) * cnt;
            if ((rr & 3) == 0) ps_stage_in<true>(tile, tj * Xp + off * rr, in, cnt);
            else ps_stage_in<false>(tile, tj * Xp + off * rr, in, cnt);
        }
        off += k.C[s];
    }
    __syncthreads();
    const int o1 = k.C[0] * k.tile_a, o2 = o1 + k.C[1], o3 = o2 + k.C[2], o4 = o3 + k.C[3], o5 = o4 + k.ncls;
    const int CV = VEC ? (k.Ctot >> 2) : k.Ctot, rowv = T * r * CV, total = r * rowv;
    const float inv_rowv = 1.0f / (float)rowv, inv_cv = 1.0f / (float)CV, inv_r = 1.0f / (float)r;
    const size_t Wf = (size_t)k.B * r;
    auto channel = [&](int ch, int xpix, size_t pix) -> float {
        int sc;
        if (ch < o1) sc = ch % k.C[0];
        else if (ch < o2) sc = k.C[0] + (ch - o1);
        else if (ch < o3) sc = k.C[0] + k.C[1] + (ch - o2);
        else if (ch < o4) sc = k.C[0] + k.C[1] + k.C[2] + (ch - o3);
        else {
            const float* z = k.logits + pix * k.ncls;
            if (ch < o5) return z[ch - o4];
            int am = 0;
            float m = z[0];
            for (int j = 1; j < k.ncls; ++j)
                if (z[j] > m) { m = z[j]; am = j; }
            return (float)am;
        }
        const int x = xpix + sc * rr;
        return tile[x + (x >> 6)];
    };
    for (int f = threadIdx.x; f < total; f += NT) {
        const int u = tdiv(f, inv_rowv), rem = f - u * rowv;
        const int lc = tdiv(rem, inv_cv), cv = rem - lc * CV;
        const int tj = tdiv(lc, inv_r), v = lc - tj * r;
        const size_t pix = ((size_t)q.n * k.A * r + (size_t)q.ii * r + u) * Wf + (size_t)q.jb * T * r + lc;
        const int xpix = tj * Xp + v * r + u;
        if constexpr (VEC) {
            f32x4 val;
#pragma unroll
            for (int e = 0; e < 4; ++e) val[e] = channel(4 * cv + e, xpix, pix);
            st4(k.out + pix * k.Ctot + 4 * cv, val);
        } else {
            k.out[pix * k.Ctot + cv] = channel(cv, xpix, pix);
        }
    }
}

struct CriticPsBwdArgs {
    const float* dout;
    float* dsrc[4];
    float* dlogits;
    int A, B, r, T, C[4], tile_a, ncls, Ctot, any_src;
};
// backward: the tile's r fine rows of dout (T * r * Ctot contiguous floats each) go to LDS as they are — pixel stride Ctot + 8, row stride
// + 1, so that the 64 pixels of a coarse pixel fall on different banks — and are read back in the coarse order of every wanted source;
// the tile_a copies of `a` are summed t = 0, 1, 2 as in critic_input_bwd_kernel.  dlogits is a plain strided copy
template <bool VEC>
__global__ void __launch_bounds__(NT) critic_ps_bwd_kernel(CriticPsBwdArgs k) {
    __shared__ float raw[CRITIC_PS_RAW];
    const PsTile q = ps_tile_of(blockIdx.x, k.A, k.B, k.T);
    const int r = k.r, rr = r * r, T = k.T, Ctot = k.Ctot;
    const int Ps = Ctot + 8, Rs = T * r * Ps + 1;
    const size_t Wf = (size_t)k.B * r;
    const size_t pix0 = ((size_t)q.n * k.A * r + (size_t)q.ii * r) * Wf + (size_t)q.jb * T * r;    // + u * Wf + lc
    const int o1 = k.C[0] * k.tile_a, o2 = o1 + k.C[1], o3 = o2 + k.C[2], o4 = o3 + k.C[3];
    const float inv_r = 1.0f / (float)r;
    if (k.dlogits) {
        const int rown = T * r * k.ncls, total = r * rown;
        const float inv_rown = 1.0f / (float)rown, inv_ncls = 1.0f / (float)k.ncls;
        for (int f = threadIdx.x; f < total; f += NT) {
            const int u = tdiv(f, inv_rown), rem = f - u * rown;
            const int lc = tdiv(rem, inv_ncls), j = rem - lc * k.ncls;
            const size_t pix = pix0 + (size_t)u * Wf + lc;
            k.dlogits[pix * k.ncls + j] = k.dout[pix * Ctot + o4 + j];
        }
    }
    if (!k.any_src) return;
    {
        const int CV = VEC ? (Ctot >> 2) : Ctot, rowv = T * r * CV, total = r * rowv;
        const float inv_rowv = 1.0f / (float)rowv, inv_cv = 1.0f / (float)CV;
        for (int f = threadIdx.x; f < total; f += NT) {
            const int u = tdiv(f, inv_rowv), rem = f - u * rowv;
            const int lc = tdiv(rem, inv_cv), cv = rem - lc * CV;
            const float* g = k.dout + (pix0 + (size_t)u * Wf + lc) * Ctot;
            float* dst = raw + u * Rs + lc * Ps;
            if constexpr (VEC) {
                const f32x4 gv = ld4(g + 4 * cv);
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[4 * cv + e] = gv[e];
            } else {
                dst[cv] = g[cv];
            }
        }
    }
    __syncthreads();
    const int Cs = k.C[0] + k.C[1] + k.C[2] + k.C[3], Xp = Cs * rr;
    const float inv_xp = 1.0f / (float)Xp, inv_rr = 1.0f / (float)rr;
    const size_t cpix = ((size_t)q.n * k.A + q.ii) * k.B + (size_t)q.jb * T;
    for (int x = threadIdx.x; x < T * Xp; x += NT) {
        const int tj = tdiv(x, inv_xp), y = x - tj * Xp;
        int sc = tdiv(y, inv_rr);
        const int vu = y - sc * rr;
        const int v = tdiv(vu, inv_r), u = vu - v * r;
        const float* g = raw + u * Rs + (tj * r + v) * Ps;
        int s = 0, o = 0;       // source, its first channel in dout
        if (sc >= k.C[0]) { sc -= k.C[0]; s = 1; o = o1; }
        if (s == 1 && sc >= k.C[1]) { sc -= k.C[1]; s = 2; o = o2; }
        if (s == 2 && sc >= k.C[2]) { sc -= k.C[2]; s = 3; o = o3; }
        float* d = s == 0 ? k.dsrc[0] : (s == 1 ? k.dsrc[1] : (s == 2 ? k.dsrc[2] : k.dsrc[3]));
        if (!d) continue;
        const int Cn = s == 0 ? k.C[0] : (s == 1 ? k.C[1] : (s == 2 ? k.C[2] : k.C[3]));
        float val;
        if (s == 0) {
            val = 0.f;
            for (int t = 0; t < k.tile_a; ++t) val += g[t * Cn + sc];
        } else {
            val = g[o + sc];
        }
        d[((cpix + tj) * Cn + sc) * rr + vu] = val;
    }
}

}  // namespace

extern "C" {

size_t pnp_bn_workspace_bytes(int64_t P, int32_t C) {
    int nblk, rpb;
    colreduce_plan(P, &nblk, &rpb);
    return (size_t)nblk * 2 * C * sizeof(float);
}

int pnp_bn_stats(const float* x, float* mean, float* var, int64_t P, int32_t C, void* workspace, size_t workspace_bytes,
                 void* stream) {
    PNP_REQUIRE(x && mean && var && P > 0 && C > 0, "pnp_bn_stats: bad argument");
    ColArgs a{};
    a.x = x; a.P = P; a.C = C;
    return run_colreduce<0>(a, mean, var, workspace, workspace_bytes, (hipStream_t)stream, "pnp_bn_stats");
}

int pnp_bn_stats_update(const float* x, float* mean, float* var, float* moving_mean, float* moving_var, int64_t P, int32_t C, float decay,
                        void* workspace, size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(x && mean && var && moving_mean && moving_var && P > 0 && C > 0, "pnp_bn_stats_update: bad argument");
    ColArgs a{};
    a.x = x; a.P = P; a.C = C;
    return run_colreduce<0>(a, mean, var, workspace, workspace_bytes, (hipStream_t)stream, "pnp_bn_stats_update", moving_mean, moving_var, decay);
}

int pnp_bn_stats_finish(float* parts, int32_t nparts, const float* shift, float* mean, float* var, float* moving_mean,
                        float* moving_var, int64_t P, int32_t C, float decay, void* stream) {
    PNP_REQUIRE(parts && shift && mean && var && nparts > 0 && P > 0 && C > 0, "pnp_bn_stats_finish: bad argument");
    PNP_REQUIRE((moving_mean != nullptr) == (moving_var != nullptr), "pnp_bn_stats_finish: moving_mean and moving_var go together");
    return launch_colreduce_final<0>(parts, shift, mean, var, nparts, C, (long long)P, moving_mean, moving_var, decay, (hipStream_t)stream,
                                     "pnp_bn_stats_finish");
}

int pnp_bn_update_moving(float* moving_mean, float* moving_var, const float* mean, const float* var, int64_t P, int32_t C,
                         float decay, void* stream) {
    PNP_REQUIRE(moving_mean && moving_var && mean && var && P > 0 && C > 0, "pnp_bn_update_moving: bad argument");
    hipLaunchKernelGGL(bn_update_moving_kernel, dim3(pnp_cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, moving_mean,
                       moving_var, mean, var, (long long)P, C, decay);
    PNP_CHECK_LAUNCH("pnp_bn_update_moving");
    return PNP_OK;
}

int pnp_bn_apply(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                 const float* shortcut, int32_t Cs, float* y, int64_t P, int32_t C, float eps, float alpha, void* stream) {
    return pnp_bn_apply_h(x, mean, var, gamma, beta, shortcut, Cs, y, nullptr, P, C, eps, alpha, stream);
}

int pnp_bn_apply_h(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                   const float* shortcut, int32_t Cs, float* y, void* yh, int64_t P, int32_t C, float eps, float alpha, void* stream) {
    PNP_REQUIRE(x && mean && var && gamma && beta && y && P > 0 && C > 0, "pnp_bn_apply: bad argument");
    if (shortcut) PNP_REQUIRE(Cs > 0 && Cs <= C && ((C - Cs) % 2) == 0, "pnp_bn_apply: bad shortcut channels %d vs %d", Cs, C);
    BnApplyArgs a{x, mean, var, gamma, beta, shortcut, y, (long long)P, C, shortcut ? Cs : C, eps, alpha, (__bf16*)yh};
    const bool vec = (C % 4 == 0) && (!shortcut || (Cs % 4 == 0 && ((C - Cs) / 2) % 4 == 0));
    const size_t nvec = (size_t)P * (vec ? C / 4 : C);
    if (vec) hipLaunchKernelGGL(bn_apply_kernel<true>, grid_rows(P, C / 4), dim3(NT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(grid_for(nvec)), dim3(NT), 0, (hipStream_t)stream, a);
    PNP_CHECK_LAUNCH("pnp_bn_apply");
    return PNP_OK;
}

int pnp_bn_bwd_reduce(const float* dout, const float* out, const float* x, const float* mean, const float* var, const float* gamma,
                      const float* beta, float* dgamma, float* dbeta, int64_t P, int32_t C, float eps, float alpha, void* workspace,
                      size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(dout && x && mean && var && dgamma && dbeta && P > 0 && C > 0, "pnp_bn_bwd_reduce: bad argument");
    PNP_REQUIRE(alpha < 0.f || out || (gamma && beta), "pnp_bn_bwd_reduce: a fused activation needs `out`, or gamma and beta to recompute its sign");
    PNP_REQUIRE((size_t)P * C < (1ull << 32), "pnp_bn_bwd_reduce: tensor exceeds 2^32 elements");
    ColArgs ca{};
    ca.x = x; ca.dout = dout; ca.out = out; ca.mean = mean; ca.var = var; ca.P = P; ca.C = C; ca.eps = eps; ca.alpha = alpha;
    ca.gamma = gamma; ca.beta = beta;
    return run_colreduce<1>(ca, dbeta, dgamma, workspace, workspace_bytes, (hipStream_t)stream, "pnp_bn_bwd_reduce");
}

int pnp_bn_bwd_apply(const float* dout, const float* out, const float* x, const float* mean, const float* var,
                     const float* gamma, const float* beta, const float* dgamma, const float* dbeta, float* dx, float* dshortcut, int32_t Cs,
                     int64_t P, int64_t P_norm, int32_t C, float eps, float alpha, int32_t training, float keep_prob,
                     uint64_t seed, uint32_t stream_id, void* stream) {
    return pnp_bn_bwd_apply_h(dout, out, x, mean, var, gamma, beta, dgamma, dbeta, dx, nullptr, dshortcut, Cs, P, P_norm, C, eps, alpha,
                              training, keep_prob, seed, stream_id, stream);
}

int pnp_bn_bwd_apply_h(const float* dout, const float* out, const float* x, const float* mean, const float* var,
                       const float* gamma, const float* beta, const float* dgamma, const float* dbeta, float* dx, void* dxh,
                       float* dshortcut, int32_t Cs, int64_t P, int64_t P_norm, int32_t C, float eps, float alpha, int32_t training,
                       float keep_prob, uint64_t seed, uint32_t stream_id, void* stream) {
    PNP_REQUIRE(dout && x && mean && var && gamma && (dx || dxh) && P > 0 && P_norm >= P && C > 0, "pnp_bn_bwd_apply: bad argument");
    PNP_REQUIRE(!training || (dgamma && dbeta), "pnp_bn_bwd_apply: training mode needs the dgamma / dbeta sums");
    PNP_REQUIRE(alpha < 0.f || out || (beta && !dshortcut), "pnp_bn_bwd_apply: a fused activation needs `out`, or beta (and no shortcut) to recompute its sign");
    PNP_REQUIRE((size_t)P * C < (1ull << 32), "pnp_bn_bwd_apply: tensor exceeds 2^32 elements");
    if (dshortcut) PNP_REQUIRE(Cs > 0 && Cs <= C && ((C - Cs) % 2) == 0, "pnp_bn_bwd_apply: bad shortcut channels");
    hipStream_t st = (hipStream_t)stream;
    BnBwdArgs a{};
    a.dout = dout; a.out = out; a.x = x; a.mean = mean; a.var = var; a.gamma = gamma; a.beta = beta; a.dgamma = dgamma; a.dbeta = dbeta;
    a.dx = dx; a.dshortcut = dshortcut; a.P = P; a.P_norm = P_norm; a.C = C; a.Cs = dshortcut ? Cs : C; a.eps = eps; a.alpha = alpha;
    a.training = training;
    a.do_drop = keep_prob < 1.f;
    a.drop_key = pnp_drop_key(seed, stream_id);
    a.drop_thresh = pnp_drop_thresh(keep_prob);
    a.sp = pnp_step_params_ptr(); a.drop_sid = stream_id;
    a.drop_keep = keep_prob < 1.f ? keep_prob : 1.f;
    a.dxh = (__bf16*)dxh;
    const bool vec = (C % 4 == 0) && (!dshortcut || (Cs % 4 == 0 && ((C - Cs) / 2) % 4 == 0));
    const size_t nvec = (size_t)P * (vec ? C / 4 : C);
    if (vec) hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid_rows(P, C / 4), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(grid_for(nvec)), dim3(NT), 0, st, a);
    PNP_CHECK_LAUNCH("pnp_bn_bwd_apply");
    return PNP_OK;
}

int pnp_bn_bwd(const float* dout, const float* out, const float* x, const float* mean, const float* var,
               const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, float* dshortcut, int32_t Cs, int64_t P,
               int32_t C, float eps, float alpha, int32_t training, float keep_prob, uint64_t seed, uint32_t stream_id,
               void* workspace, size_t workspace_bytes, void* stream) {
    return pnp_bn_bwd_acc(dout, out, x, mean, var, gamma, beta, dx, dgamma, dbeta, nullptr, nullptr, dshortcut, Cs, P, C, eps, alpha, training,
                          keep_prob, seed, stream_id, workspace, workspace_bytes, stream);
}

int pnp_bn_bwd_acc(const float* dout, const float* out, const float* x, const float* mean, const float* var,
                   const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, float* dgamma_acc, float* dbeta_acc, float* dshortcut,
                   int32_t Cs, int64_t P, int32_t C, float eps, float alpha, int32_t training, float keep_prob, uint64_t seed,
                   uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream) {
    return pnp_bn_bwd_acc_h(dout, out, x, mean, var, gamma, beta, dx, nullptr, dgamma, dbeta, dgamma_acc, dbeta_acc, dshortcut, Cs, P, C, eps,
                            alpha, training, keep_prob, seed, stream_id, workspace, workspace_bytes, stream);
}

int pnp_bn_bwd_acc_h(const float* dout, const float* out, const float* x, const float* mean, const float* var,
                     const float* gamma, const float* beta, float* dx, void* dxh, float* dgamma, float* dbeta, float* dgamma_acc,
                     float* dbeta_acc, float* dshortcut, int32_t Cs, int64_t P, int32_t C, float eps, float alpha, int32_t training,
                     float keep_prob, uint64_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(dout && x && mean && var && dgamma && dbeta && P > 0 && C > 0, "pnp_bn_bwd: bad argument");
    PNP_REQUIRE(alpha < 0.f || out || (gamma && beta && !dshortcut), "pnp_bn_bwd: a fused activation needs `out`, or beta (and no shortcut) to recompute its sign");
    PNP_REQUIRE((size_t)P * C < (1ull << 32), "pnp_bn_bwd: tensor exceeds 2^32 elements");
    PNP_REQUIRE((dgamma_acc != nullptr) == (dbeta_acc != nullptr), "pnp_bn_bwd_acc: dgamma_acc and dbeta_acc go together");
    ColArgs ca{};
    ca.x = x; ca.dout = dout; ca.out = out; ca.mean = mean; ca.var = var; ca.P = P; ca.C = C; ca.eps = eps; ca.alpha = alpha;
    ca.gamma = gamma; ca.beta = beta;
    if (int e = run_colreduce<1>(ca, dbeta, dgamma, workspace, workspace_bytes, (hipStream_t)stream, "pnp_bn_bwd", nullptr, nullptr, 0.f,
                                 dbeta_acc, dgamma_acc))
        return e;
    return pnp_bn_bwd_apply_h(dout, out, x, mean, var, gamma, beta, dgamma, dbeta, dx, dxh, dshortcut, Cs, P, P, C, eps, alpha, training,
                              keep_prob, seed, stream_id, stream);
}

int pnp_dropout(const float* x, float* y, size_t n, float keep_prob, uint64_t seed, uint32_t stream_id, void* stream) {
    PNP_REQUIRE(y, "pnp_dropout: bad argument");
    return pnp_dropout_h(x, y, nullptr, n, keep_prob, seed, stream_id, stream);
}

int pnp_dropout_h(const float* x, float* y, void* yh, size_t n, float keep_prob, uint64_t seed, uint32_t stream_id, void* stream) {
    PNP_REQUIRE(x && (y || yh) && keep_prob > 0.f, "pnp_dropout: bad argument");
    PNP_REQUIRE(n < (1ull << 32), "pnp_dropout: tensor exceeds 2^32 elements");
    if (n == 0) return PNP_OK;
    const float keepv = keep_prob < 1.f ? keep_prob : 1.f;      // tf.nn.dropout divides: div(x, keep_prob) * mask
    const uint32_t thresh = keep_prob < 1.f ? pnp_drop_thresh(keep_prob) : 0u;
    hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, (hipStream_t)stream, x, y, n,
                       pnp_drop_key(seed, stream_id), thresh, keepv, (__bf16*)yh, pnp_step_params_ptr(), stream_id);
    PNP_CHECK_LAUNCH("pnp_dropout");
    return PNP_OK;
}

int pnp_add(const float* x, const float* y, float* out, size_t n, void* stream) {
    PNP_REQUIRE(x && y && out, "pnp_add: null pointer");
    if (n == 0) return PNP_OK;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, (hipStream_t)stream, x, y, out, n);
    PNP_CHECK_LAUNCH("pnp_add");
    return PNP_OK;
}

int pnp_axpby(const float* x, float* y, size_t n, float a, float b, void* stream) {
    PNP_REQUIRE(x && y, "pnp_axpby: null pointer");
    if (n == 0) return PNP_OK;
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n / 4 + 1)), dim3(NT), 0, (hipStream_t)stream, x, y, n, a, b);
    PNP_CHECK_LAUNCH("pnp_axpby");
    return PNP_OK;
}

int pnp_maxpool2_fwd(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    PNP_REQUIRE(x && y && N > 0 && C > 0 && H > 0 && W > 0 && (H % 2) == 0 && (W % 2) == 0, "pnp_maxpool2_fwd: bad argument (H,W must be even)");
    const size_t total = (size_t)N * (H / 2) * (W / 2) * ((C % 4 == 0) ? C / 4 : C);
    hipLaunchKernelGGL(maxpool2_kernel<false>, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, x,
                       (const float*)nullptr, y, N, H, W, C);
    PNP_CHECK_LAUNCH("pnp_maxpool2_fwd");
    return PNP_OK;
}

int pnp_maxpool2_bwd(const float* x, const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    PNP_REQUIRE(x && dy && dx && N > 0 && C > 0 && H > 0 && W > 0 && (H % 2) == 0 && (W % 2) == 0, "pnp_maxpool2_bwd: bad argument");
    const size_t total = (size_t)N * (H / 2) * (W / 2) * ((C % 4 == 0) ? C / 4 : C);
    hipLaunchKernelGGL(maxpool2_kernel<true>, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, x, dy, dx, N, H, W, C);
    PNP_CHECK_LAUNCH("pnp_maxpool2_bwd");
    return PNP_OK;
}

int pnp_ps_fwd(const float* x, float* y, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, void* stream) {
    PNP_REQUIRE(x && y && N > 0 && A > 0 && B > 0 && r > 0 && nc > 0, "pnp_ps_fwd: bad argument");
    const size_t total = (size_t)N * A * B * nc * r * r;
    if (const int T = ps_tile_T(B, nc * r * r)) {
        hipLaunchKernelGGL(ps_tile_kernel<false>, dim3((unsigned)(N * A * (B / T))), dim3(NT), 0, (hipStream_t)stream, x, y, N, A, B, r, nc, T);
        PNP_CHECK_LAUNCH("pnp_ps_fwd");
        return PNP_OK;
    }
    hipLaunchKernelGGL(ps_kernel<false>, dim3(grid_for(total, 256 * 16)), dim3(NT), 0, (hipStream_t)stream, x, y, N, A, B, r, nc);
    PNP_CHECK_LAUNCH("pnp_ps_fwd");
    return PNP_OK;
}

int pnp_ps_bwd(const float* dy, float* dx, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, void* stream) {
    PNP_REQUIRE(dy && dx && N > 0 && A > 0 && B > 0 && r > 0 && nc > 0, "pnp_ps_bwd: bad argument");
    const size_t total = (size_t)N * A * B * nc * r * r;
    if (const int T = ps_tile_T(B, nc * r * r)) {
        hipLaunchKernelGGL(ps_tile_kernel<true>, dim3((unsigned)(N * A * (B / T))), dim3(NT), 0, (hipStream_t)stream, dy, dx, N, A, B, r, nc, T);
        PNP_CHECK_LAUNCH("pnp_ps_bwd");
        return PNP_OK;
    }
    hipLaunchKernelGGL(ps_kernel<true>, dim3(grid_for(total, 256 * 16)), dim3(NT), 0, (hipStream_t)stream, dy, dx, N, A, B, r, nc);
    PNP_CHECK_LAUNCH("pnp_ps_bwd");
    return PNP_OK;
}

int pnp_critic_input_fwd(const float* a, int32_t Ca, int32_t tile_a, const float* b, int32_t Cb, const float* c, int32_t Cc,
                         const float* d, int32_t Cd, const float* logits, int32_t ncls, float* out, int64_t P, void* stream) {
    PNP_REQUIRE(a && b && c && d && logits && out && P > 0 && Ca > 0 && tile_a > 0 && Cb > 0 && Cc > 0 && Cd > 0 && ncls > 0,
                "pnp_critic_input_fwd: bad argument");
    CriticArgs k{a, b, c, d, logits, out, (long long)P, Ca, tile_a, Cb, Cc, Cd, ncls, Ca * tile_a + Cb + Cc + Cd + ncls + 1};
    if ((k.Ctot & 3) == 0)
        hipLaunchKernelGGL(critic_input_fwd_kernel<true>, dim3(grid_for((size_t)P * (k.Ctot / 4), 256 * 16)), dim3(NT), 0, (hipStream_t)stream, k);
    else
        hipLaunchKernelGGL(critic_input_fwd_kernel<false>, dim3(grid_for((size_t)P * k.Ctot, 256 * 16)), dim3(NT), 0, (hipStream_t)stream, k);
    PNP_CHECK_LAUNCH("pnp_critic_input_fwd");
    return PNP_OK;
}

int pnp_critic_input_bwd(const float* dout, float* da, int32_t Ca, int32_t tile_a, float* db, int32_t Cb, float* dc, int32_t Cc,
                         float* dd, int32_t Cd, float* dlogits, int32_t ncls, int64_t P, void* stream) {
    PNP_REQUIRE(dout && P > 0 && Ca > 0 && tile_a > 0 && Cb > 0 && Cc > 0 && Cd > 0 && ncls > 0, "pnp_critic_input_bwd: bad argument");
    CriticBwdArgs k{dout, da, db, dc, dd, dlogits, (long long)P, Ca, tile_a, Cb, Cc, Cd, ncls, Ca * tile_a + Cb + Cc + Cd + ncls + 1};
    hipLaunchKernelGGL(critic_input_bwd_kernel, dim3(grid_for((size_t)P * (Ca + Cb + Cc + Cd + ncls), 256 * 16)), dim3(NT), 0,
                       (hipStream_t)stream, k);
    PNP_CHECK_LAUNCH("pnp_critic_input_bwd");
    return PNP_OK;
}

int pnp_ps_pad_fwd(const float* x, float* xp, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, int32_t p, void* stream) {
    PNP_REQUIRE(x && xp && N > 0 && A > 0 && B > 0 && r > 0 && nc > 0 && p >= 0, "pnp_ps_pad_fwd: bad argument");
    PNP_REQUIRE(nc * r * r <= 4096 && p <= r, "pnp_ps_pad_fwd: needs nc*r*r <= 4096 and p <= r");
    const int T = ps_fused_T(B, 4096 / (nc * r * r));
    const dim3 grid((unsigned)(N * A * (B / T)));
    if ((nc & 3) == 0) hipLaunchKernelGGL(ps_pad_fwd_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, x, xp, A, B, r, nc, p, T);
    else hipLaunchKernelGGL(ps_pad_fwd_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, x, xp, A, B, r, nc, p, T);
    PNP_CHECK_LAUNCH("pnp_ps_pad_fwd");
    return PNP_OK;
}

int pnp_ps_pad_bwd(const float* dxp, float* dx, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, int32_t p, void* stream) {
    PNP_REQUIRE(dxp && dx && N > 0 && A > 0 && B > 0 && r > 0 && nc > 0 && p >= 0, "pnp_ps_pad_bwd: bad argument");
    PNP_REQUIRE(nc * r * r <= 4096 && p <= r, "pnp_ps_pad_bwd: needs nc*r*r <= 4096 and p <= r");
    const int T = ps_fused_T(B, 4096 / (nc * r * r));
    const dim3 grid((unsigned)(N * A * (B / T)));
    if ((nc & 3) == 0) hipLaunchKernelGGL(ps_pad_bwd_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, dxp, dx, A, B, r, nc, p, T);
    else hipLaunchKernelGGL(ps_pad_bwd_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, dxp, dx, A, B, r, nc, p, T);
    PNP_CHECK_LAUNCH("pnp_ps_pad_bwd");
    return PNP_OK;
}

int pnp_critic_input_ps_fwd(const float* a, int32_t Ca, int32_t tile_a, const float* b, int32_t Cb, const float* c, int32_t Cc,
                            const float* d, int32_t Cd, const float* logits, int32_t ncls, float* out, int32_t N, int32_t A, int32_t B,
                            int32_t r, void* stream) {
    PNP_REQUIRE(a && b && c && d && logits && out && N > 0 && A > 0 && B > 0 && r > 0 && Ca > 0 && tile_a > 0 && Cb > 0 && Cc > 0 && Cd > 0 &&
                    ncls > 0, "pnp_critic_input_ps_fwd: bad argument");
    const int Xp = (Ca + Cb + Cc + Cd) * r * r;
    PNP_REQUIRE(Xp <= 4096, "pnp_critic_input_ps_fwd: needs (Ca+Cb+Cc+Cd)*r*r <= 4096");
    CriticPsArgs k{{a, b, c, d}, logits, out, A, B, r, ps_fused_T(B, 4096 / Xp), {Ca, Cb, Cc, Cd}, tile_a, ncls,
                   Ca * tile_a + Cb + Cc + Cd + ncls + 1};
    const dim3 grid((unsigned)(N * A * (B / k.T)));
    if ((k.Ctot & 3) == 0) hipLaunchKernelGGL(critic_ps_fwd_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(critic_ps_fwd_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, k);
    PNP_CHECK_LAUNCH("pnp_critic_input_ps_fwd");
    return PNP_OK;
}

int pnp_critic_input_ps_bwd(const float* dout, float* da, int32_t Ca, int32_t tile_a, float* db, int32_t Cb, float* dc, int32_t Cc,
                            float* dd, int32_t Cd, float* dlogits, int32_t ncls, int32_t N, int32_t A, int32_t B, int32_t r, void* stream) {
    PNP_REQUIRE(dout && N > 0 && A > 0 && B > 0 && r > 0 && Ca > 0 && tile_a > 0 && Cb > 0 && Cc > 0 && Cd > 0 && ncls > 0,
                "pnp_critic_input_ps_bwd: bad argument");
    const int Ctot = Ca * tile_a + Cb + Cc + Cd + ncls + 1;
    const int Xp = (Ca + Cb + Cc + Cd) * r * r;
    // LDS: r rows of T*r pixels at stride Ctot+8, + 1 per row
    const int capT = (CRITIC_PS_RAW / r - 1) / (r * (Ctot + 8));
    PNP_REQUIRE(Xp <= 4096 && capT >= 1, "pnp_critic_input_ps_bwd: needs (Ca+Cb+Cc+Cd)*r*r <= 4096 and r*(r*(Ctot+8)+1) <= %d", CRITIC_PS_RAW);
    const int any_src = (da || db || dc || dd) ? 1 : 0;
    if (!any_src && !dlogits) return PNP_OK;
    const int cap_x = 4096 / Xp;
    CriticPsBwdArgs k{dout, {da, db, dc, dd}, dlogits, A, B, r, ps_fused_T(B, capT < cap_x ? capT : cap_x), {Ca, Cb, Cc, Cd}, tile_a, ncls,
                      Ctot, any_src};
    const dim3 grid((unsigned)(N * A * (B / k.T)));
    if ((Ctot & 3) == 0) hipLaunchKernelGGL(critic_ps_bwd_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(critic_ps_bwd_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, k);
    PNP_CHECK_LAUNCH("pnp_critic_input_ps_bwd");
    return PNP_OK;
}

}  // extern "C"
