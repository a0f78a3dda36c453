// entropy.hip — normalised mean Shannon entropy of the softmax of a logits tensor and its gradient, in one streaming pass
// (entropy minimisation on the unlabelled target's predictions; not in the reference).
//
//   p_i = softmax(z_i),  H_i = -sum_k p_ik log p_ik,  L = sum_i H_i / (P ln C),  dL/dz_ij = -p_ij (log p_ij + H_i) / (P ln C)
//
// log p comes from the log-softmax (z - max - log sum exp), never from logf(p): a class hundreds of logits behind has p == 0 and a
// finite log p, its term is 0 * finite = 0.  The gradient of a plain mean needs no global sum, so the pass that reads the logits writes
// the gradient and the per-block partial sums of H_i; a second one-block launch adds the partials in a fixed order in double.
#include "pnp_common.h"

#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int MAXC = 8;
constexpr int PIX_PER_THREAD = 8;      // grid sizing only: two four-pixel groups per thread before the grid cap makes it more
constexpr int MAX_BLOCKS = 2048;

inline int entropy_blocks(long long P) {
    long long b = (P + (long long)NT * PIX_PER_THREAD - 1) / ((long long)NT * PIX_PER_THREAD);
    if (b > MAX_BLOCKS) b = MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

// one pixel: z[0..C) -> H (returned); g[0..C) = -gk * p (log p + H) when GRAD
template <int C, bool GRAD>
__device__ __forceinline__ float entropy_pixel(const float* z, int ncls, float gk, float* g) {
    float m = z[0];
#pragma unroll
    for (int j = 1; j < C; ++j)
        if (j < ncls) m = fmaxf(m, z[j]);
    float e[C], s = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        e[j] = j < ncls ? expf(z[j] - m) : 0.f;
        s += e[j];
    }
    const float ls = logf(s), inv = 1.0f / s;
    float lp[C], H = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        lp[j] = j < ncls ? (z[j] - m) - ls : 0.f;
        e[j] *= inv;
        H = fmaf(-e[j], lp[j], H);
    }
    if (GRAD) {
#pragma unroll
        for (int j = 0; j < C; ++j) g[j] = -gk * e[j] * (lp[j] + H);
    }
    return H;
}

// VEC5: ncls == 5 and 16-byte aligned bases — four pixels are 80 bytes = five float4 loads (and stores) per thread; the P % 4 pixels
// behind the last whole group take the scalar loop, which is the whole kernel otherwise (any 1 <= ncls <= MAXC, any alignment).
template <bool VEC5, bool GRAD>
__global__ void __launch_bounds__(NT) softmax_entropy_kernel(const float* __restrict__ logits, float* __restrict__ dlogits,
                                                             float* __restrict__ part, long long P, int ncls, float gk) {
    __shared__ float lds[4];
    float acc[1] = {0.f};
    const long long gs = (long long)gridDim.x * NT;
    const long long t0 = (long long)blockIdx.x * NT + threadIdx.x;
    long long first = 0;
    if (VEC5) {
        const long long ngrp = P >> 2;
        const float4* __restrict__ in = reinterpret_cast<const float4*>(logits);
        float4* __restrict__ out = reinterpret_cast<float4*>(dlogits);
        for (long long q = t0; q < ngrp; q += gs) {
            float f[20];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float4 v = in[q * 5 + k];
                f[4 * k] = v.x, f[4 * k + 1] = v.y, f[4 * k + 2] = v.z, f[4 * k + 3] = v.w;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[0] += entropy_pixel<5, GRAD>(f + 5 * r, 5, gk, f + 5 * r);
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < 5; ++k) out[q * 5 + k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
            }
        }
        first = ngrp << 2;
    }
    for (long long i = first + t0; i < P; i += gs) {
        float z[MAXC];
#pragma unroll
        for (int j = 0; j < MAXC; ++j) z[j] = j < ncls ? logits[i * ncls + j] : 0.f;
        acc[0] += entropy_pixel<MAXC, GRAD>(z, ncls, gk, z);
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < MAXC; ++j)
                if (j < ncls) dlogits[i * ncls + j] = z[j];
        }
    }
    // block sum in a fixed order: shuffle tree per wave, then the four waves
    float x = acc[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// one block: thread t adds partials t, t + NT, ... in double, then a fixed tree over the block -> out[0] = sum * scale
__global__ void __launch_bounds__(NT) softmax_entropy_final_kernel(const float* __restrict__ part, int nblk, double scale,
                                                                   float* __restrict__ out) {
    __shared__ double red[NT];
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += NT) a += (double)part[b];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(red[0] * scale);
}

template <bool VEC5>
void launch_entropy(const float* logits, float* dlogits, float* part, long long P, int ncls, float gk, int nblk, hipStream_t st) {
    if (dlogits)
        hipLaunchKernelGGL((softmax_entropy_kernel<VEC5, true>), dim3(nblk), dim3(NT), 0, st, logits, dlogits, part, P, ncls, gk);
    else
        hipLaunchKernelGGL((softmax_entropy_kernel<VEC5, false>), dim3(nblk), dim3(NT), 0, st, logits, dlogits, part, P, ncls, gk);
}

}  // namespace

extern "C" {

size_t pnp_softmax_entropy_workspace_bytes(int64_t P, int32_t ncls) {
    (void)ncls;
    return (size_t)entropy_blocks(P) * sizeof(float);
}

int pnp_softmax_entropy(const float* logits, int64_t P, int32_t ncls, float coef, float* dlogits, float* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(logits && out && workspace && P > 0 && ncls > 0, "pnp_softmax_entropy: bad argument");
    PNP_REQUIRE(ncls <= MAXC, "pnp_softmax_entropy: ncls = %d, at most %d classes are served", (int)ncls, MAXC);
    PNP_REQUIRE(workspace_bytes >= pnp_softmax_entropy_workspace_bytes(P, ncls), "pnp_softmax_entropy: workspace too small (%zu < %zu bytes)",
                workspace_bytes, pnp_softmax_entropy_workspace_bytes(P, ncls));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = entropy_blocks(P);
    float* part = (float*)workspace;
    // 1 / (P ln C); a single class has entropy 0 and no normaliser (soft_entropy of paste.hip): value and gradient are 0
    const double scale = ncls > 1 ? 1.0 / ((double)P * std::log((double)ncls)) : 0.0;
    const float gk = (float)((double)coef * scale);
    const bool vec5 = ncls == 5 && P >= 4 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)dlogits & 15) == 0;
    if (vec5)
        launch_entropy<true>(logits, dlogits, part, (long long)P, ncls, gk, nblk, st);
    else
        launch_entropy<false>(logits, dlogits, part, (long long)P, ncls, gk, nblk, st);
    PNP_CHECK_LAUNCH("softmax_entropy_kernel");
    hipLaunchKernelGGL(softmax_entropy_final_kernel, dim3(1), dim3(NT), 0, st, (const float*)part, nblk, scale, out);
    PNP_CHECK_LAUNCH("softmax_entropy_final_kernel");
    return PNP_OK;
}

}  // extern "C"
