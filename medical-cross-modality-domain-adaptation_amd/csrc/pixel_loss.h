// pixel_loss.h — the skeleton of the loss terms that are a plain mean over pixels of a function of softmax(logits):
// one streaming pass that reads the logits (and the term's extra [P][ncls] inputs), writes the gradient and the per-block partial sums
// of the per-pixel contributions, then one block that adds the partials in a fixed order in double (block_sum.h).  The gradient of a
// plain mean needs no global sum, so the pass that reads the logits writes it.  No atomics, no host read: stream-ordered, capturable,
// bit-identical from run to run.
//
// A term is a struct with
//   static constexpr int NEXTRA                       how many extra [P][ncls] float inputs a pixel reads (0: the logits alone)
//   struct Args : Extra<NEXTRA>                       what the kernel gets by value: the extra inputs and whatever else the term reads
//   template <int C> struct Lane                      per-thread state, built once from (args, ncls) before the loops; block_end(args,
//                                                     ncls) is called once per block, by every thread, behind the float block sum
//   static constexpr bool SIDE                        the pixel also gives one byte and one float, stored to args.labels[P] (uint8_t) and
//                                                     args.conf[P] (as one uint32_t and one float4 per group on the vector path)
//   template <int C, bool GRAD> static __device__ float pixel(const float* z, const float* const* x, int ncls, float gk, float* g,
//                                                             Lane<C>& lane, uint32_t& lab, float& conf)
//       z[0..C) the logits (entries >= ncls are 0), x[k][0..C) extra input k -> the pixel's contribution; g[0..C) = gk * its gradient
//       when GRAD (g may alias z; entries >= ncls are not stored); lab (< 256) and conf are read only when SIDE
// and a host entry point that checks its arguments, computes scale (out[0] = scale * sum of contributions, in double) and
// gk = (float)(coef * scale), and calls pixel_loss::run<TERM>, or run_stream<TERM> and a second launch of its own.  Plain<NEXTRA> is the
// base of a term that has neither state nor side outputs: it supplies everything but pixel, and every option is absent at compile time.
#pragma once
#include "block_sum.h"
#include "pnp_common.h"

namespace pixel_loss {

constexpr int NT = 256;
constexpr int PIX_PER_THREAD = 8;      // grid sizing only: two four-pixel groups per thread before the grid cap makes it more
constexpr int MAX_BLOCKS = 2048;

inline int blocks(long long P) {
    long long b = (P + (long long)NT * PIX_PER_THREAD - 1) / ((long long)NT * PIX_PER_THREAD);
    if (b > MAX_BLOCKS) b = MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

// one float per block of the streaming pass
inline size_t workspace_bytes(long long P) { return (size_t)blocks(P) * sizeof(float); }

// the softmax prefix of one pixel: m = max z, e[j] = expf(z[j] - m) (0 past ncls) -> their sum, added in ascending j
template <int C>
__device__ __forceinline__ float softmax_exp(const float* z, int ncls, float* e, float& m) {
    m = z[0];
#pragma unroll
    for (int j = 1; j < C; ++j)
        if (j < ncls) m = fmaxf(m, z[j]);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        e[j] = j < ncls ? expf(z[j] - m) : 0.f;
        s += e[j];
    }
    return s;
}

// the term's extra inputs (NEXTRA == 0: one slot that nothing reads).  Plain pointers: the kernel promises the compiler nothing about
// them (the logits, the gradient and the partials are __restrict__), so an extra input may alias another one, never an output
template <int N>
struct Extra {
    const float* p[N > 0 ? N : 1];
};

// a term of N extra inputs without per-thread state and without side outputs
template <int N>
struct Plain {
    static constexpr int NEXTRA = N;
    static constexpr bool SIDE = false;
    using Args = Extra<N>;
    template <int C>
    struct Lane {
        __device__ Lane(const Args&, int) {}
        __device__ void block_end(const Args&, int) {}
    };
};

// VEC5: ncls == 5 and every base aligned for its vector type — four pixels are 80 bytes = five float4 loads of each input (and five
// stores) per thread; the P % 4 pixels behind the last whole group take the scalar loop, which is the whole kernel otherwise (any
// 1 <= ncls <= MAXC, any alignment).  C, the length of a pixel's register arrays, is one value per instance: the tail of a VEC5 instance
// runs at 5 as well (entries past ncls only ever add +0.f, so the bits are those of MAXC), and a term's Lane<C> serves both loops.
template <typename TERM, bool VEC5, bool GRAD>
__global__ void __launch_bounds__(NT) stream_kernel(const float* __restrict__ logits, float* __restrict__ dlogits, float* __restrict__ part,
                                                    long long P, int ncls, float gk, const typename TERM::Args args) {
    constexpr int C = VEC5 ? 5 : MAXC, NX = TERM::NEXTRA, NQ = NX > 0 ? NX : 1;
    __shared__ float lds[4];
    typename TERM::template Lane<C> lane(args, ncls);
    float acc = 0.f;
    const long long gs = (long long)gridDim.x * NT;
    const long long t0 = (long long)blockIdx.x * NT + threadIdx.x;
    long long first = 0;
    if constexpr (VEC5) {
        const long long ngrp = P >> 2;
        const float4* __restrict__ in = reinterpret_cast<const float4*>(logits);
        float4* __restrict__ out = reinterpret_cast<float4*>(dlogits);
        for (long long g = t0; g < ngrp; g += gs) {
            float f[20], q[NQ][20], c[4];
            uint32_t lab[4];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float4 v = in[g * 5 + k];
                f[4 * k] = v.x, f[4 * k + 1] = v.y, f[4 * k + 2] = v.z, f[4 * k + 3] = v.w;
#pragma unroll
                for (int n = 0; n < NX; ++n) {
                    const float4 u = reinterpret_cast<const float4*>(args.p[n])[g * 5 + k];
                    q[n][4 * k] = u.x, q[n][4 * k + 1] = u.y, q[n][4 * k + 2] = u.z, q[n][4 * k + 3] = u.w;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* x[NQ] = {};      // (null, not the unread q, without extras: that pointer cost <Entropy, true, true> 2 VGPRs)
#pragma unroll
                for (int n = 0; n < NX; ++n) x[n] = q[n] + 5 * r;
                acc += TERM::template pixel<5, GRAD>(f + 5 * r, x, 5, gk, f + 5 * r, lane, lab[r], c[r]);
            }
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < 5; ++k) out[g * 5 + k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
            }
            if constexpr (TERM::SIDE) {
                reinterpret_cast<uint32_t*>(args.labels)[g] = lab[0] | lab[1] << 8 | lab[2] << 16 | lab[3] << 24;
                reinterpret_cast<float4*>(args.conf)[g] = make_float4(c[0], c[1], c[2], c[3]);
            }
        }
        first = ngrp << 2;
    }
    for (long long i = first + t0; i < P; i += gs) {
        float z[C], q[NQ][C], c;
        uint32_t lab;
        const float* x[NQ] = {};
#pragma unroll
        for (int j = 0; j < C; ++j) {
            z[j] = j < ncls ? logits[i * ncls + j] : 0.f;
#pragma unroll
            for (int n = 0; n < NX; ++n) q[n][j] = j < ncls ? args.p[n][i * ncls + j] : 0.f;
        }
#pragma unroll
        for (int n = 0; n < NX; ++n) x[n] = q[n];
        acc += TERM::template pixel<C, GRAD>(z, x, ncls, gk, z, lane, lab, c);
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < C; ++j)
                if (j < ncls) dlogits[i * ncls + j] = z[j];
        }
        if constexpr (TERM::SIDE) {
            args.labels[i] = (uint8_t)lab;
            args.conf[i] = c;
        }
    }
    // block sum in a fixed order: shuffle tree per wave, then the four waves pairwise
    float s = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    lane.block_end(args, ncls);
}

// one block: the partials in a fixed order in double -> out[0] = sum * scale.  (static on purpose: a kernel defined in a header needs
// internal linkage, so every source that includes this one carries its own copy, each in its own code object)
static __global__ void __launch_bounds__(NT) final_kernel(const float* __restrict__ part, int nblk, double scale, float* __restrict__ out) {
    __shared__ double red[NT];
    const double sum = block_sum_of_list<NT>(part, nblk, red);
    if (threadIdx.x == 0) out[0] = (float)(sum * scale);
}

template <typename TERM, bool VEC5>
void launch_stream(const float* logits, const typename TERM::Args& args, float* dlogits, float* part, long long P, int ncls, float gk,
                   int nblk, hipStream_t st) {
    if (dlogits)
        hipLaunchKernelGGL((stream_kernel<TERM, VEC5, true>), dim3(nblk), dim3(NT), 0, st, logits, dlogits, part, P, ncls, gk, args);
    else
        hipLaunchKernelGGL((stream_kernel<TERM, VEC5, false>), dim3(nblk), dim3(NT), 0, st, logits, dlogits, part, P, ncls, gk, args);
}

// PNP_CHECK_LAUNCH with the entry point in front: the kernels are shared, `who` says which term failed
inline bool launch_failed(const char* who, const char* kernel) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) pnp_set_error("%s: %s: launch failed: %s", who, kernel, hipGetErrorString(e));
    return e != hipSuccess;
}

// the first launch of a term's entry point (`who`): blocks(P) workgroups of the instance that the operands allow.  args: the term's
// extra inputs and whatever else it reads; dlogits may be null (value only); part: one float per workgroup
template <typename TERM>
int run_stream(const char* who, const float* logits, const typename TERM::Args& args, long long P, int ncls, float gk, float* dlogits,
               float* part, hipStream_t st) {
    const int nblk = blocks(P);
    uintptr_t bases = (uintptr_t)logits | (uintptr_t)dlogits;      // VEC5 needs every base it reads or writes 16-byte aligned
    for (int n = 0; n < TERM::NEXTRA; ++n) bases |= (uintptr_t)args.p[n];
    bool vec5 = ncls == 5 && P >= 4;
    if constexpr (TERM::SIDE) {                                    // (four confidences are one float4, four label bytes one uint32_t)
        bases |= (uintptr_t)args.conf;
        vec5 = vec5 && ((uintptr_t)args.labels & 3) == 0;
    }
    if (vec5 && (bases & 15) == 0)
        launch_stream<TERM, true>(logits, args, dlogits, part, P, ncls, gk, nblk, st);
    else
        launch_stream<TERM, false>(logits, args, dlogits, part, P, ncls, gk, nblk, st);
    return launch_failed(who, "pixel_loss::stream_kernel") ? PNP_ELAUNCH : PNP_OK;
}

// what the entry point of a term with one output does behind its argument checks: the two launches.  workspace: workspace_bytes(P) bytes
template <typename TERM>
int run(const char* who, const float* logits, const typename TERM::Args& args, long long P, int ncls, double scale, float gk,
        float* dlogits, float* out, void* workspace, hipStream_t st) {
    float* part = (float*)workspace;
    if (const int rc = run_stream<TERM>(who, logits, args, P, ncls, gk, dlogits, part, st)) return rc;
    hipLaunchKernelGGL(final_kernel, dim3(1), dim3(NT), 0, st, (const float*)part, blocks(P), scale, out);
    return launch_failed(who, "pixel_loss::final_kernel") ? PNP_ELAUNCH : PNP_OK;
}

}  // namespace pixel_loss
