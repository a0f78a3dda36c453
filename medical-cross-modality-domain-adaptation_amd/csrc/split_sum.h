// split_sum.h — the sums over reduction-split partials of the convolution kernels, one body per summation ORDER.  No
// atomics: the order of the additions is fixed, two runs give the same bits.  A header of templates, instantiated where used
// (conv_igemm.hip, conv_x3_wgrad.hip), like block_sum.h and pixel_loss.h.
//   serial_kernel<EPI>  one thread per value: s = 0.f, then the partials z = 0 .. nsplit - 1 in order; EPI says where s goes
//   sliced_kernel<V>    many partials of a small gradient: 16 slices per value, slice s adds the partials s, s + 16, ... in order, then the
//                       16 slice sums are added in order 0 .. 15 through LDS; V floats per lane (1: any n; 4: n % 4 == 0, 16-byte aligned)
// (conv_wino.hip's wino_splitsum_kernel is not one of these: it sums in place and its first term is S[0], not zero.)
#pragma once
#include "conv_common.h"

namespace split_sum {
namespace {

using pnpconv::ConvArgs;

// ---- where a serial sum goes: begin() once per thread in front of the loop, put(i, s) per value ----------------------------------
// store, or add into what is there (the accumulating filter-gradient entry points)
struct Plain {
    static constexpr const char* label = "split_sum::serial_kernel<Plain>";
    float* out;
    int accumulate;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void put(size_t i, float s) const { out[i] = accumulate ? out[i] + s : s; }
};
// forward conv with a split reduction: the dropout of the fused conv -> dropout (same element-index hash as the un-split epilogue)
struct Drop {
    static constexpr const char* label = "split_sum::serial_kernel<Drop>";
    float* out;
    uint32_t drop_key, drop_thresh;
    float drop_keep;
    const pnp_step_params* sp;
    uint32_t drop_sid;
    __device__ __forceinline__ void begin() { drop_key = pnp_eff_drop_key(drop_key, sp, drop_sid); }
    __device__ __forceinline__ void put(size_t i, float s) const { out[i] = pnp_drop_keep((uint32_t)i, drop_key, drop_thresh) ? s / drop_keep : 0.f; }
};
// split partials of one stride phase ([nsplit][M][K] row-major) -> scattered to the phase's pixels of dx (a.y)
struct Scatter {
    static constexpr const char* label = "split_sum::serial_kernel<Scatter>";
    ConvArgs a;
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void put(size_t i, float s) const {
        const int m = (int)(i / a.K);
        a.y[pnpconv::out_row(a, m, true) + (i - (size_t)m * a.K)] = s;
    }
};

template <class EPI>
__global__ void serial_kernel(const float* __restrict__ part, size_t n, int nsplit, size_t stride, EPI epi) {
    epi.begin();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += gs) {
        float s = 0.f;
        for (int z = 0; z < nsplit; ++z) s += part[(size_t)z * stride + i];
        epi.put(i, s);
    }
}

// n values, partial z at part + z * stride
template <class EPI>
int launch_serial(const float* part, size_t n, int nsplit, size_t stride, const EPI& epi, hipStream_t st) {
    int nb = pnp_cdiv((long long)n, 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(serial_kernel<EPI>, dim3(nb), dim3(256), 0, st, part, n, nsplit, stride, epi);
    PNP_CHECK_LAUNCH(EPI::label);
    return PNP_OK;
}

template <int V> struct Lane;
template <> struct Lane<1> { typedef float type; static constexpr const char* label = "split_sum::sliced_kernel<1>"; };
template <> struct Lane<4> { typedef f32x4 type; static constexpr const char* label = "split_sum::sliced_kernel<4>"; };

// out[n] (+)= the partials [nparts][n]: a workgroup covers 64 values x 16 slices with (64 / V) * 16 threads
template <int V>
__global__ void __launch_bounds__(64 / V * 16) sliced_kernel(const float* __restrict__ part, float* __restrict__ out, int n, int nparts, int accumulate) {
    typedef typename Lane<V>::type T;
    constexpr int NC = 64 / V;
    __shared__ T red[16][NC];
    const int c = threadIdx.x % NC, s = threadIdx.x / NC;
    const int e = (blockIdx.x * NC + c) * V;
    T v = {};
    if (e < n)
        for (int z = s; z < nparts; z += 16) v += *reinterpret_cast<const T*>(part + (size_t)z * n + e);
    red[s][c] = v;
    __syncthreads();
    if (s == 0 && e < n) {          // v is slice 0's sum: a sum that started from +0.f is never -0.f, so this is 0.f + red[0] bit for bit
#pragma unroll
        for (int j = 1; j < 16; ++j) v += red[j][c];
        T* o = reinterpret_cast<T*>(out + e);
        *o = accumulate ? *o + v : v;
    }
}

template <int V>
int launch_sliced(const float* part, float* out, int n, int nparts, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(sliced_kernel<V>, dim3((unsigned)pnp_cdiv((long long)n, 64)), dim3(64 / V * 16), 0, st, part, out, n, nparts, accumulate);
    PNP_CHECK_LAUNCH(Lane<V>::label);
    return PNP_OK;
}

}  // namespace
}  // namespace split_sum
