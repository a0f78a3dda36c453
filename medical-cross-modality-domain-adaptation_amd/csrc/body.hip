// Label-free body crop of a resident volume: the intensity histogram of a float32 volume between its own minimum and
// maximum, and the mask of the voxels whose BIN lies above a given bin.  body.py puts Otsu's rule (host, exact integers) between the two
// and the largest-component and bounding-box kernels behind them.
//
//   pnp_volume_histogram         four launches, no host synchronisation
//     body_init_kernel           range <- the keys of an empty min / max (0xffffffff, 0), hist <- 0
//     body_minmax_kernel         per lane the min / max of the order-preserving uint32 keys (augment.hip's key_of), a wave reduction by
//                                shuffles, the four waves of a workgroup through LDS, then ONE atomicMin and ONE atomicMax per workgroup
//     body_range_kernel          one lane turns the two keys back into the floats lo, hi, in place
//     body_hist_kernel           per workgroup an LDS histogram of nbins uint32 (LDS atomics; a lane merges the equal bins of the four
//                                neighbouring voxels it loaded into one add), then one global atomicAdd per non-empty bin
//   pnp_volume_threshold_mask    one launch: mask = bin(v) > k, four voxels per lane, one 4-byte store when the mask address allows it
//
// The three passes over v share one walk (for_each_voxel): v may start at any 4-byte address, so up to three head voxels bring the walk
// to a 16-byte boundary, the body is read as float4 and up to three tail voxels finish it; head and tail belong to workgroup 0.
//
// The bin of a voxel is ONE __device__ function (bin_of) of (v, lo, hi, nbins), written in single IEEE round-to-nearest operations with
// contraction off: the histogram and the mask cannot disagree about a voxel on a bin edge, and numpy's float32 arithmetic restates it bit
// for bit (tests/body_ref.py).  Integer atomics only: bit-identical from run to run.
#include "pnp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;          // one pass of the capped grid covers 1024 x 256 x 4 = 2^20 voxels
constexpr int kMaxBins = 1024;

// order-preserving key of a finite float (augment.hip): negative values flip all bits, the others set the sign bit
__device__ __forceinline__ uint32_t key_of(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ float bin_scale(float lo, float hi, int nbins) {
#pragma clang fp contract(off)
    return __fdiv_rn((float)nbins, __fsub_rn(hi, lo));
}

// the bin of v in [lo, hi]: min(nbins - 1, (int)((v - lo) * scale)), every operation rounded once, nothing contracted or reassociated.
// v >= lo, so the product is >= 0 and at most nbins (1 + 2^-22): the conversion truncates a small non-negative number.
__device__ __forceinline__ int bin_of(float v, float lo, float scale, int nbins) {
#pragma clang fp contract(off)
    const float t = __fmul_rn(__fsub_rn(v, lo), scale);
    return max(0, min(nbins - 1, (int)t));          // the max never acts on finite input: it keeps a NaN's bin inside the table
}

struct Walk {
    int head;          // voxels in front of the first 16-byte boundary (0 .. 3, at most n)
    long long n4;      // float4 packs of the body
    int tail;          // voxels behind the last pack (0 .. 3)
};

__host__ __device__ __forceinline__ Walk walk_of(const float* v, long long n) {
    Walk w;
    const long long h = (long long)(((16u - (unsigned)((uintptr_t)v & 15u)) & 15u) >> 2);
    w.head = (int)(h < n ? h : n);
    w.n4 = (n - w.head) >> 2;
    w.tail = (int)(n - w.head - 4 * w.n4);
    return w;
}

// one(i, x): a single voxel of the head or the tail; four(i, p): the aligned pack that starts at voxel i
template <typename One, typename Four>
__device__ __forceinline__ void for_each_voxel(const float* __restrict__ v, long long n, One one, Four four) {
    const Walk w = walk_of(v, n);
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < w.head) one((long long)t, v[t]);
        const long long t0 = w.head + 4 * w.n4;
        if (t < w.tail) one(t0 + t, v[t0 + t]);
    }
    const float4* __restrict__ p = reinterpret_cast<const float4*>(v + w.head);
    const long long gs = (long long)gridDim.x * kThreads;
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < w.n4; j += gs) four(w.head + 4 * j, p[j]);
}

__global__ void __launch_bounds__(kThreads) body_init_kernel(uint32_t* __restrict__ range_keys, uint32_t* __restrict__ hist, int nbins) {
    for (int i = threadIdx.x; i < nbins; i += kThreads) hist[i] = 0u;
    if (threadIdx.x == 0) {
        range_keys[0] = 0xffffffffu;
        range_keys[1] = 0u;
    }
}

__global__ void __launch_bounds__(kThreads) body_minmax_kernel(const float* __restrict__ v, long long n, uint32_t* __restrict__ range_keys) {
    __shared__ uint32_t slo[kThreads / 64], shi[kThreads / 64];
    uint32_t lo = 0xffffffffu, hi = 0u;
    for_each_voxel(
        v, n,
        [&](long long, float x) {
            const uint32_t k = key_of(x);
            lo = min(lo, k);
            hi = max(hi, k);
        },
        [&](long long, float4 p) {
            const uint32_t k0 = key_of(p.x), k1 = key_of(p.y), k2 = key_of(p.z), k3 = key_of(p.w);
            lo = min(min(lo, min(k0, k1)), min(k2, k3));
            hi = max(max(hi, max(k0, k1)), max(k2, k3));
        });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        slo[wave] = lo;
        shi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            lo = min(lo, slo[w]);
            hi = max(hi, shi[w]);
        }
        if (lo <= hi) {          // a workgroup beyond the data saw nothing
            atomicMin(&range_keys[0], lo);
            atomicMax(&range_keys[1], hi);
        }
    }
}

__global__ void __launch_bounds__(64) body_range_kernel(uint32_t* __restrict__ range_keys) {
    if (threadIdx.x == 0) {
        const uint32_t klo = range_keys[0], khi = range_keys[1];
        float* r = reinterpret_cast<float*>(range_keys);
        r[0] = float_of(klo);
        r[1] = float_of(khi);
    }
}

__global__ void __launch_bounds__(kThreads) body_hist_kernel(const float* __restrict__ v, long long n, const float* __restrict__ range,
                                                             int nbins, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kMaxBins];
    for (int i = threadIdx.x; i < nbins; i += kThreads) h[i] = 0u;
    __syncthreads();
    const float lo = range[0], hi = range[1];
    if (hi == lo) {               // a constant volume: everything is bin 0 (the scale would be a division by zero)
        if (blockIdx.x == 0 && threadIdx.x == 0) hist[0] = (uint32_t)n;
        return;
    }
    const float scale = bin_scale(lo, hi, nbins);
    for_each_voxel(
        v, n, [&](long long, float x) { atomicAdd(&h[bin_of(x, lo, scale, nbins)], 1u); },
        [&](long long, float4 p) {
            // neighbours along the fastest axis mostly share a bin: equal bins in a row become one add
            const int b0 = bin_of(p.x, lo, scale, nbins), b1 = bin_of(p.y, lo, scale, nbins), b2 = bin_of(p.z, lo, scale, nbins),
                      b3 = bin_of(p.w, lo, scale, nbins);
            int cur = b0;
            uint32_t cnt = 1u;
            const int rest[3] = {b1, b2, b3};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (rest[k] == cur) {
                    ++cnt;
                } else {
                    atomicAdd(&h[cur], cnt);
                    cur = rest[k];
                    cnt = 1u;
                }
            }
            atomicAdd(&h[cur], cnt);
        });
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += kThreads) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

template <bool PACKED>
__global__ void __launch_bounds__(kThreads) body_mask_kernel(const float* __restrict__ v, long long n, const float* __restrict__ range,
                                                             int nbins, int k, uint8_t* __restrict__ mask) {
    const float lo = range[0], hi = range[1];
    const bool flat = hi == lo;                                       // a constant volume has no body: all zeros
    const float scale = flat ? 0.f : bin_scale(lo, hi, nbins);
    auto in_body = [&](float x) -> uint32_t { return (!flat && bin_of(x, lo, scale, nbins) > k) ? 1u : 0u; };
    for_each_voxel(
        v, n, [&](long long i, float x) { mask[i] = (uint8_t)in_body(x); },
        [&](long long i, float4 p) {
            const uint32_t m0 = in_body(p.x), m1 = in_body(p.y), m2 = in_body(p.z), m3 = in_body(p.w);
            if constexpr (PACKED) {
                *reinterpret_cast<uint32_t*>(mask + i) = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
            } else {
                mask[i] = (uint8_t)m0;
                mask[i + 1] = (uint8_t)m1;
                mask[i + 2] = (uint8_t)m2;
                mask[i + 3] = (uint8_t)m3;
            }
        });
}

int blocks_for(const float* v, long long n) {
    const Walk w = walk_of(v, n);
    const long long want = (w.n4 + kThreads - 1) / kThreads;
    return (int)(want < 1 ? 1 : want > kMaxBlocks ? kMaxBlocks : want);         // workgroup 0 always exists: head and tail are its own
}

}  // namespace

extern "C" {

int pnp_volume_histogram(const float* v, int64_t n, int32_t nbins, float* range, uint32_t* hist, void* stream) {
    PNP_REQUIRE(v && range && hist, "pnp_volume_histogram: null pointer");
    PNP_REQUIRE(n >= 1 && n < (1ll << 31), "pnp_volume_histogram: n = %lld outside [1, 2^31)", (long long)n);
    PNP_REQUIRE(nbins >= 2 && nbins <= kMaxBins, "pnp_volume_histogram: nbins = %d outside [2, %d]", (int)nbins, kMaxBins);
    PNP_REQUIRE((uintptr_t)v % 4 == 0 && (uintptr_t)range % 4 == 0 && (uintptr_t)hist % 4 == 0,
                "pnp_volume_histogram: v, range and hist must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint32_t* keys = reinterpret_cast<uint32_t*>(range);
    const int blocks = blocks_for(v, n);
    hipLaunchKernelGGL(body_init_kernel, dim3(1), dim3(kThreads), 0, st, keys, hist, (int)nbins);
    PNP_CHECK_LAUNCH("body_init_kernel");
    hipLaunchKernelGGL(body_minmax_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, v, (long long)n, keys);
    PNP_CHECK_LAUNCH("body_minmax_kernel");
    hipLaunchKernelGGL(body_range_kernel, dim3(1), dim3(64), 0, st, keys);
    PNP_CHECK_LAUNCH("body_range_kernel");
    hipLaunchKernelGGL(body_hist_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, v, (long long)n, (const float*)range, (int)nbins, hist);
    PNP_CHECK_LAUNCH("body_hist_kernel");
    return PNP_OK;
}

int pnp_volume_threshold_mask(const float* v, int64_t n, const float* range, int32_t nbins, int32_t k, uint8_t* mask, void* stream) {
    PNP_REQUIRE(v && range && mask, "pnp_volume_threshold_mask: null pointer");
    PNP_REQUIRE(n >= 1 && n < (1ll << 31), "pnp_volume_threshold_mask: n = %lld outside [1, 2^31)", (long long)n);
    PNP_REQUIRE(nbins >= 2 && nbins <= kMaxBins, "pnp_volume_threshold_mask: nbins = %d outside [2, %d]", (int)nbins, kMaxBins);
    PNP_REQUIRE(k >= 0 && k <= nbins - 1, "pnp_volume_threshold_mask: k = %d outside [0, %d]", (int)k, (int)nbins - 1);
    PNP_REQUIRE((uintptr_t)v % 4 == 0 && (uintptr_t)range % 4 == 0, "pnp_volume_threshold_mask: v and range must be 4-byte aligned");
    const uintptr_t v0 = (uintptr_t)v, v1 = v0 + (uintptr_t)n * 4, m0 = (uintptr_t)mask, m1 = m0 + (uintptr_t)n;
    PNP_REQUIRE(m1 <= v0 || v1 <= m0, "pnp_volume_threshold_mask: mask overlaps v");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = blocks_for(v, n);
    // the pack that starts at voxel head + 4 j is stored at mask + head + 4 j: one 4-byte store when that address is a multiple of 4
    if ((m0 + (uintptr_t)walk_of(v, n).head) % 4 == 0)
        hipLaunchKernelGGL(body_mask_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, v, (long long)n, range, (int)nbins, (int)k, mask);
    else
        hipLaunchKernelGGL(body_mask_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, v, (long long)n, range, (int)nbins, (int)k, mask);
    PNP_CHECK_LAUNCH("body_mask_kernel");
    return PNP_OK;
}

}  // extern "C"
