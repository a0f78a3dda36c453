// conv_x3_common.h — what the split-bf16 ("x3") convolution kernels share: conv_wino_x3.hip (+ the operand writers of conv_wino.hip),
// conv_x3_direct.hip, conv_x3_wgrad.hip, conv_x3_narrow.hip.  The arithmetic contract of the family (the split and the kept products:
// tests/test_split_bf16_host.py emulates it on the host), the wait-count / LDS-DMA helpers of the specialised loader waves (conv_bf16r.hip
// uses those too), and the host-side run-time switch of a route.
#pragma once
#include <atomic>
#include <cstdlib>
#include "conv_common.h"

namespace pnpconv {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_vm0() { wait_vm<0>(); }

// one LDS-DMA piece: 16 bytes per lane, global (buffer descriptor + per-lane voffset + scalar soffset) -> LDS (wave-uniform dst + 16 x lane);
// AUX = cache policy bits.  The builtin only exists in the device pass (in the host pass clang silently drops the whole kernel's launch
// stub over it).
template <int AUX = 0>
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, lds_void* dst, unsigned voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 16, voff, soff, 0, AUX);
#endif
}

// v = hi + mid + lo EXACTLY: hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid) (round-to-nearest-even: v_cvt_pk_bf16_f32; both
// differences are exact in fp32)
__device__ __forceinline__ void split3(float v, __bf16& hi, __bf16& mid, __bf16& lo) {
    hi = (__bf16)v;
    const float r1 = v - (float)hi;
    mid = (__bf16)r1;
    lo = (__bf16)(r1 - (float)mid);
}
__device__ __forceinline__ void split3(const f32x4 v, bf16x4& hi, bf16x4& mid, bf16x4& lo) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        __bf16 h, m, l;
        split3(v[c], h, m, l);
        hi[c] = h; mid[c] = m; lo[c] = l;
    }
}
// the three planes of four values, `plane_bytes` (an int in LDS, a size_t in memory) apart
template <class Stride>
__device__ __forceinline__ void store3(void* p, Stride plane_bytes, const bf16x4 hi, const bf16x4 mid, const bf16x4 lo) {
    unsigned char* b = static_cast<unsigned char*>(p);
    *reinterpret_cast<bf16x4*>(b) = hi;
    *reinterpret_cast<bf16x4*>(b + plane_bytes) = mid;
    *reinterpret_cast<bf16x4*>(b + 2 * plane_bytes) = lo;
}

// one value of a pre-split image (the filter kernels): its planes are `pstride` elements apart
__device__ __forceinline__ void split3_write(unsigned short* p, size_t pstride, float v) {
    __bf16 hi, mid, lo;
    split3(v, hi, mid, lo);
    p[0] = __builtin_bit_cast(unsigned short, hi);
    p[pstride] = __builtin_bit_cast(unsigned short, mid);
    p[2 * pstride] = __builtin_bit_cast(unsigned short, lo);
}

// The kept plane products (plane of the one operand, plane of the other), smallest first.  A bf16 x bf16 product is exact in fp32 and plane
// p is below 2^-8p of the value, so   a b = hi.hi + (hi.mid + mid.hi) + (hi.lo + mid.mid + lo.hi) + [mid.lo + lo.mid + lo.lo];
// the three in brackets are below 2^-24 |a b| each — under fp32's own rounding of the product — and are dropped: six MFMAs per fp32 one, the
// small terms accumulated first.
constexpr int kTermX[6] = {2, 1, 0, 1, 0, 0}, kTermW[6] = {0, 1, 2, 0, 1, 0};

// Run-time switch of a route: the environment variable `env` read on first use (`dflt` without it), or what the setter stored.  A setter
// value is clamped to [0, hi]; the environment's only with `clamp_env` (negative values read as "not set yet": the route is off).
struct ModeSwitch {
    const char* env;
    int dflt, hi;
    bool clamp_env;
    std::atomic<int> v{-1};
    int clamp(int m) const { return m > hi ? hi : m; }
    int get() {
        int m = v.load(std::memory_order_relaxed);
        if (m < 0) {
            const char* e = getenv(env);
            m = e ? atoi(e) : dflt;
            if (e && clamp_env) m = clamp(m < 0 ? 0 : m);
            v.store(m, std::memory_order_relaxed);
        }
        return m;
    }
    // mode < 0 only queries; returns the previous mode
    int set(int mode) {
        const int prev = get();
        if (mode >= 0) v.store(clamp(mode), std::memory_order_relaxed);
        return prev;
    }
};

// the dropout arguments of a kernel's argument block, from the entry point's
template <class Args>
inline void copy_dropout(Args& x, const ConvArgs& a) {
    x.do_drop = a.do_drop; x.drop_thresh = a.drop_thresh; x.drop_key = a.drop_key; x.drop_keep = a.drop_keep; x.sp = a.sp; x.drop_sid = a.drop_sid;
}

}  // namespace pnpconv
