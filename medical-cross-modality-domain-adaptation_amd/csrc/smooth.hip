// Anti-alias prefilter of a resident volume: a separable Gaussian (any symmetric or asymmetric 2r + 1 tap filter per axis,
// r <= 32) of a float32 volume [X, Y, Z], z fastest, borders replicated (index clamped into [0, n - 1]: scipy's mode="nearest").
//
//   pnp_volume_smooth            up to three out-of-place passes in the order X, Y, Z; an axis with r == 0 is not touched at all
//   smooth_axis_kernel<VEC>      the passes along X and Y.  Element (o, a, i) of an [outer, n, inner] view lies at (o n + a) inner + i: X is
//                                (1, X, Y Z), Y is (X, Y, Z) — the filtered axis is strided, the lanes run along the contiguous inner index
//                                (16-byte loads when inner % 4 == 0 and the pointers allow, dwords otherwise).  A thread keeps kTA outputs
//                                along the axis in registers and slides over kTA + 2r inputs, each loaded once and fed to the outputs it
//                                belongs to; the tap index is the same in every lane, so the weights come from the kernel arguments.
//   smooth_z_kernel              the pass along Z: a workgroup stages 4 m rows (one per wave and round), each a segment of the row plus
//                                2 rz halo, in LDS, then every lane reads 2 rz + 1 consecutive LDS words per output (conflict-free: lanes
//                                are consecutive along z).  A row of at most kZSeg voxels is one segment: the workgroup reads nothing it
//                                does not own, so that launch is safe IN PLACE; longer rows are cut into segments and run out of place.
//
// Every output is one fmaf chain over the taps k = 0 .. 2r in ascending order, starting from 0: fp32, no atomics, nothing depends on the
// launch geometry — the result is bit-identical from run to run and between the in-place and the out-of-place call.
#include <cmath>
#include <string.h>

#include "pnp_common.h"

namespace {

constexpr int kMaxRadius = 32;
constexpr int kMaxExtentXY = 4096;
constexpr int kThreads = 256;
constexpr int kTA = 8;                                   // outputs along the filtered axis per thread of smooth_axis_kernel
constexpr int kZSeg = 2048;                              // longest row segment of smooth_z_kernel
constexpr int kZCap = 4 * (kZSeg + 2 * kMaxRadius);      // its LDS tile in floats (33 KiB): one row per wave even at the longest segment
constexpr int kZMaxRounds = 8;

struct SmoothW {
    float w[2 * kMaxRadius + 1];
};

template <int VEC>
struct VecOf;
template <>
struct VecOf<1> {
    typedef float type;
};
template <>
struct VecOf<4> {
    typedef f32x4 type;
};

__device__ __forceinline__ float fma_v(float w, float v, float acc) { return fmaf(w, v, acc); }
__device__ __forceinline__ f32x4 fma_v(float w, f32x4 v, f32x4 acc) {
    f32x4 o;
    o.x = fmaf(w, v.x, acc.x);
    o.y = fmaf(w, v.y, acc.y);
    o.z = fmaf(w, v.z, acc.z);
    o.w = fmaf(w, v.w, acc.w);
    return o;
}

// src != dst always (the planner below never runs this kernel in place).  inner_v = inner / VEC, chunks = ceil(n / kTA);
// outer * chunks * inner_v <= X Y Z < 2^31 threads, every offset below is an element index of the volume.
template <int VEC>
__global__ __launch_bounds__(kThreads) void smooth_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, int outer, int n,
                                                               int inner_v, int chunks, int r, SmoothW W) {
    typedef typename VecOf<VEC>::type V;
    const long long total = (long long)outer * chunks * inner_v;
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int iv = (int)(idx % inner_v);
    const int rest = (int)(idx / inner_v);
    const int c = rest % chunks, o = rest / chunks;
    const int a0 = c * kTA;
    const V* s = reinterpret_cast<const V*>(src) + (size_t)o * n * inner_v + iv;
    V* d = reinterpret_cast<V*>(dst) + (size_t)o * n * inner_v + iv;
    V acc[kTA];
#pragma unroll
    for (int t = 0; t < kTA; ++t) acc[t] = V(0.f);
    const int taps = 2 * r;
#pragma unroll 2
    for (int j = 0; j < kTA + taps; ++j) {
        const int a = min(max(a0 - r + j, 0), n - 1);
        const V v = s[(size_t)a * inner_v];
#pragma unroll
        for (int t = 0; t < kTA; ++t) {
            const int k = j - t;                        // the same in every lane
            if (k >= 0 && k <= taps) acc[t] = fma_v(W.w[k], v, acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < kTA; ++t)
        if (a0 + t < n) d[(size_t)(a0 + t) * inner_v] = acc[t];
}

// rows = X Y rows of Z voxels.  Workgroup b: segment b % nseg (voxels z0 .. z0 + len - 1, len <= seg), rows (b / nseg) 4 m .. + 4 m - 1.
// LDS row lr starts at lr (seg + 2 r); 4 m (seg + 2 r) <= kZCap (the host's choice of m).  With nseg == 1 src may be dst.
__global__ __launch_bounds__(kThreads) void smooth_z_kernel(const float* src, float* dst, int rows, int Z, int seg, int nseg, int m, int r,
                                                            SmoothW W) {
    __shared__ float tile[kZCap];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sidx = (int)(blockIdx.x % (unsigned)nseg);
    const long long row0 = (long long)(blockIdx.x / (unsigned)nseg) * (4 * m);
    const int z0 = sidx * seg;
    const int len = min(seg, Z - z0);
    const int stride = seg + 2 * r;
    const int wd = len + 2 * r;
    for (int q = 0; q < m; ++q) {
        const int lr = q * 4 + wave;
        const long long row = row0 + lr;
        if (row < rows) {
            const float* p = src + (size_t)row * Z;
            float* t = tile + lr * stride;
            for (int c = lane; c < wd; c += 64) t[c] = p[min(max(z0 - r + c, 0), Z - 1)];
        }
    }
    __syncthreads();
    const int taps = 2 * r;
    for (int q = 0; q < m; ++q) {
        const int lr = q * 4 + wave;
        const long long row = row0 + lr;
        if (row < rows) {
            const float* t = tile + lr * stride;
            float* p = dst + (size_t)row * Z + z0;
            for (int c = lane; c < len; c += 64) {
                float acc = 0.f;
                for (int k = 0; k <= taps; ++k) acc = fmaf(W.w[k], t[c + k], acc);
                p[c] = acc;
            }
        }
    }
}

// ---- the order of buffers --------------------------------------------------------------------------------------------------------------
// Passes run in the order X, Y, Z over the axes with r > 0.  Every pass is out of place, except that the Z pass of rows of at most kZSeg
// voxels may also run in place.  A pass that is not the last writes the first of (dst, slot 0, slot 1) that is not its own input and — when
// the last pass cannot run in place — is not dst; the last pass writes dst.  One pass alone that cannot run in place, asked for in place,
// writes slot 0 and is copied back.  In place dst is src: free from the second pass on, since the first has read it.
struct SmoothPlan {
    int npass;
    int axis[3];       // 0 = X, 1 = Y, 2 = Z
    int out[3];        // 0 = dst, 1 = slot 0, 2 = slot 1
    bool copy_back;
    int slots;
};

bool z_in_place_ok(int Z) { return Z <= kZSeg; }

SmoothPlan smooth_plan(int Z, int rx, int ry, int rz, bool in_place) {
    SmoothPlan P;
    memset(&P, 0, sizeof(P));
    if (rx > 0) P.axis[P.npass++] = 0;
    if (ry > 0) P.axis[P.npass++] = 1;
    if (rz > 0) P.axis[P.npass++] = 2;
    int cur = in_place ? 0 : -1;          // which buffer holds the current data: -1 = src (distinct from dst), 0 = dst, 1 / 2 = slots
    for (int i = 0; i < P.npass; ++i) {
        const bool last = i == P.npass - 1;
        const bool last_capable = P.axis[P.npass - 1] == 2 && z_in_place_ok(Z);
        int out = 0;
        if (last) {
            if (cur == 0 && !last_capable) {      // one pass alone, in place
                out = 1;
                P.copy_back = true;
            }
        } else {
            const bool next_last = i + 1 == P.npass - 1;
            for (out = 0; out < 3; ++out)
                if (out != cur && !(out == 0 && next_last && !last_capable)) break;
        }
        P.out[i] = out;
        if (out > P.slots) P.slots = out;
        cur = out;
    }
    return P;
}

size_t slot_bytes(long long n) { return (((size_t)n * sizeof(float)) + 255) / 256 * 256; }

bool dims_ok(int X, int Y, int Z) {
    return X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxExtentXY && Y <= kMaxExtentXY && (long long)X * Y * Z < (1ll << 31);
}
bool radii_ok(int rx, int ry, int rz) {
    return rx >= 0 && ry >= 0 && rz >= 0 && rx <= kMaxRadius && ry <= kMaxRadius && rz <= kMaxRadius;
}

int launch_axis(const float* in, float* out, int outer, int n, long long inner, int r, const SmoothW& W, hipStream_t st) {
    const bool wide = inner % 4 == 0 && ((uintptr_t)in | (uintptr_t)out) % 16 == 0;
    const int inner_v = (int)(wide ? inner / 4 : inner);
    const int chunks = pnp_cdiv(n, kTA);
    const long long total = (long long)outer * chunks * inner_v;
    const unsigned nb = (unsigned)pnp_cdiv(total, kThreads);
    if (wide)
        hipLaunchKernelGGL(smooth_axis_kernel<4>, dim3(nb), dim3(kThreads), 0, st, in, out, outer, n, inner_v, chunks, r, W);
    else
        hipLaunchKernelGGL(smooth_axis_kernel<1>, dim3(nb), dim3(kThreads), 0, st, in, out, outer, n, inner_v, chunks, r, W);
    PNP_CHECK_LAUNCH("smooth_axis_kernel");
    return PNP_OK;
}

int launch_z(const float* in, float* out, long long rows, int Z, int r, const SmoothW& W, hipStream_t st) {
    const int nseg = pnp_cdiv(Z, kZSeg);
    const int seg = nseg == 1 ? Z : kZSeg;
    int m = kZCap / (4 * (seg + 2 * r));          // >= 1: seg <= kZSeg, r <= kMaxRadius
    m = m > kZMaxRounds ? kZMaxRounds : m;
    const long long nb = (long long)pnp_cdiv(rows, 4 * m) * nseg;
    hipLaunchKernelGGL(smooth_z_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, in, out, (int)rows, Z, seg, nseg, m, r, W);
    PNP_CHECK_LAUNCH("smooth_z_kernel");
    return PNP_OK;
}

}  // namespace

extern "C" {

size_t pnp_volume_smooth_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t rx, int32_t ry, int32_t rz) {
    if (!dims_ok(X, Y, Z) || !radii_ok(rx, ry, rz)) return 0;
    const int a = smooth_plan(Z, rx, ry, rz, true).slots, b = smooth_plan(Z, rx, ry, rz, false).slots;      // one answer for both calls
    return (a > b ? a : b) * slot_bytes((long long)X * Y * Z);
}

int pnp_volume_smooth(const float* src, float* dst, int32_t X, int32_t Y, int32_t Z, const float* wx, int32_t rx, const float* wy,
                      int32_t ry, const float* wz, int32_t rz, void* workspace, size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(src && dst, "pnp_volume_smooth: null pointer");
    PNP_REQUIRE(X >= 1 && Y >= 1 && Z >= 1, "pnp_volume_smooth: extents %d x %d x %d must be at least 1", (int)X, (int)Y, (int)Z);
    PNP_REQUIRE(X <= kMaxExtentXY && Y <= kMaxExtentXY, "pnp_volume_smooth: X = %d, Y = %d above %d", (int)X, (int)Y, kMaxExtentXY);
    const long long n = (long long)X * Y * Z;
    PNP_REQUIRE(n < (1ll << 31), "pnp_volume_smooth: X * Y * Z = %lld is not below 2^31", n);
    PNP_REQUIRE(radii_ok(rx, ry, rz), "pnp_volume_smooth: radii %d, %d, %d outside [0, %d]", (int)rx, (int)ry, (int)rz, kMaxRadius);
    const float* wp[3] = {wx, wy, wz};
    const int32_t rr[3] = {rx, ry, rz};
    SmoothW W[3];
    memset(W, 0, sizeof(W));
    for (int a = 0; a < 3; ++a) {
        PNP_REQUIRE((wp[a] == nullptr) <= (rr[a] == 0), "pnp_volume_smooth: axis %d: null weights with radius %d", a, (int)rr[a]);
        for (int k = 0; rr[a] > 0 && k <= 2 * rr[a]; ++k) {
            PNP_REQUIRE(std::isfinite(wp[a][k]), "pnp_volume_smooth: axis %d: weight %d is not finite", a, k);
            W[a].w[k] = wp[a][k];
        }
    }
    const bool in_place = src == dst;
    const size_t bytes = (size_t)n * sizeof(float);
    if (!in_place) {
        const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
        PNP_REQUIRE(a + bytes <= b || b + bytes <= a, "pnp_volume_smooth: src and dst overlap partially (in place means dst == src)");
    }
    const size_t need = pnp_volume_smooth_workspace_bytes(X, Y, Z, rx, ry, rz);
    PNP_REQUIRE(workspace_bytes >= need && (workspace || need == 0),
                "pnp_volume_smooth: workspace too small: %zu bytes < %zu (pnp_volume_smooth_workspace_bytes)", workspace ? workspace_bytes : (size_t)0,
                need);
    hipStream_t st = (hipStream_t)stream;
    const SmoothPlan P = smooth_plan(Z, rx, ry, rz, in_place);
    if (P.npass == 0) {
        if (!in_place && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            pnp_set_error("pnp_volume_smooth: the device-to-device copy failed");
            return PNP_ELAUNCH;
        }
        return PNP_OK;
    }
    float* buf[3] = {dst, (float*)workspace, (float*)((char*)workspace + slot_bytes(n))};
    const float* cur = src;
    for (int i = 0; i < P.npass; ++i) {
        float* out = buf[P.out[i]];
        int rc;
        if (P.axis[i] == 0)
            rc = launch_axis(cur, out, 1, X, (long long)Y * Z, rx, W[0], st);
        else if (P.axis[i] == 1)
            rc = launch_axis(cur, out, X, Y, Z, ry, W[1], st);
        else
            rc = launch_z(cur, out, (long long)X * Y, Z, rz, W[2], st);
        if (rc != PNP_OK) return rc;
        cur = out;
    }
    if (P.copy_back && hipMemcpyAsync(dst, cur, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        pnp_set_error("pnp_volume_smooth: the device-to-device copy failed");
        return PNP_ELAUNCH;
    }
    return PNP_OK;
}

}  // extern "C"
