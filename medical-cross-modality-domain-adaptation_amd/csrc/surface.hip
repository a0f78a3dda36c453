// surface.hip — 3-D surface-distance metrics of label volumes: the semantics of medpy.metric.binary asd / assd / hd / hd95 with
// connectivity 1, on the device from the label volumes to the per-class rows.
//
//   border pass   one pass over both int32 label volumes (z fastest): per voxel a per-class border bitmask for the prediction and for
//                 the ground truth (a voxel of class c with one of its 6 face neighbours outside class c or outside the volume) and
//                 per-class border counts
//   exact EDT     squared Euclidean distance transform of one border set by three 1-D min-plus passes, f'(i) = min_j f(j) + (s (i-j))^2
//                 (z, then y, then x).  Brute force per output: exact and independent of the order of the min.  A workgroup stages a
//                 tile of whole lines in LDS and owns them, so every pass runs in place; each thread keeps kR outputs per LDS read.
//                 With unit spacing every value is an integer below 2^24: fp32 holds it exactly and the transform is bit-exact.
//   gather        sqrt (double) of the other side's EDT at this side's border voxels: fixed-grid block partials of the fp64 sum and of
//                 the maximum (summed in a fixed order afterwards: run-to-run bitwise deterministic) and a compacted list of the
//                 squared distances of both directions
//   final         per class: the fixed-order sums, then the two order statistics of the pooled list around 0.95 (n-1) by radix
//                 selection over the fp32 bit patterns (non-negative floats order like uint32) and numpy's linear interpolation
#include <math.h>
#include <algorithm>
#include "pnp_common.h"

namespace {

constexpr int kMaxExtent = 1024;
constexpr int kMaxCls = 32;
constexpr int kEdtThreads = 256;
constexpr int kR = 8;                    // outputs per thread per LDS read
constexpr int kTileFloats = 8192;        // 32 KiB of LDS per EDT workgroup (4 workgroups per CU)
constexpr int kGatherBlocks = 1024;      // fixed: the partials, and so the order of the fp64 sum, depend on nothing else
constexpr int kBlock = 256;
constexpr int kFinalThreads = 1024;
static_assert(kFinalThreads == kGatherBlocks, "final kernel reduces one partial per thread");

__device__ __forceinline__ float inf_f() { return __int_as_float(0x7f800000); }

// one output chunk of a 1-D min-plus pass: m[r] = min_j f[j * fstride] + (s (i0 + r - j))^2, r < kR
__device__ __forceinline__ void minplus_chunk(const float* f, int fstride, int n, int i0, float s, float (&m)[kR]) {
#pragma unroll
    for (int r = 0; r < kR; ++r) m[r] = inf_f();
    float cj = (float)i0;                // i0 - j, an exact integer in fp32 (|i0 - j| < 1024)
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const float fj = f[j * fstride];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const float t = (cj + (float)r) * s;           // s (i0 + r - j): exactly 0 at i = j (an fma with r * s would not be)
            m[r] = fminf(m[r], fmaf(t, t, fj));
        }
        cj -= 1.f;
    }
}

// ---- pass along z (the contiguous axis; always the first pass): T whole lines per workgroup, lanes across the outputs of a line,
// so that a wave reads one f[j] as a broadcast.  The feature set comes from `src`: a uint8 mask (BIT == 0) or bit `bit` of a
// uint32 border bitmask.
template <int BIT>
__global__ void __launch_bounds__(kEdtThreads) edt_pass_z_kernel(const void* __restrict__ src, uint32_t bit, float* __restrict__ d,
                                                                  int Z, long long nlines, int T, float s) {
    extern __shared__ float tile[];
    const long long line0 = (long long)blockIdx.x * T;
    const int nl = (int)min((long long)T, nlines - line0);
    const long long base = line0 * Z;
    for (int i = threadIdx.x; i < nl * Z; i += blockDim.x) {
        bool feat;
        if (BIT) feat = (((const uint32_t*)src)[base + i] & bit) != 0u;
        else feat = ((const uint8_t*)src)[base + i] != 0;
        tile[i] = feat ? 0.f : inf_f();
    }
    __syncthreads();
    const int nch = (Z + kR - 1) / kR;
    for (int w = threadIdx.x; w < nl * nch; w += blockDim.x) {
        const int l = w / nch, i0 = (w - l * nch) * kR;
        float m[kR];
        minplus_chunk(tile + l * Z, 1, Z, i0, s, m);
        float* out = d + base + (long long)l * Z;
#pragma unroll
        for (int r = 0; r < kR; ++r)
            if (i0 + r < Z) out[i0 + r] = m[r];
    }
}

// ---- pass along y or x: T consecutive z columns (lanes) x the whole line of n elements; f[j][lane] reads are conflict-free.
// Element j of the line of (outer, z) lies at outer * ostride + j * ls + z.
__global__ void __launch_bounds__(kEdtThreads) edt_pass_lanes_kernel(float* __restrict__ d, int n, long long ls, long long ostride, int Z,
                                                                      int T, int logT, float s) {
    extern __shared__ float tile[];
    const int z0 = blockIdx.x * T;
    const int nz = min(T, Z - z0);
    const long long base = (long long)blockIdx.y * ostride + z0;
    for (int i = threadIdx.x; i < n * T; i += blockDim.x) {
        const int j = i >> logT, t = i & (T - 1);
        tile[i] = t < nz ? d[base + j * ls + t] : inf_f();
    }
    __syncthreads();
    const int nch = (n + kR - 1) / kR;
    for (int w = threadIdx.x; w < nch * T; w += blockDim.x) {
        const int t = w & (T - 1), i0 = (w >> logT) * kR;
        if (t >= nz) continue;
        float m[kR];
        minplus_chunk(tile + t, T, n, i0, s, m);
#pragma unroll
        for (int r = 0; r < kR; ++r)
            if (i0 + r < n) d[base + (i0 + r) * ls + t] = m[r];
    }
}

// ---- border bitmasks and per-class border counts of both volumes
__device__ __forceinline__ uint32_t border_bit(const int32_t* __restrict__ lab, long long v, int x, int y, int z, int X, int Y, int Z,
                                               int ncls) {
    const int l = lab[v];
    if (l < 0 || l >= ncls) return 0u;
    const long long sy = Z, sx = (long long)Y * Z;
    const bool inner = x > 0 && x < X - 1 && y > 0 && y < Y - 1 && z > 0 && z < Z - 1;
    if (!inner) return 1u << l;                            // a neighbour outside the volume is outside the class
    const bool same = lab[v - 1] == l && lab[v + 1] == l && lab[v - sy] == l && lab[v + sy] == l && lab[v - sx] == l && lab[v + sx] == l;
    return same ? 0u : (1u << l);
}

__global__ void __launch_bounds__(kBlock) border_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt,
                                                        uint32_t* __restrict__ mp, uint32_t* __restrict__ mg,
                                                        unsigned long long* __restrict__ cls, int X, int Y, int Z, int ncls) {
    __shared__ unsigned int cnt[2][kMaxCls];
    if (threadIdx.x < 2 * kMaxCls) cnt[threadIdx.x / kMaxCls][threadIdx.x % kMaxCls] = 0u;
    __syncthreads();
    const long long V = (long long)X * Y * Z;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long long)gridDim.x * blockDim.x) {
        const unsigned vv = (unsigned)v, xy = vv / (unsigned)Z;       // V <= 2^30
        const int z = (int)(vv - xy * (unsigned)Z), y = (int)(xy % (unsigned)Y), x = (int)(xy / (unsigned)Y);
        const uint32_t bp = border_bit(pred, v, x, y, z, X, Y, Z, ncls);
        const uint32_t bg = border_bit(gt, v, x, y, z, X, Y, Z, ncls);
        mp[v] = bp;
        mg[v] = bg;
        if (bp) atomicAdd(&cnt[0][__ffs(bp) - 1], 1u);
        if (bg) atomicAdd(&cnt[1][__ffs(bg) - 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2 * ncls) {
        const int side = threadIdx.x / ncls, c = threadIdx.x % ncls;
        if (cnt[side][c]) atomicAdd(&cls[c * 3 + side], (unsigned long long)cnt[side][c]);
    }
}

// counters zeroed, row 0 (background: not a structure) NaN
__global__ void surface_init_kernel(unsigned long long* cls, int ncls, double* out) {
    const int t = threadIdx.x;
    if (t < 3 * ncls) cls[t] = 0ull;
    if (t < 7) out[t] = __longlong_as_double(0x7ff8000000000000ll);
}

// ---- gather: this side's border voxels of class `bit` read the other side's EDT
__global__ void __launch_bounds__(kBlock) gather_kernel(const uint32_t* __restrict__ mask, uint32_t bit, const float* __restrict__ edt,
                                                        long long V, float* __restrict__ list, unsigned long long* __restrict__ listcnt,
                                                        double* __restrict__ psum, float* __restrict__ pmax) {
    __shared__ double ss[kBlock];
    __shared__ float sm[kBlock];
    double acc = 0.0;
    float mx = 0.f;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    // the trip count is uniform over the block (every thread runs the rounded-up count) so that the wave-wide ballot sees every lane
    const long long vend = ((V + stride - 1) / stride) * stride;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < vend; v += stride) {
        const bool take = v < V && (mask[v] & bit) != 0u;
        const float e = take ? edt[v] : 0.f;
        const unsigned long long act = __ballot(take);
        if (act) {
            const int leader = __ffsll((long long)act) - 1;
            unsigned long long pos = 0;
            if (lane == leader) pos = atomicAdd(listcnt, (unsigned long long)__popcll(act));
            pos = __shfl(pos, leader);
            if (take) list[pos + __popcll(act & ((1ull << lane) - 1ull))] = e;
        }
        if (take) {
            acc += sqrt((double)e);
            mx = fmaxf(mx, e);
        }
    }
    ss[threadIdx.x] = acc;
    sm[threadIdx.x] = mx;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            ss[threadIdx.x] += ss[threadIdx.x + h];
            sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        psum[blockIdx.x] = ss[0];
        pmax[blockIdx.x] = sm[0];
    }
}

// radix selection of the order statistics k[0], k[1] of n non-negative floats (as uint32 bit patterns), 8 bits per round, one workgroup
__device__ void radix_select2(const uint32_t* __restrict__ u, unsigned long long n, unsigned long long k0, unsigned long long k1,
                             uint32_t* res) {
    __shared__ unsigned int hist[2][256];
    __shared__ uint32_t s_pre[2];
    __shared__ unsigned long long s_k[2];
    if (threadIdx.x == 0) {
        s_pre[0] = s_pre[1] = 0u;
        s_k[0] = k0;
        s_k[1] = k1;
    }
    const int lane = threadIdx.x & 63;
    uint32_t msk = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 512; i += blockDim.x) hist[i >> 8][i & 255] = 0u;
        __syncthreads();
        const uint32_t p0 = s_pre[0], p1 = s_pre[1];
        const unsigned long long nround = ((n + blockDim.x - 1) / blockDim.x) * blockDim.x;
        for (unsigned long long i = threadIdx.x; i < nround; i += blockDim.x) {
            const uint32_t x = i < n ? u[i] : 0u;
            const uint32_t dg = (x >> shift) & 255u;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const bool take = i < n && (x & msk) == (q ? p1 : p0);
                // wave-uniform digits (the common case: many equal distances) cost one LDS atomic per wave
                const unsigned long long act = __ballot(take);
                if (!act) continue;
                const int leader = __ffsll((long long)act) - 1;
                const uint32_t d0 = __shfl(dg, leader);
                if (__ballot(take && dg == d0) == act) {
                    if (lane == leader) atomicAdd(&hist[q][d0], (unsigned int)__popcll(act));
                } else if (take) {
                    atomicAdd(&hist[q][dg], 1u);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const int q = threadIdx.x;
            unsigned long long k = s_k[q];
            int b = 0;
            for (; b < 255; ++b) {
                if (k < hist[q][b]) break;
                k -= hist[q][b];
            }
            s_pre[q] |= (uint32_t)b << shift;
            s_k[q] = k;
        }
        msk |= 255u << shift;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        res[0] = s_pre[0];
        res[1] = s_pre[1];
    }
}

__global__ void __launch_bounds__(kFinalThreads) surface_final_kernel(const double* __restrict__ psum, const float* __restrict__ pmax,
                                                                      const unsigned long long* __restrict__ cls, const float* __restrict__ list,
                                                                      int c, double* __restrict__ out) {
    __shared__ double ss[2][kFinalThreads];
    __shared__ float sm[2][kFinalThreads];
    __shared__ uint32_t sel[2];
    const unsigned long long np = cls[c * 3 + 0], ng = cls[c * 3 + 1];
    double* row = out + (size_t)c * 7;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (np == 0 || ng == 0) {                          // an empty set: no distance is defined
        if (threadIdx.x < 7) row[threadIdx.x] = threadIdx.x == 0 ? (double)np : threadIdx.x == 1 ? (double)ng : qnan;
        return;
    }
    const int t = threadIdx.x;
    ss[0][t] = psum[t];
    ss[1][t] = psum[kGatherBlocks + t];
    sm[0][t] = pmax[t];
    sm[1][t] = pmax[kGatherBlocks + t];
    __syncthreads();
    for (int h = kFinalThreads / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                ss[q][t] += ss[q][t + h];
                sm[q][t] = fmaxf(sm[q][t], sm[q][t + h]);
            }
        }
        __syncthreads();
    }
    // numpy.percentile(..., 95), method 'linear': virtual index (n - 1) * 0.95, its floor and the next index, lerp in double
    const unsigned long long n = np + ng;
    const double vi = __dmul_rn((double)(n - 1), 0.95);
    const double lo = floor(vi);
    const unsigned long long klo = (unsigned long long)lo;
    const unsigned long long khi = klo + 1 < n ? klo + 1 : n - 1;
    radix_select2((const uint32_t*)list, n, klo, khi, sel);
    __syncthreads();
    if (t == 0) {
        const double a = sqrt((double)__uint_as_float(sel[0])), b = sqrt((double)__uint_as_float(sel[1]));
        const double g = __dsub_rn(vi, lo);
        const double diff = __dsub_rn(b, a);
        const double h95 = g >= 0.5 ? __dsub_rn(b, __dmul_rn(diff, __dsub_rn(1.0, g))) : __dadd_rn(a, __dmul_rn(diff, g));
        row[0] = (double)np;
        row[1] = (double)ng;
        row[2] = ss[0][0];
        row[3] = ss[1][0];
        row[4] = sqrt((double)sm[0][0]);
        row[5] = sqrt((double)sm[1][0]);
        row[6] = h95;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t mp, mg, edt, list, psum, pmax, cls, total;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

Layout layout_of(long long V, int ncls) {
    Layout L;
    size_t o = 0;
    L.mp = o;   o += align256((size_t)V * 4);
    L.mg = o;   o += align256((size_t)V * 4);
    L.edt = o;  o += align256((size_t)V * 4);
    L.list = o; o += align256((size_t)V * 2 * 4);        // pooled list of one class: at most every voxel once per side
    L.psum = o; o += align256((size_t)2 * kGatherBlocks * 8);
    L.pmax = o; o += align256((size_t)2 * kGatherBlocks * 4);
    L.cls = o;  o += (size_t)ncls * 3 * 8;               // per class: border count (pred, gt), list counter — unrounded tail
    L.total = o;
    return L;
}

bool extents_ok(long long X, long long Y, long long Z) {
    return X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxExtent && Y <= kMaxExtent && Z <= kMaxExtent;
}

bool spacing_ok(float s) { return isfinite(s) && s > 0.f; }

int pow2_floor(int v) {
    int p = 1;
    while (p * 2 <= v) p *= 2;
    return p;
}

// three passes: z from the feature source, then y, then x, in place in `d`
int edt3d(const void* src, bool bitmask, uint32_t bit, float* d, int X, int Y, int Z, float sx, float sy, float sz, hipStream_t st,
          const char* who) {
    const long long nlines = (long long)X * Y;
    const int Tz = std::max(1, std::min(256, kTileFloats / Z));
    const dim3 gz((unsigned)((nlines + Tz - 1) / Tz));
    const size_t ldsz = (size_t)Tz * Z * sizeof(float);
    if (bitmask) hipLaunchKernelGGL(edt_pass_z_kernel<1>, gz, dim3(kEdtThreads), ldsz, st, src, bit, d, Z, nlines, Tz, sz);
    else hipLaunchKernelGGL(edt_pass_z_kernel<0>, gz, dim3(kEdtThreads), ldsz, st, src, bit, d, Z, nlines, Tz, sz);
    PNP_CHECK_LAUNCH(who);
    // lanes across z: T columns, a power of two with T * n floats within the tile budget, no wider than z needs
    auto lanes = [&](int n, long long ls, long long ostride, int nouter, float s) -> int {
        int T = std::min(64, pow2_floor(kTileFloats / n));
        while (T > 1 && T / 2 >= Z) T /= 2;
        int logT = 0;
        while ((1 << logT) < T) ++logT;
        hipLaunchKernelGGL(edt_pass_lanes_kernel, dim3((unsigned)((Z + T - 1) / T), (unsigned)nouter), dim3(kEdtThreads),
                           (size_t)n * T * sizeof(float), st, d, n, ls, ostride, Z, T, logT, s);
        PNP_CHECK_LAUNCH(who);
        return PNP_OK;
    };
    int rc = lanes(Y, Z, (long long)Y * Z, X, sy);                 // y: lines (x, z), element stride Z
    if (rc) return rc;
    return lanes(X, (long long)Y * Z, Z, Y, sx);                  // x: lines (y, z), element stride Y * Z
}

}  // namespace

extern "C" {

int pnp_edt3d_sq(const uint8_t* mask, float* dist_sq, int64_t X, int64_t Y, int64_t Z, float sx, float sy, float sz, void* stream) {
    PNP_REQUIRE(extents_ok(X, Y, Z), "pnp_edt3d_sq: extents %lld x %lld x %lld outside [1, %d]", (long long)X, (long long)Y, (long long)Z,
                kMaxExtent);
    PNP_REQUIRE(spacing_ok(sx) && spacing_ok(sy) && spacing_ok(sz), "pnp_edt3d_sq: spacing (%g, %g, %g) must be finite and > 0", sx, sy, sz);
    PNP_REQUIRE(mask && dist_sq, "pnp_edt3d_sq: null pointer");
    return edt3d(mask, false, 0u, dist_sq, (int)X, (int)Y, (int)Z, sx, sy, sz, (hipStream_t)stream, "pnp_edt3d_sq");
}

size_t pnp_surface_workspace_bytes(int64_t X, int64_t Y, int64_t Z, int32_t ncls) {
    if (!extents_ok(X, Y, Z) || ncls < 2 || ncls > kMaxCls) return 0;
    return layout_of(X * Y * Z, ncls).total;
}

int pnp_surface_distances(const int32_t* pred, const int32_t* gt, int64_t X, int64_t Y, int64_t Z, int32_t ncls, float sx, float sy,
                          float sz, double* out, void* workspace, size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(extents_ok(X, Y, Z), "pnp_surface_distances: extents %lld x %lld x %lld outside [1, %d]", (long long)X, (long long)Y,
                (long long)Z, kMaxExtent);
    PNP_REQUIRE(ncls >= 2 && ncls <= kMaxCls, "pnp_surface_distances: ncls %d outside [2, %d]", (int)ncls, kMaxCls);
    PNP_REQUIRE(spacing_ok(sx) && spacing_ok(sy) && spacing_ok(sz), "pnp_surface_distances: spacing (%g, %g, %g) must be finite and > 0",
                sx, sy, sz);
    PNP_REQUIRE(pred && gt && out && workspace, "pnp_surface_distances: null pointer");
    const long long V = X * Y * Z;
    const Layout L = layout_of(V, ncls);
    PNP_REQUIRE(workspace_bytes >= L.total, "pnp_surface_distances: workspace %zu bytes < %zu (pnp_surface_workspace_bytes)",
                workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* mp = (uint32_t*)(ws + L.mp);
    uint32_t* mg = (uint32_t*)(ws + L.mg);
    float* edt = (float*)(ws + L.edt);
    float* list = (float*)(ws + L.list);
    double* psum = (double*)(ws + L.psum);
    float* pmax = (float*)(ws + L.pmax);
    unsigned long long* cls = (unsigned long long*)(ws + L.cls);

    hipLaunchKernelGGL(surface_init_kernel, dim3(1), dim3(128), 0, st, cls, (int)ncls, out);
    PNP_CHECK_LAUNCH("surface_init_kernel");
    const unsigned nb = (unsigned)std::min<long long>((V + kBlock - 1) / kBlock, 4096);
    hipLaunchKernelGGL(border_kernel, dim3(nb), dim3(kBlock), 0, st, pred, gt, mp, mg, cls, (int)X, (int)Y, (int)Z, (int)ncls);
    PNP_CHECK_LAUNCH("border_kernel");
    for (int c = 1; c < ncls; ++c) {
        const uint32_t bit = 1u << c;
        for (int dir = 0; dir < 2; ++dir) {
            // dir 0: prediction border -> EDT of the ground-truth border; dir 1: the other way round
            int rc = edt3d(dir == 0 ? (const void*)mg : (const void*)mp, true, bit, edt, (int)X, (int)Y, (int)Z, sx, sy, sz, st,
                           "pnp_surface_distances");
            if (rc) return rc;
            hipLaunchKernelGGL(gather_kernel, dim3(kGatherBlocks), dim3(kBlock), 0, st, dir == 0 ? mp : mg, bit, edt, V, list, cls + c * 3 + 2,
                               psum + dir * kGatherBlocks, pmax + dir * kGatherBlocks);
            PNP_CHECK_LAUNCH("gather_kernel");
        }
        hipLaunchKernelGGL(surface_final_kernel, dim3(1), dim3(kFinalThreads), 0, st, psum, pmax, cls, list, c, out);
        PNP_CHECK_LAUNCH("surface_final_kernel");
    }
    return PNP_OK;
}

}  // extern "C"
