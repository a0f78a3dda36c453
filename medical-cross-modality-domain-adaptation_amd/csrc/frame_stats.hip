// Per-frame class statistics of a resident label volume: for every frame z and class c of a uint8 volume [X, Y, Z], z
// fastest, the voxel count and the bounding box (xmin, xmax, ymin, ymax) of the voxels of frame z that carry label c — what the foreground
// sampler of volume_source.py needs to know where the classes are.
//
//   pnp_label_frame_stats        two launches: the table is initialised to "absent" (0, X, -1, Y, -1), then accumulated into
//   frame_stats_init_kernel      the initialisation, a grid-stride store
//   frame_stats_kernel<VEC>      z is the contiguous axis, so the frame of a voxel is its offset within its column.  A lane owns VEC
//                                consecutive frames (one load of VEC bytes: 16, 8 or 4 when Z is a multiple and the base is aligned so, 1
//                                otherwise — the plain path of ragged Z and misaligned bases) and KEEPS them while it walks columns; the TZ
//                                lanes next to each other cover one tile of a column's frames (at most 64 frames, blockIdx.x), the CL = 256 / TZ
//                                lane rows cover CL neighbouring columns, so a wave reads one contiguous piece of memory.  A workgroup walks
//                                the columns of its chunk (blockIdx.y) CL at a time.
//                                Reduction, in three levels.  Per lane and frame: the run of equal labels along the lane's own walk, in
//                                registers (label, count, box) — label maps are piecewise constant, and the all-one-class volume is one run
//                                per lane and frame.  Per workgroup: a run that ends goes into the tile's [frames, ncls, 5] table in LDS
//                                (int32 add / min / max).  Per grid: the entries a workgroup has seen (count > 0) go into the global table,
//                                five atomics each.
//
// int32 add / min / max only: the result does not depend on the order of arrival, i.e. it is bit-identical from run to run.
#include "pnp_common.h"

namespace {

constexpr int kMaxExtentXY = 4096;
constexpr int kMaxCls = 8;
constexpr int kThreads = 256;
// Every column chunk adds its [Z, ncls, 5] entries to the global table, whatever the tile height: the global atomics grow with the number
// of CHUNKS, not of workgroups.  So the frames are cut into tiles low enough that about two workgroups per CU need few chunks, and high
// enough that a lane row still reads 64 contiguous bytes.  Measured on an MI355X, 256 x 256 x 200, 5 classes in blocks, the call under HIP
// events: tile 256 / 512 workgroups 93 us, 64 / 512 56 us, 64 / 256 54 us, 32 / 512 71 us.
constexpr int kTileFrames = 64;           // frames of one workgroup's LDS table: 64 x 8 x 5 int32 = 10 KiB at most
constexpr int kTargetBlocks = 512;        // workgroups wanted: tiles x chunks

template <int VEC>
struct PackOf;
template <>
struct PackOf<1> {
    typedef uint8_t type;
};
template <>
struct PackOf<4> {
    typedef uint32_t type;
};
template <>
struct PackOf<8> {
    typedef uint2 type;
};
template <>
struct PackOf<16> {
    typedef uint4 type;
};

__device__ __forceinline__ uint32_t word_of(uint8_t p, int) { return p; }
__device__ __forceinline__ uint32_t word_of(uint32_t p, int) { return p; }
__device__ __forceinline__ uint32_t word_of(uint2 p, int w) { return w == 0 ? p.x : p.y; }
__device__ __forceinline__ uint32_t word_of(uint4 p, int w) { return w == 0 ? p.x : w == 1 ? p.y : w == 2 ? p.z : p.w; }

__global__ __launch_bounds__(kThreads) void frame_stats_init_kernel(int32_t* __restrict__ stats, long long entries, int X, int Y) {
    const long long step = (long long)gridDim.x * kThreads;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < entries; e += step) {
        int32_t* s = stats + e * 5;
        s[0] = 0;
        s[1] = X;
        s[2] = -1;
        s[3] = Y;
        s[4] = -1;
    }
}

// one finished run of `cnt` voxels of class `cls` -> the workgroup's entry `row` (a frame of the tile)
__device__ __forceinline__ void run_to_lds(int32_t* sm, int row, int ncls, int cls, int cnt, int xlo, int xhi, int ylo, int yhi) {
    if (cls < ncls && cnt > 0) {
        int32_t* s = sm + (row * ncls + cls) * 5;
        atomicAdd(s + 0, cnt);
        atomicMin(s + 1, xlo);
        atomicMax(s + 2, xhi);
        atomicMin(s + 3, ylo);
        atomicMax(s + 4, yhi);
    }
}

// G = Z / VEC lane groups per column; tile blockIdx.x owns the groups [blockIdx.x TZ, (blockIdx.x + 1) TZ) of every column; chunk blockIdx.y
// owns the columns [blockIdx.y cpb, (blockIdx.y + 1) cpb) of the NC = X Y columns.  TZ CL <= 256, TZ VEC <= kTileFrames.
template <int VEC>
__global__ __launch_bounds__(kThreads) void frame_stats_kernel(const uint8_t* __restrict__ label, int X, int Y, int Z, int ncls, int NC, int G,
                                                               int TZ, int CL, int cpb, int32_t* __restrict__ stats) {
    typedef typename PackOf<VEC>::type pack_t;
    extern __shared__ int32_t sm[];
    const int tid = threadIdx.x;
    const int rows = TZ * VEC;
    for (int e = tid; e < rows * ncls; e += kThreads) {
        int32_t* s = sm + e * 5;
        s[0] = 0;
        s[1] = X;
        s[2] = -1;
        s[3] = Y;
        s[4] = -1;
    }
    __syncthreads();

    const int zl = tid % TZ, cl = tid / TZ;
    const int g = blockIdx.x * TZ + zl;
    if (cl < CL && g < G) {
        // the lane's runs, one per frame it owns; 255 is never flushed (ncls <= 8), so the empty first run needs no flag
        int cur[VEC], cnt[VEC], xlo[VEC], xhi[VEC], ylo[VEC], yhi[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            cur[k] = 255;
            cnt[k] = 0;
            xlo[k] = xhi[k] = ylo[k] = yhi[k] = 0;
        }
        const int c0 = blockIdx.y * cpb;
        const int c1 = min(c0 + cpb, NC);
        const uint8_t* base = label + (size_t)g * VEC;
        for (int col = c0 + cl; col < c1; col += CL) {
            const int x = col / Y, y = col - x * Y;
            const pack_t p = *reinterpret_cast<const pack_t*>(base + (size_t)col * Z);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int l = (int)((word_of(p, k / 4) >> (8 * (k % 4))) & 0xffu);
                if (l == cur[k]) {
                    ++cnt[k];
                    xhi[k] = x;                      // the walk ascends in col, so x never decreases
                    ylo[k] = min(ylo[k], y);
                    yhi[k] = max(yhi[k], y);
                } else {
                    run_to_lds(sm, zl * VEC + k, ncls, cur[k], cnt[k], xlo[k], xhi[k], ylo[k], yhi[k]);
                    cur[k] = l;
                    cnt[k] = 1;
                    xlo[k] = xhi[k] = x;
                    ylo[k] = yhi[k] = y;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) run_to_lds(sm, zl * VEC + k, ncls, cur[k], cnt[k], xlo[k], xhi[k], ylo[k], yhi[k]);
    }
    __syncthreads();

    const int f0 = blockIdx.x * TZ * VEC;
    for (int e = tid; e < rows * ncls; e += kThreads) {
        const int32_t* s = sm + e * 5;
        const int f = f0 + e / ncls;
        if (s[0] > 0 && f < Z) {
            int32_t* d = stats + ((size_t)f * ncls + e % ncls) * 5;
            atomicAdd(d + 0, s[0]);
            atomicMin(d + 1, s[1]);
            atomicMax(d + 2, s[2]);
            atomicMin(d + 3, s[3]);
            atomicMax(d + 4, s[4]);
        }
    }
}

template <int VEC>
int launch_stats(const uint8_t* label, int X, int Y, int Z, int ncls, int32_t* stats, hipStream_t st) {
    const int NC = X * Y;                                         // <= 4096^2
    const int G = Z / VEC;
    const int ntile = pnp_cdiv(G, kTileFrames / VEC);
    const int TZ = pnp_cdiv(G, ntile);                            // <= kTileFrames / VEC <= 64: even tiles
    const int CL = kThreads / TZ;
    const int nchunk_want = ntile >= kTargetBlocks ? 1 : kTargetBlocks / ntile;
    const int cpb = CL * pnp_cdiv(pnp_cdiv(NC, nchunk_want), CL);     // a multiple of CL, so every lane row starts a chunk on its own column
    const int nchunk = pnp_cdiv(NC, cpb);                         // <= kTargetBlocks
    const size_t lds = (size_t)TZ * VEC * ncls * 5 * sizeof(int32_t);
    hipLaunchKernelGGL(frame_stats_kernel<VEC>, dim3((unsigned)ntile, (unsigned)nchunk), dim3(kThreads), lds, st, label, X, Y, Z, ncls, NC, G, TZ,
                       CL, cpb, stats);
    PNP_CHECK_LAUNCH("frame_stats_kernel");
    return PNP_OK;
}

}  // namespace

extern "C" {

int pnp_label_frame_stats(const uint8_t* label, int32_t X, int32_t Y, int32_t Z, int32_t ncls, int32_t* stats, void* stream) {
    PNP_REQUIRE(label && stats, "pnp_label_frame_stats: null pointer");
    PNP_REQUIRE(X >= 1 && Y >= 1 && X <= kMaxExtentXY && Y <= kMaxExtentXY, "pnp_label_frame_stats: X = %d, Y = %d outside [1, %d]", (int)X,
                (int)Y, kMaxExtentXY);
    PNP_REQUIRE(Z >= 1, "pnp_label_frame_stats: Z = %d must be at least 1", (int)Z);
    const long long n = (long long)X * Y * Z;
    PNP_REQUIRE(n < (1ll << 31), "pnp_label_frame_stats: X * Y * Z = %lld is not below 2^31", n);
    PNP_REQUIRE(ncls >= 1 && ncls <= kMaxCls, "pnp_label_frame_stats: ncls = %d outside [1, %d]", (int)ncls, kMaxCls);
    PNP_REQUIRE((uintptr_t)stats % 4 == 0, "pnp_label_frame_stats: stats must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long entries = (long long)Z * ncls;
    const long long want = (entries + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(frame_stats_init_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(kThreads), 0, st, stats, entries, (int)X, (int)Y);
    PNP_CHECK_LAUNCH("frame_stats_init_kernel");
    // every column starts at base + col * Z: a VEC-byte load of every lane is aligned when the base and Z are multiples of VEC
    const uintptr_t a = (uintptr_t)label;
    if (Z % 16 == 0 && a % 16 == 0) return launch_stats<16>(label, X, Y, Z, ncls, stats, st);
    if (Z % 8 == 0 && a % 8 == 0) return launch_stats<8>(label, X, Y, Z, ncls, stats, st);
    if (Z % 4 == 0 && a % 4 == 0) return launch_stats<4>(label, X, Y, Z, ncls, stats, st);
    return launch_stats<1>(label, X, Y, Z, ncls, stats, st);
}

}  // extern "C"
