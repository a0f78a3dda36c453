// Volume inference, the way back: logits on the network's [H, W] plane -> labels on the scan's own grid.
//
//   paste_labels_kernel   one launch per batch: a lane owns one voxel column (x, y) of the slicing order and walks the batch's nb frames.
//                         Per column, once: the output-plane coordinates (two explicit fmaf chains), the clamp, the four corner offsets
//                         and the two weights.  Per frame: every class's logit interpolated bilinearly between the four corners, the
//                         first strict maximum, one byte.
//
// Lanes adjacent in a wave are adjacent in y (y fastest over the flat column index), so they read adjacent w of the logits: 4 * ncls
// contiguous bytes per corner and lane, one contiguous run per corner row and wave.  Stores, by the destination's stride pattern:
//   |sz| == 1 (z fastest: the array order of a NIfTI reader)   the lane's nb bytes are contiguous; it computes them in ADDRESS order
//                         (frames descending when sz = -1), stores single bytes up to the first 4-byte boundary, then packed dwords, then
//                         the remaining bytes: z0 and the column base are not aligned in general.
//   otherwise (the file stores the slicing axis first)          one byte per frame and lane; with |sy| == 1 a wave's 64 lanes write 64
//                         adjacent bytes with one store instruction.
// Every output element has exactly one writer (the host refuses strides under which two voxels collide): no atomics.
#include <algorithm>
#include <math.h>

#include "pnp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxExtent = 4096;
constexpr int MAXC = 8;        // loss_optim.hip's

struct PasteArgs {
    const float* logits;       // [B, H, W, ncls]
    unsigned char* vol;        // the allocation's first element
    long long origin;          // element offset of voxel (0, 0) of frame 0
    long long sx, sy, sz;      // element strides, any sign
    long long plane;           // H * W * ncls
    float inv[6];
    int H, W, ncls, nb, z0, X, Y;
};

struct Corners {
    int o00, o01, o10, o11;    // float offsets inside one [H, W, ncls] plane
    float ti, tj, ui, uj;
};

__device__ __forceinline__ int label_at(const float* __restrict__ p, const Corners& k, int ncls) {
    int am = 0;
    float best = 0.f;
    for (int c = 0; c < ncls; ++c) {
        const float a = fmaf(p[k.o01 + c], k.tj, p[k.o00 + c] * k.uj);        // along j at i0
        const float b = fmaf(p[k.o11 + c], k.tj, p[k.o10 + c] * k.uj);        // along j at i1
        const float r = fmaf(b, k.ti, a * k.ui);
        if (c == 0 || r > best) {
            best = r;
            am = c;
        }
    }
    return am;
}

__global__ void __launch_bounds__(kThreads) paste_labels_kernel(const PasteArgs A) {
    const int g = blockIdx.x * kThreads + threadIdx.x;        // flat column index, y fastest (X * Y <= 2^24)
    if (g >= A.X * A.Y) return;
    const int x = g / A.Y, y = g - x * A.Y;
    float pi = fmaf(A.inv[0], (float)x, fmaf(A.inv[1], (float)y, A.inv[2]));
    float pj = fmaf(A.inv[3], (float)x, fmaf(A.inv[4], (float)y, A.inv[5]));
    pi = fminf(fmaxf(pi, 0.f), (float)(A.H - 1));             // fmaxf(NaN, 0) = 0: clamped before any integer conversion
    pj = fminf(fmaxf(pj, 0.f), (float)(A.W - 1));
    const float fi = floorf(pi), fj = floorf(pj);
    const int i0 = (int)fi, j0 = (int)fj;
    const int i1 = min(i0 + 1, A.H - 1), j1 = min(j0 + 1, A.W - 1);
    Corners k;
    k.ti = pi - fi;                                           // exact
    k.tj = pj - fj;
    k.ui = 1.f - k.ti;
    k.uj = 1.f - k.tj;
    k.o00 = (i0 * A.W + j0) * A.ncls;
    k.o01 = (i0 * A.W + j1) * A.ncls;
    k.o10 = (i1 * A.W + j0) * A.ncls;
    k.o11 = (i1 * A.W + j1) * A.ncls;
    const int nb = A.nb, ncls = A.ncls;
    const long long col = A.origin + (long long)x * A.sx + (long long)y * A.sy + (long long)A.z0 * A.sz;      // frame z0 of this column
    const float* __restrict__ lg = A.logits;
    if (A.sz == 1 || A.sz == -1) {
        // t counts bytes from the lowest address: frame t (sz = 1) or nb - 1 - t (sz = -1)
        const bool up = A.sz == 1;
        unsigned char* dst = A.vol + (up ? col : col - (nb - 1));
        int t = 0;
        for (; t < nb && (((uintptr_t)(dst + t)) & 3u); ++t)
            dst[t] = (unsigned char)label_at(lg + (long long)(up ? t : nb - 1 - t) * A.plane, k, ncls);
        for (; t + 4 <= nb; t += 4) {
            unsigned int w = 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                w |= (unsigned int)label_at(lg + (long long)(up ? t + u : nb - 1 - t - u) * A.plane, k, ncls) << (8 * u);
            *(unsigned int*)(dst + t) = w;
        }
        for (; t < nb; ++t)
            dst[t] = (unsigned char)label_at(lg + (long long)(up ? t : nb - 1 - t) * A.plane, k, ncls);
    } else {
        for (int b = 0; b < nb; ++b)
            A.vol[col + (long long)b * A.sz] = (unsigned char)label_at(lg + (long long)b * A.plane, k, ncls);
    }
}

long long abs_ll(long long v) { return v < 0 ? -v : v; }

}  // namespace

extern "C" {

int pnp_paste_labels(const float* logits, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0, const float* inv,
                     int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                     void* stream) {
    PNP_REQUIRE(logits && inv && vol, "pnp_paste_labels: null pointer");
    PNP_REQUIRE(B >= 1 && H >= 1 && W >= 1, "pnp_paste_labels: logits [%d, %d, %d] must be at least [1, 1, 1]", (int)B, (int)H, (int)W);
    PNP_REQUIRE(X >= 1 && Y >= 1, "pnp_paste_labels: source extents %d x %d must be at least 1 x 1", (int)X, (int)Y);
    PNP_REQUIRE(H <= kMaxExtent && W <= kMaxExtent, "pnp_paste_labels: output plane %d x %d above %d", (int)H, (int)W, kMaxExtent);
    PNP_REQUIRE(X <= kMaxExtent && Y <= kMaxExtent, "pnp_paste_labels: source extents %d x %d above %d", (int)X, (int)Y, kMaxExtent);
    PNP_REQUIRE(ncls >= 1 && ncls <= MAXC, "pnp_paste_labels: ncls %d outside [1, %d]", (int)ncls, MAXC);
    PNP_REQUIRE(nb >= 1 && nb <= B, "pnp_paste_labels: nb = %d outside [1, B = %d]", (int)nb, (int)B);
    PNP_REQUIRE(z0 >= 0, "pnp_paste_labels: z0 = %d is negative", (int)z0);
    PNP_REQUIRE(vol_elems >= 1, "pnp_paste_labels: vol_elems = %lld, at least one element is needed", (long long)vol_elems);
    // the extreme corners of the box, in 128-bit integers: a stride is any int64
    const __int128 ext[3] = {X - 1, Y - 1, nb - 1};
    const __int128 str[3] = {sx, sy, sz};
    __int128 lo = (__int128)origin + (__int128)z0 * sz, hi = lo;
    for (int d = 0; d < 3; ++d) {
        const __int128 span = ext[d] * str[d];
        if (span < 0) lo += span; else hi += span;
    }
    PNP_REQUIRE(lo >= 0 && hi < (__int128)vol_elems, "pnp_paste_labels: the box addresses elements outside [0, %lld) (origin %lld, strides %lld %lld %lld)",
                (long long)vol_elems, (long long)origin, (long long)sx, (long long)sy, (long long)sz);
    // one writer per element: over the axes of extent > 1, sorted by |stride|, each stride covers the whole run of the one before it
    long long as[3];
    long long ae[3];
    int n = 0;
    const long long full[3] = {X, Y, nb};
    for (int d = 0; d < 3; ++d)
        if (full[d] > 1) {
            as[n] = abs_ll((long long)str[d]);        // |stride| <= vol_elems here: the corner check passed with extent > 1
            ae[n] = full[d];
            ++n;
        }
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (as[b] < as[a]) {
                std::swap(as[a], as[b]);
                std::swap(ae[a], ae[b]);
            }
    __int128 need = 1;
    for (int d = 0; d < n; ++d) {
        PNP_REQUIRE((__int128)as[d] >= need, "pnp_paste_labels: strides %lld %lld %lld let two voxels of a %d x %d x %d box collide",
                    (long long)sx, (long long)sy, (long long)sz, (int)X, (int)Y, (int)nb);
        need = (__int128)as[d] * ae[d];
    }
    PasteArgs A;
    A.logits = logits;
    A.vol = vol;
    A.origin = origin;
    A.sx = sx; A.sy = sy; A.sz = sz;
    A.plane = (long long)H * W * ncls;
    for (int i = 0; i < 6; ++i) A.inv[i] = inv[i];
    A.H = H; A.W = W; A.ncls = ncls; A.nb = nb; A.z0 = z0; A.X = X; A.Y = Y;
    const unsigned blocks = (unsigned)(((long long)X * Y + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(paste_labels_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, A);
    PNP_CHECK_LAUNCH("paste_labels_kernel");
    return PNP_OK;
}

}  // extern "C"
