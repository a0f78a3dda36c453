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
// The destination is one Box in every argument block.  paste_labels_kernel writes its columns with three hand-written loops (head bytes,
// dwords, tail bytes); the soft kernels share one frame loop with the same store paths, walk_column (with pack_label), one argument
// block, SoftArgs<MAXM> (8 or 64 members), and one host launcher: after the column prologue that decides whether the lane writes at all
// they differ in the per-frame functor they hand to the walk.  (The labels kernel on walk_column cuts a column into the same bytes and
// dwords but ran 19.0 -> 21.1 us per batch: profiles/paste_refactor.txt.)
//
//   paste_ensemble_kernel   the same lane layout and the same walk for M <= 8 members: per voxel every member's
//                         logits are interpolated through that member's own inverse map (the very expressions of label_at), passed
//                         through softmax and summed in a fixed order; the label is the first strict maximum of the sum, and on request
//                         the mean probabilities (class-major fp32 planes) and the normalised entropy go to the same element index.
//                         A member's corner data is recomputed per frame from its six kernel-argument floats: 8 members x 8 values kept
//                         per lane would be 64 VGPRs or an indexed private array (scratch); the ~30 VALU operations per member and frame
//                         stand against 4 * ncls dependent-address loads, ncls expf and ncls divisions.
//
//   paste_tiles_kernel       the same lane layout, walk and one-writer rule for M <= 64 members that each cover a PART of
//                         the box: a column is written iff at least one member covers it (a union), and the covering members' softmax is
//                         blended with a separable window that trusts a plane's centre more than its border.  Per column, once: every
//                         member's two coordinate chains, kept as one covering bit per member (two VGPRs), and the wave's union of those
//                         bits (two SGPRs).  Per frame: the wave walks the set bits of the union, so the member's pointer and map are scalar
//                         loads from the kernel-argument block, and a lane whose own bit is clear skips the member; the covering member's
//                         corner data and weight are recomputed from its six floats as above.  No accumulator volume, no atomics.
//
//   fuse_views_kernel        M <= 8 finished probability volumes of ONE grid (the views of a multi-planar prediction) -> label,
//                         weighted mean probabilities over the views that cover a voxel, normalised entropy.  Pure streaming, no map: a lane
//                         owns four consecutive elements (one float4 per plane) where the bases allow it, single elements otherwise.
#include <algorithm>
#include <math.h>

#include "pnp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxExtent = 4096;

// where a launch writes: the X x Y x nb box of voxel columns and frames z0 .. z0 + nb - 1
struct Box {
    unsigned char* vol;        // the allocation's first element
    long long origin;          // element offset of voxel (0, 0) of frame 0
    long long sx, sy, sz;      // element strides, any sign
    long long plane;           // H * W * ncls: the floats from one frame's logits to the next
    int nb, z0, X, Y;
};

struct PasteArgs {
    const float* logits;       // [B, H, W, ncls]
    Box box;
    float inv[6];
    int H, W, ncls;
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

// a column is inside the field of view iff its UNCLAMPED plane coordinates lie in [-0.5, H - 0.5] x [-0.5, W - 0.5] (NaN: outside)
__device__ __forceinline__ bool in_fov(float pi, float pj, int H, int W) {
    return pi >= -0.5f && pi <= (float)H - 0.5f && pj >= -0.5f && pj <= (float)W - 0.5f;
}

// FOV (pnp_paste_labels_fov): a column outside the field of view writes nothing; coverage does not depend on the frame, so
// the lane returns before the store paths, which are unchanged
template <bool FOV>
__global__ void __launch_bounds__(kThreads) paste_labels_kernel(const PasteArgs A) {
    const int g = blockIdx.x * kThreads + threadIdx.x;        // flat column index, y fastest (X * Y <= 2^24)
    if (g >= A.box.X * A.box.Y) return;
    const int x = g / A.box.Y, y = g - x * A.box.Y;
    float pi = fmaf(A.inv[0], (float)x, fmaf(A.inv[1], (float)y, A.inv[2]));
    float pj = fmaf(A.inv[3], (float)x, fmaf(A.inv[4], (float)y, A.inv[5]));
    if constexpr (FOV) {
        if (!in_fov(pi, pj, A.H, A.W)) return;
    }
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
    const Box& D = A.box;
    const int nb = D.nb, ncls = A.ncls;
    const long long col = D.origin + (long long)x * D.sx + (long long)y * D.sy + (long long)D.z0 * D.sz;      // frame z0 of this column
    const float* __restrict__ lg = A.logits;
    if (D.sz == 1 || D.sz == -1) {
        // t counts bytes from the lowest address: frame t (sz = 1) or nb - 1 - t (sz = -1)
        const bool up = D.sz == 1;
        unsigned char* dst = D.vol + (up ? col : col - (nb - 1));
        int t = 0;
        for (; t < nb && (((uintptr_t)(dst + t)) & 3u); ++t)
            dst[t] = (unsigned char)label_at(lg + (long long)(up ? t : nb - 1 - t) * D.plane, k, ncls);
        for (; t + 4 <= nb; t += 4) {
            unsigned int w = 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                w |= (unsigned int)label_at(lg + (long long)(up ? t + u : nb - 1 - t - u) * D.plane, k, ncls) << (8 * u);
            *(unsigned int*)(dst + t) = w;
        }
        for (; t < nb; ++t)
            dst[t] = (unsigned char)label_at(lg + (long long)(up ? t : nb - 1 - t) * D.plane, k, ncls);
    } else {
        for (int b = 0; b < nb; ++b)
            D.vol[col + (long long)b * D.sz] = (unsigned char)label_at(lg + (long long)b * D.plane, k, ncls);
    }
}

constexpr int kMaxMembers = 8;
constexpr int kGroup = 4;      // members are summed in runs of 4: see ensemble_at
constexpr int kMaxTiles = 64;

// the argument block of the soft kernels: paste_ensemble_kernel's at MAXM = kMaxMembers, paste_tiles_kernel's at kMaxTiles
template <int MAXM>
struct SoftArgs {
    const float* logits[MAXM]; // [B, H, W, ncls] each
    float inv[6 * MAXM];
    Box box;
    float* prob;               // nullable: ncls planes of vol_elems floats
    float* entropy;            // nullable: vol_elems floats
    long long vol_elems;
    float scale;               // paste_ensemble_kernel: 1.0f / M; paste_tiles_kernel: 1.0f / ramp
    int M, H, W, ncls;
};
using EnsembleArgs = SoftArgs<kMaxMembers>;
using TilesArgs = SoftArgs<kMaxTiles>;
static_assert(sizeof(TilesArgs) < 4096, "the member table travels by value in the kernel-argument block");

// the unclamped plane coordinates of voxel column (fx, fy) under the six-entry map iv: the two fmaf chains of the contract
__device__ __forceinline__ void plane_coords(const float* iv, float fx, float fy, float& pi, float& pj) {
    pi = fmaf(iv[0], fx, fmaf(iv[1], fy, iv[2]));
    pj = fmaf(iv[3], fx, fmaf(iv[4], fy, iv[5]));
}

// one member at one voxel: the logits of plane p ([H, W, NCLS]) interpolated at the unclamped coordinates (pi, pj), r[c] = expf(r_c - max r),
// returns their sum over ascending c (the softmax is r[c] / s).  Shared by paste_ensemble_kernel and paste_tiles_kernel.  Keep it free of
// contractible a * b + c pairs (every multiply-add here is an explicit fmaf): tiles_at's contract(off) does not reach inlined callees, and
// its exact-doubling property needs the same bits from every call.
template <int NCLS>
__device__ __forceinline__ float softmax_at(const float* __restrict__ p, float pi, float pj, int H, int W, float (&r)[NCLS]) {
    pi = fminf(fmaxf(pi, 0.f), (float)(H - 1));               // as paste_labels_kernel: NaN -> 0, clamped before any integer conversion
    pj = fminf(fmaxf(pj, 0.f), (float)(W - 1));
    const float fi = floorf(pi), fj = floorf(pj);
    const int i0 = (int)fi, j0 = (int)fj;
    const int i1 = min(i0 + 1, H - 1), j1 = min(j0 + 1, W - 1);
    const float ti = pi - fi, tj = pj - fj;
    const float ui = 1.f - ti, uj = 1.f - tj;
    const float* __restrict__ p00 = p + (i0 * W + j0) * NCLS;
    const float* __restrict__ p01 = p + (i0 * W + j1) * NCLS;
    const float* __restrict__ p10 = p + (i1 * W + j0) * NCLS;
    const float* __restrict__ p11 = p + (i1 * W + j1) * NCLS;
    float mx = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
        const float a = fmaf(p01[c], tj, p00[c] * uj);        // the three steps of label_at
        const float b = fmaf(p11[c], tj, p10[c] * uj);
        r[c] = fmaf(b, ti, a * ui);
        mx = c == 0 ? r[c] : fmaxf(mx, r[c]);
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
        r[c] = expf(r[c] - mx);
        s += r[c];
    }
    return s;
}

// the first strict maximum of v
template <int NCLS>
__device__ __forceinline__ int first_max(const float (&v)[NCLS]) {
    int am = 0;
    float best = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c)
        if (c == 0 || v[c] > best) {
            best = v[c];
            am = c;
        }
    return am;
}

// acc[c] = sum over the members of softmax_c(interpolated logits), frame offset `off` (floats); returns the first strict maximum of acc.
// Order of the sum: members 0 .. 3 ascending into one accumulator, members 4 .. 7 ascending into a second one, then first + second.  For
// M <= 4 that is the plain ascending sum; the split makes M = 8 copies of one member sum to exactly 8 p (p + p + p + p is exact in
// binary floating point, a run of 8 is not: 5 p and 7 p round), which the exactness of P = acc * (1 / M) for M = 8 needs.
template <int NCLS>
__device__ __forceinline__ int ensemble_at(const EnsembleArgs& A, float fx, float fy, long long off, float (&acc)[NCLS]) {
    float hi[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) acc[c] = hi[c] = 0.f;
    for (int m = 0; m < A.M; ++m) {
        float pi, pj;
        plane_coords(A.inv + 6 * m, fx, fy, pi, pj);
        float r[NCLS];
        const float s = softmax_at<NCLS>(A.logits[m] + off, pi, pj, A.H, A.W, r);
        if (m < kGroup) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) acc[c] += r[c] / s;
        } else {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) hi[c] += r[c] / s;
        }
    }
    // first_max, fused with the second run's add: as two loops the add becomes a branch, and the M = 5 launches measured 0.4 % slower
    int am = 0;
    float best = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
        if (A.M > kGroup) acc[c] += hi[c];
        if (c == 0 || acc[c] > best) {
            best = acc[c];
            am = c;
        }
    }
    return am;
}

// the normalised entropy of the probabilities P (a term with P_c == 0 contributes 0); inv_logn = 1 / logf(NCLS), 0 for NCLS == 1
template <int NCLS>
__device__ __forceinline__ float soft_entropy(const float (&P)[NCLS], float inv_logn) {
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c)
        if (P[c] > 0.f) h = fmaf(P[c], logf(P[c]), h);
    return NCLS == 1 ? 0.f : -h * inv_logn;
}

// the probabilities P and their normalised entropy of one voxel at element index e (plain dword stores, one writer per element)
template <int NCLS>
__device__ __forceinline__ void store_soft(float* prob, float* entropy, long long vol_elems, long long e, const float (&P)[NCLS], float inv_logn) {
    if (prob) {
#pragma unroll
        for (int c = 0; c < NCLS; ++c) prob[(long long)c * vol_elems + e] = P[c];
    }
    if (entropy) entropy[e] = soft_entropy<NCLS>(P, inv_logn);
}

// the z-fastest store path of the soft kernels, one label per call in address order (t counts elements from e0, the lowest address): labels
// collect in `w` at their byte lane; a word that fills all four lanes goes out as one aligned dword, the head (before the first 4-byte
// boundary) and the tail as single bytes
__device__ __forceinline__ void pack_label(unsigned char* vol, long long e0, long long e, int t, int nb, unsigned int lab, unsigned int& w, int& first) {
    const unsigned int lane = (unsigned int)((uintptr_t)(vol + e) & 3u);
    w |= lab << (8u * lane);
    if (lane == 3u || t == nb - 1) {
        if (t - first == 3) {
            *(unsigned int*)(vol + e - 3) = w;                        // lane == 3 and four labels: an aligned dword
        } else {
            for (int q = first; q <= t; ++q) vol[e0 + q] = (unsigned char)(w >> (8u * (unsigned int)((uintptr_t)(vol + e0 + q) & 3u)));
        }
        w = 0u;
        first = t + 1;
    }
}

// One voxel column (x, y) of the box: the frame loop of the soft kernels and the three store paths of paste_labels_kernel in one loop.
// at(off, e) returns the label of the frame whose logits start `off` floats into a member's batch, and stores whatever else the kernel
// writes at element e itself.  t counts elements from the lowest address when z is fastest: frame t (sz = 1) or nb - 1 - t (sz = -1);
// otherwise t is the frame.
template <class At>
__device__ __forceinline__ void walk_column(const Box& D, int x, int y, At at) {
    const int nb = D.nb;
    const long long col = D.origin + (long long)x * D.sx + (long long)y * D.sy + (long long)D.z0 * D.sz;      // frame z0 of this column
    const bool zfast = D.sz == 1 || D.sz == -1, up = D.sz != -1;
    const long long e0 = up ? col : col - (nb - 1);
    unsigned int w = 0u;
    int first = 0;
    for (int t = 0; t < nb; ++t) {
        const int b = up ? t : nb - 1 - t;
        const long long e = zfast ? e0 + t : col + (long long)b * D.sz;
        const unsigned int lab = (unsigned int)at((long long)b * D.plane, e);
        if (!zfast) {
            D.vol[e] = (unsigned char)lab;
            continue;
        }
        pack_label(D.vol, e0, e, t, nb, lab, w, first);
    }
}

// FOV (pnp_paste_ensemble_fov): a column that ANY member's map takes outside its plane writes nothing (the same two fmaf chains as
// ensemble_at, before the clamp)
template <int NCLS, bool FOV>
__global__ void __launch_bounds__(kThreads) paste_ensemble_kernel(const EnsembleArgs A) {
    const int g = blockIdx.x * kThreads + threadIdx.x;        // flat column index, y fastest, as in paste_labels_kernel
    if (g >= A.box.X * A.box.Y) return;
    const int x = g / A.box.Y, y = g - x * A.box.Y;
    const float fx = (float)x, fy = (float)y;
    if constexpr (FOV) {
        for (int m = 0; m < A.M; ++m) {
            float pi, pj;
            plane_coords(A.inv + 6 * m, fx, fy, pi, pj);
            if (!in_fov(pi, pj, A.H, A.W)) return;
        }
    }
    const bool soft = A.prob || A.entropy;
    const float inv_logn = NCLS > 1 ? 1.f / logf((float)NCLS) : 0.f;
    walk_column(A.box, x, y, [&](long long off, long long e) {
        float acc[NCLS];
        const int lab = ensemble_at<NCLS>(A, fx, fy, off, acc);
        if (soft) {
            float P[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) P[c] = acc[c] * A.scale;
            store_soft<NCLS>(A.prob, A.entropy, A.vol_elems, e, P, inv_logn);
        }
        return lab;
    });
}

// ---- tiled inference (pnp_paste_tiles) ---------------------------------------------------------------------------------------
// g(p; n) = min(1, max(d, 0.5) / ramp), d = min(p + 0.5, (n - 0.5) - p): the distance to the nearer border of the field of view in plane
// pixels, at least half a pixel, over the ramp.  Inside the field of view 0.5 / ramp <= g <= 1.  (No a * b + c pair here either: see softmax_at.)
__device__ __forceinline__ float window(float p, int n, float inv_ramp) {
    const float d = fminf(p + 0.5f, ((float)n - 0.5f) - p);
    return fminf(1.f, fmaxf(d, 0.5f) * inv_ramp);
}

// acc[c] = sum of w_m softmax_c(member m) and wsum = sum of w_m over the members whose bit is set in `mine`, ascending m, each product
// rounded before its sum: contraction is switched off for this function's own arithmetic (the compiler otherwise fuses w q + acc for
// some classes and not for others), so equal members give equal acc_c and a member given twice doubles acc and wsum exactly.  `wave` is
// the union of the wave's masks: m, the member's pointer and its map are wave-uniform.  Returns the first strict maximum of acc.
template <int NCLS>
__device__ __forceinline__ int tiles_at(const TilesArgs& A, unsigned long long wave, unsigned long long mine, float fx, float fy, long long off,
                                        float (&acc)[NCLS], float& wsum) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < NCLS; ++c) acc[c] = 0.f;
    wsum = 0.f;
    for (unsigned long long rest = wave; rest; rest &= rest - 1ull) {
        const int m = __builtin_ctzll(rest);
        if (!((mine >> m) & 1ull)) continue;
        float pi, pj;
        plane_coords(A.inv + 6 * m, fx, fy, pi, pj);
        const float wm = window(pi, A.H, A.scale) * window(pj, A.W, A.scale);
        float r[NCLS];
        const float s = softmax_at<NCLS>(A.logits[m] + off, pi, pj, A.H, A.W, r);
#pragma unroll
        for (int c = 0; c < NCLS; ++c) acc[c] += wm * (r[c] / s);
        wsum += wm;
    }
    return first_max<NCLS>(acc);
}

template <int NCLS>
__global__ void __launch_bounds__(kThreads) paste_tiles_kernel(const TilesArgs A) {
    const int g = blockIdx.x * kThreads + threadIdx.x;        // flat column index, y fastest, as in paste_labels_kernel
    if (g >= A.box.X * A.box.Y) return;
    const int x = g / A.box.Y, y = g - x * A.box.Y;
    const float fx = (float)x, fy = (float)y;
    // coverage depends on the column only: one bit per member, once
    unsigned long long mine = 0ull, wave = 0ull;
    for (int m = 0; m < A.M; ++m) {
        float pi, pj;
        plane_coords(A.inv + 6 * m, fx, fy, pi, pj);
        const bool in = in_fov(pi, pj, A.H, A.W);
        if (in) mine |= 1ull << m;
        if (__builtin_amdgcn_ballot_w64(in)) wave |= 1ull << m;
    }
    if (!mine) return;                                        // covered by no member: nothing of vol, prob, entropy is written
    const bool soft = A.prob || A.entropy;
    const float inv_logn = NCLS > 1 ? 1.f / logf((float)NCLS) : 0.f;
    walk_column(A.box, x, y, [&](long long off, long long e) {
        float acc[NCLS], wsum;
        const int lab = tiles_at<NCLS>(A, wave, mine, fx, fy, off, acc, wsum);
        if (soft) {
            float P[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) P[c] = acc[c] / wsum;
            store_soft<NCLS>(A.prob, A.entropy, A.vol_elems, e, P, inv_logn);
        }
        return lab;
    });
}

// ---- multi-planar fusion (pnp_fuse_views) ------------------------------------------------------------------------------------
constexpr int kMaxViews = 8;
constexpr int kFuseBlocks = 2048;          // 256 CUs x 8 blocks of 256 threads: the grid of a pass, the rest is the grid's stride

struct FuseArgs {
    const float* probs[kMaxViews];         // ncls planes of vol_elems floats each
    float w[kMaxViews];
    unsigned char* label;
    float* prob;               // nullable; may be probs[0]
    float* entropy;            // nullable
    long long vol_elems;
    long long head;            // elements before the first 16-byte boundary of the float planes (0 without the wide path)
    long long nvec;            // groups of four elements from `head` on that go through 16-byte accesses (0: everything is scalar)
    int n_views;
    int label_word;            // label + head is 4-byte aligned: a group's four labels go out as one dword
};

// one element's accumulators: add(p, w) takes view v's NCLS values and its weight, v ascending.  Products are rounded
// before their sum (no contraction, as in tiles_at): classes that are bit-identical in every view stay bit-identical in acc.
template <int NCLS>
struct Fuse {
    float acc[NCLS];
    float wsum;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int c = 0; c < NCLS; ++c) acc[c] = 0.f;
        wsum = 0.f;
    }
    __device__ __forceinline__ void add(const float (&p)[NCLS], float w) {
#pragma clang fp contract(off)
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) s += p[c];
        if (s > 0.5f) {                    // the view covers this element (a NaN sum does not)
#pragma unroll
            for (int c = 0; c < NCLS; ++c) acc[c] += w * p[c];
            wsum += w;
        }
    }
    // P (all 0 where no view covers) and the first strict maximum of P
    __device__ __forceinline__ int finish(float (&P)[NCLS]) const {
#pragma unroll
        for (int c = 0; c < NCLS; ++c) P[c] = wsum > 0.f ? acc[c] / wsum : 0.f;
        return first_max<NCLS>(P);
    }
    // store_soft's entropy of P; +0 where no view covers
    __device__ __forceinline__ float entropy(const float (&P)[NCLS], float inv_logn) const {
        return wsum > 0.f ? soft_entropy<NCLS>(P, inv_logn) : 0.f;
    }
};

// Work items of the wide path: group i covers elements head + 4 i .. head + 4 i + 3, every plane read and written as one float4 per lane
// (consecutive lanes, consecutive groups: 1 KiB per wave and instruction).  The scalar items are the `head` elements before the groups
// and the tail after them — all elements when the bases or vol_elems do not allow 16-byte accesses — one element per lane and pass.
// Every lane reads all inputs of its elements before its first store: prob may be probs[0].
template <int NCLS>
__global__ void __launch_bounds__(kThreads) fuse_views_kernel(const FuseArgs A) {
    const long long stride = (long long)gridDim.x * kThreads;
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const float inv_logn = NCLS > 1 ? 1.f / logf((float)NCLS) : 0.f;
    const long long n = A.vol_elems;
    for (long long i = gid; i < A.nvec; i += stride) {
        const long long e = A.head + 4 * i;
        Fuse<NCLS> f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u].clear();
        for (int v = 0; v < A.n_views; ++v) {
            float4 q[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) q[c] = *(const float4*)(A.probs[v] + (long long)c * n + e);
            const float w = A.w[v];
            float p[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = q[c].x;
            f[0].add(p, w);
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = q[c].y;
            f[1].add(p, w);
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = q[c].z;
            f[2].add(p, w);
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = q[c].w;
            f[3].add(p, w);
        }
        float P[4][NCLS], h[4];
        unsigned int lab = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lab |= (unsigned int)f[u].finish(P[u]) << (8 * u);
            h[u] = f[u].entropy(P[u], inv_logn);
        }
        if (A.prob) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) *(float4*)(A.prob + (long long)c * n + e) = make_float4(P[0][c], P[1][c], P[2][c], P[3][c]);
        }
        if (A.entropy) *(float4*)(A.entropy + e) = make_float4(h[0], h[1], h[2], h[3]);
        if (A.label_word) {
            *(unsigned int*)(A.label + e) = lab;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) A.label[e + u] = (unsigned char)(lab >> (8 * u));
        }
    }
    const long long body_end = A.head + 4 * A.nvec, nscalar = n - 4 * A.nvec;
    for (long long i = gid; i < nscalar; i += stride) {
        const long long e = i < A.head ? i : body_end + (i - A.head);
        Fuse<NCLS> f;
        f.clear();
        for (int v = 0; v < A.n_views; ++v) {
            float p[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = A.probs[v][(long long)c * n + e];
            f.add(p, A.w[v]);
        }
        float P[NCLS];
        A.label[e] = (unsigned char)f.finish(P);
        store_soft<NCLS>(A.prob, nullptr, n, e, P, inv_logn);
        if (A.entropy) A.entropy[e] = f.entropy(P, inv_logn);
    }
}

long long abs_ll(long long v) { return v < 0 ? -v : v; }

// the argument checks both entry points share (everything but the null pointers), with the caller's name in the text
int check_paste(const char* who, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0, int32_t X, int32_t Y, int64_t vol_elems,
                int64_t origin, int64_t sx, int64_t sy, int64_t sz) {
    PNP_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: logits [%d, %d, %d] must be at least [1, 1, 1]", who, (int)B, (int)H, (int)W);
    PNP_REQUIRE(X >= 1 && Y >= 1, "%s: source extents %d x %d must be at least 1 x 1", who, (int)X, (int)Y);
    PNP_REQUIRE(H <= kMaxExtent && W <= kMaxExtent, "%s: output plane %d x %d above %d", who, (int)H, (int)W, kMaxExtent);
    PNP_REQUIRE(X <= kMaxExtent && Y <= kMaxExtent, "%s: source extents %d x %d above %d", who, (int)X, (int)Y, kMaxExtent);
    PNP_REQUIRE(ncls >= 1 && ncls <= MAXC, "%s: ncls %d outside [1, %d]", who, (int)ncls, MAXC);
    PNP_REQUIRE(nb >= 1 && nb <= B, "%s: nb = %d outside [1, B = %d]", who, (int)nb, (int)B);
    PNP_REQUIRE(z0 >= 0, "%s: z0 = %d is negative", who, (int)z0);
    PNP_REQUIRE(vol_elems >= 1, "%s: vol_elems = %lld, at least one element is needed", who, (long long)vol_elems);
    // the extreme corners of the box, in 128-bit integers: a stride is any int64
    const __int128 ext[3] = {X - 1, Y - 1, nb - 1};
    const __int128 str[3] = {sx, sy, sz};
    __int128 lo = (__int128)origin + (__int128)z0 * sz, hi = lo;
    for (int d = 0; d < 3; ++d) {
        const __int128 span = ext[d] * str[d];
        if (span < 0) lo += span; else hi += span;
    }
    PNP_REQUIRE(lo >= 0 && hi < (__int128)vol_elems, "%s: the box addresses elements outside [0, %lld) (origin %lld, strides %lld %lld %lld)", who,
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
        PNP_REQUIRE((__int128)as[d] >= need, "%s: strides %lld %lld %lld let two voxels of a %d x %d x %d box collide", who,
                    (long long)sx, (long long)sy, (long long)sz, (int)X, (int)Y, (int)nb);
        need = (__int128)as[d] * ae[d];
    }
    return PNP_OK;
}

// the destination of a checked call, and its grid: one lane per voxel column
Box make_box(uint8_t* vol, int64_t origin, int64_t sx, int64_t sy, int64_t sz, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0,
             int32_t X, int32_t Y) {
    Box D;
    D.vol = vol;
    D.origin = origin;
    D.sx = sx; D.sy = sy; D.sz = sz;
    D.plane = (long long)H * W * ncls;
    D.nb = nb; D.z0 = z0; D.X = X; D.Y = Y;
    return D;
}
unsigned column_blocks(const Box& D) { return (unsigned)(((long long)D.X * D.Y + kThreads - 1) / kThreads); }

// launches KERNEL<ncls, ...> (the further template arguments follow the kernel's name) on `blocks` blocks with the argument block A
#define PNP_LAUNCH_CASE(n, KERNEL, ...) \
    case n: hipLaunchKernelGGL((KERNEL<n, ##__VA_ARGS__>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, A); break;
#define PNP_LAUNCH_NCLS(...)                                                                                                \
    switch (ncls) {                                                                                                         \
        PNP_LAUNCH_CASE(1, __VA_ARGS__) PNP_LAUNCH_CASE(2, __VA_ARGS__) PNP_LAUNCH_CASE(3, __VA_ARGS__) PNP_LAUNCH_CASE(4, __VA_ARGS__) \
        PNP_LAUNCH_CASE(5, __VA_ARGS__) PNP_LAUNCH_CASE(6, __VA_ARGS__) PNP_LAUNCH_CASE(7, __VA_ARGS__) PNP_LAUNCH_CASE(8, __VA_ARGS__) \
    }

// the two label entry points: the same checks, arguments and launch, with and without the field-of-view rule
template <bool FOV>
int paste_labels_launch(const char* who, const float* logits, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0,
                        const float* inv, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy,
                        int64_t sz, void* stream) {
    PNP_REQUIRE(logits && inv && vol, "%s: null pointer", who);
    if (const int rc = check_paste(who, B, H, W, ncls, nb, z0, X, Y, vol_elems, origin, sx, sy, sz)) return rc;
    PasteArgs A;
    A.logits = logits;
    A.box = make_box(vol, origin, sx, sy, sz, H, W, ncls, nb, z0, X, Y);
    for (int i = 0; i < 6; ++i) A.inv[i] = inv[i];
    A.H = H; A.W = W; A.ncls = ncls;
    hipLaunchKernelGGL(paste_labels_kernel<FOV>, dim3(column_blocks(A.box)), dim3(kThreads), 0, (hipStream_t)stream, A);
    PNP_CHECK_LAUNCH("paste_labels_kernel");
    return PNP_OK;
}

// the three soft entry points: the same checks, member table, box and grid.  pnp_paste_tiles alone has 64 member slots, takes `ramp`
// (checked between the member checks and check_paste; 1 / ramp is its `scale`, 1 / M the ensemble's, whose entry points pass a ramp
// that is not read) and launches paste_tiles_kernel.
enum class Soft { Ensemble, EnsembleFov, Tiles };
template <Soft KIND>
int paste_soft_launch(const char* who, int32_t M, const float* const* logits, const float* inv, float ramp, int32_t B, int32_t H, int32_t W,
                      int32_t ncls, int32_t nb, int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx,
                      int64_t sy, int64_t sz, float* prob, float* entropy, void* stream) {
    constexpr bool tiles = KIND == Soft::Tiles;
    constexpr int MAXM = tiles ? kMaxTiles : kMaxMembers;
    PNP_REQUIRE(M >= 1 && M <= MAXM, "%s: M = %d members outside [1, %d]", who, (int)M, MAXM);
    PNP_REQUIRE(logits && vol, "%s: null pointer", who);
    PNP_REQUIRE(inv, "%s: null inv (6 floats per member)", who);
    for (int m = 0; m < M; ++m) PNP_REQUIRE(logits[m], "%s: member %d of %d is a null pointer", who, m, (int)M);
    if constexpr (tiles)
        PNP_REQUIRE(std::isfinite(ramp) && ramp >= 1.f, "%s: ramp = %g must be finite and at least 1 (plane pixels)", who, (double)ramp);
    if (const int rc = check_paste(who, B, H, W, ncls, nb, z0, X, Y, vol_elems, origin, sx, sy, sz)) return rc;
    PNP_REQUIRE((__int128)ncls * vol_elems <= (__int128)INT64_MAX, "%s: ncls * vol_elems = %d * %lld overflows int64", who, (int)ncls,
                (long long)vol_elems);
    SoftArgs<MAXM> A;
    for (int m = 0; m < MAXM; ++m) {                          // unused slots repeat member 0
        A.logits[m] = logits[m < M ? m : 0];
        for (int i = 0; i < 6; ++i) A.inv[6 * m + i] = inv[6 * (m < M ? m : 0) + i];
    }
    A.box = make_box(vol, origin, sx, sy, sz, H, W, ncls, nb, z0, X, Y);
    A.prob = prob;
    A.entropy = entropy;
    A.vol_elems = vol_elems;
    A.scale = 1.0f / (tiles ? ramp : (float)M);
    A.M = M; A.H = H; A.W = W; A.ncls = ncls;
    const unsigned blocks = column_blocks(A.box);
    if constexpr (tiles) {
        PNP_LAUNCH_NCLS(paste_tiles_kernel)
    } else {
        PNP_LAUNCH_NCLS(paste_ensemble_kernel, KIND == Soft::EnsembleFov)
    }
    PNP_CHECK_LAUNCH(tiles ? "paste_tiles_kernel" : "paste_ensemble_kernel");
    return PNP_OK;
}

int fuse_views_launch(const char* who, int32_t n_views, const float* const* probs, const float* weights, int32_t ncls, int64_t vol_elems,
                      uint8_t* label, float* prob, float* entropy, void* stream) {
    PNP_REQUIRE(n_views >= 1 && n_views <= kMaxViews, "%s: n_views = %d outside [1, %d]", who, (int)n_views, kMaxViews);
    PNP_REQUIRE(ncls >= 1 && ncls <= MAXC, "%s: ncls %d outside [1, %d]", who, (int)ncls, MAXC);
    PNP_REQUIRE(vol_elems >= 1, "%s: vol_elems = %lld, at least one element is needed", who, (long long)vol_elems);
    PNP_REQUIRE((__int128)ncls * vol_elems * 4 <= (__int128)INT64_MAX, "%s: ncls * vol_elems = %d * %lld floats overflow int64", who, (int)ncls,
                (long long)vol_elems);
    PNP_REQUIRE(probs && label, "%s: null pointer", who);
    for (int v = 0; v < n_views; ++v) {
        PNP_REQUIRE(probs[v], "%s: view %d of %d is a null pointer", who, v, (int)n_views);
        if (weights)
            PNP_REQUIRE(std::isfinite(weights[v]) && weights[v] > 0.f, "%s: weight %d = %g must be positive and finite", who, v, (double)weights[v]);
    }
    uintptr_t low = (uintptr_t)prob | (uintptr_t)entropy;             // a null pointer adds no bits
    for (int v = 0; v < n_views; ++v) low |= (uintptr_t)probs[v];
    PNP_REQUIRE((low & 3u) == 0, "%s: a float buffer is not aligned to 4 bytes", who);
    // byte ranges of every buffer: the views, then prob, entropy, label.  prob == probs[0] is the one overlap that is served.
    struct Range { uintptr_t lo, hi; const char* name; };
    Range r[kMaxViews + 3];
    int nr = 0;
    const uintptr_t planes = (uintptr_t)ncls * (uintptr_t)vol_elems * 4u;
    for (int v = 0; v < n_views; ++v) r[nr++] = {(uintptr_t)probs[v], (uintptr_t)probs[v] + planes, "a view"};
    if (prob) r[nr++] = {(uintptr_t)prob, (uintptr_t)prob + planes, "prob"};
    if (entropy) r[nr++] = {(uintptr_t)entropy, (uintptr_t)entropy + (uintptr_t)vol_elems * 4u, "entropy"};
    r[nr++] = {(uintptr_t)label, (uintptr_t)label + (uintptr_t)vol_elems, "label"};
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b) {
            if (a == 0 && prob && b == n_views && r[a].lo == r[b].lo) continue;
            PNP_REQUIRE(r[a].hi <= r[b].lo || r[b].hi <= r[a].lo, "%s: %s overlaps %s (buffers %d and %d; only prob == probs[0] may alias)", who,
                        r[a].name, r[b].name, a, b);
        }
    FuseArgs A;
    for (int v = 0; v < kMaxViews; ++v) {
        A.probs[v] = probs[v < n_views ? v : 0];
        A.w[v] = weights && v < n_views ? weights[v] : 1.f;
    }
    A.label = label;
    A.prob = prob;
    A.entropy = entropy;
    A.vol_elems = vol_elems;
    A.n_views = n_views;
    // 16-byte accesses need every float plane on one phase of the 16-byte grid: bases that differ from a boundary by the same number of
    // floats (float-aligned at least), and planes a multiple of four floats apart (or a single plane).  `head` elements lead up to it.
    bool wide = ncls == 1 || vol_elems % 4 == 0;
    const uintptr_t phase = (uintptr_t)A.probs[0] & 15u;
    for (int v = 0; v < n_views && wide; ++v) wide = ((uintptr_t)A.probs[v] & 15u) == phase;
    if (prob) wide = wide && ((uintptr_t)prob & 15u) == phase;
    if (entropy) wide = wide && ((uintptr_t)entropy & 15u) == phase;
    A.head = wide ? (long long)(((16u - phase) & 15u) / 4u) : 0;
    if (A.head > vol_elems) A.head = vol_elems;
    A.nvec = wide ? (vol_elems - A.head) / 4 : 0;
    A.label_word = (((uintptr_t)label + (uintptr_t)A.head) & 3u) == 0;
    const long long items = std::max(A.nvec, vol_elems - 4 * A.nvec);
    const unsigned blocks = (unsigned)std::min<long long>((items + kThreads - 1) / kThreads, kFuseBlocks);
    PNP_LAUNCH_NCLS(fuse_views_kernel)
    PNP_CHECK_LAUNCH("fuse_views_kernel");
    return PNP_OK;
}

}  // namespace

extern "C" {

int pnp_fuse_views(int32_t n_views, const float* const* probs, const float* weights, int32_t ncls, int64_t vol_elems, uint8_t* label,
                   float* prob, float* entropy, void* stream) {
    return fuse_views_launch("pnp_fuse_views", n_views, probs, weights, ncls, vol_elems, label, prob, entropy, stream);
}

int pnp_paste_labels(const float* logits, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0, const float* inv,
                     int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                     void* stream) {
    return paste_labels_launch<false>("pnp_paste_labels", logits, B, H, W, ncls, nb, z0, inv, X, Y, vol, vol_elems, origin, sx, sy, sz, stream);
}

int pnp_paste_labels_fov(const float* logits, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0, const float* inv,
                         int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                         void* stream) {
    return paste_labels_launch<true>("pnp_paste_labels_fov", logits, B, H, W, ncls, nb, z0, inv, X, Y, vol, vol_elems, origin, sx, sy, sz, stream);
}

int pnp_paste_ensemble(int32_t M, const float* const* logits, const float* inv, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb,
                       int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                       float* prob, float* entropy, void* stream) {
    return paste_soft_launch<Soft::Ensemble>("pnp_paste_ensemble", M, logits, inv, 0.f, B, H, W, ncls, nb, z0, X, Y, vol, vol_elems, origin, sx, sy,
                                             sz, prob, entropy, stream);
}

int pnp_paste_ensemble_fov(int32_t M, const float* const* logits, const float* inv, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb,
                           int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                           float* prob, float* entropy, void* stream) {
    return paste_soft_launch<Soft::EnsembleFov>("pnp_paste_ensemble_fov", M, logits, inv, 0.f, B, H, W, ncls, nb, z0, X, Y, vol, vol_elems, origin,
                                                sx, sy, sz, prob, entropy, stream);
}

int pnp_paste_tiles(int32_t M, const float* const* logits, const float* inv, float ramp, int32_t B, int32_t H, int32_t W, int32_t ncls,
                    int32_t nb, int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy,
                    int64_t sz, float* prob, float* entropy, void* stream) {
    return paste_soft_launch<Soft::Tiles>("pnp_paste_tiles", M, logits, inv, ramp, B, H, W, ncls, nb, z0, X, Y, vol, vol_elems, origin, sx, sy, sz,
                                          prob, entropy, stream);
}

}  // extern "C"
