// boundary.hip — the boundary loss of Kervadec et al. (MIDL 2019) on the segmenter's logits (not in the reference):
// signed distance maps of the one-hot labels of a batch, computed on the device every step, and the loss / gradient pass over them.
//
//   phi_c(h, w) = d outside class c, -(d - 1) inside it;  d = Euclidean distance in pixels to the nearest pixel of the same slice whose
//                 membership in c differs (one_hot2dist of the paper's code); 0 where the class is absent from or fills the slice
//   p_i = softmax(z_i),  s_i = sum_k p_ik phi_ik,  L = sum_i s_i / (P nsel),  dL/dz_ij = p_ij (phi_ij - s_i) / (P nsel)
//
// The transform is exact and separable.  Row pass: per (slice, row) the membership bits of every selected class are gathered with wave
// ballots into 64-bit words, and each pixel finds the nearest bit of the opposite membership in its row with count-leading/trailing-
// zeros; ONE signed 16-bit number per pixel and class goes to the workspace (+r: not a member, the nearest member of the row is r away;
// -r: a member, the nearest non-member of the row is r away; +-ROW_NONE: the row holds none).  A pixel's distance to its own kind is 0,
// so the sign carries the second row distance the column pass needs.  Column pass: a block stages a strip of columns of every selected
// class in LDS; a thread takes min_k g(k, w)^2 + (h - k)^2 for eight consecutive rows of a column at once, in exact integers (one LDS
// read per row k serves the eight), over the rows that hold a pixel of the kind it looks for; one sqrtf at the end.  A block writes every
// class of its pixels, so the partial lines of the per-class stores meet in one L2.
// No atomics, no host read, fixed order: stream-ordered, capturable, bit-identical from run to run.
#include "pixel_loss.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {

constexpr int NT = 256;
constexpr int MAX_EXTENT = 1024;
constexpr int MAX_WORDS = MAX_EXTENT / 64;
constexpr int ROW_NONE = 0x7FFF;          // row distance where the row holds no pixel of the opposite membership
constexpr int NO_DIST = 1 << 29;          // squared distance "none": above 2 * 1023^2, and NO_DIST + 1023^2 fits an int
constexpr int LDS_TILES = 16 * 1024;      // column pass: the strip width halves from 64 until the tiles of all selected classes fit this
constexpr int MIN_STRIP = 2;              // (blocks enough to fill the chip at B = 16); 8 classes x 1024 rows x 2 columns x 2 bytes = 32 KB at most

inline int popcount32(uint32_t v) { return __builtin_popcount(v); }

// strip width of the column pass (a power of two) for nsel tiles of H rows of int16
inline int strip_width(int H, int nsel) {
    int tw = 64;
    while (tw > MIN_STRIP && (size_t)nsel * H * tw * sizeof(int16_t) > (size_t)LDS_TILES) tw >>= 1;
    return tw;
}

// ---- row pass: one block per (b, h) ------------------------------------------------------------------------------------------------
// nearest set bit of `words` (nw words) to position w, w itself excluded; ROW_NONE if there is none
__device__ __forceinline__ int nearest_bit(const unsigned long long* words, int nw, int w) {
    const int wi = w >> 6, bit = w & 63;
    int best = ROW_NONE;
    unsigned long long m = words[wi] & ((1ull << bit) - 1ull);          // bits below w in its own word, then the words to the left
    for (int i = wi;;) {
        if (m) {
            best = w - (i * 64 + 63 - __clzll((long long)m));
            break;
        }
        if (--i < 0) break;
        m = words[i];
    }
    m = words[wi] & ((~0ull << bit) << 1);                               // bits above w (bit == 63: none), then the words to the right
    for (int i = wi;;) {
        if (m) {
            const int d = i * 64 + __ffsll((long long)m) - 1 - w;
            best = d < best ? d : best;
            break;
        }
        if (++i >= nw) break;
        m = words[i];
    }
    return best;
}

__global__ void __launch_bounds__(NT) sdist_row_kernel(const float* __restrict__ onehot, int16_t* __restrict__ rowd, int H, int W, int ncls,
                                                       uint32_t class_mask, int nsel) {
    __shared__ unsigned long long member[MAXC][MAX_WORDS];
    __shared__ unsigned long long valid[MAX_WORDS];
    __shared__ unsigned char bits[MAX_EXTENT];
    const long long row = blockIdx.x;                  // b * H + h
    const int b = (int)(row / H), h = (int)(row % H);
    const float* __restrict__ src = onehot + (size_t)row * W * ncls;
    const int nw = (W + 63) >> 6;
    // (uniform trip count: every lane of a wave takes part in the ballots)
    for (int w0 = 0; w0 < nw * 64; w0 += NT) {
        const int w = w0 + (int)threadIdx.x;
        unsigned mine = 0;
        if (w < W) {
            for (int c = 0; c < ncls; ++c) mine |= (src[(size_t)w * ncls + c] > 0.5f ? 1u : 0u) << c;
            bits[w] = (unsigned char)mine;
        }
        if (w < nw * 64) {                             // whole waves: nw * 64 is a multiple of the wave size
            const unsigned long long v = __ballot(w < W);
            int s = 0;
            for (int c = 0; c < ncls; ++c) {
                if (!((class_mask >> c) & 1u)) continue;
                const unsigned long long mb = __ballot((mine >> c) & 1u);
                if ((threadIdx.x & 63) == 0) member[s][w >> 6] = mb;
                ++s;
            }
            if ((threadIdx.x & 63) == 0) valid[w >> 6] = v;
        }
    }
    __syncthreads();
    // the words a pixel searches: members if it is outside the class, valid non-members if it is inside
    __shared__ unsigned long long other[MAXC][MAX_WORDS];
    for (int i = threadIdx.x; i < nsel * nw; i += NT) other[i / nw][i % nw] = ~member[i / nw][i % nw] & valid[i % nw];
    __syncthreads();
    for (int w = threadIdx.x; w < W; w += NT) {
        const unsigned mine = bits[w];
        int s = 0;
        for (int c = 0; c < ncls; ++c) {
            if (!((class_mask >> c) & 1u)) continue;
            const bool in = (mine >> c) & 1u;
            const int d = nearest_bit(in ? other[s] : member[s], nw, w);
            rowd[(((size_t)b * nsel + s) * H + h) * W + w] = (int16_t)(in ? -d : d);
            ++s;
        }
    }
}

// ---- column pass: one block per (b, strip of TW columns), every class ------------------------------------------------------------
constexpr int KR = 8;                     // rows per thread: one LDS read of row k serves KR outputs of its column
constexpr int MAX_PARTS = 8;              // blocks that share one strip

// m[r] = min over rows k in [klo, khi] of g(k)^2 + (h0 + r - k)^2, r < KR, where g(k) is row k's distance to the membership `sgn` looks
// for: sgn = +1 members (the outputs of pixels outside the class), sgn = -1 non-members (pixels inside it).  Exact integers.
__device__ __forceinline__ void minplus_rows(const int16_t* col, int TW, int klo, int khi, int h0, int sgn, int (&m)[KR]) {
#pragma unroll
    for (int r = 0; r < KR; ++r) m[r] = NO_DIST;
#pragma unroll 2
    for (int k = klo; k <= khi; ++k) {
        const int u = sgn * (int)col[k * TW];
        const int g = u <= 0 ? 0 : (u == ROW_NONE ? NO_DIST : __mul24(u, u));      // 0: row k's pixel is itself of that kind
        const int t = h0 - k;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int d = g + __mul24(t + r, t + r);
            m[r] = d < m[r] ? d : m[r];
        }
    }
}

__global__ void __launch_bounds__(NT) sdist_col_kernel(const int16_t* __restrict__ rowd, float* __restrict__ phi, int H, int W, int ncls,
                                                       uint32_t class_mask, int nsel, int TW, int tw_shift, int nstrips, int parts) {
    extern __shared__ int16_t tile[];                  // [nsel][H][TW]
    // rows[s] = {first, last row that holds a member; first, last row that holds a non-member} of selected class s in this slice.
    // +ROW_NONE (-ROW_NONE) at ANY pixel of a row says the whole row holds no member (no non-member), so the first column of the strip
    // tells.  Rows outside a range cannot hold the nearest pixel: the minimum runs over the range only, and a class that is absent from
    // the slice or fills it (an empty range) has no distance at all: phi = 0.
    __shared__ int rows[MAXC][4];
    __shared__ int cls_of[MAXC];
    // `parts` blocks share a strip: each stages all of it (a minimum may come from any row) and takes a share of its outputs, so that
    // a batch of 16 slices of 256 x 256 puts 2 048 blocks on the chip instead of 512
    const int part = blockIdx.x % parts, strip = (blockIdx.x / parts) % nstrips, b = blockIdx.x / (parts * nstrips);
    const int w0 = strip * TW;
    const int n = H * TW;
    for (int s = 0; s < nsel; ++s) {
        const int16_t* __restrict__ src = rowd + ((size_t)b * nsel + s) * H * W;
        for (int i = threadIdx.x; i < n; i += NT) {
            const int h = i >> tw_shift, w = w0 + (i & (TW - 1));
            tile[s * n + i] = w < W ? src[(size_t)h * W + w] : (int16_t)ROW_NONE;
        }
    }
    if (threadIdx.x == 0) {
        int s = 0;
        for (int c = 0; c < ncls; ++c)
            if ((class_mask >> c) & 1u) cls_of[s++] = c;
    }
    __syncthreads();
    // one wave per class (fixed shuffle trees: no atomics)
    for (int s = threadIdx.x >> 6; s < nsel; s += NT / 64) {
        int mlo = H, mhi = -1, olo = H, ohi = -1;
        for (int k = threadIdx.x & 63; k < H; k += 64) {
            const int v = tile[s * n + k * TW];
            if (v != ROW_NONE) mlo = k < mlo ? k : mlo, mhi = k > mhi ? k : mhi;
            if (v != -ROW_NONE) olo = k < olo ? k : olo, ohi = k > ohi ? k : ohi;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mlo = min(mlo, __shfl_xor(mlo, o, 64)), mhi = max(mhi, __shfl_xor(mhi, o, 64));
            olo = min(olo, __shfl_xor(olo, o, 64)), ohi = max(ohi, __shfl_xor(ohi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) rows[s][0] = mlo, rows[s][1] = mhi, rows[s][2] = olo, rows[s][3] = ohi;
    }
    __syncthreads();
    // one item = KR consecutive rows of one column of one selected class; lanes run along the strip's columns
    const int nch = (H + KR - 1) / KR;
    const int items = nsel * nch * TW, ipb = (items + parts - 1) / parts;
    const int it_end = min(items, (part + 1) * ipb);
    for (int it = part * ipb + threadIdx.x; it < it_end; it += NT) {
        const int wl = it & (TW - 1), rest = it >> tw_shift;
        const int s = rest / nch, h0 = (rest - s * nch) * KR, w = w0 + wl;
        if (w >= W) continue;
        const int16_t* col = tile + s * n + wl;
        // own row distances; g_out / g_in: the largest of them among the item's pixels outside / inside the class (0: there is none).
        // A pixel whose own row puts a candidate at distance g cannot gain from a row g or more away, so the minimum of the item runs
        // over rows h0 - (g - 1) ... h0 + KR - 1 + (g - 1) only (ROW_NONE: over the whole range of the class).
        int own[KR], g_out = 0, g_in = 0;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            own[r] = h0 + r < H ? (int)col[(h0 + r) * TW] : 0;
            g_out = max(g_out, own[r]);
            g_in = max(g_in, -own[r]);
        }
        const int mlo = rows[s][0], mhi = rows[s][1], olo = rows[s][2], ohi = rows[s][3];
        const bool both = mlo <= mhi && olo <= ohi;     // the class is neither absent from the slice nor filling it
        int d2[KR], m[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) d2[r] = NO_DIST;
        if (both && g_out > 0) {
            minplus_rows(col, TW, max(mlo, h0 - (g_out - 1)), min(mhi, h0 + KR - 1 + (g_out - 1)), h0, +1, m);
#pragma unroll
            for (int r = 0; r < KR; ++r) d2[r] = own[r] > 0 ? m[r] : d2[r];
        }
        if (both && g_in > 0) {
            minplus_rows(col, TW, max(olo, h0 - (g_in - 1)), min(ohi, h0 + KR - 1 + (g_in - 1)), h0, -1, m);
#pragma unroll
            for (int r = 0; r < KR; ++r) d2[r] = own[r] < 0 ? m[r] : d2[r];
        }
        float* __restrict__ dst = phi + (((size_t)b * H + h0) * W + w) * ncls + cls_of[s];
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            if (h0 + r >= H) break;
            float v = 0.f;
            if (d2[r] < NO_DIST) {
                const float d = sqrtf((float)d2[r]);
                v = own[r] > 0 ? d : 1.0f - d;
            }
            dst[(size_t)r * W * ncls] = v;
        }
    }
    // the classes that are not selected: 0
    const uint32_t rest_mask = ~class_mask & ((1u << ncls) - 1u);
    if (rest_mask) {
        const int ppb = (n + parts - 1) / parts, i_end = min(n, (part + 1) * ppb);
        for (int i = part * ppb + threadIdx.x; i < i_end; i += NT) {
            const int h = i >> tw_shift, w = w0 + (i & (TW - 1));
            if (w >= W) continue;
            float* __restrict__ dst = phi + (((size_t)b * H + h) * W + w) * ncls;
            for (int c = 0; c < ncls; ++c)
                if ((rest_mask >> c) & 1u) dst[c] = 0.f;
        }
    }
}

// ---- loss pass: a term of the per-pixel skeleton (pixel_loss.h) ------------------------------------------------------------------------
// one pixel: z[0..C), q = x[0][0..C) (phi) -> s = sum_k p_k q_k (returned); g[0..C) = gk * p (q - s) when GRAD
struct BoundaryTerm : pixel_loss::Plain<1> {
    template <int C, bool GRAD>
    static __device__ __forceinline__ float pixel(const float* z, const float* const* x, int ncls, float gk, float* g, Lane<C>&, uint32_t&, float&) {
        const float* q = x[0];
        float e[C], m;
        const float inv = 1.0f / pixel_loss::softmax_exp<C>(z, ncls, e, m);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            e[j] *= inv;
            s = fmaf(e[j], j < ncls ? q[j] : 0.f, s);
        }
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < C; ++j) g[j] = gk * e[j] * ((j < ncls ? q[j] : 0.f) - s);
        }
        return s;
    }
};

// the served domain of the transform; 0 with the message set otherwise
bool sdist_domain(int32_t B, int32_t H, int32_t W, int32_t ncls, uint32_t class_mask) {
    if (B < 1 || H < 1 || W < 1 || ncls < 1) {
        pnp_set_error("pnp_signed_distance_2d: bad argument (B = %d, H = %d, W = %d, ncls = %d)", (int)B, (int)H, (int)W, (int)ncls);
        return false;
    }
    if (ncls > MAXC) {
        pnp_set_error("pnp_signed_distance_2d: ncls = %d, at most %d classes are served", (int)ncls, MAXC);
        return false;
    }
    if (H > MAX_EXTENT || W > MAX_EXTENT) {
        pnp_set_error("pnp_signed_distance_2d: H = %d, W = %d, extents of at most %d are served", (int)H, (int)W, MAX_EXTENT);
        return false;
    }
    if ((long long)B * H > 0x7FFFFFFFll) {
        pnp_set_error("pnp_signed_distance_2d: B * H = %lld rows, at most 2^31 - 1 are served", (long long)B * H);
        return false;
    }
    if (class_mask >> ncls) {
        pnp_set_error("pnp_signed_distance_2d: class_mask 0x%x names a class beyond ncls = %d", (unsigned)class_mask, (int)ncls);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

size_t pnp_signed_distance_2d_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t ncls, uint32_t class_mask) {
    if (B < 1 || H < 1 || W < 1 || ncls < 1 || ncls > MAXC) return 0;
    return (size_t)B * popcount32(class_mask & ((1u << ncls) - 1u)) * H * W * sizeof(int16_t);
}

int pnp_signed_distance_2d(const float* onehot, int32_t B, int32_t H, int32_t W, int32_t ncls, uint32_t class_mask, float* phi,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!sdist_domain(B, H, W, ncls, class_mask)) return PNP_EINVAL;
    const int nsel = popcount32(class_mask);
    const size_t need = pnp_signed_distance_2d_workspace_bytes(B, H, W, ncls, class_mask);
    PNP_REQUIRE(onehot && phi && (workspace || need == 0), "pnp_signed_distance_2d: bad argument (null pointer)");
    PNP_REQUIRE(workspace_bytes >= need, "pnp_signed_distance_2d: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    int16_t* rowd = (int16_t*)workspace;
    if (nsel > 0) {
        hipLaunchKernelGGL(sdist_row_kernel, dim3((unsigned)((long long)B * H)), dim3(NT), 0, st, onehot, rowd, (int)H, (int)W, (int)ncls,
                           class_mask, nsel);
        PNP_CHECK_LAUNCH("sdist_row_kernel");
    }
    const int tw = strip_width(H, nsel);
    int tw_shift = 0;
    while ((1 << tw_shift) < tw) ++tw_shift;
    const int nstrips = (W + tw - 1) / tw;
    // one block per NT outputs-of-eight-rows of a strip, at most MAX_PARTS blocks per strip (each stages the whole strip)
    const long long items = (long long)nsel * ((H + KR - 1) / KR) * tw;
    const int parts = (int)std::min<long long>(MAX_PARTS, std::max<long long>(1, items / NT));
    PNP_REQUIRE((long long)B * nstrips * parts <= 0x7FFFFFFFll, "pnp_signed_distance_2d: B * strips = %lld blocks, at most 2^31 - 1 are served",
                (long long)B * nstrips * parts);
    const size_t lds = (size_t)nsel * H * tw * sizeof(int16_t);
    hipLaunchKernelGGL(sdist_col_kernel, dim3((unsigned)(B * nstrips * parts)), dim3(NT), lds, st, (const int16_t*)rowd, phi, (int)H, (int)W,
                       (int)ncls, class_mask, nsel, tw, tw_shift, nstrips, parts);
    PNP_CHECK_LAUNCH("sdist_col_kernel");
    return PNP_OK;
}

size_t pnp_boundary_loss_workspace_bytes(int64_t P, int32_t ncls) {
    (void)ncls;
    return pixel_loss::workspace_bytes(P);
}

int pnp_boundary_loss(const float* logits, const float* phi, int64_t P, int32_t ncls, int32_t nsel, float coef, float* dlogits, float* out,
                      void* workspace, size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(logits && phi && out && workspace && P > 0 && ncls > 0, "pnp_boundary_loss: bad argument");
    PNP_REQUIRE(ncls <= MAXC, "pnp_boundary_loss: ncls = %d, at most %d classes are served", (int)ncls, MAXC);
    PNP_REQUIRE(nsel >= 0 && nsel <= ncls, "pnp_boundary_loss: nsel = %d selected classes of ncls = %d", (int)nsel, (int)ncls);
    PNP_REQUIRE(workspace_bytes >= pnp_boundary_loss_workspace_bytes(P, ncls), "pnp_boundary_loss: workspace too small (%zu < %zu bytes)",
                workspace_bytes, pnp_boundary_loss_workspace_bytes(P, ncls));
    // 1 / (P nsel); no selected class: value and gradient are 0
    const double scale = nsel > 0 ? 1.0 / ((double)P * (double)nsel) : 0.0;
    const float gk = (float)((double)coef * scale);
    return pixel_loss::run<BoundaryTerm>("pnp_boundary_loss", logits, {{phi}}, (long long)P, ncls, scale, gk, dlogits, out, workspace,
                                         (hipStream_t)stream);
}

}  // extern "C"
