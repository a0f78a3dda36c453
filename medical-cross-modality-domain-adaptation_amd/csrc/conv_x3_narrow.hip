// conv_x3_narrow.hip — the segmenter head's 5x5, 40 -> 5 logits convolution (stride 1, dilation 1, fp32 geometry, zero / no padding) and
// its data gradient on the bf16 matrix pipe with split operands: the arithmetic of conv_x3_direct.hip (an fp32 value IS the sum of three
// bf16 planes, six plane products reproduce the fp32 product to 2^-26, fp32 accumulation) for a layer whose ONE side has 5 channels.  The
// vector-ALU kernel (conv_fwd_narrow_kernel) needs one LDS operand per FMA and the implicit GEMM with C = 5 runs on its scalar loader;
// here the 5-channel side is the 16-row MFMA operand (v_mfma_f32_16x16x32_bf16: A = filters, B = 16 pixels of one image row) and the taps
// are LDS offsets of one staged patch.  DESIGN §25.
//
// Both kernels: 256 threads, PERSISTENT workgroups (two per CU: 79 KB / 73 KB of LDS each) over the tiles, every wave loads, splits
// (v_cvt_pk_bf16_f32) and stores its share of the patch, then runs its share of the MFMAs; the next tile's global loads are in flight
// under the MFMAs, and the second workgroup of the CU computes while this one stages.  Two __syncthreads per tile, no raw
// barriers, no atomics, no allocation: deterministic and capturable.
//
//   forward (KIND 0)   tile = 8 x 16 outputs, patch 12 x 20 pixels x 3 planes x 96 B (40 channels + 8 ZERO channels: the 5 pixels x 48
//     values of one output pixel and one tap row are 240 contiguous values = 8 k-slabs of 32 with the last 16 on the next pixel, all of
//     them under zero filter columns; the 96-byte pixel pitch makes every ds_read_b128 lane group hit 16 distinct 16-byte slots).  Wave w
//     owns k-slabs 2w and 2w + 1 of all five tap rows — its 30 filter fragments stay in REGISTERS for the whole launch — and all eight
//     output rows: per (slab, patch row) three ds_read_b128 feed up to 30 MFMAs.  The four waves' partial sums meet in LDS and are added in
//     a fixed order; dropout exactly as conv_fwd_narrow_kernel (same counter hash on the flat output index).
//     Reads past a patch row's end (the zero-filter columns of its last outputs) land on the next row, the next plane or the zeroed tail.
//   data gradient (KIND 1)   tile = 16 x 16 pixels of dx (ragged tiles are masked in the epilogue: 260 = 16 x 16 + 4), dy patch 20 x 20
//     pixels x 3 planes x 16 B (5 channels + 3 ZERO channels), reduction index (tap, channel of 8) = 7 k-slabs of 32 (28 taps, 3 dead:
//     zero filter columns reading tap 0), the 40 outputs three row blocks of 16 (8 dead rows read a zero block).  The flipped, transposed
//     filter image lives in LDS for the whole launch; wave w owns rows 4w .. 4w + 3 of the tile.  Epilogue: + residual, 16-byte stores.
// The filter images are written by x3n_filter_kernel into the caller's workspace (forward as is, data gradient flipped and transposed).
// PNP_X3_NARROW / pnp_conv2d_x3_narrow(): 0 off, 1 where a launch fills the chip (>= 256 tiles) and the direction measured faster at
// B = 16, 2 wherever the shapes allow; PNP_X3_DIRECT=0 turns the route off as well.
#include "conv_x3_common.h"

using namespace pnpconv;

namespace {

constexpr int XC = 40, XK = 5, XR = 5;             // the layer class: 5x5, 40 -> 5
constexpr int NCU = 256;

// forward
constexpr int F_TH = 8, F_TW = 16, F_PH = F_TH + XR - 1, F_PW = F_TW + XR - 1, F_NPX = F_PH * F_PW;      // 12 x 20 = 240 patch pixels
constexpr int F_PXB = 96;                          // bytes per pixel and plane: 40 channels + 8 zero channels
constexpr int F_PLANE = F_NPX * F_PXB;             // 23 040
constexpr int F_TAIL = 64;                         // zeroed: the last plane's reads past its end (32 B)
constexpr int F_PATCH = 3 * F_PLANE + F_TAIL;      // 69 184
constexpr int F_ROWV = F_TW * XK;                  // 80 output values per tile row
constexpr int F_RED = 4 * F_TH * F_ROWV * 4;       // 10 240 B: [wave][row][pixel][filter] partial sums
constexpr int F_LDS = F_PATCH + F_RED;             // 79 424
constexpr int F_NSLAB = 8;                         // k-slabs of 32 per tap row: 5 pixels x 48 = 240 values + 16 of the next pixel
constexpr size_t F_IMG = (size_t)F_NSLAB * XR * 3 * 64 * 16;      // 122 880 B: [slab][tap row][plane][lane][8] bf16, fragment order

// data gradient
constexpr int D_T = 16, D_P = D_T + XR - 1, D_NPX = D_P * D_P;     // 20 x 20 = 400 patch pixels
constexpr int D_PLANE = D_NPX * 16;                // 6 400
constexpr int D_PATCH = 3 * D_PLANE;               // 19 200
constexpr int D_NSLAB = 7;                         // 28 taps x 8 channels
constexpr int D_FSP = XC * 64;                     // 2 560 B per (slab, plane): 40 rows of 32 bf16
constexpr int D_FILT = D_NSLAB * 3 * D_FSP;        // 53 760 B = the global image [slab][plane][row][32]
constexpr int D_LDS = D_FILT + D_PATCH + 64;       // 73 024 (64 zero bytes for the dead rows of the third block)
constexpr int D_NPI = D_P / 2;                     // patch rows per loader thread: 10

// timing experiments only (-DPNP_X3N_ABLATE=1: no MFMAs; 2: no global loads, split or patch stores): never the shipped library
#ifndef PNP_X3N_ABLATE
#define PNP_X3N_ABLATE 0
#endif
constexpr int kX3nAblate = PNP_X3N_ABLATE;

struct X3nArgs {
    const float* x;               // forward: x [N][H][W][40]; data gradient: dy [N][H][W][5]
    const unsigned short* w3;     // filter image
    float* y;                     // forward: y [N][OH][OW][5]; data gradient: dx [N][OH][OW][40]
    const float* res_add;         // data gradient: [N][OH][OW][40] or null
    int N, H, W, OH, OW, pad_t, pad_l;
    int tiles_x, tiles_y, nitems;
    int do_drop;
    uint32_t drop_thresh, drop_key;
    float drop_keep;
    const pnp_step_params* sp;
    uint32_t drop_sid;
};

// KIND 0: forward; 1: data gradient (a convolution of dy with the flipped, transposed filter)
template <int KIND>
__global__ void __launch_bounds__(256, 2) conv_x3_direct_kernel_narrow(X3nArgs a) {
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int p16 = lane & 15, g = lane >> 4;
    const int tpi = a.tiles_x * a.tiles_y;
    int id = blockIdx.x;
    if (id >= a.nitems) return;                      // (uniform; the grid never exceeds the items)
    if constexpr (KIND == 0) {
        __shared__ __attribute__((aligned(256))) unsigned char lds[F_LDS];
        float* const red = reinterpret_cast<float*>(lds + F_PATCH);
        // this wave's filter fragments: A[row = filter p16][k = 8 g + e] of slabs 2 wave, 2 wave + 1, every tap row and plane
        bf16x8 wf[2][XR][3];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int r = 0; r < XR; ++r)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    wf[jj][r][p] = *reinterpret_cast<const bf16x8*>(a.w3 + ((size_t)(((2 * wave + jj) * XR + r) * 3 + p) * 64 + lane) * 8);
        // the zero channels of every pixel and the tail: written once, never by the loaders
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        for (int q = t; q < F_NPX; q += 256)
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<f32x4*>(lds + p * F_PLANE + q * F_PXB + 2 * XC) = z4;
        if (t < F_TAIL / 16) *reinterpret_cast<f32x4*>(lds + 3 * F_PLANE + t * 16) = z4;
        f32x4 st[F_PH];
        auto origin = [&](int it, int& n, int& oh0, int& ow0) {
            n = it / tpi;
            const int r = it - n * tpi;
            oh0 = (r / a.tiles_x) * F_TH;
            ow0 = (r % a.tiles_x) * F_TW;
        };
        // thread (pc, j) of the first 200 owns float4 j of patch column pc in every patch row: one base address per tile, the row a uniform
        // offset (the index arithmetic of a flat split over all 256 threads is hoisted out of the tile loop and costs 40 registers)
        const int lpc = t / (XC / 4), lj = t - lpc * (XC / 4);
        const bool lact = t < F_PW * (XC / 4);
        auto load = [&](int it) {
            int n, oh0, ow0;
            origin(it, n, oh0, ow0);
            const int iw = ow0 - a.pad_l + lpc;
            const bool cok = lact & ((unsigned)iw < (unsigned)a.W);
            const float* xp = a.x + (((size_t)n * a.H) * a.W + iw) * XC + lj * 4;
#pragma unroll
            for (int i = 0; i < F_PH; ++i) {
                const int ih = oh0 - a.pad_t + i;
                f32x4 v = z4;
                if (cok & ((unsigned)ih < (unsigned)a.H)) v = *reinterpret_cast<const f32x4*>(xp + (ptrdiff_t)ih * a.W * XC);
                st[i] = v;
            }
        };
        auto store = [&]() {
            if (!lact) return;
            unsigned char* d0 = lds + lpc * F_PXB + lj * 8;
#pragma unroll
            for (int i = 0; i < F_PH; ++i) {
                bf16x4 hi, mi, lo;
                split3(st[i], hi, mi, lo);
                unsigned char* d = d0 + i * F_PW * F_PXB;
                *reinterpret_cast<bf16x4*>(d) = hi;
                *reinterpret_cast<bf16x4*>(d + F_PLANE) = mi;
                *reinterpret_cast<bf16x4*>(d + 2 * F_PLANE) = lo;
            }
        };
        const uint32_t dkey = a.do_drop ? pnp_eff_drop_key(a.drop_key, a.sp, a.drop_sid) : 0u;
        load(id);
        for (; id < a.nitems; id += gridDim.x) {
            if (kX3nAblate != 2) store();            // (every wave is past the MFMAs of the previous tile: the second barrier below)
            if (kX3nAblate != 2 && id + (int)gridDim.x < a.nitems) load(id + gridDim.x);      // lands under the MFMAs
            __syncthreads();
            f32x4 acc[F_TH];
#pragma unroll
            for (int o = 0; o < F_TH; ++o) acc[o] = z4;
            // B[k = 8 g + e][col = pixel p16]: the 32 values of slab j behind pixel (pr, p16) of the patch
            const unsigned char* xb = lds + p16 * F_PXB + (2 * wave) * 64 + g * 16;
            // step = (slab jj, patch row pr); the next step's fragments are read before this step's MFMAs, and nothing moves across a step
            // (the scheduler otherwise hoists reads past the 256 registers of two waves per SIMD)
            bf16x8 xf[2][3];
            auto x_frag = [&](int step, int p) {
                return *reinterpret_cast<const bf16x8*>(xb + p * F_PLANE + (step % F_PH) * F_PW * F_PXB + (step / F_PH) * 64);
            };
#pragma unroll
            for (int p = 0; p < 3; ++p) xf[0][p] = x_frag(0, p);
#pragma unroll
            for (int step = 0; step < 2 * F_PH; ++step) {
                const int jj = step / F_PH, pr = step % F_PH, cur = step & 1;
                if (step + 1 < 2 * F_PH) {
#pragma unroll
                    for (int p = 0; p < 3; ++p) xf[cur ^ 1][p] = x_frag(step + 1, p);
                }
#pragma unroll
                for (int r = 0; r < XR; ++r) {
                    const int o = pr - r;            // patch row pr is tap row r of output row pr - r
                    if (o < 0 || o >= F_TH || kX3nAblate == 1) continue;
#pragma unroll
                    for (int trm = 0; trm < 6; ++trm)
                        acc[o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[jj][r][kTermW[trm]], xf[cur][kTermX[trm]], acc[o], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // D[row = filter 4 g + i][col = pixel p16]: filters 0..3 on lane group 0, filter 4 on group 1
            float* rw = red + wave * (F_TH * F_ROWV);
            if (g == 0) {
#pragma unroll
                for (int o = 0; o < F_TH; ++o)
#pragma unroll
                    for (int i = 0; i < 4; ++i) rw[o * F_ROWV + p16 * XK + i] = acc[o][i];
            } else if (g == 1) {
#pragma unroll
                for (int o = 0; o < F_TH; ++o) rw[o * F_ROWV + p16 * XK + 4] = acc[o][0];
            }
            __syncthreads();
            int n, oh0, ow0;
            origin(id, n, oh0, ow0);
            for (int e = t; e < F_TH * F_ROWV; e += 256) {
                const int o = e / F_ROWV, rem = e - o * F_ROWV;
                float v = (red[e] + red[F_TH * F_ROWV + e]) + (red[2 * F_TH * F_ROWV + e] + red[3 * F_TH * F_ROWV + e]);
                const size_t idx = (((size_t)n * a.OH + oh0 + o) * a.OW + ow0) * XK + rem;      // 80 contiguous floats per tile row
                if (a.do_drop) v = pnp_drop_keep((uint32_t)idx, dkey, a.drop_thresh) ? v / a.drop_keep : 0.f;
                a.y[idx] = v;
            }
        }
    } else {
        __shared__ __attribute__((aligned(256))) unsigned char lds[D_LDS];
        unsigned char* const patch = lds + D_FILT;
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        for (int i = t; i < D_FILT / 16; i += 256)
            *reinterpret_cast<f32x4*>(lds + i * 16) = *reinterpret_cast<const f32x4*>(reinterpret_cast<const unsigned char*>(a.w3) + (size_t)i * 16);
        for (int i = t; i < (D_PATCH + 64) / 16; i += 256) *reinterpret_cast<f32x4*>(patch + i * 16) = z4;      // zero channels 5..7, zero block
        float st[D_NPI];
        auto origin = [&](int it, int& n, int& oh0, int& ow0) {
            n = it / tpi;
            const int r = it - n * tpi;
            oh0 = (r / a.tiles_x) * D_T;
            ow0 = (r % a.tiles_x) * D_T;
        };
        // thread (half, rem) of the first 200 owns float rem of the 100 of patch rows half, half + 2, ...: one base address per tile
        const int lhalf = t / (D_P * XK), lrem = t - lhalf * (D_P * XK);
        const int lpc = lrem / XK, lc = lrem - lpc * XK;
        const bool lact = t < 2 * D_P * XK;
        auto load = [&](int it) {
            int n, oh0, ow0;
            origin(it, n, oh0, ow0);
            const int iw = ow0 - a.pad_l + lpc;
            const bool cok = lact & ((unsigned)iw < (unsigned)a.W);
            const float* xp = a.x + (((size_t)n * a.H) * a.W + iw) * XK + lc;
#pragma unroll
            for (int i = 0; i < D_NPI; ++i) {
                const int ih = oh0 - a.pad_t + 2 * i + lhalf;
                float v = 0.f;
                if (cok & ((unsigned)ih < (unsigned)a.H)) v = xp[(ptrdiff_t)ih * a.W * XK];
                st[i] = v;
            }
        };
        auto store = [&]() {
            if (!lact) return;
            unsigned char* d0 = patch + (lhalf * D_P + lpc) * 16 + lc * 2;
#pragma unroll
            for (int i = 0; i < D_NPI; ++i) {
                __bf16 h, m, l;
                split3(st[i], h, m, l);
                unsigned char* d = d0 + 2 * i * D_P * 16;
                *reinterpret_cast<__bf16*>(d) = h;
                *reinterpret_cast<__bf16*>(d + D_PLANE) = m;
                *reinterpret_cast<__bf16*>(d + 2 * D_PLANE) = l;
            }
        };
        // lane group g of slab j reads tap 4 j + g (dead taps 25..27: tap 0 under zero filter columns)
        int toff[D_NSLAB];
#pragma unroll
        for (int j = 0; j < D_NSLAB; ++j) {
            const int tp = 4 * j + g, tt = tp < XR * XR ? tp : 0;
            toff[j] = ((tt / XR) * D_P + (tt % XR)) * 16;
        }
        // A[row = channel 16 blk + p16][k = 8 g + e]; rows 40..47 of the third block read the zero block
        int woff[3];
#pragma unroll
        for (int blk = 0; blk < 3; ++blk) woff[blk] = (16 * blk + p16) * 64 + g * 16;
        const bool dead = p16 >= 8;                  // (third block)
        load(id);
        __syncthreads();                             // the zeroed patch before the first store
        for (; id < a.nitems; id += gridDim.x) {
            if (kX3nAblate != 2) store();
            if (kX3nAblate != 2 && id + (int)gridDim.x < a.nitems) load(id + gridDim.x);      // lands under the MFMAs
            __syncthreads();
            int n, oh0, ow0;
            origin(id, n, oh0, ow0);
            if (oh0 + 4 * wave < a.OH) {             // (uniform: a ragged tile's waves below the image have nothing to do)
                f32x4 acc[4][3];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                    for (int blk = 0; blk < 3; ++blk) acc[rr][blk] = z4;
#pragma unroll
                for (int j = 0; j < D_NSLAB; ++j) {
                    bf16x8 wf[3][3];                 // [blk][plane]
#pragma unroll
                    for (int blk = 0; blk < 3; ++blk)
#pragma unroll
                        for (int p = 0; p < 3; ++p) {
                            const int o = (blk == 2 && dead) ? D_FILT + D_PATCH : (j * 3 + p) * D_FSP + woff[blk];
                            wf[blk][p] = *reinterpret_cast<const bf16x8*>(lds + o);
                        }
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        bf16x8 xf[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p)
                            xf[p] = *reinterpret_cast<const bf16x8*>(patch + p * D_PLANE + ((4 * wave + rr) * D_P + p16) * 16 + toff[j]);
#pragma unroll
                        for (int blk = 0; blk < 3; ++blk)
#pragma unroll
                            for (int trm = 0; trm < (kX3nAblate == 1 ? 0 : 6); ++trm)
                                acc[rr][blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[blk][kTermW[trm]], xf[kTermX[trm]], acc[rr][blk], 0, 0, 0);
                    }
                }
                // D[row = channel 16 blk + 4 g + i][col = pixel p16]: four consecutive channels per lane
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int oh = oh0 + 4 * wave + rr, ow = ow0 + p16;
#pragma unroll
                    for (int blk = 0; blk < 3; ++blk) {
                        const int ch = 16 * blk + 4 * g;
                        if (oh < a.OH && ow < a.OW && ch < XC) {
                            const size_t off = (((size_t)n * a.OH + oh) * a.OW + ow) * XC + ch;
                            f32x4 v = acc[rr][blk];
                            if (a.res_add) v += *reinterpret_cast<const f32x4*>(a.res_add + off);
                            *reinterpret_cast<f32x4*>(a.y + off) = v;
                        }
                    }
                }
            }
            __syncthreads();                         // every wave is past its reads of this patch
        }
    }
}

// the filter images.  FLIP = false (forward): [slab 8][tap row 5][plane 3][lane 64][8] bf16 in fragment order: lane (row = lane % 16,
// g = lane / 16), element e is reduction index q = 32 slab + 8 g + e of tap row r: tap column q / 48, channel q % 48 of filter `row` (zero
// for rows >= 5, columns >= 5, channels >= 40); w is [5][5][40][5].  FLIP = true (data gradient): [slab 7][plane 3][channel 40][32] bf16,
// k = 8 (tap % 4) + dy channel of tap 4 slab + k / 8 (zero for taps >= 25, dy channels >= 5), taps reversed, roles transposed
template <bool FLIP>
__global__ void __launch_bounds__(256) x3n_filter_kernel(const float* __restrict__ w, unsigned short* __restrict__ w3) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    size_t base, pstride;
    if (!FLIP) {
        if (i >= F_NSLAB * XR * 64 * 8) return;
        const int e = i & 7, lane = (i >> 3) & 63, sr = i >> 9;
        const int r = sr % XR, slab = sr / XR;
        const int row = lane & 15, q = 32 * slab + 8 * (lane >> 4) + e;
        const int s = q / 48, ch = q - s * 48;
        if (row < XK && s < XR && ch < XC) v = w[((size_t)(r * XR + s) * XC + ch) * XK + row];
        base = ((size_t)((slab * XR + r) * 3) * 64 + lane) * 8 + e;
        pstride = 64 * 8;
    } else {
        if (i >= D_NSLAB * XC * 32) return;
        const int kk = i & 31, row = (i >> 5) % XC, j = (i >> 5) / XC;
        const int tp = 4 * j + (kk >> 3), e = kk & 7;
        if (tp < XR * XR && e < XK) v = w[((size_t)(XR * XR - 1 - tp) * XC + row) * XK + e];
        base = ((size_t)(j * 3) * XC + row) * 32 + kk;
        pstride = (size_t)XC * 32;
    }
    split3_write(w3 + base, pstride, v);
}

ModeSwitch x3n_switch{"PNP_X3_NARROW", 1, 2, false};

// mode 1 takes a direction only if it measured faster than the old kernel at B = 16 (profiles/x3_narrow_joint_ab.txt)
constexpr bool kShips[2] = {true, true};

long long x3n_items(const pnp_conv_geom* g, int kind) {
    return kind == 0 ? (long long)g->N * (g->OH / F_TH) * (g->OW / F_TW) : (long long)g->N * pnp_cdiv(g->H, D_T) * pnp_cdiv(g->W, D_T);
}

}  // namespace

namespace pnpconv {

// g = the FORWARD geometry; kind 0: forward, 1: data gradient.  Geometry only: every epilogue the old kernels of this layer have is here.
bool x3n_chosen(const pnp_conv_geom* g, int kind) {
    const int mode = x3n_switch.get();
    if (x3d_route_mode() <= 0 || mode <= 0) return false;
    if (g->dtype != PNP_DTYPE_F32 || g->pad_mode != PNP_PAD_ZERO || g->R != XR || g->S != XR || g->stride != 1 || g->dil != 1 || g->C != XC || g->K != XK)
        return false;
    if (g->pad_t < 0 || g->pad_l < 0 || g->pad_t > XR - 1 || g->pad_l > XR - 1 || g->OH <= 0 || g->OW <= 0) return false;
    if ((long long)g->N * g->H * g->W * XC >= (1ll << 30) || (long long)g->N * g->OH * g->OW * XK >= (1ll << 30)) return false;
    if (kind == 0 && ((g->OH % F_TH) != 0 || (g->OW % F_TW) != 0)) return false;
    // mode 1: at least 256 tiles (a persistent launch of fewer leaves CUs idle), and only a direction that measured faster
    return mode >= 2 || (kShips[kind != 0] && x3n_items(g, kind) >= 256);
}

size_t x3n_filter_bytes(int kind) { return kind == 0 ? F_IMG : (size_t)D_FILT; }

// forward (kind 0: a = make_args(x, w, y, g)) or data gradient (kind 1: a = make_args(dy, w, dx, d), d = the convolution of dy, w the FORWARD
// filter; honours a.res_add) of a layer x3n_chosen() takes
int launch_x3_narrow(const ConvArgs& a, int kind, void* ws, size_t ws_bytes, hipStream_t st) {
    PNP_REQUIRE(a.ep_scale == nullptr && a.y_h == nullptr && a.o_s == 0 && a.ups == 1 && a.stat_ws == nullptr, "launch_x3_narrow: unsupported epilogue");
    PNP_REQUIRE(a.R == XR && a.S == XR && a.C == (kind ? XK : XC) && a.K == (kind ? XC : XK) && (kind || ((a.OH % F_TH) == 0 && (a.OW % F_TW) == 0)),
                "launch_x3_narrow: layer not on this route");
    const size_t fbytes = x3n_filter_bytes(kind);
    if (!ws || ws_bytes < fbytes) {
        pnp_set_error("launch_x3_narrow: workspace too small (%zu < %zu)", ws_bytes, fbytes);
        return PNP_EWORKSPACE;
    }
    unsigned short* w3 = (unsigned short*)ws;
    const int cls = prof_class(kind);
    const int total = XR * XR * XC * XK;
    {
        PnpProfScope ps(cls, st, 0.0, 4.0 * total + (double)fbytes, "x3n_filter_kernel<%s>", kind ? "true" : "false");
        if (kind) hipLaunchKernelGGL((x3n_filter_kernel<true>), dim3((unsigned)pnp_cdiv(D_NSLAB * XC * 32, 256)), dim3(256), 0, st, a.w, w3);
        else hipLaunchKernelGGL((x3n_filter_kernel<false>), dim3((unsigned)pnp_cdiv(F_NSLAB * XR * 64 * 8, 256)), dim3(256), 0, st, a.w, w3);
        PNP_CHECK_LAUNCH("x3n_filter_kernel");
    }
    X3nArgs x{};
    x.x = a.x; x.w3 = w3; x.y = a.y; x.res_add = kind ? a.res_add : nullptr;
    x.N = a.N; x.H = a.H; x.W = a.W; x.OH = a.OH; x.OW = a.OW; x.pad_t = a.pad_t; x.pad_l = a.pad_l;
    x.tiles_x = kind ? pnp_cdiv(a.OW, D_T) : a.OW / F_TW;
    x.tiles_y = kind ? pnp_cdiv(a.OH, D_T) : a.OH / F_TH;
    const long long nitems = (long long)a.N * x.tiles_x * x.tiles_y;
    x.nitems = (int)nitems;
    copy_dropout(x, a);
    const dim3 grid((unsigned)(nitems > 2 * NCU ? 2 * NCU : nitems));
    // flops = six plane products per useful fp32 multiply-add of the layer (§10.1): priced against the dense bf16 peak
    const double fl = 6.0 * 2.0 * (double)a.M * XR * XR * XC * XK;
    const double by = 4.0 * ((double)a.N * a.H * a.W * a.C + (double)a.M * a.K) + (double)fbytes;
    PnpProfScope ps(cls, st, fl, by, "conv_x3_direct_kernel_narrow<%d>", kind);
    if (kind) hipLaunchKernelGGL((conv_x3_direct_kernel_narrow<1>), grid, dim3(256), 0, st, x);
    else hipLaunchKernelGGL((conv_x3_direct_kernel_narrow<0>), grid, dim3(256), 0, st, x);
    PNP_CHECK_LAUNCH("conv_x3_direct_kernel_narrow");
    return PNP_OK;
}

}  // namespace pnpconv

extern "C" int32_t pnp_conv2d_x3_narrow(int32_t mode) { return x3n_switch.set(mode); }
