// conv_x3_direct.hip — DIRECT 3x3 stride-1 convolutions of the narrow layers (32 / 64 input channels) on the bf16 matrix pipe with split
// operands (round 6; prototype and ablations: tools/experiments/x3_direct_conv.hip, profiles/r06_x3_direct_conv_prototype.txt).
//
// The 64-channel 3x3 layers on the large maps (the critics' cls1 / cls2 blocks, reference adversarial.py:337-366) are where neither route is
// good: the direct fp32-MFMA kernels stop at 0.6-0.7 of 157 TF/s, F(4x4) on the fp32 pipe is bound by its own 2.25x transformed tensors
// (cls1 64->64 at B = 16: 2.95 GB through HBM per convolution, 0.593 ms), and split-bf16 Winograd operands would add 50 % to that traffic.
// Here the split-bf16 idea (conv_wino_x3.hip: an fp32 value IS the sum of three bf16 planes, six plane products reproduce the fp32 product
// to 2^-26) runs WITHOUT Winograd:
//   * a workgroup owns a 16 x 16 output tile x 64 filters.  The tile's 18 x 18 halo patch of 32 input channels is loaded ONCE per channel
//     half by three loader waves (global fp32 -> VGPR -> hi / mid / lo bf16 -> LDS [plane][pixel][64 B], the split spread over five stages),
//     double-buffered across halves: the nine taps are LDS address offsets, every input value crosses L2 -> CU once per tile;
//   * filters come as a pre-split image [filter block][half][tap][plane][64 filters][32 channels] bf16 (x3d_filter_kernel: forward as is,
//     data gradient flipped and transposed) — 12 KB per (half, tap) stage, streamed by one loader wave with LDS-DMA into three buffers;
//   * four consumer waves (64 pixels x 64 filters each): per stage 12 filter-fragment reads after the barrier, the 12 pixel-fragment reads
//     of the NEXT tap issued before it (same patch: no barrier in between), 48 v_mfma_f32_32x32x16_bf16; the second pixel row of a 32-pixel
//     block is rotated by two columns so that every ds_read_b128 lane group sees 16 distinct 16-byte slots; one raw s_barrier per stage;
//   * persistent workgroups (one per CU) over (tile, filter block) items, loaders running ahead; the stages of an item fully unrolled.
// Epilogue = conv_common.h's conv_epilogue restated for a TILED pixel order (a 32-row MFMA block is two image rows of 16 pixels): dropout
// (same counter hash on the flat output index, a division like tf.nn.dropout), residual add (data gradients), batch-norm statistics
// partials (one per consumer wave = 64 pixels), then stores of 128 contiguous bytes per pixel.  Accuracy: every product exact, one fp32
// chain of 9 C terms — 8e-7 of max|ref| on 64 -> 64 (the direct fp32 kernel 2.9e-6, F(4x4) 1.2e-6 .. 8e-6).
// Entry: plan_fwd / plan_dgrad (conv_igemm.hip) give the layers x3d_chosen() takes the route X3D — also layers the Winograd planner owns,
// which keep that route's (larger) workspace; the fused inference BN is not in this epilogue.  PNP_X3_DIRECT / pnp_conv2d_x3_direct(): 0 off, 1 where a launch fills the chip, 2 wherever the shapes allow.
// The strided layers (conv_x3_direct_kernel_strided below, PNP_X3_STRIDED): forward and stride-phase data gradient as sums of stride-1
// sub-convolutions on the same LDS layout, MFMA order and epilogue; the plan's route X3S, through x3s_chosen().
// The FILTER gradient of the stride-1 layers with 64 filters is conv_x3_wgrad.hip (PNP_X3_WGRAD), under this file's mode (x3d_route_mode()).
// Where the shared pieces live: the split, the kept-products table, the wait-count / LDS-DMA helpers and the run-time switch of a route are
// conv_x3_common.h's (for the whole split-bf16 family); the two kernels below differ only in how they enumerate items, patch slots and
// filter stages (static and unrolled / run-time cursors) and call ONE copy of everything else — filter_lane_offsets / filter_dma /
// filter_pipeline, patch_store, consumer_lanes / consumer_stage, tile_epilogue — written once in front of them.
#include "conv_x3_common.h"

using namespace pnpconv;

namespace {

constexpr int TH = 16, TW = 16, PH = TH + 2, PW = TW + 2, NPX = PH * PW;      // 324 patch pixels
constexpr int ROWB = 64;                           // bytes per LDS row: 32 channels of one plane
constexpr int PLANE_P = NPX * ROWB;                // 20 736 B per patch plane
constexpr int PATCH = 3 * PLANE_P;                 // 62 208 B per patch (one channel half)
constexpr int NF = 3;                              // filter stage buffers: NF - 1 stages in flight
constexpr int LDS_BYTES = 2 * PATCH + NF * 3 * 64 * ROWB;      // 161 280 B (filter stage of a 64-filter block: 3 planes x 4 096 B = 12 288 B)
constexpr int NPL = 192;                           // patch-loader lanes (3 waves)
constexpr int NPI = (NPX * 8 + NPL - 1) / NPL;     // float4 loads per patch-loader lane: 14

__device__ __forceinline__ int swz(int row) { return (row >> 2) & 3; }

struct X3dArgs {
    const float* x;               // [N][H][W][C]
    const unsigned short* w3;     // [K / 64][C / 32][9][3][64][32] bf16
    float* y;                     // [N][OH][OW][K]
    int N, H, W, C, K, OH, OW, pad_t, pad_l;
    int M;                        // N OH OW
    int do_drop;
    uint32_t drop_thresh, drop_key;
    float drop_keep;
    const pnp_step_params* sp;
    uint32_t drop_sid;
    const float* res_add;         // [M][K] or null
    float* stat_ws;               // [parts][2][K] or null; part = 4 tile + consumer wave
    const float* stat_shift;
};

// ============================ the pieces both kernels are built from ============================
// a (half, tap) filter stage of a block of KW filters: [plane][KW filters][64 B]
template <int KW>
struct FStage {
    static constexpr int PLANE = KW * ROWB;        // bytes per filter plane of a stage
    static constexpr int BYTES = 3 * PLANE;        // bytes per stage
    static constexpr int NPC = BYTES / 1024;       // LDS-DMA pieces per stage (1 KiB each)
    static constexpr int TN = KW / 32;             // 32-filter MFMA blocks
};

// filter loader: the lane's source offsets of the pieces of a stage.  Piece i (1 KiB = 16 rows of 64 B): lane (lrow = lane / 4,
// lchk = lane % 4) fetches chunk lchk ^ swz(row) of its row
template <int KW>
__device__ __forceinline__ void filter_lane_offsets(int lane, unsigned (&vo)[FStage<KW>::NPC]) {
    const int lrow = lane >> 2, lchk = lane & 3;
    constexpr int PPP = KW / 16;                   // pieces per plane
#pragma unroll
    for (int i = 0; i < FStage<KW>::NPC; ++i) {
        const int row = (i % PPP) * 16 + lrow;     // row within the plane (filter index); plane = i / PPP
        vo[i] = (unsigned)((i / PPP) * FStage<KW>::PLANE + row * ROWB + ((lchk ^ swz(row)) << 4));
    }
}
// ... and the DMA of image stage `stg` into the buffer of global stage g
template <int KW>
__device__ __forceinline__ void filter_dma(__amdgpu_buffer_rsrc_t rw, unsigned char* filt0, int g, const unsigned (&vo)[FStage<KW>::NPC], int stg) {
    unsigned char* bp = filt0 + (g % NF) * FStage<KW>::BYTES;
#pragma unroll
    for (int i = 0; i < FStage<KW>::NPC; ++i) dma16(rw, (lds_void*)(bp + i * 1024), vo[i], stg * FStage<KW>::BYTES);
}
// ... and its pipeline: issue(g) starts global stage g (NPC loads); one barrier per stage, NF - 1 stages ahead of the consumers
template <int NPC, class Issue>
__device__ __forceinline__ void filter_pipeline(int gstages, Issue&& issue) {
#pragma unroll
    for (int b = 0; b < NF - 1; ++b)
        if (b < gstages) issue(b);
    for (int g = 0; g < gstages; ++g) {
        // stage g has landed; up to NF - 2 younger stages stay in flight (the tail issues nothing: drain)
        if (g + NF - 2 < gstages) wait_vm<NPC * (NF - 2)>();
        else wait_vm0();
        __builtin_amdgcn_s_barrier();
        if (g + NF - 1 < gstages) issue(g + NF - 1);                 // into the buffer of stage g - 1: every consumer is past it
    }
    wait_vm0();
}

// patch loader: float4 i0 .. i1 - 1 of lane pl's share of a patch, split into the three planes of the patch buffer pb
__device__ __forceinline__ void patch_store(unsigned char* pb, int pl, const f32x4 (&st)[NPI], int i0, int i1) {
#pragma unroll
    for (int i = 0; i < NPI; ++i) {
        if (i < i0 || i >= i1) continue;
        const int e = pl + i * NPL;
        if (e >= NPX * 8) continue;
        const int q = e >> 3, j = e & 7;
        bf16x4 hi, mi, lo;
        split3(st[i], hi, mi, lo);
        store3(pb + q * ROWB + (((j >> 1) ^ swz(q)) << 4) + (j & 1) * 8, PLANE_P, hi, mi, lo);
    }
}

// consumers: 64 pixels (4 output rows x 16) x KW filters per wave.
// MFMA: A = pixels (rows), B = filters (columns): D[pixel][filter], lane = filter l31 of block tn, rows (i & 3) + 8 (i >> 2) + 4 h.
// Pixel of MFMA row r in 32-pixel block tm: r < 16: image row 4 w + 2 tm, column r; else the next image row, column (r - 2) mod 16 — the
// rotation makes the patch index q of the second row congruent (mod 16) to the first row's: 16 distinct bank slots per lane group.
__device__ __forceinline__ int tile_col(int r) { return (r < 16) ? r : ((r - 16 + 14) & 15); }
// ... and the pixel of accumulator element i of block tm, in a tile at (oh0, ow0).  (The sums keep this order: another association of the
// same terms costs the stride-1 kernels six registers.)
__device__ __forceinline__ void tile_pixel(int oh0, int ow0, int wave, int h, int tm, int i, int& orow, int& ocol) {
    const int r = (i & 3) + 8 * (i >> 2) + 4 * h;
    orow = oh0 + 4 * wave + 2 * tm + (r >> 4);
    ocol = ow0 + tile_col(r);
}
template <int TN>
struct Lanes {
    int l31, h;
    int aq[2];                                     // [tm]: the lane's patch pixel at tap (0, 0)
    int woff[TN][2];                               // [tn][ks]: the lane's fragment within a plane of a filter stage
};
template <int TN>
__device__ __forceinline__ Lanes<TN> consumer_lanes(int lane, int wave) {
    Lanes<TN> L;
    L.l31 = lane & 31;
    L.h = lane >> 5;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) L.aq[tm] = (4 * wave + 2 * tm + (L.l31 >> 4)) * PW + tile_col(L.l31);
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) L.woff[tn][ks] = (tn * 32 + L.l31) * ROWB + (((2 * ks + L.h) ^ swz(tn * 32 + L.l31)) << 4);
    return L;
}
// 16-channel slice ks of plane p of patch pixel q
__device__ __forceinline__ bf16x8 x_frag(const unsigned char* A, int q, int h, int ks, int p) {
    return *reinterpret_cast<const bf16x8*>(A + p * PLANE_P + q * ROWB + (((2 * ks + h) ^ swz(q)) << 4));
}

// One stage: the tap at patch offset dq of patch A against filter stage B.  12 filter-fragment reads after the barrier, the 12
// pixel-fragment reads of the NEXT tap (patch offset dqn; < 0: this is the patch's last) issued before the MFMAs — same patch, no barrier
// in between — and 6 x 2 x 2 x TN MFMAs.  first: the patch only became visible with this barrier, nothing was prefetched.
// xf [ks][plane][tm]: this tap's pixel fragments; xn [plane][tm]: the next tap's first slice, read one stage ahead
template <int KW>
__device__ __forceinline__ void consumer_stage(const Lanes<FStage<KW>::TN>& L, const unsigned char* A, const unsigned char* B, int dq, int dqn, bool first,
                                               f32x16 (&acc)[2][FStage<KW>::TN], bf16x8 (&xf)[2][3][2], bf16x8 (&xn)[3][2]) {
    constexpr int TN = FStage<KW>::TN, PLANE_F = FStage<KW>::PLANE;
    wait_lgkm0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (first) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) xf[0][p][tm] = x_frag(A, L.aq[tm] + dq, L.h, 0, p);
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) xf[0][p][tm] = xn[p][tm];
    }
    bf16x8 wf[2][3][TN];                           // [ks][plane][tn]
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) wf[0][p][tn] = *reinterpret_cast<const bf16x8*>(B + p * PLANE_F + L.woff[tn][0]);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) xf[1][p][tm] = x_frag(A, L.aq[tm] + dq, L.h, 1, p);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) wf[1][p][tn] = *reinterpret_cast<const bf16x8*>(B + p * PLANE_F + L.woff[tn][1]);
    }
    if (dqn >= 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) xn[p][tm] = x_frag(A, L.aq[tm] + dqn, L.h, 0, p);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int trm = 0; trm < 6; ++trm)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[ks][kTermX[trm]][tm], wf[ks][kTermW[trm]][tn], acc[tm][tn], 0, 0, 0);
}

// Epilogue (conv_common.h: conv_epilogue, for the tiled pixel order): phases of pure loads / arithmetic, then stores.  mlin_of(tm, i) = the
// linear output pixel of accumulator element i of pixel block tm (recomputed where it is used: no index arrays kept live); n0 = the
// block's first filter, part = the statistics partial of this wave, out_bytes = the extent of y (and of res_add, which may be null)
template <int TN, class Args, class MLin>
__device__ __forceinline__ void tile_epilogue(f32x16 (&acc)[2][TN], const Args& a, uint32_t dkey, const float* res_add, unsigned out_bytes, int n0, int part,
                                              int l31, int h, MLin&& mlin_of) {
    int ncol[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) ncol[tn] = n0 + tn * 32 + l31;
#define X3_FOR                                                       \
    _Pragma("unroll") for (int tm = 0; tm < 2; ++tm)                 \
        _Pragma("unroll") for (int tn = 0; tn < TN; ++tn)            \
            _Pragma("unroll") for (int i = 0; i < 16; ++i)
    if (a.do_drop) {
        X3_FOR {
            const uint32_t idx = (uint32_t)((size_t)mlin_of(tm, i) * a.K + ncol[tn]);
            const float kept = acc[tm][tn][i] / a.drop_keep;         // (divided whether kept or not: a select, no branch per element)
            acc[tm][tn][i] = pnp_drop_keep(idx, dkey, a.drop_thresh) ? kept : 0.f;
        }
    }
    if (res_add) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(res_add, out_bytes);
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {              // (one pixel block at a time: all loads, then all adds)
            f32x16 rv[TN];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) rv[tn][i] = bload1(rr, (unsigned)(mlin_of(tm, i) * a.K + ncol[tn]) * 4u);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[tm][tn][i] += rv[tn][i];
        }
    }
    if (a.stat_ws) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const float shift = a.stat_shift ? a.stat_shift[ncol[tn]] : 0.f;
            float ssum = 0.f, ssq = 0.f;
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float d = acc[tm][tn][i] - shift;
                    ssum += d;
                    ssq = fmaf(d, d, ssq);
                }
            const float s_ = ssum + __shfl_xor(ssum, 32, 64);      // the two half-waves hold the same filter, disjoint pixels
            const float q_ = ssq + __shfl_xor(ssq, 32, 64);
            if (h == 0) {
                a.stat_ws[((size_t)part * 2 + 0) * a.K + ncol[tn]] = s_;
                a.stat_ws[((size_t)part * 2 + 1) * a.K + ncol[tn]] = q_;
            }
        }
    }
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(a.y, out_bytes);
    X3_FOR bstore1(ry, (unsigned)(mlin_of(tm, i) * a.K + ncol[tn]) * 4u, acc[tm][tn][i]);
#undef X3_FOR
}

// NH = C / 32 channel halves (1 or 2); KW = filters per block (64; 32 for the 32-filter layers: the data gradient of a 32 -> 64 layer);
// KIND 0 / 1 only names the symbol (forward / data gradient: the difference is the filter image)
template <int NH, int KW, int KIND>
__global__ void __launch_bounds__(512, 1) conv_x3_direct_kernel(X3dArgs a) {
    constexpr int NSTG = 9 * NH;
    constexpr int FSTG = FStage<KW>::BYTES, NPC = FStage<KW>::NPC, TN = FStage<KW>::TN;
    static_assert(NSTG % NF == 0, "the filter buffer of a stage must not depend on the item");
    __shared__ __attribute__((aligned(256))) unsigned char lds[LDS_BYTES];
    unsigned char* const patch0 = lds;
    unsigned char* const filt0 = lds + 2 * PATCH;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tiles_x = a.OW / TW, tiles_y = a.OH / TH, KB = a.K / KW;
    const int nitems = a.N * tiles_x * tiles_y * KB;
    int myitems = 0;
    for (int i = blockIdx.x; i < nitems; i += gridDim.x) ++myitems;
    if (myitems == 0) return;                       // (uniform for the workgroup)
    const int gstages = myitems * NSTG;
    // item -> (filter block, image, tile origin); consecutive items = the filter blocks of one tile (its patch is in L2 for the second)
    auto item_origin = [&](int it, int& kb, int& tile, int& n, int& oh0, int& ow0) {
        const int id = blockIdx.x + it * gridDim.x;
        tile = id / KB;
        kb = id - tile * KB;
        n = tile / (tiles_x * tiles_y);
        const int r = tile - n * tiles_x * tiles_y;
        oh0 = (r / tiles_x) * TH;
        ow0 = (r % tiles_x) * TW;
    };

    if (wave == 4) {
        // ============================ filter loader: one 12 KB stage per barrier, LDS-DMA ============================
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(reinterpret_cast<const float*>(a.w3), (unsigned)(KB * NSTG * FSTG));
        unsigned vo[NPC];
        filter_lane_offsets<KW>(lane, vo);
        filter_pipeline<NPC>(gstages, [&](int g) {
            const int it = g / NSTG, s = g - it * NSTG;
            const int kb = (int)((blockIdx.x + it * gridDim.x) % KB);
            filter_dma<KW>(rw, filt0, g, vo, kb * NSTG + s);
        });
        return;
    }
    if (wave > 4) {
        // ============================ patch loaders: global fp32 -> three bf16 planes -> LDS ============================
        const int pl = (wave - 5) * 64 + lane;                        // 0..191
        f32x4 st[NPI];
        auto load = [&](int slot) {                                   // slot = item * NH + half
            int kb, tile, n, oh0, ow0;
            item_origin(slot / NH, kb, tile, n, oh0, ow0);
            const int hsel = slot % NH;
#pragma unroll
            for (int i = 0; i < NPI; ++i) {
                const int e = pl + i * NPL;
                const int q = e >> 3, j = e & 7;
                const int pr = q / PW, pc = q - pr * PW;
                const int ih = oh0 - a.pad_t + pr, iw = ow0 - a.pad_l + pc;
                const bool ok = (e < NPX * 8) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) v = *reinterpret_cast<const f32x4*>(a.x + (((size_t)n * a.H + ih) * a.W + iw) * a.C + hsel * 32 + j * 4);
                st[i] = v;
            }
        };
        auto store = [&](int slot, int i0, int i1) { patch_store(patch0 + (slot & 1) * PATCH, pl, st, i0, i1); };
        const int nslots = myitems * NH;
        load(0);
        wait_vm0();
        store(0, 0, NPI);
        for (int g = 0; g < gstages; ++g) {
            const int slot = g / 9, j = g - slot * 9;
            if (j == 0) wait_lgkm0();                                  // this slot's patch is in LDS
            __builtin_amdgcn_s_barrier();
            if (j == 0 && slot + 1 < nslots) load(slot + 1);
            // split + LDS stores of the next patch spread over stages 3..7 (3 float4 per lane each): the vector ALU work of one stage stays
            // well under the consumers' MFMA time, so this wave is never the last at a barrier
            if (j >= 3 && j <= 7 && slot + 1 < nslots) {
                if (j == 3) wait_vm0();
                if (j == 3) store(slot + 1, 0, 3);
                else if (j == 4) store(slot + 1, 3, 6);
                else if (j == 5) store(slot + 1, 6, 9);
                else if (j == 6) store(slot + 1, 9, 12);
                else store(slot + 1, 12, NPI);
            }
        }
        return;
    }
    // ============================ consumers: 64 pixels (4 output rows x 16) x 64 filters per wave ============================
    const Lanes<TN> L = consumer_lanes<TN>(lane, wave);
    f32x16 acc[2][TN];                              // [tm (pixel block)][tn (filter block)]
    bf16x8 xf[2][3][2], xn[3][2];
    const uint32_t dkey = a.do_drop ? pnp_eff_drop_key(a.drop_key, a.sp, a.drop_sid) : 0u;
    for (int it = 0; it < myitems; ++it) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;
        const int slot0 = it * NH;                   // (NH = 1: the patch buffer alternates with the item; NH = 2: half hsel is buffer hsel)
#pragma unroll
        for (int s = 0; s < NSTG; ++s) {
            const int hsel = s / 9, tap = s % 9;     // (static after unrolling; the filter buffer of global stage NSTG it + s is s mod NF)
            const int pbuf = (slot0 + hsel) & 1;
            consumer_stage<KW>(L, patch0 + pbuf * PATCH, filt0 + (s % NF) * FSTG, (tap / 3) * PW + tap % 3,
                               tap != 8 ? ((tap + 1) / 3) * PW + (tap + 1) % 3 : -1, tap == 0, acc, xf, xn);
        }
        int kb, tile, n, oh0, ow0;
        item_origin(it, kb, tile, n, oh0, ow0);
        tile_epilogue<TN>(acc, a, dkey, a.res_add, (unsigned)((size_t)a.M * a.K * 4), kb * KW, tile * 4 + wave, L.l31, L.h, [&](int tm, int i) {
            int orow, ocol;
            tile_pixel(oh0, ow0, wave, L.h, tm, i, orow, ocol);
            return (n * a.OH + orow) * a.OW + ocol;
        });
    }
}

// the filter image: [K / KW][C / 32][tap][plane][KW filters][32 channels] bf16 (KW = 64; 32 for a 32-filter layer).  FLIP = false: w is [3][3][C][K] (forward); true: w is the
// FORWARD filter [3][3][K][C] of a data gradient computed as a convolution of dy (C = the forward's K): taps reversed, roles transposed
template <bool FLIP>
__global__ void __launch_bounds__(256) x3d_filter_kernel(const float* __restrict__ w, unsigned short* __restrict__ w3, int C, int K, int KW) {
    const int NH = C >> 5, KB = K / KW;
    const int total = KB * NH * 9 * KW * 32;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = e & 31, o = (e >> 5) % KW;
    int r = (e >> 5) / KW;
    const int tap = r % 9; r /= 9;
    const int hf = r % NH, kb = r / NH;
    const int ic = hf * 32 + i, oc = kb * KW + o;
    const float v = FLIP ? w[((size_t)(8 - tap) * K + oc) * C + ic] : w[((size_t)tap * C + ic) * K + oc];
    const size_t base = ((((size_t)kb * NH + hf) * 9 + tap) * 3) * ((size_t)KW * 32) + (size_t)o * 32 + i;
    split3_write(w3 + base, (size_t)KW * 32, v);
}

// ============================ strided layers: sums of stride-1 sub-convolutions over the input's stride phases ============================
// A stride-s convolution is the sum over the s x s input phases x_ab[i][j] = x[s i + a][s j + b] of stride-1 convolutions with the
// sub-filters w[a + s t][b + s u]; a stride-phase data gradient is, per output phase, ONE stride-1 correlation of dy with a flipped sub-filter
// whose outputs land s pixels apart (plan_phases).  Both are GROUPS of PHASES here: an item (group, 16 x 16 tile of the group's output grid,
// 64 filters) accumulates over channel half x phase x the phase's T x U taps, one patch per (half, phase), the taps LDS offsets into it.
// The forward is one group of s^2 phases; the data gradient s^2 groups of one phase each (all in one persistent launch).  Same LDS layout,
// MFMA order, filter stages (of FSTG bytes, now from a [group][filter block][half][stage][plane][64][32] image) and epilogue as above; the
// stage schedule is a run-time loop (channel halves and phases vary per layer and, for the data gradient, per item).
constexpr int X3S_MAXPH = 16;

struct X3sPhase {
    int T, U;              // taps (rows, columns): 1..3
    int ih0, iw0;          // input pixel of patch (0, 0) for the grid origin: patch (pr, pc) of the tile at (oh0, ow0) = si (oh0 + pr) + ih0, ...
};
struct X3sGroup {
    int first_item, tiles_x, tiles_y;
    int ph0, nph, nst;     // phases [ph0, ph0 + nph); nst = stages per channel half (sum of T U)
    int o_h0, o_w0;        // output pixel of grid point (i, j) = (o_h0 + o_s i, o_w0 + o_s j)
    int fbase;             // first stage of the group in the filter image
};
struct X3sArgs {
    const float* x;               // [N][H][W][C]
    const unsigned short* w3;     // filter image
    float* y;                     // [N][OHt][OWt][K]
    int N, H, W, C, K, NH, si;
    int OHt, OWt, o_s;
    int ngroups, nitems;
    unsigned w3_bytes;
    X3sGroup grp[X3S_MAXPH];
    X3sPhase ph[X3S_MAXPH];
    int do_drop;
    uint32_t drop_thresh, drop_key;
    float drop_keep;
    const pnp_step_params* sp;
    uint32_t drop_sid;
    float* stat_ws;               // (one group only) [parts][2][K]; part = 4 tile + consumer wave
    const float* stat_shift;
};

__device__ __forceinline__ int x3s_group(const X3sArgs& a, int id) {
    int gi = 0;
    for (int i = 1; i < a.ngroups; ++i)
        if (id >= a.grp[i].first_item) gi = i;
    return gi;
}

// KIND 0 / 1 only names the symbol (forward / data gradient)
template <int KIND>
__global__ void __launch_bounds__(512, 1) conv_x3_direct_kernel_strided(X3sArgs a) {
    constexpr int KW = 64;
    constexpr int FSTG = FStage<KW>::BYTES, NPC = FStage<KW>::NPC, TN = FStage<KW>::TN;
    __shared__ __attribute__((aligned(256))) unsigned char lds[LDS_BYTES];
    unsigned char* const patch0 = lds;
    unsigned char* const filt0 = lds + 2 * PATCH;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int KB = a.K / KW, NH = a.NH;
    int myitems = 0, gstages = 0, nslots = 0;
    for (int i = blockIdx.x; i < a.nitems; i += gridDim.x) {
        const X3sGroup& G = a.grp[x3s_group(a, i)];
        ++myitems;
        gstages += NH * G.nst;
        nslots += NH * G.nph;
    }
    if (myitems == 0) return;                       // (uniform for the workgroup)
    // item -> (group, filter block, group-local tile, image, tile origin in the group's grid)
    auto item_origin = [&](int it, int& gi, int& kb, int& tile, int& n, int& oh0, int& ow0) {
        const int id = blockIdx.x + it * gridDim.x;
        gi = x3s_group(a, id);
        const X3sGroup& G = a.grp[gi];
        const int loc = id - G.first_item;
        tile = loc / KB;
        kb = loc - tile * KB;
        n = tile / (G.tiles_x * G.tiles_y);
        const int r = tile - n * G.tiles_x * G.tiles_y;
        oh0 = (r / G.tiles_x) * TH;
        ow0 = (r % G.tiles_x) * TW;
    };
    // (item, half, phase index in the group) cursor over the patch slots / (item, half, stage) cursor over the filter stages
    struct Cur { int it, hh, k; };

    if (wave == 4) {
        // ============================ filter loader: one 12 KB stage per barrier, LDS-DMA ============================
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(reinterpret_cast<const float*>(a.w3), a.w3_bytes);
        unsigned vo[NPC];
        filter_lane_offsets<KW>(lane, vo);
        Cur c{0, 0, 0};
        int gi, kb, tile, n, oh0, ow0;
        item_origin(0, gi, kb, tile, n, oh0, ow0);
        filter_pipeline<NPC>(gstages, [&](int g) {
            const X3sGroup& G = a.grp[gi];
            filter_dma<KW>(rw, filt0, g, vo, G.fbase + (kb * NH + c.hh) * G.nst + c.k);
            if (++c.k == G.nst) {
                c.k = 0;
                if (++c.hh == NH) {
                    c.hh = 0;
                    if (++c.it < myitems) item_origin(c.it, gi, kb, tile, n, oh0, ow0);
                }
            }
        });
        return;
    }
    if (wave > 4) {
        // ============================ patch loaders: global fp32 -> three bf16 planes -> LDS ============================
        // slot k + 1 is split and stored during the LAST stage of slot k (its buffer was slot k - 1's), and slot k + 2's global loads
        // are issued right behind: every load has at least one full stage of MFMA work to land in
        const int pl = (wave - 5) * 64 + lane;
        f32x4 st[NPI];
        Cur lc{0, 0, 0};                             // the slot whose data the registers hold / will hold
        auto load = [&]() {
            int gi, kb, tile, n, oh0, ow0;
            item_origin(lc.it, gi, kb, tile, n, oh0, ow0);
            const X3sPhase P = a.ph[a.grp[gi].ph0 + lc.k];
            const int rmax = TH - 1 + P.T, cmax = TW - 1 + P.U;       // patch rows / columns the phase's taps read
#pragma unroll
            for (int i = 0; i < NPI; ++i) {
                const int e = pl + i * NPL;
                const int q = e >> 3, j = e & 7;
                const int pr = q / PW, pc = q - pr * PW;
                const int ih = a.si * (oh0 + pr) + P.ih0, iw = a.si * (ow0 + pc) + P.iw0;
                const bool ok = (e < NPX * 8) & (pr < rmax) & (pc < cmax) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) v = *reinterpret_cast<const f32x4*>(a.x + (((size_t)n * a.H + ih) * a.W + iw) * a.C + lc.hh * 32 + j * 4);
                st[i] = v;
            }
        };
        auto advance = [&](Cur& c) {
            const int id = blockIdx.x + c.it * gridDim.x;
            if (++c.k == a.grp[x3s_group(a, id)].nph) {
                c.k = 0;
                if (++c.hh == NH) { c.hh = 0; ++c.it; }
            }
        };
        auto store = [&](int slot) { patch_store(patch0 + (slot & 1) * PATCH, pl, st, 0, NPI); };
        auto taps_of = [&](const Cur& c) {
            const int id = blockIdx.x + c.it * gridDim.x;
            const X3sPhase& P = a.ph[a.grp[x3s_group(a, id)].ph0 + c.k];
            return P.T * P.U;
        };
        load();
        wait_vm0();
        store(0);
        advance(lc);
        if (nslots > 1) load();
        Cur sc{0, 0, 0};                             // the slot the consumers are on
        int k = 0, j = 0, ns = taps_of(sc);
        for (int g = 0; g < gstages; ++g) {
            if (j == 0) wait_lgkm0();                // this slot's patch is in LDS
            __builtin_amdgcn_s_barrier();
            if (j == ns - 1) {
                if (k + 1 < nslots) {
                    wait_vm0();
                    store(k + 1);
                    advance(lc);
                    if (k + 2 < nslots) load();
                }
                ++k;
                j = 0;
                advance(sc);
                if (k < nslots) ns = taps_of(sc);
            } else {
                ++j;
            }
        }
        return;
    }
    // ============================ consumers: 64 pixels (4 output rows x 16) x 64 filters per wave ============================
    const Lanes<TN> L = consumer_lanes<TN>(lane, wave);
    f32x16 acc[2][TN];
    bf16x8 xf[2][3][2], xn[3][2];
    const uint32_t dkey = a.do_drop ? pnp_eff_drop_key(a.drop_key, a.sp, a.drop_sid) : 0u;
    int g = 0, slot = 0;
    for (int it = 0; it < myitems; ++it) {
        int gi, kb, tile, n, oh0, ow0;
        item_origin(it, gi, kb, tile, n, oh0, ow0);
        const X3sGroup& G = a.grp[gi];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.f;
        for (int hh = 0; hh < NH; ++hh) {
            for (int pk = 0; pk < G.nph; ++pk, ++slot) {
                const X3sPhase P = a.ph[G.ph0 + pk];
                const unsigned char* A = patch0 + (slot & 1) * PATCH;
                // taps row by row: (tr, tc) and its patch offset dq walk along with tap
                for (int tap = 0, ntap = P.T * P.U, tc = 0, dq = 0; tap < ntap; ++tap, ++g) {
                    const bool wrap = tc + 1 == P.U;
                    const int dqn = wrap ? dq + PW - tc : dq + 1;
                    consumer_stage<KW>(L, A, filt0 + (g % NF) * FSTG, dq, tap + 1 < ntap ? dqn : -1, tap == 0, acc, xf, xn);
                    tc = wrap ? 0 : tc + 1;
                    dq = dqn;
                }
            }
        }
        // the output pixel scattered by the group's (o_s, o_h0, o_w0); no residual on this route
        tile_epilogue<TN>(acc, a, dkey, nullptr, (unsigned)((size_t)a.N * a.OHt * a.OWt * a.K * 4), kb * KW, tile * 4 + wave, L.l31, L.h, [&](int tm, int i) {
            int orow, ocol;
            tile_pixel(oh0, ow0, wave, L.h, tm, i, orow, ocol);
            return (n * a.OHt + G.o_h0 + a.o_s * orow) * a.OWt + G.o_w0 + a.o_s * ocol;
        });
    }
}

// the strided layers' filter image: [group][K / 64][C / 32][stage of the group][plane][64 filters][32 channels] bf16.  Stage e of the flat
// list (groups in order) is forward filter tap (tr[e], tc[e]); FLIP = false: w is [R][S][C][K] (forward); true: w is the forward filter
// [R][S][K][C] of a data gradient computed as a correlation of dy (C = the forward's K), roles transposed (the flip is in the tap list)
struct X3sTaps {
    int ngroups, R, S;
    int st0[X3S_MAXPH + 1];       // first flat stage of each group
    int tr[64], tc[64];
};
template <bool FLIP>
__global__ void __launch_bounds__(256) x3s_filter_kernel(const float* __restrict__ w, unsigned short* __restrict__ w3, int C, int K, X3sTaps tp) {
    const int NH = C >> 5, KB = K / 64;
    const long long total = (long long)KB * NH * tp.st0[tp.ngroups] * 64 * 32;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e & 31), o = (int)((e >> 5) & 63);
    const int simg = (int)(e >> 11);                 // stage of the image
    int gi = 0;
    for (int q = 1; q < tp.ngroups; ++q)
        if (simg >= KB * NH * tp.st0[q]) gi = q;
    const int nst = tp.st0[gi + 1] - tp.st0[gi];
    const int loc = simg - KB * NH * tp.st0[gi];
    const int s = loc % nst, khh = loc / nst;
    const int hf = khh % NH, kb = khh / NH;
    const int r = tp.tr[tp.st0[gi] + s], c = tp.tc[tp.st0[gi] + s];
    const int ic = hf * 32 + i, oc = kb * 64 + o;
    const float v = FLIP ? w[(((size_t)r * tp.S + c) * K + oc) * C + ic] : w[(((size_t)r * tp.S + c) * C + ic) * K + oc];
    split3_write(w3 + (size_t)simg * 3 * 64 * 32 + (size_t)o * 32 + i, 64 * 32, v);
}

// PNP_X3_DIRECT / pnp_conv2d_x3_direct() and the strided layers' share of the route, PNP_X3_STRIDED / pnp_conv2d_x3_strided()
ModeSwitch x3d_switch{"PNP_X3_DIRECT", 1, 2, false}, x3s_switch{"PNP_X3_STRIDED", 1, 1, false};

// mode 1: layers with at least one (tile, filter block) item per CU — a persistent launch of fewer leaves CUs idle and the old route wins;
// mode 2: wherever the shapes allow (tests)
bool dims_ok(int R, int S, int stride, int dil, int C, int K, int OH, int OW, long long M) {
    if (!(R == 3 && S == 3 && stride == 1 && dil == 1 && (C == 32 || C == 64) && (K == 32 || K == 64 || K == 128) && (OH % TH) == 0 && (OW % TW) == 0 &&
          M * (long long)K < (1ll << 30)))
        return false;
    return x3d_switch.get() >= 2 || (M / (TH * TW)) * (K == 32 ? 1 : K / 64) >= 256;
}

// a strided layer's groups, phases and filter stages (kind 0: the forward of g; 1: its data gradient); false: not this route
struct X3sPlan {
    int ngroups, nitems, stride;
    X3sGroup grp[X3S_MAXPH];
    X3sPhase ph[X3S_MAXPH];
    X3sTaps taps;
};

bool x3s_plan(const pnp_conv_geom* g, int kind, X3sPlan* pl) {
    if (x3d_switch.get() <= 0 || x3s_switch.get() <= 0 || g->dtype != PNP_DTYPE_F32 || g->pad_mode != PNP_PAD_ZERO || g->dil != 1) return false;
    const int s = g->stride;
    if (s < 2 || s > 4 || g->R < s || g->S < s || g->R > 3 * s || g->S > 3 * s) return false;
    const int Cin = kind == 0 ? g->C : g->K, Kout = kind == 0 ? g->K : g->C;      // channels of the convolution this kernel computes
    if ((Cin % 32) != 0 || (Kout % 64) != 0) return false;
    const long long out_elems = kind == 0 ? (long long)g->N * g->OH * g->OW * g->K : (long long)g->N * g->H * g->W * g->C;
    if (out_elems >= (1ll << 30) || (long long)g->R * g->S > 64) return false;
    X3sPlan p{};
    p.stride = s;
    int ns = 0, items = 0;
    auto add_group = [&](int GH, int GW, int o_h0, int o_w0) -> bool {
        if (GH <= 0 || GW <= 0 || (GH % TH) != 0 || (GW % TW) != 0) return false;
        X3sGroup& G = p.grp[p.ngroups++];
        G.first_item = items;
        G.tiles_x = GW / TW; G.tiles_y = GH / TH;
        G.o_h0 = o_h0; G.o_w0 = o_w0;
        G.fbase = (Kout / 64) * (Cin / 32) * ns;          // (stages of the groups before this one; ns = their taps)
        items += g->N * G.tiles_x * G.tiles_y * (Kout / 64);
        return true;
    };
    if (kind == 0) {
        if (!add_group(g->OH, g->OW, 0, 0)) return false;
        X3sGroup& G = p.grp[0];
        G.ph0 = 0; G.nph = s * s; G.nst = g->R * g->S;
        p.taps.st0[0] = 0;
        for (int ra = 0; ra < s; ++ra)
            for (int cb = 0; cb < s; ++cb) {
                X3sPhase& P = p.ph[ra * s + cb];
                P.T = (g->R - ra + s - 1) / s; P.U = (g->S - cb + s - 1) / s;
                P.ih0 = ra - g->pad_t; P.iw0 = cb - g->pad_l;
                for (int t = 0; t < P.T; ++t)
                    for (int u = 0; u < P.U; ++u) { p.taps.tr[ns] = ra + s * t; p.taps.tc[ns] = cb + s * u; ++ns; }
            }
        p.taps.st0[1] = ns;
    } else {
        DgradPhase dp[16];
        const int nph = plan_phases(g, dp);
        if (nph != s * s) return false;
        for (int i = 0; i < nph; ++i) {
            const DgradPhase& q = dp[i];
            if (q.T > 3 || q.U > 3) return false;
            p.taps.st0[i] = ns;
            if (!add_group(q.I, q.J, q.h0, q.w0)) return false;
            X3sGroup& G = p.grp[i];
            G.ph0 = i; G.nph = 1; G.nst = q.T * q.U;
            X3sPhase& P = p.ph[i];
            P.T = q.T; P.U = q.U; P.ih0 = -q.pad_t; P.iw0 = -q.pad_l;
            for (int t = 0; t < q.T; ++t)                 // correlation tap (t, u) = forward tap (pa + s (T-1-t), pb + s (U-1-u))
                for (int u = 0; u < q.U; ++u) { p.taps.tr[ns] = q.pa + s * (q.T - 1 - t); p.taps.tc[ns] = q.pb + s * (q.U - 1 - u); ++ns; }
        }
        p.taps.st0[nph] = ns;
    }
    if (ns != g->R * g->S) return false;
    p.nitems = items;
    p.taps.ngroups = p.ngroups; p.taps.R = g->R; p.taps.S = g->S;
    // mode 1: at least one item per CU (a persistent launch of fewer leaves CUs idle), and only where it measured faster than the fp32-pipe
    // kernels — phase patches that serve >= 4 taps on average (k5s2: 25 taps over 4 patches), or data gradients of <= 64 dy channels (k3s2
    // 64@256, whose 1x1 / 1x2 phases run at 40-65 TF/s on the fp32 pipe); k3s2 with 2.25 taps per patch is bound by its patch loads
    // elsewhere (256@64, 512@32: 0.8-0.9x).  Mode 2: wherever the shapes allow (tests)
    if (x3d_switch.get() < 2 && (items < 256 || !(g->R * g->S >= 4 * s * s || (kind == 1 && Cin <= 64)))) return false;
    if (pl) *pl = p;
    return true;
}

// The pre-split filter image (6 bytes per filter value) at the head of the caller's workspace: the workspace is checked and
// launch(image, blocks) — the route's filter kernel, one thread of 256 per value — runs under its own profile row.  Returns the image, or
// null with the error in rc.
template <class Launch>
unsigned short* filter_image(const char* who, const char* kernel, int cls, bool flip, size_t fbytes, void* ws, size_t ws_bytes, hipStream_t st, int& rc, Launch&& launch) {
    rc = PNP_EWORKSPACE;
    if (!ws || ws_bytes < fbytes) {
        pnp_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, fbytes);
        return nullptr;
    }
    const long long total = (long long)(fbytes / 6);
    PnpProfScope ps(cls, st, 0.0, 4.0 * total + 6.0 * total, "%s<%s>", kernel, flip ? "true" : "false");
    launch((unsigned short*)ws, dim3((unsigned)pnp_cdiv(total, 256)));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        pnp_set_error("%s: launch failed: %s", kernel, hipGetErrorString(e));
        rc = PNP_ELAUNCH;
        return nullptr;
    }
    rc = PNP_OK;
    return (unsigned short*)ws;
}

}  // namespace

namespace pnpconv {

int x3d_route_mode() { return x3d_switch.get(); }

bool x3s_chosen(const pnp_conv_geom* g, int kind) { return x3s_plan(g, kind, nullptr); }

size_t x3s_filter_bytes(const pnp_conv_geom* g) { return (size_t)g->R * g->S * g->C * g->K * 6; }

// forward (kind 0: a = make_args(x, w, y, g)) or stride-phase data gradient (kind 1: a = make_args(dy, w, dx, g), w the FORWARD filter) of a
// strided layer x3s_chosen() takes; g = the forward geometry
int launch_x3_strided(const ConvArgs& a, const pnp_conv_geom* g, int kind, void* ws, size_t ws_bytes, hipStream_t st) {
    X3sPlan pl;
    if (!x3s_plan(g, kind, &pl)) {
        pnp_set_error("launch_x3_strided: layer not on this route");
        return PNP_EINVAL;
    }
    const size_t fbytes = x3s_filter_bytes(g);
    const int cls = prof_class(kind);
    const int Cin = kind == 0 ? g->C : g->K, Kout = kind == 0 ? g->K : g->C;
    int rc;
    unsigned short* w3 = filter_image("launch_x3_strided", "x3s_filter_kernel", cls, kind != 0, fbytes, ws, ws_bytes, st, rc, [&](unsigned short* img, dim3 blocks) {
        if (kind) hipLaunchKernelGGL((x3s_filter_kernel<true>), blocks, dim3(256), 0, st, a.w, img, Cin, Kout, pl.taps);
        else hipLaunchKernelGGL((x3s_filter_kernel<false>), blocks, dim3(256), 0, st, a.w, img, Cin, Kout, pl.taps);
    });
    if (!w3) return rc;
    X3sArgs x{};
    x.x = a.x; x.w3 = w3; x.y = a.y;
    x.N = g->N; x.C = Cin; x.K = Kout; x.NH = Cin / 32;
    if (kind == 0) { x.H = g->H; x.W = g->W; x.si = g->stride; x.OHt = g->OH; x.OWt = g->OW; x.o_s = 1; }
    else { x.H = g->OH; x.W = g->OW; x.si = 1; x.OHt = g->H; x.OWt = g->W; x.o_s = g->stride; }
    x.ngroups = pl.ngroups; x.nitems = pl.nitems;
    x.w3_bytes = (unsigned)fbytes;
    for (int i = 0; i < pl.ngroups; ++i) x.grp[i] = pl.grp[i];
    for (int i = 0; i < X3S_MAXPH; ++i) x.ph[i] = pl.ph[i];
    copy_dropout(x, a);
    x.stat_ws = kind == 0 ? a.stat_ws : nullptr; x.stat_shift = a.stat_shift;
    const dim3 grid((unsigned)(pl.nitems > 256 ? 256 : pl.nitems));
    // flops = the bf16 MFMA flops the kernel EXECUTES: six plane products per useful fp32 multiply-add (every forward tap exactly once per
    // output pixel of the forward, or per input pixel of the data gradient)
    const double fl = 6.0 * 2.0 * (double)g->N * g->OH * g->OW * g->R * g->S * g->C * g->K;
    const double by = 4.0 * ((double)g->N * x.H * x.W * Cin + (double)g->N * x.OHt * x.OWt * Kout) + 6.0 * g->R * g->S * g->C * g->K;
    PnpProfScope ps(cls, st, fl, by, "conv_x3_direct_kernel_strided<%d>", kind);
    if (kind) hipLaunchKernelGGL((conv_x3_direct_kernel_strided<1>), grid, dim3(512), 0, st, x);
    else hipLaunchKernelGGL((conv_x3_direct_kernel_strided<0>), grid, dim3(512), 0, st, x);
    PNP_CHECK_LAUNCH("conv_x3_direct_kernel_strided");
    return PNP_OK;
}

bool x3d_chosen(const pnp_conv_geom* g) {
    return x3d_switch.get() > 0 && g->dtype == PNP_DTYPE_F32 && (g->pad_mode == PNP_PAD_ZERO || (g->pad_t == 0 && g->pad_l == 0)) && dims_ok(g->R, g->S, g->stride, g->dil, g->C, g->K, g->OH, g->OW, (long long)g->N * g->OH * g->OW);
}

// one partial per consumer wave: 64 pixels (4 rows x 16) — M / 64 of them
int x3d_stats_parts(const pnp_conv_geom* g) { return (int)(((long long)g->N * g->OH * g->OW) / 64); }

size_t x3d_filter_bytes(int C, int K) { return (size_t)9 * C * K * 6; }

int launch_x3_direct(const ConvArgs& a, int kind, bool flip_transpose, void* ws, size_t ws_bytes, hipStream_t st) {
    PNP_REQUIRE(a.ep_scale == nullptr && a.y_h == nullptr && a.o_s == 0 && a.ups == 1, "launch_x3_direct: unsupported epilogue");
    const int cls = prof_class(kind);
    const int KW = a.K == 32 ? 32 : 64;
    int rc;
    unsigned short* w3 = filter_image("launch_x3_direct", "x3d_filter_kernel", cls, flip_transpose, x3d_filter_bytes(a.C, a.K), ws, ws_bytes, st, rc, [&](unsigned short* img, dim3 blocks) {
        if (flip_transpose) hipLaunchKernelGGL((x3d_filter_kernel<true>), blocks, dim3(256), 0, st, a.w, img, a.C, a.K, KW);
        else hipLaunchKernelGGL((x3d_filter_kernel<false>), blocks, dim3(256), 0, st, a.w, img, a.C, a.K, KW);
    });
    if (!w3) return rc;
    X3dArgs x{};
    x.x = a.x; x.w3 = w3; x.y = a.y;
    x.N = a.N; x.H = a.H; x.W = a.W; x.C = a.C; x.K = a.K; x.OH = a.OH; x.OW = a.OW; x.pad_t = a.pad_t; x.pad_l = a.pad_l; x.M = a.M;
    copy_dropout(x, a);
    x.res_add = a.res_add; x.stat_ws = a.stat_ws; x.stat_shift = a.stat_shift;
    const long long nitems = (long long)a.N * (a.OH / TH) * (a.OW / TW) * (a.K / KW);
    const dim3 grid((unsigned)(nitems > 256 ? 256 : nitems));
    // flops = the bf16 MFMA flops the kernel EXECUTES (six plane products per fp32 multiply-add): its roof is the dense bf16 peak
    const double fl = 6.0 * 2.0 * (double)a.M * 9.0 * a.C * a.K;
    const double by = 4.0 * ((double)a.N * a.H * a.W * a.C + (double)a.M * a.K) + 6.0 * 9.0 * a.C * a.K;
    PnpProfScope ps(cls, st, fl, by, "conv_x3_direct_kernel<%d, %d, %d>", a.C / 32, KW, kind);
#define X3D_LAUNCH(NH_, KW_, KIND_) hipLaunchKernelGGL((conv_x3_direct_kernel<NH_, KW_, KIND_>), grid, dim3(512), 0, st, x)
    if (a.C == 32) {
        if (KW == 32) { if (kind == 0) X3D_LAUNCH(1, 32, 0); else X3D_LAUNCH(1, 32, 1); }
        else { if (kind == 0) X3D_LAUNCH(1, 64, 0); else X3D_LAUNCH(1, 64, 1); }
    } else {
        if (KW == 32) { if (kind == 0) X3D_LAUNCH(2, 32, 0); else X3D_LAUNCH(2, 32, 1); }
        else { if (kind == 0) X3D_LAUNCH(2, 64, 0); else X3D_LAUNCH(2, 64, 1); }
    }
#undef X3D_LAUNCH
    PNP_CHECK_LAUNCH("conv_x3_direct_kernel");
    return PNP_OK;
}

}  // namespace pnpconv

extern "C" int32_t pnp_conv2d_x3_direct(int32_t mode) { return x3d_switch.set(mode); }

// the strided layers' share of that route (PNP_X3_STRIDED): 0 off, 1 on (where pnp_conv2d_x3_direct's mode allows)
extern "C" int32_t pnp_conv2d_x3_strided(int32_t mode) { return x3s_switch.set(mode); }
