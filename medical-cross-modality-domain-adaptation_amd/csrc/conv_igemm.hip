// conv_igemm.hip — NHWC x HWIO implicit-GEMM convolution on gfx950 fp32 matrix cores.
//
// Replaces tf.nn.conv2d / tf.nn.atrous_conv2d (+ tf.pad SYMMETRIC, + tf.nn.dropout) at
// /root/reference/layers.py:18,24,67,73,86,92 and their TF-autodiff gradients.
//
// GEMM view (no im2col buffer is ever materialised):
//   fwd  : Y[M=N*OH*OW][K]   = A[M][R*S*C] * Wm[R*S*C][K]       A gathered from x on the fly
//   dgrad: the same kernel on dy with flipped/transposed filters; stride > 1: one stride-1 correlation per stride phase (plan_phases)
//   wgrad: dW[R*S*C][K]      = At[R*S*C][P=N*OH*OW] * dY[P][K]  split over P across workgroups
//
// Matrix core: v_mfma_f32_32x32x2_f32 (exact fp32 fma chain, 64 FLOP/clk/SIMD = the 157 TF fp32 peak).
// Workgroup = 4 waves (256 threads); BK = 32 reduction elements per LDS stage; LDS double-buffered; global loads go through
// buffer descriptors (out-of-range offset = hardware zero: no branches for padding / ragged edges); a stage is a 4-slice register
// pipeline (Frag): ds_reads of slice q+1, the next stage's global loads and its LDS stores all fly under MFMAs; 1 barrier / stage.
//
// Kernels:
//   conv_taps_kernel        zero/VALID padding, C % 32 == 0, filter shapes 1x1..3x3 / 5x5, any stride (forward, stride-1 data gradient,
//                           stride-phase sub-filters): taps unrolled, scalar offsets; optional fused inference-BN epilogue
//   conv_fwd_kernel         everything else on the matrix cores (any C, in-kernel SYMMETRIC mirror, filters smaller than the stride)
//   conv_wgrad_kernel       filter gradient; reduction over pixels split across workgroups + split_sum.h's serial_kernel<Plain>
//   flip_transpose(_phase)_kernel, sympad_fwd/bwd_kernel, bn_fold_kernel, naive_conv_kernel
// The partial sums of every split reduction are split_sum.h's (serial_kernel<Plain / Drop / Scatter>, sliced_kernel<1>); the vector-ALU
// kernels of the K <= 16 layers (routes NARROW, WGD) live in conv_valu.hip.
// Host planners: choose_tile / choose_split (dispatch-round filling), plan_phases (strided data gradients), wgrad_plan_split, ring_tile
// answer "can / should this family take the layer", like the route files' predicates (conv_common.h).  plan_fwd / plan_dgrad /
// plan_wgrad alone COMBINE them: one cascade per pass, read by the workspace / partial-row / route queries (pnp_conv2d_*_workspace_bytes,
// pnp_conv2d_fwd_stats*_parts, pnp_conv2d_wino_chosen, pnp_conv2d_route; tests/test_abi.py) and by the entry points, which switch on the route.
// The plan also fixes the reduction split and the workspace layout (dgrad_ws): the launchers receive the planned split count and only fit
// it to the bytes the caller brought (fit_split); none of them calls choose_split / wgrad_plan_split.
// Shared pieces: conv_mma.h holds Frag and the stage schedule — PNP_MMA_STAGE is the whole stage of conv_taps_kernel, conv_wgrad_kernel,
// conv_wgrad_ring_kernel and conv_wino.hip's two GEMMs; conv_common.h the argument block, tile mapping, loads and epilogues.
//
// LDS layouts (dwords):
//   fwd  A tile  [BM][36]     row = output pixel, 32 k's contiguous (+4 pad). A fragments are read with
//                             ONE ds_read_b128 per 4 MFMAs: lane l takes k = 8q+4*(l>>5)+{0..3}; MFMA j of the
//                             group then contracts k-pair {8q+j, 8q+4+j} (a k-permutation, legal because the
//                             B fragment uses the same pairing).  Stride 36 dwords => 16-B slot = 9*row mod 16,
//                             a bijection over each b128 lane group => conflict-free (SQ_LDS_BANK_CONFLICT = 0 measured).
//   B tile       [32][BN+4]   row = k, n contiguous; fragment = ds_read_b32, lanes 0-31 consecutive => conflict-free.
//   wgrad A tile [32][BM+4]   row = pixel (reduction index), m' contiguous; ds_read_b32 like B.
#include "conv_common.h"
#include "conv_mma.h"
#include "split_sum.h"

using namespace pnpconv;

// Timing-experiment builds only (make variant NAME=trace EXTRA=-DPNP_TRACE=1): wave 0 of the first 256 workgroups of the two tap-unrolled
// forward kernels writes the shader clock at kernel entry, after the tile set-up, at the start of the main loop, after every stage's
// barrier, and around the epilogue; tools/experiments/stage_trace.py reads it back (pnp_debug_trace_read).  Never in the shipped library.
#ifdef PNP_TRACE
constexpr int TRACE_WG = 512, TRACE_N = 192;
__device__ unsigned long long g_trace[TRACE_WG][TRACE_N];
#define PNP_TRACE_MARK(slot)                                                                             \
    do {                                                                                                 \
        const unsigned tr_ = blockIdx.x - (gridDim.x > 4352u ? 4096u : 0u);      /* big launches: workgroups of the steady state */  \
        if (threadIdx.x == 0 && tr_ < (unsigned)TRACE_WG && (slot) < TRACE_N) g_trace[tr_][(slot)] = __builtin_readcyclecounter(); \
    } while (0)
extern "C" int pnp_debug_trace_read(void* host, size_t bytes) {
    if (bytes > sizeof(unsigned long long) * TRACE_WG * TRACE_N) bytes = sizeof(unsigned long long) * TRACE_WG * TRACE_N;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_trace), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#else
#define PNP_TRACE_MARK(slot) do { } while (0)
#endif

namespace {

// ---- B tile (weights for fwd, dy for wgrad): row-major [rows][ncols] global matrix ------------
template <int BN, bool VEC>
struct BLoader {
    static constexpr int C4 = BN / 4;             // float4 columns per row
    static constexpr int RP = NTHREADS / C4;      // rows per pass
    static constexpr int NP = BK / RP;            // passes
    static constexpr int LD = BN + 4;
    f32x4 reg[NP];
    int bcol, brow;
    __device__ __forceinline__ void init(int t) {
        bcol = t % C4;
        brow = t / C4;
    }
    // rows [k0, k0+32) of a [nrows][ncols] matrix, columns [n0, n0+BN)
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rb, int k0, int nrows, int ncols, int n0) {
        const int n = n0 + 4 * bcol;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int k = k0 + brow + RP * i;
            const bool rok = k < nrows;
            const unsigned base = (unsigned)(k * ncols + n) * 4u;
            if constexpr (VEC) {      // ncols % 4 == 0
                reg[i] = bload4(rb, (rok && n < ncols) ? base : OOB);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) reg[i][e] = bload1(rb, (rok && n + e < ncols) ? base + 4u * e : OOB);
            }
        }
    }
    __device__ __forceinline__ void store(float* lds) const {
#pragma unroll
        for (int i = 0; i < NP; ++i)
            *reinterpret_cast<f32x4*>(lds + (brow + RP * i) * LD + 4 * bcol) = reg[i];
    }
};

// ---- fwd A tile: [BM pixels][32 k] gathered from x ---------------------------------------------
// MODE 0: C % 32 == 0 (whole stage shares one filter tap), 1: C % 4 == 0, 2: any C (scalar)
template <int BM, int MODE, bool UPS>
struct FwdALoader {
    static constexpr int NR = BM / 32;   // rows per thread
    static constexpr int LD = BK + 4;
    f32x4 reg[NR];
    int kg, mrow;
    int pixbase[NR], vh0[NR], vw0[NR];
    unsigned valid;
    __device__ __forceinline__ void init(int t, int m0, const ConvArgs& a) {
        kg = t & 7;
        mrow = t >> 3;
        valid = 0;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            int m = m0 + mrow + 32 * i;
            bool ok = m < a.M;
            if (!ok) m = 0;
            int n, oh, ow;
            split_row(a, m, n, oh, ow);
            pixbase[i] = n * a.H * a.W;
            vh0[i] = oh * a.stride - a.pad_t;
            vw0[i] = ow * a.stride - a.pad_l;
            if (ok) valid |= 1u << i;
        }
    }
    // byte offset of x[pixel(i, tap rs)][c], or OOB when the tap reads padding / the row is past M
    __device__ __forceinline__ unsigned offset(const ConvArgs& a, int i, int rs, int c, bool kok) const {
        int r = rs / a.S;
        int s = rs - r * a.S;
        int ih = 0, iw = 0;
        bool ok = kok && ((valid >> i) & 1u);
        ok = map_coord<UPS>(vh0[i] + r * a.dil, a.H, a.ups, a.pad_mode, ih) & ok;
        ok = map_coord<UPS>(vw0[i] + s * a.dil, a.W, a.ups, a.pad_mode, iw) & ok;
        return ok ? (unsigned)((pixbase[i] + ih * a.W + iw) * a.C + c) * 4u : OOB;
    }
    // MODE 4 (C % 4 == 0, C >= 16, zero padding, no upsampling): (tap row, tap col, channel) of this thread's 4 k's are carried
    // from stage to stage (k advances by 32: at most two channel wraps because C >= 16) instead of being re-derived by two integer
    // divisions, and the zero-padding test is two unsigned compares — ~40 VALU per stage instead of ~150.  The C = 16 layers at
    // 256^2 and the 40 -> 5 output convolution are VALU-bound on this arithmetic, not on the MFMAs.
    int i_k, i_c, i_s, i_r;
    int rowoff[NR];
    __device__ __forceinline__ void init4(const ConvArgs& a, int k_first) {
        i_k = k_first + 4 * kg;
        const int rs = i_k / a.C;
        i_c = i_k - rs * a.C;
        i_r = rs / a.S;
        i_s = rs - i_r * a.S;
#pragma unroll
        for (int i = 0; i < NR; ++i) rowoff[i] = (pixbase[i] + vh0[i] * a.W + vw0[i]) * a.C;
    }
    __device__ __forceinline__ void load4(const ConvArgs& a, __amdgpu_buffer_rsrc_t rx) {
        const bool kok = i_k < a.Kred;
        const int dh = i_r * a.dil, dw = i_s * a.dil;
        const int tsh = (dh * a.W + dw) * a.C + i_c;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const bool ok = kok & (((valid >> i) & 1u) != 0) & ((unsigned)(vh0[i] + dh) < (unsigned)a.H) &
                            ((unsigned)(vw0[i] + dw) < (unsigned)a.W);
            reg[i] = bload4(rx, ok ? (unsigned)((rowoff[i] + tsh) * 4) : OOB);
        }
        i_k += BK;
        i_c += BK;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const bool c1 = i_c >= a.C;
            i_c -= c1 ? a.C : 0;
            i_s += c1 ? 1 : 0;
            const bool c2 = i_s >= a.S;
            i_s -= c2 ? a.S : 0;
            i_r += c2 ? 1 : 0;
        }
    }
    __device__ __forceinline__ void load(const ConvArgs& a, __amdgpu_buffer_rsrc_t rx, int k0) {
        if constexpr (MODE == 4) {          // stages are visited in order: the carried state IS k0
            load4(a, rx);
            return;
        }
        if constexpr (MODE == 0) {
            int rs = k0 / a.C;                 // block-uniform
            int c = k0 - rs * a.C + 4 * kg;
            const bool kok = k0 < a.Kred;
#pragma unroll
            for (int i = 0; i < NR; ++i) reg[i] = bload4(rx, offset(a, i, rs, c, kok));
        } else if constexpr (MODE == 1) {
            int kf = k0 + 4 * kg;
            int rs = kf / a.C;
            int c = kf - rs * a.C;
            const bool kok = kf < a.Kred;      // C%4==0 => Kred%4==0 => whole float4 in range
#pragma unroll
            for (int i = 0; i < NR; ++i) reg[i] = bload4(rx, offset(a, i, rs, c, kok));
        } else {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int kf = k0 + 4 * kg + e;
                    int rs = kf / a.C;
                    reg[i][e] = bload1(rx, offset(a, i, rs, kf - rs * a.C, kf < a.Kred));
                }
        }
    }
    __device__ __forceinline__ void store(float* lds) const {
#pragma unroll
        for (int i = 0; i < NR; ++i)
            *reinterpret_cast<f32x4*>(lds + (mrow + 32 * i) * LD + 4 * kg) = reg[i];
    }
};

// ---- wgrad A tile: [32 pixels][BM m'] gathered from x, m' = (r*S+s)*C + c ----------------------
// MODE 1: C % 4 == 0 (a thread's 4 consecutive m' share the tap), 2: any C
template <int BM, int MODE>
struct WgradALoader {
    static constexpr int C4 = BM / 4;
    static constexpr int RP = NTHREADS / C4;
    static constexpr int NP = BK / RP;
    static constexpr int LD = BM + 4;
    f32x4 reg[NP];
    int acol, arow;
    int rs_u, c_u;          // MODE 1: this thread's tap and channel (fixed for the whole kernel)
    bool mok;               // MODE 1: m' in range
    int mm;                 // first m' of this thread
    // MODE 3 (stride 1, zero padding, OW >= 32, C % 4 == 0): the reduction index p (output pixel) advances by 32 per stage, so the
    // pixel coordinates and the input byte offset are carried incrementally — no integer division and ~12 VALU per row per stage
    // instead of ~70 (three divisions) in the general path.
    int l_ow[NP], l_oh[NP], l_off[NP];
    int l_dh, l_dw;         // tap displacement: r*dil - pad_t, s*dil - pad_l
    __device__ __forceinline__ void init(int t, int mm0, const ConvArgs& a, int p_first = 0) {
        acol = t % C4;
        arow = t / C4;
        mm = mm0 + 4 * acol;
        mok = mm < a.Kred;
        int m_ = mok ? mm : 0;
        rs_u = m_ / a.C;
        c_u = m_ - rs_u * a.C;
        if constexpr (MODE == 3) {
            const int r = rs_u / a.S, s = rs_u - r * a.S;
            l_dh = r * a.dil - a.pad_t;
            l_dw = s * a.dil - a.pad_l;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int p = p_first + arow + RP * i;
                const int n = p / a.OHW;
                const int rem = p - n * a.OHW;
                l_oh[i] = rem / a.OW;
                l_ow[i] = rem - l_oh[i] * a.OW;
                l_off[i] = (((n * a.H + l_oh[i] + l_dh) * a.W + l_ow[i] + l_dw) * a.C + c_u) * 4;
            }
        }
    }
    // MODE 3: fetch the rows at the current position, then advance every row by 32 output pixels
    __device__ __forceinline__ void load_advance(const ConvArgs& a, __amdgpu_buffer_rsrc_t rx, int pend) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            // (no test against the end of the pixel range: splits end on stage boundaries, and rows past the LAST pixel either land
            // past the end of x -> 0 from the hardware, or meet a dy row past the end of dy -> 0)
            const bool ok = mok & ((unsigned)(l_oh[i] + l_dh) < (unsigned)a.H) & ((unsigned)(l_ow[i] + l_dw) < (unsigned)a.W);
            reg[i] = bload4(rx, ok ? (unsigned)l_off[i] : OOB);
            l_ow[i] += BK;
            l_off[i] += BK * a.C * 4;
            const bool ww = l_ow[i] >= a.OW;                    // at most one wrap per step because OW >= 32
            l_ow[i] -= ww ? a.OW : 0;
            l_oh[i] += ww ? 1 : 0;
            l_off[i] += ww ? (a.W - a.OW) * a.C * 4 : 0;
            const bool hw = l_oh[i] >= a.OH;
            l_oh[i] -= hw ? a.OH : 0;
            l_off[i] += hw ? (a.H - a.OH) * a.W * a.C * 4 : 0;
        }
    }
    __device__ __forceinline__ unsigned offset(const ConvArgs& a, int p, int rs, int c, bool ok) const {
        int n = p / a.OHW;
        int rem = p - n * a.OHW;
        int oh = rem / a.OW;
        int ow = rem - oh * a.OW;
        int r = rs / a.S;
        int s = rs - r * a.S;
        int ih = 0, iw = 0;
        ok = map_coord<false>(oh * a.stride - a.pad_t + r * a.dil, a.H, 1, a.pad_mode, ih) & ok;
        ok = map_coord<false>(ow * a.stride - a.pad_l + s * a.dil, a.W, 1, a.pad_mode, iw) & ok;
        return ok ? (unsigned)(((n * a.H + ih) * a.W + iw) * a.C + c) * 4u : OOB;
    }
    __device__ __forceinline__ void load(const ConvArgs& a, __amdgpu_buffer_rsrc_t rx, int p0, int pend) {
        if constexpr (MODE == 3) {          // stages are visited in order: the carried state IS p0
            load_advance(a, rx, pend);
            return;
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = p0 + arow + RP * i;
            const bool pok = p < pend;
            const int pp = pok ? p : 0;
            if constexpr (MODE <= 1 || MODE == 3) {
                reg[i] = bload4(rx, offset(a, pp, rs_u, c_u, pok && mok));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int m_ = mm + e;
                    const int rs = m_ / a.C;
                    reg[i][e] = bload1(rx, offset(a, pp, rs, m_ - rs * a.C, pok && m_ < a.Kred));
                }
            }
        }
    }
    __device__ __forceinline__ void store(float* lds) const {
#pragma unroll
        for (int i = 0; i < NP; ++i)
            *reinterpret_cast<f32x4*>(lds + (arow + RP * i) * LD + 4 * acol) = reg[i];
    }
};

// ================================ forward / dgrad kernel ========================================
// KIND 0 = forward, 1 = data gradient of a stride-1 convolution, 2 = data gradient of a strided convolution (input = dy
// zero-upsampled by `ups`).  0 and 1 run the same code; the distinct symbol lets rocprof separate forward from backward
// launches.  Only KIND 2 carries the integer division of the upsampling test.
template <int BM, int BN, int WM, int WN, int MODE, int KIND, bool VECB>
__device__ __forceinline__ void conv_fwd_body(ConvArgs a, const int blk) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BK + 4, LDB = BN + 4;
    constexpr int ASZ = BM * LDA, BSZ = BK * LDB;
    __shared__ __attribute__((aligned(16))) float lds[2 * (ASZ + BSZ)];

    if constexpr (KIND != 2) a.ups = 1;
    // Two workgroups share a CU (one wave each per SIMD).  Their stage loops run at the same rate, so whatever phase offset they
    // start with persists; dispatched together they stay aligned and the matrix pipe idles whenever both are in the non-MFMA part of
    // a stage (barrier, first fragment reads, LDS stores).  Starting every second dispatch wave late by about that part's length
    // de-phases them for the whole kernel.  (Speed only: nothing depends on which workgroups share a CU.)
    if (a.stagger > 0 && ((blk >> 8) & 1)) {
        for (int i = 0; i < a.stagger; ++i) __builtin_amdgcn_s_sleep(16);
    }
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nblk = a.nblk_m * a.nblk_n;
    const int z = blk / nblk;                      // reduction split (data gradients only; a.nsplit == 1 otherwise)
    int bid = blk - z * nblk;
    if (a.xcd_swizzle) bid = xcd_remap(bid, nblk);
    int mt, nt;
    tile_coords(bid, a.nblk_m, a.nblk_n, a.gn, mt, nt);
    const int m0 = mt * BM, n0 = nt * BN;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);

    FwdALoader<BM, MODE, KIND == 2> la;
    BLoader<BN, VECB> lb;
    la.init(t, m0, a);
    if constexpr (MODE == 4) la.init4(a, z * a.chunks_per_split * BK);
    lb.init(t);

    Acc<TM, TN> acc;
    acc.zero();

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, a.w_bytes);
    const int nchunks_total = (a.Kred + BK - 1) / BK;
    const int c_begin = z * a.chunks_per_split;
    const int c_end = (c_begin + a.chunks_per_split < nchunks_total) ? c_begin + a.chunks_per_split : nchunks_total;
    const int nchunks = c_end - c_begin;
    // Reduction order.  MODE 0 (C % 32 == 0): channel-group major, filter tap minor — the R*S stages that re-read the same input
    // pixels (shifted by one tap) run back to back, so the re-reads hit the XCD's L2.  The sum is order-independent up to fp32
    // rounding; the filter rows are visited in the matching order.  Stage index past c_end: every offset out of range -> zeros.
    auto stage_k0 = [&](int ci) {
        int k0 = ci * BK;
        if constexpr (MODE == 0) {
            const int rs_n = a.R * a.S;
            const int cc = ci / rs_n;
            k0 = (ci - cc * rs_n) * a.C + cc * BK;
        }
        return (ci < c_end) ? k0 : a.Kred;
    };
    {
        const int k0 = stage_k0(c_begin);
        la.load(a, rx, k0);
        lb.load(rw, k0, a.Kred, a.K, n0);
    }
    la.store(lds);
    lb.store(lds + 2 * ASZ);
    __syncthreads();
    Frag<TM, TN, true, LDA, LDB> f0, f1;
    f0.load(lds, lds + 2 * ASZ, 0, wm0, wn0, lane);
    // Main loop — ONE basic block per stage (no branches: the prefetch past the last stage reads out of range = zeros
    // and lands in the LDS buffer nobody reads).  Per stage and wave: 64 MFMAs in 4 slices of 16; under slice q the
    // ds_reads of slice q+1 are in flight; the next stage's global loads are issued under slice 0 and written to the
    // other LDS buffer under slice 3; only the 6 reads of the next stage's slice 0 are exposed after the barrier.  (Not PNP_MMA_STAGE:
    // here the stores follow ALL MFMAs of slice 3, a different schedule.)
    for (int c = 0; c < nchunks; ++c) {
        const int cur = c & 1;
        const float* As = lds + cur * ASZ;
        const float* Bs = lds + 2 * ASZ + cur * BSZ;
        float* An = lds + (cur ^ 1) * ASZ;
        float* Bn = lds + 2 * ASZ + (cur ^ 1) * BSZ;
        const int k0 = stage_k0(c_begin + c + 1);
        // ---- slice 0
        f1.load(As, Bs, 1, wm0, wn0, lane);
        la.load(a, rx, k0);
        lb.load(rw, k0, a.Kred, a.K, n0);
        f0.mma(acc);
        // interleave: the 6 ds_reads first, then per MFMA a handful of the address VALU/SALU and, when its address is
        // ready, one buffer_load — the ~130 address instructions of the next stage ride in the shadow of the 16 MFMAs
        // (64 cycles each) instead of in front of them.
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
        for (int i = 0; i < 4 * TM * TN; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x006, 10, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        PNP_SCHED_FENCE();
        // ---- slice 1
        f0.load(As, Bs, 2, wm0, wn0, lane);
        PNP_SCHED_FENCE();
        f1.mma(acc);
        PNP_SCHED_FENCE();
        // ---- slice 2
        f1.load(As, Bs, 3, wm0, wn0, lane);
        PNP_SCHED_FENCE();
        f0.mma(acc);
        PNP_SCHED_FENCE();
        // ---- slice 3: MFMAs first, THEN the LDS stores of the next stage.  The stores need the global loads issued under slice 0;
        // measured load-to-use latency under this traffic is ~3000 cycles (ablation: load->LDS->barrier chain alone 2.3 us per
        // stage), so waiting for them before the slice-3 MFMAs (2100 cycles after issue) stalled the matrix pipe ~20 %.
        f1.mma(acc);
        PNP_SCHED_FENCE();
        la.store(An);
        lb.store(Bn);
        PNP_SCHED_FENCE();
        __syncthreads();
        f0.load(An, Bn, 0, wm0, wn0, lane);
    }

    conv_epilogue<TM, TN>(a, acc, a.y + (size_t)z * a.split_stride, m0, n0, wm0, wn0, lane, mt * WM + wave / WN, z == 0);
}

template <int BM, int BN, int WM, int WN, int MODE, int KIND, bool VECB>
__global__ void __launch_bounds__(NTHREADS, 2) conv_fwd_kernel(ConvArgs a) {
    conv_fwd_body<BM, BN, WM, WN, MODE, KIND, VECB>(a, (int)blockIdx.x);
}

// ---- all stride phases of a strided data gradient in ONE launch (small feature maps) -------------------------------------------------
// A k5 s4 critic layer on a 16^2 -> 4^2 map has 16 phases of 256 GEMM rows each: one launch per phase (16 workgroups, reduction split
// 32 ways, + a scatter-reduce) cost 16 x (17 + 4.5) us for 3.4 GFLOP.  Here the workgroups of all phases share one grid; a workgroup
// looks up its phase (sub-filter extent / padding / output lattice / filter block) in the kernel arguments and runs the general
// C % 32 == 0 stage loop, writing its rows straight to the phase's pixels (no reduction split, no second kernel).
struct PhaseDesc {
    int w_off;              // float offset of the phase's flipped sub-filter [T][U][K][C]
    int R, S, OH, OW, pad_t, pad_l, o_h0, o_w0;
    int first_blk, nblk_m;
};
struct GroupArgs {
    ConvArgs base;          // everything the phases share (x = dy, y = dx, H/W = dy's extent, C, K, output lattice o_s/o_H/o_W, tiles in N)
    PhaseDesc ph[16];
    int nph;
};

template <int BM, int BN, int WM, int WN>
__global__ void __launch_bounds__(NTHREADS, 2) conv_dgrad_phases_kernel(GroupArgs g) {
    int p = 0;
    for (int i = 1; i < g.nph; ++i) p = ((int)blockIdx.x >= g.ph[i].first_blk) ? i : p;
    const PhaseDesc d = g.ph[p];
    ConvArgs a = g.base;
    a.w = g.base.w + d.w_off;
    a.R = d.R; a.S = d.S; a.OH = d.OH; a.OW = d.OW; a.pad_t = d.pad_t; a.pad_l = d.pad_l;
    a.o_h0 = d.o_h0; a.o_w0 = d.o_w0;
    a.OHW = d.OH * d.OW;
    a.ow_sh = a.ohw_sh = -1;                  // per-phase extents: divide
    a.M = a.N * a.OHW;
    a.Kred = d.R * d.S * a.C;
    a.w_bytes = (unsigned)(a.Kred * a.K) * 4u;
    a.nblk_m = d.nblk_m;
    a.nsplit = 1;
    a.chunks_per_split = (a.Kred + BK - 1) / BK;
    conv_fwd_body<BM, BN, WM, WN, 0, 1, true>(a, (int)blockIdx.x - d.first_blk);
}

// ============ forward (any stride) / stride-1 data gradient, zero padding, C % 32 == 0, RxS filter: taps unrolled ============
// The common case on the reference path (every 3x3 SAME conv from group_2 on and their dgrads, the strided 3x3 / 5x5 critic convs,
// and the stride-phase sub-filters 1x1 ... 3x3 of their data gradients).  With the filter taps unrolled at compile time the per-stage
// address work collapses:
//   A:  voffset = pixel_base(row) + tap_shift   (1 v_add + 1 v_cndmask per row; validity = one bit per (row, tap), set up once)
//       soffset = channel-group * 128 bytes      (scalar)
//   B:  voffset = constant per thread, soffset = (tap*C + channel-group*32) * K * 4   (scalar)
// i.e. ~16 VALU per stage instead of ~130 (the general kernel re-derives tap, mirror/zero test and pixel offset per row per stage).

// Two waves per SIMD: three for the 128x64 / 128x32 tiles (their LDS would fit three workgroups; <= 168 VGPRs) measured no gain
// (tools/experiments/README.md, round 3 run 1).
template <int BM, int BN, int WM, int WN, int KIND, int R, int S>
__global__ void __launch_bounds__(NTHREADS, 2) conv_taps_kernel(ConvArgs a) {
    constexpr int NTAP = R * S;
    static_assert(NTAP <= 32, "one validity bit per tap");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BK + 4, LDB = BN + 4;
    constexpr int ASZ = BM * LDA, BSZ = BK * LDB;
    constexpr int NR = BM / 32;
    constexpr int C4 = BN / 4, RPB = NTHREADS / C4, NPB = BK / RPB;
    __shared__ __attribute__((aligned(16))) float lds[2 * (ASZ + BSZ)];

    PNP_TRACE_MARK(0);
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nblk = a.nblk_m * a.nblk_n;
    const int z = blockIdx.x / nblk;
    int bid = blockIdx.x - z * nblk;
    if (a.xcd_swizzle) bid = xcd_remap(bid, nblk);
    int mt, nt;
    tile_coords(bid, a.nblk_m, a.nblk_n, a.gn, mt, nt);
    const int m0 = mt * BM, n0 = nt * BN;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);

    // ---- per-thread A rows: byte offset of (pixel shifted by -pad) and the validity bit of every tap -------------------
    const int kg = t & 7, mrow = t >> 3;
    int abase[NR];
    unsigned amask[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        int m = m0 + mrow + 32 * i;
        const bool ok = m < a.M;
        if (!ok) m = 0;
        int n, oh, ow;
        split_row(a, m, n, oh, ow);
        const int vh0 = oh * a.stride - a.pad_t, vw0 = ow * a.stride - a.pad_l;
        abase[i] = (((n * a.H + vh0) * a.W + vw0) * a.C + 4 * kg) * 4;
        // tap (r, s) is valid iff its row AND its column are inside the image: R + S tests and R shifted ORs instead of R*S full tests
        unsigned wm = 0, mk = 0;
#pragma unroll
        for (int sx = 0; sx < S; ++sx) wm |= ((unsigned)(vw0 + sx * a.dil) < (unsigned)a.W ? 1u : 0u) << sx;
#pragma unroll
        for (int ry = 0; ry < R; ++ry) mk |= ((unsigned)(vh0 + ry * a.dil) < (unsigned)a.H ? wm : 0u) << (ry * S);
        amask[i] = ok ? mk : 0u;
    }
    // ---- per-thread B rows ------------------------------------------------------------------------------------------
    const int bcol = t % C4, brow = t / C4;
    unsigned boff[NPB];
#pragma unroll
    for (int i = 0; i < NPB; ++i)
        boff[i] = (n0 + 4 * bcol < a.K) ? (unsigned)(((brow + RPB * i) * a.K + n0 + 4 * bcol) * 4) : OOB2;

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, a.w_bytes);
    f32x4 areg[NR], breg[NPB];
    auto gload = [&](int cc, int tap) {     // tap is a compile-time constant at every call site (unrolled)
        const int tshift = (((tap / S) * a.dil * a.W + (tap % S) * a.dil) * a.C) * 4;
        const int sa = cc * (BK * 4);
        const int sb = ((tap * a.C + cc * BK) * a.K) * 4;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const unsigned vo = ((amask[i] >> tap) & 1u) ? (unsigned)(abase[i] + tshift) : OOB2;
            areg[i] = bload4s(rx, vo, sa);
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) breg[i] = bload4s(rw, boff[i], sb);
    };
    auto lstore = [&](float* An, float* Bn) {
#pragma unroll
        for (int i = 0; i < NR; ++i) *reinterpret_cast<f32x4*>(An + (mrow + 32 * i) * LDA + 4 * kg) = areg[i];
#pragma unroll
        for (int i = 0; i < NPB; ++i) *reinterpret_cast<f32x4*>(Bn + (brow + RPB * i) * LDB + 4 * bcol) = breg[i];
    };

    Acc<TM, TN> acc;
    acc.zero();

    // reduction range of this workgroup in channel groups (a.chunks_per_split is a multiple of NTAP on this path)
    const int ncc_total = a.C / BK;
    const int cc_begin = z * (a.chunks_per_split / NTAP);
    int cc_end = cc_begin + a.chunks_per_split / NTAP;
    if (cc_end > ncc_total) cc_end = ncc_total;

    PNP_TRACE_MARK(1);
    gload(cc_begin, 0);
    lstore(lds, lds + 2 * ASZ);
    __syncthreads();
    PNP_TRACE_MARK(2);
    Frag<TM, TN, true, LDA, LDB> f0, f1;
    f0.load(lds, lds + 2 * ASZ, 0, wm0, wn0, lane);
    int sc = 0;   // stage counter (LDS buffer parity)
    for (int cc = cc_begin; cc < cc_end; ++cc) {
#pragma unroll
        for (int tap = 0; tap < NTAP; ++tap) {
            const int cur = sc & 1;
            ++sc;
            const float* As = lds + cur * ASZ;
            const float* Bs = lds + 2 * ASZ + cur * BSZ;
            float* An = lds + (cur ^ 1) * ASZ;
            float* Bn = lds + 2 * ASZ + (cur ^ 1) * BSZ;
            // next stage: next tap of this channel group, or tap 0 of the next group; past the end the last group is simply
            // fetched again (valid addresses, lands in the LDS buffer nobody reads)
            const int ntap = (tap + 1 < NTAP) ? tap + 1 : 0;
            int ncc = (tap + 1 < NTAP) ? cc : cc + 1;
            ncc = (ncc < cc_end) ? ncc : cc;
            PNP_MMA_STAGE(4, 8, 4 * TM * TN, gload(ncc, ntap), lstore(An, Bn))
            PNP_TRACE_MARK(3 + sc);
            f0.load(An, Bn, 0, wm0, wn0, lane);
        }
    }
    PNP_TRACE_MARK(4 + sc);

    conv_epilogue<TM, TN>(a, acc, a.y + (size_t)z * a.split_stride, m0, n0, wm0, wn0, lane, mt * WM + wave / WN, z == 0);
    PNP_TRACE_MARK(5 + sc);
}

// ---- the same tap-unrolled convolution with THREE LDS stages and a register ring of two global-load stages (narrow tiles) ------------
// A 128x64 stage carries 32 MFMAs per wave — half of a 128x128 stage — for the same fixed part: barrier, the fragment reads of the next
// stage's first slice that can only start behind it, and a global-load-to-LDS-store distance of three slices (24 MFMAs of cover instead of
// 48).  PMC on the two-stage kernel: SQ_WAIT_INST_LDS per MFMA 1.05 against 0.50 on the wide tile, matrix-pipe utilisation 0.71 against
// 0.92.  With a third LDS stage (3 x 27 KB = 81 408 B: two workgroups still fit a CU's 160 KB, to the byte) the barrier of stage s
// publishes the data of stage s+2, so everything stage s+1 needs is already visible while stage s runs:
//   * the first-slice fragment reads of stage s+1 are issued under the LAST slice of stage s, before the barrier — nothing is exposed
//     behind it;
//   * global loads run TWO stages ahead of their LDS store (ring of two register sets: one whole stage more cover).
// Buffer rotation: stage s computes from LDS stage s % 3, stores the registers that hold stage s+2 into (s+2) % 3 (last read in stage
// s-1: every wave is past that stage's barrier), and requests stage s+3 from memory.  The ring index must be a compile-time constant, so
// the channel-group loop is unrolled by two where the tap count is odd; the host only picks this kernel when the workgroup's channel
// groups come in pairs then (C % 64 == 0 and an un-split or evenly split reduction: every layer of the model that runs narrow tiles).
template <int BM, int BN, int WM, int WN, int KIND, int R, int S>
__global__ void __launch_bounds__(NTHREADS, 2) conv_taps3_kernel(ConvArgs a) {
    constexpr int NTAP = R * S;
    static_assert(NTAP <= 32, "one validity bit per tap");
    constexpr int CCU = (NTAP & 1) ? 2 : 1;          // channel groups per loop trip: an even number of stages
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BK + 4, LDB = BN + 4;
    constexpr int ASZ = BM * LDA, BSZ = BK * LDB, STG = ASZ + BSZ;
    constexpr int NR = BM / 32;
    constexpr int C4 = BN / 4, RPB = NTHREADS / C4, NPB = BK / RPB;
    static_assert(3 * STG * 4 <= 81920, "three stages must leave room for two workgroups per CU");
    __shared__ __attribute__((aligned(16))) float lds[3 * STG];

    PNP_TRACE_MARK(0);
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nblk = a.nblk_m * a.nblk_n;
    const int z = blockIdx.x / nblk;
    int bid = blockIdx.x - z * nblk;
    if (a.xcd_swizzle) bid = xcd_remap(bid, nblk);
    int mt, nt;
    tile_coords(bid, a.nblk_m, a.nblk_n, a.gn, mt, nt);
    const int m0 = mt * BM, n0 = nt * BN;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);

    const int kg = t & 7, mrow = t >> 3;
    int abase[NR];
    unsigned amask[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        int m = m0 + mrow + 32 * i;
        const bool ok = m < a.M;
        if (!ok) m = 0;
        int n, oh, ow;
        split_row(a, m, n, oh, ow);
        const int vh0 = oh * a.stride - a.pad_t, vw0 = ow * a.stride - a.pad_l;
        abase[i] = (((n * a.H + vh0) * a.W + vw0) * a.C + 4 * kg) * 4;
        // tap (r, s) is valid iff its row AND its column are inside the image: R + S tests and R shifted ORs instead of R*S full tests
        unsigned wm = 0, mk = 0;
#pragma unroll
        for (int sx = 0; sx < S; ++sx) wm |= ((unsigned)(vw0 + sx * a.dil) < (unsigned)a.W ? 1u : 0u) << sx;
#pragma unroll
        for (int ry = 0; ry < R; ++ry) mk |= ((unsigned)(vh0 + ry * a.dil) < (unsigned)a.H ? wm : 0u) << (ry * S);
        amask[i] = ok ? mk : 0u;
    }
    const int bcol = t % C4, brow = t / C4;
    unsigned boff[NPB];
#pragma unroll
    for (int i = 0; i < NPB; ++i)
        boff[i] = (n0 + 4 * bcol < a.K) ? (unsigned)(((brow + RPB * i) * a.K + n0 + 4 * bcol) * 4) : OOB2;

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, a.w_bytes);
    struct Regs {
        f32x4 a[NR];
        f32x4 b[NPB];
    };
    Regs ring[2];
    auto gload = [&](Regs& r, int cc, int tap) {     // tap is a compile-time constant at every call site (unrolled)
        const int tshift = (((tap / S) * a.dil * a.W + (tap % S) * a.dil) * a.C) * 4;
        const int sa = cc * (BK * 4);
        const int sb = ((tap * a.C + cc * BK) * a.K) * 4;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const unsigned vo = ((amask[i] >> tap) & 1u) ? (unsigned)(abase[i] + tshift) : OOB2;
            r.a[i] = bload4s(rx, vo, sa);
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) r.b[i] = bload4s(rw, boff[i], sb);
    };
    auto lstore = [&](const Regs& r, float* An, float* Bn) {
#pragma unroll
        for (int i = 0; i < NR; ++i) *reinterpret_cast<f32x4*>(An + (mrow + 32 * i) * LDA + 4 * kg) = r.a[i];
#pragma unroll
        for (int i = 0; i < NPB; ++i) *reinterpret_cast<f32x4*>(Bn + (brow + RPB * i) * LDB + 4 * bcol) = r.b[i];
    };

    Acc<TM, TN> acc;
    acc.zero();

    const int ncc_total = a.C / BK;
    const int cc_begin = z * (a.chunks_per_split / NTAP);
    int cc_end = cc_begin + a.chunks_per_split / NTAP;
    if (cc_end > ncc_total) cc_end = ncc_total;
    const int cc_last = cc_end - 1;
    // (stage index -> (channel group, tap)) d stages after (cc, tap); past the end the last group is fetched again (never contracted)
#define PNP_T3_CC(cc, tap, d) (((cc) + ((tap) + (d)) / NTAP) < cc_end ? ((cc) + ((tap) + (d)) / NTAP) : cc_last)
#define PNP_T3_TAP(tap, d) (((tap) + (d)) % NTAP)

    // prologue: stages 0 and 1 into LDS, stage 2 in flight in ring[0]
    PNP_TRACE_MARK(1);
    int tsc = 0;
    (void)tsc;
    gload(ring[0], cc_begin, 0);
    gload(ring[1], PNP_T3_CC(cc_begin, 0, 1), PNP_T3_TAP(0, 1));
    lstore(ring[0], lds, lds + ASZ);
    gload(ring[0], PNP_T3_CC(cc_begin, 0, 2), PNP_T3_TAP(0, 2));
    lstore(ring[1], lds + STG, lds + STG + ASZ);
    __syncthreads();
    // Fragment ring of four 8-k slices: slice q of a stage is contracted while slice q+2 is being read — two slices (16 MFMAs of a 2x1
    // wave tile) of cover for every LDS read instead of one, and the lookahead runs across the stage boundary (the next stage is visible)
    Frag<TM, TN, true, LDA, LDB> fr[4];
    fr[0].load(lds, lds + ASZ, 0, wm0, wn0, lane);
    fr[1].load(lds, lds + ASZ, 1, wm0, wn0, lane);
    PNP_TRACE_MARK(2);
    int o_cur = 0, o_nxt = STG, o_st = 2 * STG;        // float offsets of the LDS stages holding s, s+1 and receiving s+2
    constexpr int NMF = 4 * TM * TN;
    for (int cc0 = cc_begin; cc0 < cc_end; cc0 += CCU) {
#pragma unroll
        for (int u = 0; u < CCU; ++u) {
            const int cc = cc0 + u;
#pragma unroll
            for (int tap = 0; tap < NTAP; ++tap) {
                const int par = (u * NTAP + tap) & 1;            // compile-time after unrolling: stage parity inside the trip
                const float* As = lds + o_cur;
                const float* Bs = As + ASZ;
                const float* An = lds + o_nxt;
                const float* Bn = An + ASZ;
                float* Ast = lds + o_st;
                float* Bst = Ast + ASZ;
                // ---- slice 0: fragments of slice 2, the global loads of stage s+3 into the ring slot stored LAST stage
                fr[2].load(As, Bs, 2, wm0, wn0, lane);
                gload(ring[par ^ 1], PNP_T3_CC(cc, tap, 3), PNP_T3_TAP(tap, 3));
                fr[0].mma(acc);
                __builtin_amdgcn_sched_group_barrier(0x100, TM + 4 * TN, 0);
#pragma unroll
                for (int i = 0; i < NMF; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x006, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                PNP_SCHED_FENCE();
                PNP_SLICE(fr[3].load(As, Bs, 3, wm0, wn0, lane), fr[1].mma(acc))
                // ---- slices 2, 3: the NEXT stage's slices 0, 1 (visible since the previous barrier); the LDS stores of stage s+2 ride
                // behind the last MFMAs; the barrier then has nothing to wait for but the slowest wave
                PNP_SLICE(fr[0].load(An, Bn, 0, wm0, wn0, lane), fr[2].mma(acc))
                fr[1].load(An, Bn, 1, wm0, wn0, lane);
                PNP_SCHED_FENCE();
                PNP_LAST_SLICE(fr[3].mma(acc), lstore(ring[par], Ast, Bst), NMF)
                __syncthreads();
                ++tsc;
                PNP_TRACE_MARK(2 + tsc);
                const int o_t = o_cur;
                o_cur = o_nxt;
                o_nxt = o_st;
                o_st = o_t;
            }
        }
    }
#undef PNP_T3_CC
#undef PNP_T3_TAP

    PNP_TRACE_MARK(3 + tsc);
    conv_epilogue<TM, TN>(a, acc, a.y + (size_t)z * a.split_stride, m0, n0, wm0, wn0, lane, mt * WM + wave / WN, z == 0);
    PNP_TRACE_MARK(4 + tsc);
}

// ===================================== wgrad kernel ============================================
// a.x = x, a.w = dy ([P][K]), a.y = dW or the split workspace.  grid.x = nblk_m*nblk_n*nsplit
template <int BM, int BN, int WM, int WN, int MODE, bool VECB>
__global__ void __launch_bounds__(NTHREADS, 2) conv_wgrad_kernel(ConvArgs a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int ASZ = BK * LDA, BSZ = BK * LDB;
    __shared__ __attribute__((aligned(16))) float lds[2 * (ASZ + BSZ)];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nblk = a.nblk_m * a.nblk_n;
    // XCD-aware order: all (tap, channel, filter) tiles of one pixel range z re-read the same x and dy rows, so they are given
    // consecutive logical ids = one XCD's L2 (the 40->5 output conv's wgrad fetched 2 GB per launch for 190 MB of operands when its 8
    // tiles per range were sprayed over the 8 XCDs).
    const int lid = a.xcd_swizzle ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int z = lid / nblk;
    int bid = lid - z * nblk;
    int mt, nt;
    tile_coords(bid, a.nblk_m, a.nblk_n, a.gn, mt, nt);
    const int mm0 = mt * BM, n0 = nt * BN;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);

    WgradALoader<BM, MODE> la;
    BLoader<BN, VECB> lb;
    la.init(t, mm0, a, z * a.chunks_per_split * BK);
    lb.init(t);

    Acc<TM, TN> acc;
    acc.zero();

    const int P = a.M;
    const int nchunks_total = (P + BK - 1) / BK;
    const int c_begin = z * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > nchunks_total) c_end = nchunks_total;
    const int nchunks = c_end - c_begin;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, a.w_bytes);
    if (nchunks > 0) {
        const int pend = (c_end * BK < P) ? c_end * BK : P;     // this split's pixel range ends here
        la.load(a, rx, c_begin * BK, pend);
        lb.load(rw, c_begin * BK, pend, a.K, n0);
        la.store(lds);
        lb.store(lds + 2 * ASZ);
        __syncthreads();
        Frag<TM, TN, false, LDA, LDB> f0, f1;
        f0.load(lds, lds + 2 * ASZ, 0, wm0, wn0, lane);
        for (int c = 0; c < nchunks; ++c) {      // same branch-free 4-slice pipeline as conv_fwd_kernel
            const int cur = c & 1;
            const float* As = lds + cur * ASZ;
            const float* Bs = lds + 2 * ASZ + cur * BSZ;
            float* An = lds + (cur ^ 1) * ASZ;
            float* Bn = lds + 2 * ASZ + (cur ^ 1) * BSZ;
            const int p0 = (c_begin + c + 1) * BK;                 // >= pend on the last stage -> zeros
            // stores behind the last MFMAs: gives the global loads a whole stage of latency cover (see conv_fwd_kernel)
            PNP_MMA_STAGE(12, 16, 4 * TM * TN, (la.load(a, rx, p0, pend), lb.load(rw, p0, pend, a.K, n0)), (la.store(An), lb.store(Bn)))
            f0.load(An, Bn, 0, wm0, wn0, lane);
        }
    }

    wgrad_epilogue<TM, TN>(a, acc, a.y + (size_t)z * a.split_stride, mm0, n0, wm0, wn0, lane);
}

// ---- filter gradient, linear pixel walk (any stride, zero padding, OW >= 32, C % 4 == 0, K % 4 == 0), with a register
// ring of DEPTH = 2 global-load stages.  Unlike the forward kernel (whose A rows are re-read for 9 taps and whose filters sit in L2), every
// stage of the filter gradient fetches pixels nobody has touched before — all (tap, channel, filter) tiles of a pixel range walk it in
// step, so the first toucher misses to HBM and the others wait on the same miss: the load latency of EVERY stage is an HBM round trip,
// longer than the one stage (~64 MFMAs per wave) of cover conv_wgrad_kernel gives it.  Here stage j + DEPTH is requested while stage j
// is contracted; the ring is indexed with compile-time constants only (loop unrolled by DEPTH), the tail is peeled.  Depths 1 and 3
// measured slower.
// UNI (PNP_WGRAD_UNI, default on; see launch_wgrad_tile): C % BM == 0, so a 128-row tile of the filter gradient holds ONE filter tap and
// the coordinates / validity / offset of a loader row depend on the pixel only — they are wave-uniform and are carried in SGPRs by the
// scalar unit (a wave's two half-waves load two consecutive pixels: two scalar rows per load, selected per lane).  The per-lane walk costs
// 1.45 VALU instructions per MFMA (PMC), this form about 0.15 (round 3: 512->512 0.613 -> 0.601 ms, g10 3.07 -> 2.98 ms).
// (UNI is folded into the last template argument — DEPTH_ = 10 + depth — so that the measured kernels keep their symbol names.)
template <int BM, int BN, int WM, int WN, int DEPTH_>
__global__ void __launch_bounds__(NTHREADS, 2) conv_wgrad_ring_kernel(ConvArgs a) {
    static_assert(DEPTH_ == 2 || DEPTH_ == 12, "a ring of two stages, per-lane or uniform rows");
    constexpr bool UNI = DEPTH_ >= 10;
    constexpr int DEPTH = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int ASZ = BK * LDA, BSZ = BK * LDB;
    constexpr int AC4 = BM / 4, ARP = NTHREADS / AC4, ANP = BK / ARP;
    constexpr int BC4 = BN / 4, BRP = NTHREADS / BC4, BNP = BK / BRP;
    __shared__ __attribute__((aligned(16))) float lds[2 * (ASZ + BSZ)];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nblk = a.nblk_m * a.nblk_n;
    const int lid = a.xcd_swizzle ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int z = lid / nblk;
    const int bid = lid - z * nblk;
    int mt, nt;
    tile_coords(bid, a.nblk_m, a.nblk_n, a.gn, mt, nt);
    const int mm0 = mt * BM, n0 = nt * BN;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);

    const int nchunks_total = (a.M + BK - 1) / BK;
    const int c_begin = z * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > nchunks_total) c_end = nchunks_total;
    const int nchunks = c_end - c_begin;

    // A rows: output pixel p = stage*32 + arow + ARP*i, this thread's 4 consecutive m' (one tap, 4 channels), carried incrementally
    const int acol = t % AC4, arow = t / AC4;
    const int mm = mm0 + 4 * acol;
    const bool mok = mm < a.Kred;
    const int m_ = mok ? mm : 0;
    const int rs_u = m_ / a.C, c_u = m_ - rs_u * a.C;
    const int r_u = rs_u / a.S, s_u = rs_u - r_u * a.S;
    // input coordinates of (output pixel, this thread's tap): ih = oh*stride + l_dh, iw = ow*stride + l_dw; the row / image wraps of the
    // OUTPUT walk are the compares ih >= ih_lim / iw >= iw_lim
    const int l_dh = r_u * a.dil - a.pad_t, l_dw = s_u * a.dil - a.pad_l;
    const int iw_lim = a.OW * a.stride + l_dw, ih_lim = a.OH * a.stride + l_dh;
    // one stage = BK consecutive output pixels = adv_h whole rows + adv_w pixels (rows of >= BK pixels: 0 rows + BK pixels; the 16^2 / 8^2
    // maps of the critics' last blocks: 2 / 4 rows + 0 pixels); at most one row wrap and one image wrap per step either way (host-checked)
    const int adv_h = BK / a.OW, adv_w = BK - adv_h * a.OW;
    const int step_w = adv_w * a.stride, step_h = adv_h * a.stride, step_off = (step_h * a.W + step_w) * a.C * 4;
    const int wrap_w = a.OW * a.stride, wrap_w_off = a.stride * (a.W - a.OW) * a.C * 4;
    const int wrap_h = a.OH * a.stride, wrap_h_off = (a.H - a.OH * a.stride) * a.W * a.C * 4;
    int l_iw[ANP], l_ih[ANP], l_off[ANP];
#pragma unroll
    for (int i = 0; i < ANP; ++i) {
        const int p = c_begin * BK + arow + ARP * i;
        const int n = p / a.OHW;
        const int rem = p - n * a.OHW;
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        l_ih[i] = oh * a.stride + l_dh;
        l_iw[i] = ow * a.stride + l_dw;
        l_off[i] = (((n * a.H + l_ih[i]) * a.W + l_iw[i]) * a.C + c_u) * 4;
    }
    // UNI: the same walk per (pass i, half-wave h) in wave-uniform registers; the tile's tap and first channel are uniform too
    static_assert(!UNI || (AC4 == 32 && ARP == 8), "UNI: a half-wave = one pixel row of 128 channels");
    const int t_rs = mm0 / a.C, t_c0 = mm0 - t_rs * a.C;
    const int t_r = t_rs / a.S, t_s = t_rs - t_r * a.S;
    const int u_dh = t_r * a.dil - a.pad_t, u_dw = t_s * a.dil - a.pad_l;
    const int u_iw_lim = a.OW * a.stride + u_dw, u_ih_lim = a.OH * a.stride + u_dh;
    const unsigned lane_c = (unsigned)((t_c0 + 4 * acol) * 4);
    int u_iw[ANP][2], u_ih[ANP][2], u_off[ANP][2];
    if constexpr (UNI) {
#pragma unroll
        for (int i = 0; i < ANP; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int p = c_begin * BK + 2 * wave + h + ARP * i;
                const int n = p / a.OHW;
                const int rem = p - n * a.OHW;
                const int oh = rem / a.OW, ow = rem - oh * a.OW;
                u_ih[i][h] = oh * a.stride + u_dh;
                u_iw[i][h] = ow * a.stride + u_dw;
                u_off[i][h] = (((n * a.H + u_ih[i][h]) * a.W + u_iw[i][h]) * a.C) * 4;
            }
    }
    // B rows (dy): constant per-thread offset inside a stage, the stage is the scalar offset
    const int bcol = t % BC4, brow = t / BC4;
    unsigned boff[BNP];
#pragma unroll
    for (int i = 0; i < BNP; ++i) boff[i] = (n0 + 4 * bcol < a.K) ? (unsigned)(((brow + BRP * i) * a.K + n0 + 4 * bcol) * 4) : OOB2;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(a.w, a.w_bytes);

    // Fetches past this split's last stage (the ring runs DEPTH ahead) read the next split's rows, or zeros past the end of the tensors;
    // those stages are never contracted.  Rows past the LAST pixel are zeros from the hardware (same argument as conv_wgrad_kernel MODE 3).
    struct Stage {
        f32x4 a[ANP];
        f32x4 b[BNP];
    };
    Stage ring[DEPTH];
    int l_chunk = c_begin;
    auto gload = [&](Stage& st) {
#pragma unroll
        for (int i = 0; i < ANP; ++i) {
            if constexpr (UNI) {
                unsigned so[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool ok = ((unsigned)u_ih[i][h] < (unsigned)a.H) & ((unsigned)u_iw[i][h] < (unsigned)a.W);
                    so[h] = ok ? (unsigned)u_off[i][h] : OOB2;          // + lane_c (< 2 KiB) stays out of range: x < 2 GiB on this path
                    u_iw[i][h] += step_w;
                    u_ih[i][h] += step_h;
                    u_off[i][h] += step_off;
                    const bool ww = u_iw[i][h] >= u_iw_lim;
                    u_iw[i][h] -= ww ? wrap_w : 0;
                    u_ih[i][h] += ww ? a.stride : 0;
                    u_off[i][h] += ww ? wrap_w_off : 0;
                    const bool hw = u_ih[i][h] >= u_ih_lim;
                    u_ih[i][h] -= hw ? wrap_h : 0;
                    u_off[i][h] += hw ? wrap_h_off : 0;
                }
                st.a[i] = bload4(rx, ((lane & 32) ? so[1] : so[0]) + lane_c);
                continue;
            }
            const bool ok = mok & ((unsigned)l_ih[i] < (unsigned)a.H) & ((unsigned)l_iw[i] < (unsigned)a.W);
            st.a[i] = bload4(rx, ok ? (unsigned)l_off[i] : OOB);
            l_iw[i] += step_w;
            l_ih[i] += step_h;
            l_off[i] += step_off;
            const bool ww = l_iw[i] >= iw_lim;                  // at most one wrap per step (adv_w < OW)
            l_iw[i] -= ww ? wrap_w : 0;
            l_ih[i] += ww ? a.stride : 0;
            l_off[i] += ww ? wrap_w_off : 0;
            const bool hw = l_ih[i] >= ih_lim;
            l_ih[i] -= hw ? wrap_h : 0;
            l_off[i] += hw ? wrap_h_off : 0;
        }
        // (readfirstlane: the stage counter is uniform, but the compiler did not prove it and wrapped every one of these loads in a
        // waterfall loop — 16 extra basic blocks per two stages, which also fenced the MFMA / load interleave)
        const int soff = __builtin_amdgcn_readfirstlane(l_chunk * BK * a.K * 4);
#pragma unroll
        for (int i = 0; i < BNP; ++i) st.b[i] = bload4s(rw, boff[i], soff);
        l_chunk = (l_chunk + 1 < nchunks_total) ? l_chunk + 1 : nchunks_total;      // rows past the end of dy read as zeros
    };
    auto lstore = [&](const Stage& st, float* An, float* Bn) {
#pragma unroll
        for (int i = 0; i < ANP; ++i) *reinterpret_cast<f32x4*>(An + (arow + ARP * i) * LDA + 4 * acol) = st.a[i];
#pragma unroll
        for (int i = 0; i < BNP; ++i) *reinterpret_cast<f32x4*>(Bn + (brow + BRP * i) * LDB + 4 * bcol) = st.b[i];
    };

    Acc<TM, TN> acc;
    acc.zero();
    if (nchunks > 0) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) gload(ring[d]);
        lstore(ring[0], lds, lds + 2 * ASZ);
        __syncthreads();
        Frag<TM, TN, false, LDA, LDB> f0, f1;
        f0.load(lds, lds + 2 * ASZ, 0, wm0, wn0, lane);
        auto stage = [&](int j, Stage& fetch_into, const Stage& store_from, bool fetch) {
            const int cur = j & 1;
            const float* As = lds + cur * ASZ;
            const float* Bs = lds + 2 * ASZ + cur * BSZ;
            float* An = lds + (cur ^ 1) * ASZ;
            float* Bn = lds + 2 * ASZ + (cur ^ 1) * BSZ;
            PNP_MMA_STAGE(12, 4 * TM + 4 * TN, 4 * TM * TN, if (fetch) gload(fetch_into), lstore(store_from, An, Bn))
            f0.load(An, Bn, 0, wm0, wn0, lane);
        };
        const int nmain = (nchunks / DEPTH) * DEPTH;
        for (int j0 = 0; j0 < nmain; j0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) stage(j0 + d, ring[d], ring[(d + 1) % DEPTH], true);
        }
        if (nchunks - nmain >= 1) stage(nmain, ring[0], ring[1], false);
    }

    wgrad_epilogue<TM, TN>(a, acc, a.y + (size_t)z * a.split_stride, mm0, n0, wm0, wn0, lane);
}

// inference-mode batch norm as one multiply-add per channel: scale = gamma * rsqrt(var + eps), shift = beta - mean * scale
__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                               const float* __restrict__ var, float* __restrict__ scale, float* __restrict__ shift, int C, float eps) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = gamma[c] * (1.0f / sqrtf(var[c] + eps));
    scale[c] = sc;
    shift[c] = beta[c] - mean[c] * sc;
}

// every stride-phase sub-filter of w [R][S][C][K] in one launch: tap (r, s) belongs to phase (pa, pb) = (r % st, s % st) and lands,
// flipped on both axes, in that phase's wt [T][U][K][C] block; the blocks are packed in (pa, pb) order (plan_phases' wt_off)
__global__ void flip_transpose_phase_kernel(const float* __restrict__ w, float* __restrict__ wt, int R, int S, int C, int K, int st) {
    __shared__ float tile[32][33];
    const int r = blockIdx.z / S, sx = blockIdx.z - r * S;
    const int pa = r % st, pb = sx % st;
    const int T = (R - pa + st - 1) / st, U = (S - pb + st - 1) / st;
    int taps_before = 0;                                             // taps of the phases packed in front of (pa, pb)
    for (int a = 0; a < st; ++a)
        for (int b = 0; b < st; ++b)
            if (a * st + b < pa * st + pb) taps_before += ((R - a + st - 1) / st) * ((S - b + st - 1) / st);
    const int tf = T - 1 - r / st, uf = U - 1 - sx / st;            // flipped position inside the phase filter
    const float* src = w + (size_t)blockIdx.z * C * K;
    float* dst = wt + ((size_t)taps_before + tf * U + uf) * K * C;
    const int c0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        int c = c0 + i, k = k0 + tx;
        tile[i][tx] = (c < C && k < K) ? src[(size_t)c * K + k] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        int k = k0 + i, c = c0 + tx;
        if (k < K && c < C) dst[(size_t)k * C + c] = tile[tx][i];
    }
}

// w [R][S][C][K] -> wt [R][S][K][C] with both spatial axes flipped (filters of the dgrad convolution)
__global__ void flip_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int R, int S, int C, int K) {
    __shared__ float tile[32][33];
    const int rs = blockIdx.z;
    const int r = rs / S, s = rs - r * S;
    const int rs_f = (R - 1 - r) * S + (S - 1 - s);
    const float* src = w + (size_t)rs * C * K;
    float* dst = wt + (size_t)rs_f * K * C;
    const int c0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        int c = c0 + i, k = k0 + tx;
        tile[i][tx] = (c < C && k < K) ? src[(size_t)c * K + k] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        int k = k0 + i, c = c0 + tx;
        if (k < K && c < C) dst[(size_t)k * C + c] = tile[tx][i];
    }
}

__global__ void naive_conv_kernel(ConvArgs a) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)a.M * a.K;
    if (idx >= total) return;
    const int k = (int)(idx % a.K);
    const int m = (int)(idx / a.K);
    const int n = m / a.OHW;
    const int rem = m - n * a.OHW;
    const int oh = rem / a.OW, ow = rem - oh * a.OW;
    float acc = 0.f;
    for (int r = 0; r < a.R; ++r)
        for (int s = 0; s < a.S; ++s) {
            int ih = 0, iw = 0;
            if (!map_coord<true>(oh * a.stride - a.pad_t + r * a.dil, a.H, a.ups, a.pad_mode, ih)) continue;
            if (!map_coord<true>(ow * a.stride - a.pad_l + s * a.dil, a.W, a.ups, a.pad_mode, iw)) continue;
            const float* xp = a.x + ((size_t)(n * a.H + ih) * a.W + iw) * a.C;
            const float* wp = a.w + (size_t)((r * a.S + s) * a.C) * a.K + k;
            for (int c = 0; c < a.C; ++c) acc = fmaf(xp[c], wp[(size_t)c * a.K], acc);
        }
    a.y[idx] = acc;
}

// tf.pad(x, p, 'SYMMETRIC') in H and W (mirror including the edge): xp[N,H+2p,W+2p,C]; one float4 (or float) per thread
__global__ void sympad_fwd_kernel(const float* __restrict__ x, float* __restrict__ xp, int N, int H, int W, int C, int p, int vec) {
    const int CV = vec ? (C >> 2) : C;
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    const size_t total = (size_t)N * Hp * Wp * CV;
    const size_t gs = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gs) {
        const int cv = (int)(i % CV);
        size_t q = i / CV;
        const int wp = (int)(q % Wp);
        q /= Wp;
        const int hp = (int)(q % Hp);
        const int n = (int)(q / Hp);
        int h = hp - p, w = wp - p;
        h = h < 0 ? -1 - h : (h >= H ? 2 * H - 1 - h : h);
        w = w < 0 ? -1 - w : (w >= W ? 2 * W - 1 - w : w);
        const size_t src = (((size_t)n * H + h) * W + w) * C;
        if (vec) *reinterpret_cast<f32x4*>(xp + i * 4) = *reinterpret_cast<const f32x4*>(x + src + 4 * cv);
        else xp[i] = x[src + cv];
    }
}

// sympad backward: dx[n,h,w,c] = sum of dxp over every padded position that mirrors onto (h,w)
__global__ void sympad_bwd_kernel(const float* __restrict__ dxp, float* __restrict__ dx, int N, int H, int W, int C,
                                  int p) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)N * H * W * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    size_t q = idx / C;
    const int w = (int)(q % W);
    q /= W;
    const int h = (int)(q % H);
    const int n = (int)(q / H);
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    // padded rows mapping to h: h+p always; (p-1-h) if h<p; (2H-1-h+p) if h >= H-p
    int hs[3], ws[3], nh = 0, nw = 0;
    hs[nh++] = h + p;
    if (h < p) hs[nh++] = p - 1 - h;
    if (h >= H - p) hs[nh++] = 2 * H - 1 - h + p;
    ws[nw++] = w + p;
    if (w < p) ws[nw++] = p - 1 - w;
    if (w >= W - p) ws[nw++] = 2 * W - 1 - w + p;
    float s = 0.f;
    for (int i = 0; i < nh; ++i)
        for (int j = 0; j < nw; ++j) s += dxp[(((size_t)n * Hp + hs[i]) * Wp + ws[j]) * C + c];
    dx[idx] = s;
}

// ------------------------------------ host side -------------------------------------------------
int check_geom(const pnp_conv_geom* g, const char* who) {
    PNP_REQUIRE(g != nullptr, "%s: null geometry", who);
    PNP_REQUIRE(g->N > 0 && g->H > 0 && g->W > 0 && g->C > 0 && g->K > 0 && g->R > 0 && g->S > 0 && g->OH > 0 &&
                    g->OW > 0 && g->stride > 0 && g->dil > 0,
                "%s: non-positive dimension", who);
    PNP_REQUIRE(g->pad_mode == PNP_PAD_ZERO || g->pad_mode == PNP_PAD_SYMMETRIC, "%s: bad pad_mode %d", who, g->pad_mode);
    PNP_REQUIRE(g->pad_t >= 0 && g->pad_l >= 0, "%s: negative padding", who);
    PNP_REQUIRE(g->dtype == PNP_DTYPE_F32 || g->dtype == PNP_DTYPE_BF16, "%s: dtype %d (PNP_DTYPE_F32 or PNP_DTYPE_BF16)", who, g->dtype);
    if (g->pad_mode == PNP_PAD_SYMMETRIC)
        PNP_REQUIRE(g->pad_t <= g->H && g->pad_l <= g->W, "%s: symmetric pad larger than the image", who);
    // last tap of the last output must not run past the (padded) input by more than the implicit zero region in
    // symmetric mode (pad-then-VALID): (OH-1)*stride + (R-1)*dil - pad_t <= H-1+pad_t
    if (g->pad_mode == PNP_PAD_SYMMETRIC) {
        PNP_REQUIRE((g->OH - 1) * g->stride + (g->R - 1) * g->dil - g->pad_t <= g->H - 1 + g->pad_t &&
                        (g->OW - 1) * g->stride + (g->S - 1) * g->dil - g->pad_l <= g->W - 1 + g->pad_l,
                    "%s: SYMMETRIC geometry reads past the mirrored border", who);
    }
    const long long xin = (long long)g->N * g->H * g->W * g->C, yout = (long long)g->N * g->OH * g->OW * g->K;
    PNP_REQUIRE(xin < (1ll << 30) && yout < (1ll << 30) && (long long)g->R * g->S * g->C * g->K < (1ll << 30),
                "%s: tensor exceeds 2^30 elements (32-bit buffer offsets)", who);
    return PNP_OK;
}

ConvArgs make_args(const float* x, const float* w, float* y, const pnp_conv_geom* g) {
    ConvArgs a{};
    a.x = x; a.w = w; a.y = y;
    a.N = g->N; a.H = g->H; a.W = g->W; a.C = g->C; a.K = g->K; a.R = g->R; a.S = g->S;
    a.OH = g->OH; a.OW = g->OW; a.stride = g->stride; a.dil = g->dil; a.pad_t = g->pad_t; a.pad_l = g->pad_l;
    a.pad_mode = g->pad_mode;
    a.dtype = g->dtype;
    a.ups = 1;
    a.M = g->N * g->OH * g->OW;
    a.Kred = g->R * g->S * g->C;
    a.OHW = g->OH * g->OW;
    a.nsplit = 1; a.chunks_per_split = 0; a.split_stride = 0;
    const bool p2 = (a.OW & (a.OW - 1)) == 0 && (a.OHW & (a.OHW - 1)) == 0;
    a.ow_sh = p2 ? __builtin_ctz((unsigned)a.OW) : -1;
    a.ohw_sh = p2 ? __builtin_ctz((unsigned)a.OHW) : -1;
    a.do_drop = 0; a.drop_keep = 1.f; a.drop_key = 0; a.drop_thresh = 0;
    static const int env_noswz = getenv("PNP_CONV_NOSWIZZLE") ? 1 : 0;
    a.xcd_swizzle = env_noswz ? 0 : 1;
    a.x_bytes = (unsigned)((size_t)g->N * g->H * g->W * g->C * sizeof(float));
    a.w_bytes = (unsigned)((size_t)g->R * g->S * g->C * g->K * sizeof(float));
    static const int env_stagger = getenv("PNP_CONV_STAGGER") ? atoi(getenv("PNP_CONV_STAGGER")) : 0;
    a.stagger = env_stagger;
    // measured on 512->2560 @32^2, B=16 (tools/bench_conv.py): forward 121.7 TF/s plain, 126.0 with groups of 4 (2: 125.9, 8: 123.6)
    static const int env_gn = getenv("PNP_CONV_GN") ? atoi(getenv("PNP_CONV_GN")) : 4;
    a.gn = env_gn;
    return a;
}

// ---- tile and reduction-split planning for the forward / data-gradient kernel -----------------------------------------------
// Tile: the widest tile that still yields >= 384 workgroups (1.5 per CU; 2 fit), else the next narrower one.  Measured at B=16
// (tools/bench_conv.py, PNP_CONV_TILE sweep): 128->128@32^2 44 TF/s with 128x128 tiles (128 workgroups) vs 70 with 128x64;
// 256->512@32^2 107 vs 100; 128->64 (dgrad) 34 with 128x64 vs 46 with 128x32.
int choose_tile(long long M, int K) {
    static const int force = getenv("PNP_CONV_TILE") ? atoi(getenv("PNP_CONV_TILE")) : -1;   // experiments: 0/1/2 = 128x{128,64,32}
    if ((K & 3) != 0) return 3;      // scalar-B variant of the narrow tile (K = 5 logits, K = 1 critic FC, ...)
    const long long mt = pnp_cdiv(M, 128);
    int tile = 2;
    if (K > 64 && mt * pnp_cdiv(K, 128) >= 384) tile = 0;
    else if (K > 32 && (mt * pnp_cdiv(K, 64) >= 384 || K > 64)) tile = 1;
    if (force >= 0 && !(force == 0 && K <= 64) && !(force <= 1 && K <= 32)) tile = force;
    return tile;
}
// Split of the reduction (data gradients only — they have a workspace for the partials): 512 workgroup slots per dispatch round
// (2 per CU).  Fewer workgroups than slots, or a nearly empty last round (g10's dgrad: 580 workgroups = 1.13 rounds, i.e. the time of
// 2), waste the chip; shorter, more numerous workgroups fill it.  Partials are summed by split_sum.h's serial_kernel (deterministic).
// Called by the planners only (fwd_split, dgrad_ws): a launcher is handed the count.
int choose_split(long long M, int K, int Kred, int tile) {
    static const int off = getenv("PNP_CONV_NOSPLIT") ? 1 : 0;
    if (off) return 1;
    const int bn = tile == 0 ? 128 : (tile == 1 ? 64 : 32);
    const long long nblk = (long long)pnp_cdiv(M, 128) * pnp_cdiv(K, bn);
    const int nch = pnp_cdiv(Kred, BK);
    const double rounds = (double)nblk / 512.0;
    int nsplit = 1;
    // (at exactly half a round — 256 tiles — two-way splitting LOSES: g4 128->128 dgrad 0.054 ms unsplit, 0.063 split)
    if (rounds <= 0.4) nsplit = (int)(512 / nblk);
    else if (rounds > 1.0 && rounds < 3.0 && (ceil(rounds) - rounds) > 0.3) {
        // a nearly empty last round: pick the split that fills the rounds best (g10's dgrad, 580 tiles = 1.13 rounds: 2 splits ->
        // 2.27 rounds cost 3 (76 %), 7 splits -> 7.93 cost 8 (99 %): 3.43 -> 2.9 ms), mild preference for fewer partials
        double best = 0.0;
        for (int ns = 1; ns <= 8; ++ns) {
            const double r = rounds * ns;
            const double score = r / ceil(r) - 0.01 * ns;
            if (score > best + 1e-9) { best = score; nsplit = ns; }
        }
    }
    const int cap = nblk <= 64 ? 32 : 8;        // a handful of tiles (4x4 / 2x2 feature maps, M = 256 rows): split deeper
    if (nsplit > cap) nsplit = cap;
    if (nsplit > nch / 8) nsplit = nch / 8;
    return nsplit < 1 ? 1 : nsplit;
}

// What a launcher does with a planned split: `want` splits of `units` reduction units (32-deep chunks; whole channel groups on the taps
// kernels) are cut down to the partials of `floats` values that fit the bytes the caller brought (a single partial is no split), then
// re-normalised so that no split is empty.
struct SplitFit { int nsplit, per; };
SplitFit fit_split(int units, int want, size_t floats, size_t ws_bytes) {
    if (want > 1 && ws_bytes < (size_t)want * floats * sizeof(float)) {
        want = (int)(ws_bytes / (floats * sizeof(float)));
        if (want < 2) want = 1;
    }
    if (want < 1) want = 1;
    const int per = pnp_cdiv(units, want);
    return {pnp_cdiv(units, per), per};
}

// filter shapes the tap-unrolled kernel is instantiated for: forward 3x3 / 5x5; data gradient 3x3 and the stride-phase sub-filters
constexpr bool taps_shape(int kind, int R, int S) {
    if (R == 3 && S == 3) return true;
    if (kind == 0) return R == 5 && S == 5;
    if (kind == 1) return R >= 1 && R <= 3 && S >= 1 && S <= 3 && !(R == 3 && S == 1) && !(R == 1 && S == 3);
    return false;
}

template <int BM, int BN, int WM, int WN, int KIND>
bool launch_taps(const ConvArgs& a, dim3 grid, hipStream_t st) {
    // three-stage kernel (conv_taps3_kernel) for the narrow tiles: its channel-group loop runs in pairs for odd tap counts
    static const int env_t3 = getenv("PNP_CONV_TAPS3") ? atoi(getenv("PNP_CONV_TAPS3")) : 1;
    // conv_taps3_kernel contracts channel groups in PAIRS when the tap count is odd (CCU = 2): every reduction split must then hold an
    // even number of groups — nothing on the device checks it (a clamped, duplicated stage would be contracted past cc_end), so the
    // condition is stated here per split, not inferred from the planner (round-3 advisor finding)
    const int cc_per = a.chunks_per_split / (a.R * a.S);
    bool pairs_ok = (a.R * a.S) % 2 == 0;
    if (!pairs_ok && cc_per > 0) {
        pairs_ok = true;
        const int ncc = a.C / BK;
        for (int z = 0; z < a.nsplit; ++z) {
            const int n = (ncc - z * cc_per) < cc_per ? (ncc - z * cc_per) : cc_per;
            if (n <= 0 || (n & 1)) pairs_ok = false;
        }
    }
    const bool t3 = env_t3 && BN <= 64 && pairs_ok;
#define PNP_TAPS(RR, SS)                                                                                                   \
    if (a.R == RR && a.S == SS) {                                                                                          \
        if constexpr (BN <= 64 && RR * SS <= 9) {     /* 5x5: 50 unrolled stages per trip and spills — stays on the two-stage kernel */ \
            if (t3) {                                                                                                      \
                PnpProfScope ps(prof_class(KIND), st, conv_flops(a), conv_bytes(a), "conv_taps3_kernel<%d, %d, %d, %d, %d, %d, %d>", BM, \
                                BN, WM, WN, KIND, RR, SS);                                                                  \
                hipLaunchKernelGGL((conv_taps3_kernel<BM, BN, WM, WN, KIND, RR, SS>), grid, dim3(NTHREADS), 0, st, a);      \
                return true;                                                                                               \
            }                                                                                                              \
        }                                                                                                                  \
        PnpProfScope ps(prof_class(KIND), st, conv_flops(a), conv_bytes(a), "conv_taps_kernel<%d, %d, %d, %d, %d, %d, %d>", BM, BN, \
                        WM, WN, KIND, RR, SS);                                                                              \
        hipLaunchKernelGGL((conv_taps_kernel<BM, BN, WM, WN, KIND, RR, SS>), grid, dim3(NTHREADS), 0, st, a);               \
        return true;                                                                                                       \
    }
    PNP_TAPS(3, 3)
    if constexpr (KIND == 0) { PNP_TAPS(5, 5) }
    if constexpr (KIND == 1) { PNP_TAPS(1, 1) PNP_TAPS(1, 2) PNP_TAPS(2, 1) PNP_TAPS(2, 2) PNP_TAPS(2, 3) PNP_TAPS(3, 2) }
#undef PNP_TAPS
    return false;
}

// want: the plan's reduction split (1: none); split_ws / split_bytes: the room for its partials
template <int BM, int BN, int WM, int WN, int KIND, bool VECB>
int launch_fwd_tile(ConvArgs& a, float* split_ws, size_t split_bytes, int want, hipStream_t st) {
    a.nblk_m = pnp_cdiv(a.M, BM);
    a.nblk_n = pnp_cdiv(a.K, BN);
    const int nch = pnp_cdiv(a.Kred, BK);
    const size_t nout = (size_t)a.M * a.K;
    if (!split_ws) want = 1;
    // tap-unrolled fast path: instantiated filter shape, zero padding, C % 32 == 0, K % 4 == 0, both tensors < 2 GiB
    static const int env_notaps = getenv("PNP_CONV_NOTAPS") ? 1 : 0;
    const bool taps = !env_notaps && VECB && KIND != 2 && a.pad_mode == PNP_PAD_ZERO && taps_shape(KIND, a.R, a.S) &&
                      (a.C % 32) == 0 && a.x_bytes < 0x80000000u && a.w_bytes < 0x80000000u;
    // taps: split in whole channel groups (R*S stages each)
    const SplitFit fit = fit_split(taps ? a.C / BK : nch, want, nout, split_bytes);
    const int nsplit = fit.nsplit;
    a.chunks_per_split = taps ? fit.per * a.R * a.S : fit.per;
    a.nsplit = nsplit;
    a.split_stride = (long long)a.M * a.K;
    float* final_out = a.y;
    const int drop_in_reduce = (nsplit > 1) ? a.do_drop : 0;
    if (nsplit > 1) { a.y = split_ws; a.do_drop = 0; }
    dim3 grid((unsigned)(a.nblk_m * a.nblk_n * nsplit));
    const int mode = (a.C % 32 == 0) ? 0 : ((a.C % 4 == 0) ? 1 : 2);
    if constexpr (VECB && KIND != 2) {
        if (taps) {
            // bf16 MFMA operands (configs[4]): the same tiles, splits and epilogue, operands rounded while they are staged (conv_bf16.hip)
            const bool launched = (a.dtype == PNP_DTYPE_BF16) ? launch_taps_bf16(a, BN == 128 ? 0 : (BN == 64 ? 1 : 2), KIND, grid, st)
                                                              : launch_taps<BM, BN, WM, WN, KIND>(a, grid, st);
            PNP_REQUIRE(launched, "conv_taps_kernel: no instance for %dx%d", a.R, a.S);
            PNP_CHECK_LAUNCH("conv_taps_kernel");
        }
    }
    if (!taps) {
        static const int env_noincr = getenv("PNP_CONV_NOINCR") ? 1 : 0;
        const int kmode = mode == 0 ? 0 : (mode == 2 ? 2 : ((KIND != 2 && a.pad_mode == PNP_PAD_ZERO && a.C >= 16 && !env_noincr) ? 4 : 1));
        PnpProfScope ps(prof_class(KIND), st, conv_flops(a), conv_bytes(a), "conv_fwd_kernel<%d, %d, %d, %d, %d, %d, %s>", BM, BN, WM, WN,
                        kmode, KIND, VECB ? "true" : "false");
        if (kmode == 0) hipLaunchKernelGGL((conv_fwd_kernel<BM, BN, WM, WN, 0, KIND, VECB>), grid, dim3(NTHREADS), 0, st, a);
        else if (kmode == 4) hipLaunchKernelGGL((conv_fwd_kernel<BM, BN, WM, WN, 4, KIND, VECB>), grid, dim3(NTHREADS), 0, st, a);
        else if (kmode == 1) hipLaunchKernelGGL((conv_fwd_kernel<BM, BN, WM, WN, 1, KIND, VECB>), grid, dim3(NTHREADS), 0, st, a);
        else hipLaunchKernelGGL((conv_fwd_kernel<BM, BN, WM, WN, 2, KIND, VECB>), grid, dim3(NTHREADS), 0, st, a);
    }
    PNP_CHECK_LAUNCH("conv_fwd_kernel");
    if (nsplit > 1) {
        if (drop_in_reduce)
            return split_sum::launch_serial(split_ws, nout, nsplit, nout, split_sum::Drop{final_out, a.drop_key, a.drop_thresh, a.drop_keep, a.sp, a.drop_sid}, st);
        if (a.o_s != 0) {
            split_sum::Scatter sc{a};
            sc.a.y = final_out;
            return split_sum::launch_serial(split_ws, nout, nsplit, nout, sc, st);
        }
        return split_sum::launch_serial(split_ws, nout, nsplit, nout, split_sum::Plain{final_out, 0}, st);
    }
    return PNP_OK;
}

// nsplit: the reduction split the plan chose for this launch (1: none), split_ws / split_bytes the room for its partials
template <int KIND>
int launch_fwd(ConvArgs& a, hipStream_t st, float* split_ws = nullptr, size_t split_bytes = 0, int nsplit = 1) {
    const int tile = choose_tile(a.M, a.K);
    if (tile == 3) return launch_fwd_tile<128, 32, 4, 1, KIND, false>(a, split_ws, split_bytes, nsplit, st);
    if (tile == 0) return launch_fwd_tile<128, 128, 2, 2, KIND, true>(a, split_ws, split_bytes, nsplit, st);
    if (tile == 1) return launch_fwd_tile<128, 64, 2, 2, KIND, true>(a, split_ws, split_bytes, nsplit, st);
    return launch_fwd_tile<128, 32, 4, 1, KIND, true>(a, split_ws, split_bytes, nsplit, st);
}

// wgrad reduction split: enough workgroups for >= 1 dispatch round (512 slots), as few nearly-empty last rounds as possible
// (512->512: 144 tiles x 8 splits = 2.25 rounds costs 3; x 7 = 1.97 rounds costs 2), few splits preferred (partials are re-read).
int wgrad_plan_split(int nblk, int nchunks) {
    int max_split = nchunks / 8;
    if (max_split < 1) max_split = 1;
    const int ns_lo = pnp_cdiv(512, nblk);                      // splits needed to fill one dispatch round
    if (ns_lo >= max_split) return max_split;
    int ns_hi = ns_lo * 3 + 2;                                  // look up to ~3 rounds
    if (ns_hi > max_split) ns_hi = max_split;
    int best = ns_lo;
    double best_score = -1.0;
    for (int ns = ns_lo; ns <= ns_hi; ++ns) {
        const double rounds = (double)nblk * ns / 512.0;
        const double eff = rounds / ceil(rounds);               // fill of the dispatch rounds
        const double score = eff - 0.02 * rounds;               // mild preference for fewer, longer workgroups
        if (score > best_score) { best_score = score; best = ns; }
    }
    return best;
}

// the ring kernel's tile by filter count: 128 x {128, 64, 32}, the narrow one with scalar dy loads where K % 4 != 0
struct RingTile { int bm, bn, wm, wn; bool vecb; };
RingTile ring_tile(int K) {
    if ((K & 3) != 0) return {128, 32, 4, 1, false};
    if (K > 64) return {128, 128, 2, 2, true};
    if (K > 32) return {128, 64, 2, 2, true};
    return {128, 32, 4, 1, true};
}
// ... and the reduction split planned for it
int ring_split(const pnp_conv_geom* g) {
    const RingTile t = ring_tile(g->K);
    return wgrad_plan_split(pnp_cdiv(g->R * g->S * g->C, t.bm) * pnp_cdiv(g->K, t.bn), pnp_cdiv((long long)g->N * g->OH * g->OW, BK));
}

// want: ring_split(g); the launch takes as many of those splits as the workspace holds
template <int BM, int BN, int WM, int WN, bool VECB>
int launch_wgrad_tile(ConvArgs& a, float* dw, float* ws, size_t ws_bytes, int want, hipStream_t st) {
    a.nblk_m = pnp_cdiv(a.Kred, BM);
    a.nblk_n = pnp_cdiv(a.K, BN);
    const int nblk = a.nblk_m * a.nblk_n;
    const size_t nout = (size_t)a.Kred * a.K;
    const SplitFit fit = fit_split(pnp_cdiv(a.M, BK), want, nout, ws_bytes);
    const int nsplit = fit.nsplit;
    a.chunks_per_split = fit.per;
    a.nsplit = nsplit;
    a.split_stride = (long long)nout;
    a.y = (nsplit > 1) ? ws : dw;
    const int accumulate = a.accumulate;           // un-split: in the kernel's epilogue; split: in the reduce kernel
    if (nsplit > 1) a.accumulate = 0;
    dim3 grid((unsigned)(nblk * nsplit));
    static const int env_nolin = getenv("PNP_CONV_NOLIN") ? 1 : 0;
    // conv_wgrad_ring_kernel walks strided outputs too, and maps whose rows are shorter than a stage when a stage is a whole number of
    // rows inside one image (16^2, 8^2: the critics' last blocks ran on conv_wgrad_kernel's per-row divisions at 0.49 of peak before)
    const bool rows_ok = a.OW >= BK || ((BK % a.OW) == 0 && a.OH > BK / a.OW && (a.OHW % BK) == 0);
    const bool lin_any = !env_nolin && a.pad_mode == PNP_PAD_ZERO && (a.C % 4) == 0 && rows_ok && a.x_bytes < 0x80000000u &&
                         a.w_bytes < 0x80000000u;
    const bool lin = lin_any && a.stride == 1 && a.OW >= BK;
    if (lin && VECB && a.dtype == PNP_DTYPE_BF16) {
        const bool launched = launch_wgrad_bf16(a, BN == 128 ? 0 : (BN == 64 ? 1 : 2), grid, st);
        PNP_REQUIRE(launched, "conv_wgrad_bf16_kernel: no instance for a %dx%d tile", BM, BN);
    } else if (lin_any && VECB) {
        // linear pixel walk with two global-load stages in flight; scalar loader rows where a tile holds one tap (PNP_WGRAD_UNI=0: off)
        static const int env_uni = getenv("PNP_WGRAD_UNI") ? atoi(getenv("PNP_WGRAD_UNI")) : 1;
        const bool uni = env_uni && (a.C % BM) == 0;
        // (the symbol rocprofv3 prints: the scalar-row variant carries 10 + depth as its last template argument)
        PnpProfScope ps(PNP_PROF_CONV_WGRAD, st, conv_flops(a), conv_bytes(a), "conv_wgrad_ring_kernel<%d, %d, %d, %d, %d>", BM, BN, WM, WN,
                        uni ? 12 : 2);
        if (uni) hipLaunchKernelGGL((conv_wgrad_ring_kernel<BM, BN, WM, WN, 12>), grid, dim3(NTHREADS), 0, st, a);
        else hipLaunchKernelGGL((conv_wgrad_ring_kernel<BM, BN, WM, WN, 2>), grid, dim3(NTHREADS), 0, st, a);
    } else {
        // scalar dy columns (K % 4 != 0) on the linear walk: MODE 3; VECB with the linear walk is the ring kernel's
        const int kmode = lin ? 3 : ((a.C % 4 == 0) ? 1 : 2);
        PnpProfScope ps(PNP_PROF_CONV_WGRAD, st, conv_flops(a), conv_bytes(a), "conv_wgrad_kernel<%d, %d, %d, %d, %d, %s>", BM, BN, WM, WN,
                        kmode, VECB ? "true" : "false");
        if (lin) {
            if constexpr (!VECB) hipLaunchKernelGGL((conv_wgrad_kernel<BM, BN, WM, WN, 3, false>), grid, dim3(NTHREADS), 0, st, a);
        } else if (a.C % 4 == 0) hipLaunchKernelGGL((conv_wgrad_kernel<BM, BN, WM, WN, 1, VECB>), grid, dim3(NTHREADS), 0, st, a);
        else hipLaunchKernelGGL((conv_wgrad_kernel<BM, BN, WM, WN, 2, VECB>), grid, dim3(NTHREADS), 0, st, a);
    }
    PNP_CHECK_LAUNCH("conv_wgrad_kernel");
    if (nsplit > 1) return split_sum::launch_serial(ws, nout, nsplit, nout, split_sum::Plain{dw, accumulate}, st);
    return PNP_OK;
}

// ---- strided data gradient, one stride-phase at a time ---------------------------------------------------------------------
// dx[h] only receives filter taps r with r = (h + pad) mod stride (mod stride), so the pixels of one residue class ("phase") form an
// ordinary stride-1 convolution of dy with the sub-filter {r = a, a+stride, ...}:
//     dx[h0 + stride*i] = sum_t dy[i + q - t] * W[a + stride*t],   q = (h0 + pad - a) / stride
// i.e. T = ceil((R-a)/stride) taps, zero padding T-1-q, output scattered with pixel stride `stride`.  The stride^2 phases together
// perform exactly the useful multiply-adds; the zero-upsampled formulation (KIND 2) multiplies stride^2 - 1 zeros for every product.

}  // namespace

namespace pnpconv {

// -> number of phases (0: decomposition not applicable, use the zero-upsampled kernel)
int plan_phases(const pnp_conv_geom* g, DgradPhase* ph) {
    static const int off = getenv("PNP_CONV_NOPHASE") ? 1 : 0;
    const int st = g->stride;
    if (off || st < 2 || st > 4 || g->dil != 1 || g->R < st || g->S < st) return 0;
    const bool sym = g->pad_mode == PNP_PAD_SYMMETRIC;
    const int Ho = sym ? g->H + 2 * g->pad_t : g->H, Wo = sym ? g->W + 2 * g->pad_l : g->W;
    const int fpt = sym ? 0 : g->pad_t, fpl = sym ? 0 : g->pad_l;
    int n = 0;
    size_t off_f = 0;
    for (int a = 0; a < st; ++a)
        for (int b = 0; b < st; ++b) {
            DgradPhase p{};
            p.pa = a; p.pb = b;
            p.T = (g->R - a + st - 1) / st;
            p.U = (g->S - b + st - 1) / st;
            p.h0 = (((a - fpt) % st) + st) % st;
            p.w0 = (((b - fpl) % st) + st) % st;
            const int qa = (p.h0 + fpt - a) / st, qb = (p.w0 + fpl - b) / st;
            p.pad_t = p.T - 1 - qa;
            p.pad_l = p.U - 1 - qb;
            if (p.pad_t < 0 || p.pad_l < 0) return 0;
            p.I = p.h0 < Ho ? (Ho - 1 - p.h0) / st + 1 : 0;
            p.J = p.w0 < Wo ? (Wo - 1 - p.w0) / st + 1 : 0;
            p.wt_off = off_f;
            off_f += (size_t)p.T * p.U * g->K * g->C;
            ph[n++] = p;
        }
    return n;
}

pnp_conv_geom phase_geom(const pnp_conv_geom* g, const DgradPhase& p) {
    pnp_conv_geom d{};
    d.N = g->N; d.H = g->OH; d.W = g->OW; d.C = g->K; d.K = g->C; d.R = p.T; d.S = p.U;
    d.OH = p.I; d.OW = p.J;
    d.stride = 1; d.dil = 1;
    d.pad_t = p.pad_t; d.pad_l = p.pad_l;
    d.pad_mode = PNP_PAD_ZERO;
    d.dtype = g->dtype;
    return d;
}

}  // namespace pnpconv

namespace {

// All phases in one launch (conv_dgrad_phases_kernel) when no single phase fills the chip: the phases' pixel tiles x 64-wide channel
// tiles together stay under one dispatch round (512 slots).  Needs the general kernel's fast mode (K % 32 == 0 channels of dy) and
// float4 filter rows (C % 4 == 0).
int phase_group_tiles(const pnp_conv_geom* g, const DgradPhase* ph, int nph, int bn) {
    int tiles = 0;
    for (int i = 0; i < nph; ++i)
        if (ph[i].I > 0 && ph[i].J > 0) tiles += pnp_cdiv((long long)g->N * ph[i].I * ph[i].J, 128) * pnp_cdiv(g->C, bn);
    return tiles;
}
bool phases_in_one_launch(const pnp_conv_geom* g, const DgradPhase* ph, int nph) {
    static const int off = getenv("PNP_CONV_NOPHASEGROUP") ? 1 : 0;
    if (off || nph < 2 || nph > 16 || (g->K % 32) != 0 || (g->C % 4) != 0 || g->C < 32) return false;
    if ((size_t)g->N * g->OH * g->OW * g->K * sizeof(float) >= 0x80000000u) return false;
    return phase_group_tiles(g, ph, nph, 64) <= 512;
}

int launch_phase_group(const float* dy, const float* wt, float* outp, const pnp_conv_geom* g, const DgradPhase* ph, int nph, int Ho, int Wo,
                       hipStream_t st) {
    GroupArgs ga{};
    pnp_conv_geom d0 = phase_geom(g, ph[0]);
    ga.base = make_args(dy, wt, outp, &d0);
    ga.base.o_s = g->stride; ga.base.o_H = Ho; ga.base.o_W = Wo;
    const bool narrow = phase_group_tiles(g, ph, nph, 64) < 256;          // more, narrower tiles when even 64-wide ones leave CUs idle
    const int bn = narrow ? 32 : 64;
    ga.base.nblk_n = pnp_cdiv(g->C, bn);
    int blk = 0, n = 0;
    double flops = 0.0, bytes = 0.0;
    for (int i = 0; i < nph; ++i) {
        const DgradPhase& p = ph[i];
        if (p.I == 0 || p.J == 0) continue;
        PhaseDesc& q = ga.ph[n++];
        q.w_off = (int)p.wt_off;
        q.R = p.T; q.S = p.U; q.OH = p.I; q.OW = p.J; q.pad_t = p.pad_t; q.pad_l = p.pad_l; q.o_h0 = p.h0; q.o_w0 = p.w0;
        q.first_blk = blk;
        q.nblk_m = pnp_cdiv((long long)g->N * p.I * p.J, 128);
        blk += q.nblk_m * ga.base.nblk_n;
        const double rows = (double)g->N * p.I * p.J;
        flops += 2.0 * rows * g->C * (double)(p.T * p.U * g->K);
        bytes += 4.0 * (rows * g->C + (double)p.T * p.U * g->K * g->C);
    }
    ga.nph = n;
    if (n == 0) return PNP_OK;
    bytes += 4.0 * (double)g->N * g->OH * g->OW * g->K;
    PnpProfScope ps(PNP_PROF_CONV_DGRAD, st, flops, bytes, "conv_dgrad_phases_kernel<128, %d, %d, %d>", bn, narrow ? 4 : 2, narrow ? 1 : 2);
    if (narrow) hipLaunchKernelGGL((conv_dgrad_phases_kernel<128, 32, 4, 1>), dim3((unsigned)blk), dim3(NTHREADS), 0, st, ga);
    else hipLaunchKernelGGL((conv_dgrad_phases_kernel<128, 64, 2, 2>), dim3((unsigned)blk), dim3(NTHREADS), 0, st, ga);
    PNP_CHECK_LAUNCH("conv_dgrad_phases_kernel");
    return PNP_OK;
}

}  // namespace

// ---- one plan per pass ---------------------------------------------------------------------------------------------------------
// plan_fwd / plan_dgrad / plan_wgrad are the ONLY code that combines the families' predicates (n16_geom_ok, narrow_fwd_ok, wino_query,
// x3d_chosen, x3s_chosen, x3n_chosen, plan_phases, x3w_chosen, n16_wgrad_ok, wgd_ok, choose_tile / choose_split, ring_split): each states the
// precedence of its pass once, top to bottom.  The workspace / partial-row / route queries read the plan, and the entry points take the
// first candidate whose workspace the caller brought and switch on its route.
// Workspace of the fp32 data-gradient kernels, in bytes: [flipped / transposed filters R*S*K*C, 256-aligned at 0][padded dx for SYMMETRIC,
// 256-aligned at filt][reduction-split partials at filt + padded], and the split each launch takes: nsplit[i] for stride phase i on route
// PHASES (parts holds the largest phase's partials), nsplit[0] otherwise.
struct DgradWs {
    size_t filt, padded, parts, total;
    int nsplit[16];
};

struct ConvPlan {
    // PNP_ROUTE_*, in order of preference; need: workspace bytes the launch asks for; nsplit: its reduction split (forward IGEMM)
    struct Cand { int route; size_t need; int nsplit; } cand[5];
    int ncand;
    size_t ws_bytes;      // what the pass's *_workspace_bytes query reports
    int stats_parts;      // partial rows of the statistics epilogue on cand[0]; 0 = none
    int tile;             // the Winograd planner's tile (0 / 2 / 4): it sizes the workspace ALSO where X3D takes the launch
    DgradWs dws;          // data gradient off the Winograd planner's layers
    void add(int route, size_t need, int nsplit = 1) { cand[ncand].route = route; cand[ncand].need = need; cand[ncand].nsplit = nsplit; ++ncand; }
    const Cand& pick(const void* ws, size_t ws_bytes) const {
        int i = 0;
        while (i + 1 < ncand && cand[i].need > 0 && !(ws && ws_bytes >= cand[i].need)) ++i;
        return cand[i];
    }
};

// forward reduction split: only layers that leave at least 3/4 of the workgroup slots empty — at half a dispatch round the extra pass over
// the partials costs more than the idle CUs (128->128@32^2, 256 tiles: 0.049 ms unsplit, 0.060 split in two)
static int fwd_split(const pnp_conv_geom* g) {
    if (g->pad_mode != PNP_PAD_ZERO) return 1;
    const long long M = (long long)g->N * g->OH * g->OW;
    const int tile = choose_tile(M, g->K);
    const int bn = tile == 0 ? 128 : (tile == 1 ? 64 : 32);
    if ((long long)pnp_cdiv(M, 128) * pnp_cdiv(g->K, bn) > 128) return 1;
    return choose_split(M, g->K, g->R * g->S * g->C, tile);
}

// what the ENTRY POINT asks of the forward: it takes a workspace / leaves statistics partials / applies the fused inference BN
enum { EP_WS = 1, EP_STATS = 2, EP_BN = 4 };

static ConvPlan plan_fwd(const pnp_conv_geom* g, unsigned ep) {
    const bool ws = ep & EP_WS, stats = ep & EP_STATS, bn = ep & EP_BN;
    ConvPlan p{};
    const WinoQuery wq = wino_query(g);          // conv_wino.hip: its plan of this layer, asked once
    p.tile = wq.tile;
    const long long M = (long long)g->N * g->OH * g->OW;
    const int ns = fwd_split(g);
    const size_t split = ns > 1 ? (size_t)ns * M * g->K * sizeof(float) : 0;
    p.ws_bytes = split;
    // the logits layer on the split-bf16 kernel (conv_x3_narrow.hip: dropout, neither statistics nor the fused BN), ahead of whatever else
    // serves it: the vector-ALU kernel, or below its floor of 8 192 pixels (mode 2 only) the implicit GEMM
    const bool x3n = !bn && !stats && x3n_chosen(g, 0);
    auto add_x3n = [&]() {
        if (x3n_filter_bytes(0) > p.ws_bytes) p.ws_bytes = x3n_filter_bytes(0);
        if (ws) p.add(PNP_ROUTE_X3N, x3n_filter_bytes(0));
    };
    if (n16_geom_ok(g)) p.add(PNP_ROUTE_N16, 0);
    else if (!bn && narrow_fwd_ok(g)) {                                // (no fused BN in the vector-ALU kernel)
        if (x3n) add_x3n();
        p.add(PNP_ROUTE_NARROW, 0);
    }
    else {
        // the direct split-bf16 kernels (conv_x3_direct.hip) have dropout, statistics and the residual add, not the fused BN
        const bool x3d = x3d_chosen(g);
        if (x3n) add_x3n();
        if (p.tile) {
            // the Winograd planner's layer: transformed filter + input + product (conv_wino.hip) — ALSO where the narrow layers then run on
            // the direct split-bf16 kernel, whose filter image is smaller
            p.ws_bytes = wq.ws_bytes;
            if (ws) p.add(x3d && !bn ? PNP_ROUTE_X3D : PNP_ROUTE_WINO, p.ws_bytes);
        } else {
            const size_t x3 = x3d ? x3d_filter_bytes(g->C, g->K) : (x3s_chosen(g, 0) ? x3s_filter_bytes(g) : 0);      // the split filter image
            if (x3 > split) p.ws_bytes = x3;
            if (x3 && ws && !bn) p.add(x3d ? PNP_ROUTE_X3D : PNP_ROUTE_X3S, x3);
            else if (split && ws && !stats && !bn) p.add(PNP_ROUTE_IGEMM, split, ns);  // need > 0: the reduction-split launch
        }
        p.add(PNP_ROUTE_IGEMM, 0);     // un-split (same result up to fp32 rounding): what runs when the workspace is missing
    }
    if (stats) {
        const int r = p.cand[0].route;
        // implicit GEMM: pixel tiles x wave rows of the tile (WM), from an un-split reduction only (the epilogue owns complete rows there);
        // Winograd: the tile slabs of its output transform; the direct split-bf16 kernels: one partial per 64 output pixels
        const int tile = choose_tile(M, g->K);
        if (r == PNP_ROUTE_IGEMM) p.stats_parts = ns > 1 ? 0 : pnp_cdiv(M, 128) * ((tile == 0 || tile == 1) ? 2 : 4);
        else if (r == PNP_ROUTE_WINO) p.stats_parts = wq.stats_parts;
        else if (r == PNP_ROUTE_X3D || r == PNP_ROUTE_X3S) p.stats_parts = x3d_stats_parts(g);
    }
    return p;
}

// The convolution of dy that a data gradient is (flipped, transposed filter; a strided layer's dy is zero-upsampled by the launch).
// SYMMETRIC: it computes the mirror-padded image, which sympad_bwd then folds onto dx.
static pnp_conv_geom dgrad_as_conv(const pnp_conv_geom* g) {
    const bool sym = g->pad_mode == PNP_PAD_SYMMETRIC;
    pnp_conv_geom d{};
    d.N = g->N; d.H = g->OH; d.W = g->OW; d.C = g->K; d.K = g->C; d.R = g->R; d.S = g->S;
    d.OH = sym ? g->H + 2 * g->pad_t : g->H;
    d.OW = sym ? g->W + 2 * g->pad_l : g->W;
    d.stride = 1; d.dil = g->dil;
    d.pad_t = g->dil * (g->R - 1) - (sym ? 0 : g->pad_t);
    d.pad_l = g->dil * (g->S - 1) - (sym ? 0 : g->pad_l);
    d.pad_mode = PNP_PAD_ZERO;
    d.dtype = g->dtype;
    return d;
}

// g: the forward geometry, d = dgrad_as_conv(g), ph[nph] = plan_phases(g).  The one place that sizes and lays out the fp32 kernels'
// workspace and splits their reductions (GEMM M = the pixels of dx, or of one phase; N = C; reduction over taps x K).
static DgradWs dgrad_ws(const pnp_conv_geom* g, const pnp_conv_geom& d, const DgradPhase* ph, int nph) {
    DgradWs w{};
    const size_t outb = (size_t)d.N * d.OH * d.OW * d.K * sizeof(float);
    w.filt = ((size_t)g->R * g->S * g->C * g->K * sizeof(float) + 255) & ~(size_t)255;
    w.padded = g->pad_mode == PNP_PAD_SYMMETRIC ? (outb + 255) & ~(size_t)255 : 0;
    if (nph > 0) {       // strided, one stride-phase at a time: the largest phase's partials
        for (int i = 0; i < nph; ++i) {
            const long long Mp = (long long)g->N * ph[i].I * ph[i].J;
            w.nsplit[i] = Mp == 0 ? 1 : choose_split(Mp, g->C, ph[i].T * ph[i].U * g->K, choose_tile(Mp, g->C));
            const size_t b = w.nsplit[i] > 1 ? (size_t)w.nsplit[i] * Mp * g->C * sizeof(float) : 0;
            if (b > w.parts) w.parts = b;
        }
    } else {
        const long long Md = (long long)(outb / sizeof(float)) / g->C;
        w.nsplit[0] = choose_split(Md, g->C, g->R * g->S * g->K, choose_tile(Md, g->C));
        if (w.nsplit[0] > 1) w.parts = (size_t)w.nsplit[0] * outb;
    }
    w.total = w.filt + w.padded + w.parts;
    return w;
}

// One candidate: pnp_conv2d_dgrad* refuses a workspace smaller than ws_bytes.
static ConvPlan plan_dgrad(const pnp_conv_geom* g) {
    ConvPlan p{};
    const bool sym = g->pad_mode == PNP_PAD_SYMMETRIC;
    const pnp_conv_geom d = dgrad_as_conv(g);
    const bool plain = g->stride == 1 && !sym && d.pad_t >= 0 && d.pad_l >= 0;      // a stride-1 zero-padded convolution of dy
    const WinoQuery wq = plain ? wino_query(&d) : WinoQuery{};
    p.tile = wq.tile;
    if (p.tile) {        // the Winograd planner's layer, as in the forward (the filter transform / image flips and transposes on the way)
        p.ws_bytes = wq.ws_bytes;
        p.add(x3d_chosen(&d) ? PNP_ROUTE_X3D : PNP_ROUTE_WINO, p.ws_bytes);
        return p;
    }
    int route;
    size_t x3 = 0;       // split filter image of the direct split-bf16 kernels
    DgradPhase ph[16];
    const int nph = plan_phases(g, ph);
    p.dws = dgrad_ws(g, d, ph, nph);
    const size_t b = p.dws.total;
    if (nph > 0) {       // strided, one stride-phase at a time
        route = x3s_chosen(g, 1) ? PNP_ROUTE_X3S : PNP_ROUTE_PHASES;       // X3S: every phase in one launch
        if (route == PNP_ROUTE_X3S) x3 = x3s_filter_bytes(g);
    } else {
        if (!sym && n16_geom_ok(&d)) route = PNP_ROUTE_N16;                            // 16 INPUT channels: a 16-output conv of dy
        else if (g->stride == 1 && narrow_fwd_ok(&d)) route = PNP_ROUTE_NARROW;        // few INPUT channels: a narrow-output conv of dy
        else if (plain && x3d_chosen(&d)) route = PNP_ROUTE_X3D;
        else if (plain && x3n_chosen(g, 1)) route = PNP_ROUTE_X3N;                     // the logits layer's (conv_x3_narrow.hip)
        else route = PNP_ROUTE_IGEMM;                                                  // (stride > 1 without phases: dy zero-upsampled)
        if (route == PNP_ROUTE_X3D) x3 = x3d_filter_bytes(d.C, d.K);
        if (route == PNP_ROUTE_X3N) x3 = x3n_filter_bytes(1);
    }
    p.ws_bytes = b > x3 ? b : x3;
    p.add(route, p.ws_bytes);
    return p;
}

// Every family against its own byte count, the 16x16x4-MFMA kernel against the query's; the ring kernel takes as many splits as fit.
static ConvPlan plan_wgrad(const pnp_conv_geom* g) {
    ConvPlan p{};
    const WinoQuery wq = wino_wgrad_query(g);
    p.tile = wq.tile;
    if (p.tile) p.add(PNP_ROUTE_WINO_WGRAD, wq.ws_bytes);             // conv_wino.hip
    if (x3w_chosen(g)) p.add(PNP_ROUTE_X3W, x3w_workspace_bytes(g));                    // conv_x3_wgrad.hip
    const size_t nout = (size_t)g->R * g->S * g->C * g->K;
    const bool wgd = wgd_ok(g);
    const int nsplit = ring_split(g);
    if (p.ncand) p.ws_bytes = p.cand[0].need;
    else if (n16_wgrad_ok(g)) p.ws_bytes = (size_t)n16_wgrad_blocks(g) * nout * sizeof(float);
    else {               // the larger of the vector-ALU kernel's slabs and the ring kernel's split partials
        const size_t mfma_ws = nsplit <= 1 ? 0 : (size_t)nsplit * nout * sizeof(float);
        p.ws_bytes = (wgd && wgd_workspace_bytes(g) > mfma_ws) ? wgd_workspace_bytes(g) : mfma_ws;
    }
    if (n16_wgrad_ok(g)) p.add(PNP_ROUTE_N16_WGRAD, p.ws_bytes);
    if (wgd) p.add(PNP_ROUTE_WGD, wgd_workspace_bytes(g));
    p.add(PNP_ROUTE_RING, 0, nsplit);
    return p;
}

static void set_dropout(ConvArgs& a, float keep_prob, uint64_t seed, uint32_t stream_id) {
    if (keep_prob >= 1.f) return;
    a.do_drop = 1;
    a.drop_keep = keep_prob;
    a.drop_key = pnp_drop_key(seed, stream_id);
    a.drop_thresh = pnp_drop_thresh(keep_prob);
    a.sp = pnp_step_params_ptr(); a.drop_sid = stream_id;
}

// the forward of g on candidate c, a = make_args(x, w, y, g) + the entry point's epilogue
static int launch_fwd_cand(const ConvPlan::Cand& c, ConvArgs& a, const pnp_conv_geom* g, void* ws, size_t ws_bytes, hipStream_t st) {
    switch (c.route) {
    case PNP_ROUTE_N16: return launch_n16_fwd(a, 0, st);
    case PNP_ROUTE_NARROW: return launch_narrow(a.x, a.w, a.y, g, a, st);
    case PNP_ROUTE_WINO: return launch_wino(a, 0, false, ws, ws_bytes, st);
    case PNP_ROUTE_X3D: return launch_x3_direct(a, 0, false, ws, ws_bytes, st);
    case PNP_ROUTE_X3S: return launch_x3_strided(a, g, 0, ws, ws_bytes, st);
    case PNP_ROUTE_X3N: return launch_x3_narrow(a, 0, ws, ws_bytes, st);
    default: return launch_fwd<0>(a, st, c.need ? (float*)ws : nullptr, ws_bytes, c.nsplit);
    }
}

// kind 0: forward (plain epilogue, workspace supplied); 2: filter gradient; else: data gradient — g = the FORWARD geometry
static ConvPlan plan_of(const pnp_conv_geom* g, int kind) { return kind == 0 ? plan_fwd(g, EP_WS) : (kind == 2 ? plan_wgrad(g) : plan_dgrad(g)); }

extern "C" {

// which kernel family serves the layer (PNP_ROUTE_*) with the workspace of the query supplied; kind 0: forward (plain epilogue), 1: data
// gradient, 2: filter gradient — g = the FORWARD geometry
int32_t pnp_conv2d_route(const pnp_conv_geom* g, int32_t kind) {
    if (!g || check_geom(g, "pnp_conv2d_route") != PNP_OK) return -1;
    return plan_of(g, kind).cand[0].route;
}

// 0: direct kernels; else the Winograd planner's output tile edge (kind 0: forward; 1: data gradient; 2: filter gradient — g = the FORWARD geometry)
int32_t pnp_conv2d_wino_chosen(const pnp_conv_geom* g, int32_t kind) {
    if (!g || check_geom(g, "pnp_conv2d_wino_chosen") != PNP_OK) return 0;
    return plan_of(g, kind).tile;
}

size_t pnp_conv2d_fwd_workspace_bytes(const pnp_conv_geom* g) { return g ? plan_fwd(g, EP_WS).ws_bytes : 0; }
size_t pnp_conv2d_dgrad_workspace_bytes(const pnp_conv_geom* g) { return g ? plan_dgrad(g).ws_bytes : 0; }
size_t pnp_conv2d_wgrad_workspace_bytes(const pnp_conv_geom* g) { return g ? plan_wgrad(g).ws_bytes : 0; }

int pnp_conv2d_fwd(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                   uint32_t stream_id, void* stream) {
    return pnp_conv2d_fwd_ws(x, w, y, g, keep_prob, seed, stream_id, nullptr, 0, stream);
}

int pnp_conv2d_fwd_ws(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                      uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = check_geom(g, "pnp_conv2d_fwd")) return e;
    PNP_REQUIRE(x && w && y, "pnp_conv2d_fwd: null pointer");
    PNP_REQUIRE(keep_prob > 0.f, "pnp_conv2d_fwd: keep_prob must be > 0");
    ConvArgs a = make_args(x, w, y, g);
    set_dropout(a, keep_prob, seed, stream_id);
    return launch_fwd_cand(plan_fwd(g, EP_WS).pick(workspace, workspace_bytes), a, g, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- forward convolution that also leaves the batch-norm statistics partials of its output (training-mode conv -> dropout -> BN) ----
// 0 parts = not available for this geometry (narrow-output vector-ALU kernels, reduction-split tiny layers): the caller runs pnp_bn_stats
// on the output instead.  With a workspace (pnp_conv2d_fwd_workspace_bytes) the Winograd and direct split-bf16 routes take their layers and
// leave their own partial rows: pnp_conv2d_fwd_stats_ws_parts says how many.
static int fwd_stats_impl(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                          uint32_t stream_id, const float* shift, float* parts, size_t parts_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, unsigned ep) {
    if (int e = check_geom(g, "pnp_conv2d_fwd_stats")) return e;
    PNP_REQUIRE(x && w && y && parts, "pnp_conv2d_fwd_stats: null pointer");
    PNP_REQUIRE(keep_prob > 0.f, "pnp_conv2d_fwd_stats: keep_prob must be > 0");
    const ConvPlan p = plan_fwd(g, ep);
    const ConvPlan::Cand& c = p.cand[0];         // the partial rows are this candidate's: no fall-back
    PNP_REQUIRE(c.need == 0 || (workspace && workspace_bytes >= c.need), "pnp_conv2d_fwd_stats_ws: workspace too small (pnp_conv2d_fwd_workspace_bytes)");
    PNP_REQUIRE(p.stats_parts > 0, "pnp_conv2d_fwd_stats: no epilogue statistics for this geometry (pnp_conv2d_fwd_stats_parts == 0)");
    if (parts_bytes < (size_t)p.stats_parts * 2 * g->K * sizeof(float)) {
        pnp_set_error("pnp_conv2d_fwd_stats: parts buffer too small (%zu < %zu)", parts_bytes, (size_t)p.stats_parts * 2 * g->K * sizeof(float));
        return PNP_EWORKSPACE;
    }
    ConvArgs a = make_args(x, w, y, g);
    set_dropout(a, keep_prob, seed, stream_id);
    a.stat_ws = parts;
    a.stat_shift = shift;
    return launch_fwd_cand(c, a, g, workspace, workspace_bytes, (hipStream_t)stream);
}

int32_t pnp_conv2d_fwd_stats_parts(const pnp_conv_geom* g) {
    return (g && check_geom(g, "pnp_conv2d_fwd_stats_parts") == PNP_OK) ? plan_fwd(g, EP_STATS).stats_parts : 0;
}

int pnp_conv2d_fwd_stats(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                         uint32_t stream_id, const float* shift, float* parts, size_t parts_bytes, void* stream) {
    return fwd_stats_impl(x, w, y, g, keep_prob, seed, stream_id, shift, parts, parts_bytes, nullptr, 0, stream, EP_STATS);
}

int32_t pnp_conv2d_fwd_stats_ws_parts(const pnp_conv_geom* g) {
    return (g && check_geom(g, "pnp_conv2d_fwd_stats_ws_parts") == PNP_OK) ? plan_fwd(g, EP_STATS | EP_WS).stats_parts : 0;
}

int pnp_conv2d_fwd_stats_ws(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                            uint32_t stream_id, const float* shift, float* parts, size_t parts_bytes, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return fwd_stats_impl(x, w, y, g, keep_prob, seed, stream_id, shift, parts, parts_bytes, workspace, workspace_bytes, stream, EP_STATS | EP_WS);
}

int pnp_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float* scale, float* shift, int32_t C,
                float eps, void* stream) {
    PNP_REQUIRE(gamma && beta && mean && var && scale && shift && C > 0, "pnp_bn_fold: bad argument");
    hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)pnp_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta, mean, var, scale,
                       shift, C, eps);
    PNP_CHECK_LAUNCH("bn_fold_kernel");
    return PNP_OK;
}

int pnp_conv2d_fwd_bn(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                      uint32_t stream_id, const float* scale, const float* shift, const float* shortcut, int32_t Cs, float alpha,
                      void* stream) {
    return pnp_conv2d_fwd_bn_ws(x, w, y, g, keep_prob, seed, stream_id, scale, shift, shortcut, Cs, alpha, nullptr, 0, stream);
}

// with a workspace of pnp_conv2d_fwd_workspace_bytes(g) bytes the layers the planner gives to the Winograd route take it (conv_wino.hip);
// the reduction is never split on this path
int pnp_conv2d_fwd_bn_ws(const float* x, const float* w, float* y, const pnp_conv_geom* g, float keep_prob, uint64_t seed,
                         uint32_t stream_id, const float* scale, const float* shift, const float* shortcut, int32_t Cs, float alpha,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (int e = check_geom(g, "pnp_conv2d_fwd_bn")) return e;
    PNP_REQUIRE(x && w && y && scale && shift, "pnp_conv2d_fwd_bn: null pointer");
    PNP_REQUIRE(keep_prob > 0.f, "pnp_conv2d_fwd_bn: keep_prob must be > 0");
    if (shortcut) PNP_REQUIRE(Cs > 0 && Cs <= g->K && ((g->K - Cs) % 2) == 0, "pnp_conv2d_fwd_bn: bad shortcut channels");
    ConvArgs a = make_args(x, w, y, g);
    set_dropout(a, keep_prob, seed, stream_id);
    a.ep_scale = scale; a.ep_shift = shift; a.ep_res = shortcut; a.ep_cs = shortcut ? Cs : g->K; a.ep_alpha = alpha;
    return launch_fwd_cand(plan_fwd(g, EP_WS | EP_BN).pick(workspace, workspace_bytes), a, g, workspace, workspace_bytes, (hipStream_t)stream);
}

int pnp_conv2d_fwd_naive(const float* x, const float* w, float* y, const pnp_conv_geom* g, void* stream) {
    if (int e = check_geom(g, "pnp_conv2d_fwd_naive")) return e;
    ConvArgs a = make_args(x, w, y, g);
    const size_t total = (size_t)a.M * a.K;
    hipLaunchKernelGGL(naive_conv_kernel, dim3((unsigned)pnp_cdiv((long long)total, 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    PNP_CHECK_LAUNCH("naive_conv_kernel");
    return PNP_OK;
}

// residual != null: dx = data gradient + residual.  Fused into the epilogue on the stride-1 MFMA paths (the residual blocks); every
// other geometry computes the gradient and adds the residual with one more pass (pnp_axpby).
static int dgrad_impl(const float* dy, const float* w, float* dx, const pnp_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream,
                      const float* residual) {
    if (int e = check_geom(g, "pnp_conv2d_dgrad")) return e;
    PNP_REQUIRE(dy && w && dx && workspace, "pnp_conv2d_dgrad: null pointer");
    const ConvPlan p = plan_dgrad(g);
    PNP_REQUIRE(workspace_bytes >= p.ws_bytes, "pnp_conv2d_dgrad: workspace too small");
    const bool sym = g->pad_mode == PNP_PAD_SYMMETRIC;
    if (sym) PNP_REQUIRE(g->pad_t == g->pad_l, "pnp_conv2d_dgrad: SYMMETRIC needs pad_t == pad_l");
    hipStream_t st = (hipStream_t)stream;
    const int route = p.cand[0].route;
    const pnp_conv_geom d = dgrad_as_conv(g);
    if (route == PNP_ROUTE_X3S) {            // every phase on the direct split-bf16 kernel, one launch (its filter image flips per phase)
        ConvArgs a = make_args(dy, w, dx, g);
        if (int e = launch_x3_strided(a, g, 1, workspace, workspace_bytes, st)) return e;
        return residual ? pnp_axpby(residual, dx, (size_t)g->N * g->H * g->W * g->C, 1.f, 1.f, stream) : PNP_OK;
    }
    if (route == PNP_ROUTE_WINO || route == PNP_ROUTE_X3D || route == PNP_ROUTE_X3N) {      // the filter transform / image flips and transposes on the way (no flip launch)
        ConvArgs a = make_args(dy, w, dx, &d);
        a.res_add = residual;
        if (route == PNP_ROUTE_X3N) return launch_x3_narrow(a, 1, workspace, workspace_bytes, st);
        return route == PNP_ROUTE_WINO ? launch_wino(a, 1, true, workspace, workspace_bytes, st)
                                       : launch_x3_direct(a, 1, true, workspace, workspace_bytes, st);
    }
    // the fp32 kernels: [flipped filters][padded dx for SYMMETRIC][reduction-split partials of the launches the plan splits]
    const DgradWs& dws = p.dws;
    float* wt = (float*)workspace;
    float* out = sym ? (float*)((char*)workspace + dws.filt) : dx;
    float* parts = (float*)((char*)workspace + dws.filt + dws.padded);
    auto split_ws = [&](int ns) { return ns > 1 ? parts : nullptr; };
    const dim3 tg((unsigned)pnp_cdiv(g->K, 32), (unsigned)pnp_cdiv(g->C, 32), (unsigned)(g->R * g->S));
    if (route == PNP_ROUTE_PHASES) {
        DgradPhase ph[16];
        const int nph = plan_phases(g, ph);
        hipLaunchKernelGGL(flip_transpose_phase_kernel, tg, dim3(256), 0, st, w, wt, g->R, g->S, g->C, g->K, g->stride);
        PNP_CHECK_LAUNCH("flip_transpose_phase_kernel");
        if (phases_in_one_launch(g, ph, nph)) {
            if (int e = launch_phase_group(dy, wt, out, g, ph, nph, d.OH, d.OW, st)) return e;
        } else {
            for (int i = 0; i < nph; ++i) {
                const DgradPhase& q = ph[i];
                if (q.I == 0 || q.J == 0) continue;
                const pnp_conv_geom dp = phase_geom(g, q);
                ConvArgs a = make_args(dy, wt + q.wt_off, out, &dp);
                a.o_s = g->stride; a.o_H = d.OH; a.o_W = d.OW; a.o_h0 = q.h0; a.o_w0 = q.w0;
                if (int e = launch_fwd<1>(a, st, split_ws(dws.nsplit[i]), dws.parts, dws.nsplit[i])) return e;
            }
        }
    } else {
        hipLaunchKernelGGL(flip_transpose_kernel, tg, dim3(256), 0, st, w, wt, g->R, g->S, g->C, g->K);
        PNP_CHECK_LAUNCH("flip_transpose_kernel");
        PNP_REQUIRE(d.pad_t >= 0 && d.pad_l >= 0, "pnp_conv2d_dgrad: forward padding exceeds the filter extent");
        ConvArgs a = make_args(dy, wt, out, &d);
        a.ups = g->stride;                                     // dy zero-upsampled by `stride`
        if (route == PNP_ROUTE_N16) {
            a.res_add = residual;
            return launch_n16_fwd(a, 1, st);
        }
        if (route == PNP_ROUTE_NARROW) {
            if (int e = launch_narrow(dy, wt, out, &d, a, st)) return e;
        } else {
            if (residual && !sym && g->stride == 1) {          // rows of the GEMM == pixels of dx, plain row-major output: fused
                a.res_add = residual;
                residual = nullptr;
            }
            const int ns = dws.nsplit[0];
            if (int e = (g->stride > 1 ? launch_fwd<2>(a, st, split_ws(ns), dws.parts, ns) : launch_fwd<1>(a, st, split_ws(ns), dws.parts, ns))) return e;
        }
    }
    if (sym) {
        if (int e = pnp_sympad_bwd(out, dx, g->N, g->H, g->W, g->C, g->pad_t, stream)) return e;
    }
    return residual ? pnp_axpby(residual, dx, (size_t)g->N * g->H * g->W * g->C, 1.f, 1.f, stream) : PNP_OK;
}

int pnp_conv2d_dgrad(const float* dy, const float* w, float* dx, const pnp_conv_geom* g, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return dgrad_impl(dy, w, dx, g, workspace, workspace_bytes, stream, nullptr);
}

int pnp_conv2d_dgrad_add(const float* dy, const float* w, const float* residual, float* dx, const pnp_conv_geom* g, void* workspace,
                         size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(residual && residual != dx, "pnp_conv2d_dgrad_add: residual must be a tensor of its own");
    return dgrad_impl(dy, w, dx, g, workspace, workspace_bytes, stream, residual);
}

static int wgrad_impl(const float* x, const float* dy, float* dw, const pnp_conv_geom* g, void* workspace, size_t workspace_bytes, void* stream,
                      int accumulate) {
    if (int e = check_geom(g, "pnp_conv2d_wgrad")) return e;
    PNP_REQUIRE(x && dy && dw, "pnp_conv2d_wgrad: null pointer");
    ConvArgs a = make_args(x, dy, dw, g);
    a.accumulate = accumulate;
    a.w_bytes = (unsigned)((size_t)g->N * g->OH * g->OW * g->K * sizeof(float));   // a.w is dy [P][K] here
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (!ws) workspace_bytes = 0;
    const size_t nout = (size_t)a.Kred * a.K;
    int nparts = 0;          // per-workgroup partials in ws, summed by split_sum::sliced_kernel<1>
    const ConvPlan::Cand c = plan_wgrad(g).pick(workspace, workspace_bytes);
    switch (c.route) {
    case PNP_ROUTE_WINO_WGRAD: return launch_wino_wgrad(a, dw, accumulate, workspace, workspace_bytes, st);
    case PNP_ROUTE_X3W: return launch_x3_wgrad(x, dy, dw, g, accumulate, workspace, workspace_bytes, st);
    case PNP_ROUTE_N16_WGRAD:
        if (int e = launch_n16_wgrad(a, ws, st)) return e;
        nparts = n16_wgrad_blocks(g);
        break;
    case PNP_ROUTE_WGD:
        if (int e = launch_wgd(x, dy, ws, g, a, st)) return e;
        nparts = wgd_blocks(g);
        break;
    default: {               // the ring kernel, with as many of the planned reduction splits as the workspace holds
        const RingTile t = ring_tile(a.K);
        if (!t.vecb) return launch_wgrad_tile<128, 32, 4, 1, false>(a, dw, ws, workspace_bytes, c.nsplit, st);
        if (t.bn == 128) return launch_wgrad_tile<128, 128, 2, 2, true>(a, dw, ws, workspace_bytes, c.nsplit, st);
        if (t.bn == 64) return launch_wgrad_tile<128, 64, 2, 2, true>(a, dw, ws, workspace_bytes, c.nsplit, st);
        return launch_wgrad_tile<128, 32, 4, 1, true>(a, dw, ws, workspace_bytes, c.nsplit, st);
    }
    }
    return split_sum::launch_sliced<1>(ws, dw, (int)nout, nparts, accumulate, st);
}

int pnp_conv2d_wgrad(const float* x, const float* dy, float* dw, const pnp_conv_geom* g, void* workspace,
                     size_t workspace_bytes, void* stream) {
    return wgrad_impl(x, dy, dw, g, workspace, workspace_bytes, stream, 0);
}

int pnp_conv2d_wgrad_acc(const float* x, const float* dy, float* dw, const pnp_conv_geom* g, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return wgrad_impl(x, dy, dw, g, workspace, workspace_bytes, stream, 1);
}

// ---- bf16-resident filter gradient (conv_bf16r.hip): x and dy as bf16 tensors; the split planner and the partial-sum kernel are the
// fp32 path's own
static int wgrad_bf16r_plan(const pnp_conv_geom* g, int* bm, int* bn) {
    const int tile = wgrad_bf16r_tile(g);
    if (tile < 0) return 0;
    *bm = tile < 2 ? 128 : 64;
    *bn = (tile & 1) ? 64 : 128;
    const long long P = (long long)g->N * g->OH * g->OW;
    const int nblk = (g->R * g->S * g->C / *bm) * (g->K / *bn);
    static const int force = getenv("PNP_BF16R_WSPLIT") ? atoi(getenv("PNP_BF16R_WSPLIT")) : 0;      // experiments: force the split count
    if (force > 0) return force;
    const int nchunks = pnp_cdiv(P, kWgradBf16rChunk);
    // The resident kernel is ~3x faster than the fp32 ring kernel while a split partial costs the same bytes, so the fp32 planner's
    // "fill >= one dispatch round of 512" over-splits here (256->256@32^2: 15 splits 0.052 ms, 7 splits 0.048 ms; round 4 sweep,
    // tools/experiments/README.md).  Cost model, microseconds: dispatch rounds x (stages per workgroup x 0.7 x tile/128^2 + 6 fixed)
    // + partials written and read back at 4 TB/s; the split with the lowest estimate wins (ties: fewer splits).  Against the fp32
    // planner on every layer at B = 16: better or equal everywhere (64->64@64^2 0.044 -> 0.030 ms, 256->256@32^2 0.053 -> 0.041,
    // cls1 64->64@256^2 0.188 -> 0.165, 512->512 equal); bf16 joint step, same box x2: 457.0 -> 460.8 slices/s.
    const double t_stage = 0.7 * ((double)*bm * *bn) / (128.0 * 128.0);
    const double nout_mb = (double)g->R * g->S * g->C * g->K * 4.0 / 1e6;
    int best = 1;
    double best_t = 1e30;
    const int max_split = nchunks / 4 < 1 ? 1 : (nchunks / 4 > 64 ? 64 : nchunks / 4);
    for (int ns = 1; ns <= max_split; ++ns) {
        const double rounds = ceil((double)nblk * ns / 512.0);
        const double t = rounds * (ceil((double)nchunks / ns) * t_stage + 6.0) + (ns > 1 ? 2.0 * ns * nout_mb / 4.0 + 3.0 : 0.0);
        if (t < best_t - 1e-9) { best_t = t; best = ns; }
    }
    return best;
}

size_t pnp_conv2d_wgrad_bf16r_workspace_bytes(const pnp_conv_geom* g) {
    int bm, bn;
    const int ns = g ? wgrad_bf16r_plan(g, &bm, &bn) : 0;
    return ns > 1 ? (size_t)ns * g->R * g->S * g->C * g->K * sizeof(float) : 0;
}

int pnp_conv2d_wgrad_bf16r(const void* xh, const void* dyh, float* dw, int32_t accumulate, const pnp_conv_geom* g, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (int e = check_geom(g, "pnp_conv2d_wgrad_bf16r")) return e;
    PNP_REQUIRE(xh && dyh && dw, "pnp_conv2d_wgrad_bf16r: null pointer");
    int bm, bn;
    const int want = wgrad_bf16r_plan(g, &bm, &bn);
    PNP_REQUIRE(want >= 1, "pnp_conv2d_wgrad_bf16r: geometry not served (pnp_conv2d_bf16r_served(g, 2))");
    ConvArgs a = make_args((const float*)xh, (const float*)dyh, dw, g);
    a.dtype = PNP_DTYPE_BF16;
    a.x_bytes = (unsigned)((size_t)g->N * g->H * g->W * g->C * 2);
    a.w_bytes = (unsigned)((size_t)g->N * g->OH * g->OW * g->K * 2);      // a.w is dy [P][K]
    a.nblk_m = a.Kred / bm;
    a.nblk_n = a.K / bn;
    const size_t nout = (size_t)a.Kred * a.K;
    float* ws = (float*)workspace;
    if (!ws) workspace_bytes = 0;
    const SplitFit fit = fit_split(pnp_cdiv(a.M, kWgradBf16rChunk), want, nout, workspace_bytes);
    const int nsplit = fit.nsplit;
    a.chunks_per_split = fit.per;
    a.nsplit = nsplit;
    a.split_stride = (long long)nout;
    a.y = (nsplit > 1) ? ws : dw;
    a.accumulate = (nsplit > 1) ? 0 : accumulate;       // un-split: in the kernel's epilogue; split: in the reduce kernel
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(a.nblk_m * a.nblk_n * nsplit));
    PNP_REQUIRE(launch_wgrad_bf16r(a, wgrad_bf16r_tile(g), grid, st), "conv_wgrad_bf16r_kernel: no instance");
    PNP_CHECK_LAUNCH("conv_wgrad_bf16r_kernel");
    if (nsplit > 1) return split_sum::launch_serial(ws, nout, nsplit, nout, split_sum::Plain{dw, (int)accumulate}, st);
    return PNP_OK;
}

int pnp_sympad_fwd(const float* x, float* xp, int32_t N, int32_t H, int32_t W, int32_t C, int32_t p, void* stream) {
    PNP_REQUIRE(x && xp && N > 0 && H > 0 && W > 0 && C > 0 && p >= 0 && p <= H && p <= W, "pnp_sympad_fwd: bad argument");
    const int vec = (C % 4 == 0) ? 1 : 0;
    const size_t total = (size_t)N * (H + 2 * p) * (W + 2 * p) * (vec ? C / 4 : C);
    long long nb = (long long)((total + 255) / 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(sympad_fwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, xp, N, H, W, C, p, vec);
    PNP_CHECK_LAUNCH("sympad_fwd_kernel");
    return PNP_OK;
}

int pnp_sympad_bwd(const float* dxp, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t p, void* stream) {
    PNP_REQUIRE(dxp && dx && N > 0 && H > 0 && W > 0 && C > 0 && p >= 0 && p <= H && p <= W, "pnp_sympad_bwd: bad argument");
    const size_t total = (size_t)N * H * W * C;
    hipLaunchKernelGGL(sympad_bwd_kernel, dim3((unsigned)pnp_cdiv((long long)total, 256)), dim3(256), 0,
                       (hipStream_t)stream, dxp, dx, N, H, W, C, p);
    PNP_CHECK_LAUNCH("sympad_bwd_kernel");
    return PNP_OK;
}

}  // extern "C"
