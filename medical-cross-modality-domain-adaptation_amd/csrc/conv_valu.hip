// conv_valu.hip — the vector-ALU family of the fp32 convolutions (routes NARROW and WGD): layers with K <= 16 filters, where an MFMA tile
// is at most half full in N.  Declared in conv_common.h like the other route files: the predicates and byte counts that plan_fwd / plan_dgrad /
// plan_wgrad (conv_igemm.hip) combine, and one launch per kernel family.
//   conv_fwd_narrow_kernel  K <= 16 outputs at stride 1 (LDS patch, filters through the scalar cache, v_pk_fma_f32): forward, and the data
//                           gradient of a layer with that few INPUT channels
//   wgrad_direct(4)_kernel  filter gradient for K <= 16 (dy through the scalar cache); per-workgroup partials [wgd_blocks][R*S*C*K], summed by
//                           the caller (split_sum.h: sliced_kernel<1>, fixed order)
#include "conv_common.h"

using namespace pnpconv;

namespace {

// ===================================== direct forward conv for narrow outputs ============================================
// K <= 16 output channels at stride 1 (the 40->5 logits conv and g1's 16->16 convs at 256^2, and their data gradients when the INPUT
// is that narrow): an MFMA tile is half to 5/6 empty in N (40->5 measured 15 TF/s, bound by the matrix pipe doing mostly zeros).  A thread owns one output pixel and its K accumulators.  The workgroup's input patch
// ((8 + (R-1)dil) x (32 + (S-1)dil) pixels x C channels) is staged once in LDS with a pixel stride of C+4 floats when C/4 is even (an odd
// number of 16-byte slots per pixel: the 64 lanes of a ds_read_b128 spread over all banks); the filter values are uniform over the
// wave and come through the scalar cache (constant address space), so the inner loop is v_pk_fma_f32 acc, x, s[w].
struct NarrowArgs {
    const float* x;
    const float* w;
    float* y;
    int N, H, W, C, K, R, S, OH, OW, dil, pad_t, pad_l;
    int PH, PW, CP;                 // patch extent (pixels) and padded pixel stride (floats)
    int do_drop;
    float drop_keep;
    uint32_t drop_thresh, drop_key;
    unsigned x_bytes;
    const pnp_step_params* sp;
    uint32_t drop_sid;
};

template <int KK, bool EXACT>
__global__ void __launch_bounds__(256) conv_fwd_narrow_kernel(NarrowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int t = threadIdx.x;
    const int tx = t & 31, ty = t >> 5;
    const int ow0 = blockIdx.x * 32, oh0 = blockIdx.y * 8, n = blockIdx.z;
    const int K = EXACT ? KK : a.K;
    const int C4 = a.C >> 2;
    // ---- stage the patch (zero outside the image) --------------------------------------------------------------------
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const int nvec = a.PH * a.PW * C4;
    for (int i = t; i < nvec; i += 256) {
        const int pix = i / C4, c4 = i - pix * C4;
        const int pr = pix / a.PW, pc = pix - pr * a.PW;
        const int ih = oh0 - a.pad_t + pr, iw = ow0 - a.pad_l + pc;
        const bool ok = ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
        const f32x4 v = bload4(rx, ok ? (unsigned)((((n * a.H + ih) * a.W + iw) * a.C + 4 * c4) * 4) : OOB);
        *reinterpret_cast<f32x4*>(xs + pix * a.CP + 4 * c4) = v;
    }
    __syncthreads();
    // ---- accumulate ---------------------------------------------------------------------------------------------------
    pnp_cfloat* wc = (pnp_cfloat*)(uintptr_t)a.w;
    constexpr int UNR = KK <= 8 ? 2 : 1;        // 4*KK filter values per channel quad live in SGPRs
    float acc[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[k] = 0.f;
    for (int r = 0; r < a.R; ++r)
        for (int sx = 0; sx < a.S; ++sx) {
            const float* xp = xs + ((ty + r * a.dil) * a.PW + tx + sx * a.dil) * a.CP;
            const int wbase = (r * a.S + sx) * a.C * K;
#pragma unroll UNR
            for (int c4 = 0; c4 < C4; ++c4) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int k = 0; k < KK; ++k)
                        if (k < K) acc[k] = fmaf(xv[e], wc[wbase + (4 * c4 + e) * K + k], acc[k]);
            }
        }
    const int oh = oh0 + ty, ow = ow0 + tx;
    if (oh < a.OH && ow < a.OW) {
        const size_t m = ((size_t)n * a.OH + oh) * a.OW + ow;
#pragma unroll
        for (int k = 0; k < KK; ++k)
            if (k < K) {
                const size_t idx = m * K + k;
                float v = acc[k];
                if (a.do_drop) v = pnp_drop_keep((uint32_t)idx, pnp_eff_drop_key(a.drop_key, a.sp, a.drop_sid), a.drop_thresh) ? v / a.drop_keep : 0.f;
                a.y[idx] = v;
            }
    }
}

// ===================================== direct filter gradient for narrow outputs ============================================
// K <= 16 output channels (g1's 16-channel convs, the 40->5 logits conv, the mask critic's first conv): an MFMA tile is at most half
// full in N and the reduction (all pixels) is long, so this one runs on the vector ALUs.  A thread owns PPT (tap, channel) pairs x K
// accumulators, walks the pixels of its workgroup's slab, reads ONE x value per pair and pixel plus the pixel's K dy values (the
// same address for a whole pixel group: a broadcast load) and issues PPT*K FMAs.  Workgroups with few pairs split their slab over G
// pixel groups and combine through LDS.  Partials [nblk][R*S*C*K] are summed by split_sum.h's sliced_kernel<1> (fixed order: deterministic).
struct WgdArgs {
    const float* x;
    const float* dy;
    float* part;
    int N, H, W, C, K, R, S, OH, OW, stride, dil, pad_t, pad_l;
    int P;             // N*OH*OW
    int npairs;        // R*S*C
    int G;             // pixel groups per workgroup (1 when a thread owns several pairs)
    int ppb;           // pixels per workgroup
    unsigned x_bytes, dy_bytes;
};


// UNI (one pixel group): the pixel index is uniform over the workgroup, so the K dy values come through the SCALAR cache into SGPRs
// (v_fmac with an SGPR operand) instead of 64 lanes x 16 B of vector-memory traffic per wave and pixel for 64 useful bytes — the
// texture-address unit, not the FMAs, bounded the first version (16->16: 0.54 ms).
template <int KK, int PPT, bool EXACT, bool UNI>
__global__ void __launch_bounds__(256) wgrad_direct_kernel(WgdArgs a) {
    extern __shared__ float red[];      // [G][npairs*K], only when G > 1
    const int t = threadIdx.x;
    if (UNI && PPT == 1 && (t & ~63) >= a.npairs) return;      // whole wave without a pair (no barrier on this path)
    const int g = (PPT == 1 && !UNI) ? t / a.npairs : 0;
    const int j0 = (PPT == 1) ? t - g * a.npairs : t;
    const bool active = g < a.G;
    const int K = EXACT ? KK : a.K;
    int coff[PPT], dh[PPT], dw[PPT];
    bool pv[PPT];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int j = j0 + q * 256;
        pv[q] = active && j < a.npairs;
        const int jj = pv[q] ? j : 0;
        const int tap = jj / a.C;
        coff[q] = jj - tap * a.C;
        const int r = tap / a.S;
        dh[q] = r * a.dil - a.pad_t;
        dw[q] = (tap - r * a.S) * a.dil - a.pad_l;
    }
    float acc[PPT][KK];
#pragma unroll
    for (int q = 0; q < PPT; ++q)
#pragma unroll
        for (int k = 0; k < KK; ++k) acc[q][k] = 0.f;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(a.dy, a.dy_bytes);
    const int p0 = blockIdx.x * a.ppb;
    const int p1 = (p0 + a.ppb < a.P) ? p0 + a.ppb : a.P;
    int p = UNI ? p0 : p0 + g;
    pnp_cfloat* dyc = (pnp_cfloat*)(uintptr_t)a.dy;
    const int OHW = a.OH * a.OW;
    int n = p / OHW;
    int rem = p - n * OHW;
    int oh = rem / a.OW;
    int ow = rem - oh * a.OW;
    // U pixels per trip: all their loads are issued before the first FMA (one pixel per trip is bound by the global-load latency:
    // 16->16 ran at 0.58 ms that way)
    constexpr int U = 4;
    for (; p < p1; p += U * a.G) {
        float dv[U][KK], xv[U][PPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pu = p + u * a.G;
            const bool pin = pu < p1;
            if constexpr (UNI) {
                const size_t base = (size_t)(pin ? pu : p) * K;      // uniform; a pixel past the slab re-reads a valid row (its x is 0)
#pragma unroll
                for (int k = 0; k < KK; ++k) dv[u][k] = (k < K) ? dyc[base + k] : 0.f;
            } else if constexpr (EXACT && (KK % 4) == 0) {
#pragma unroll
                for (int k4 = 0; k4 < KK / 4; ++k4) {
                    const f32x4 v = bload4(rd, pin ? (unsigned)((pu * KK + 4 * k4) * 4) : OOB);
                    dv[u][4 * k4] = v[0]; dv[u][4 * k4 + 1] = v[1]; dv[u][4 * k4 + 2] = v[2]; dv[u][4 * k4 + 3] = v[3];
                }
            } else {
#pragma unroll
                for (int k = 0; k < KK; ++k) dv[u][k] = (pin && k < K) ? bload1(rd, (unsigned)((pu * K + k) * 4)) : 0.f;
            }
            const int vh = oh * a.stride, vw = ow * a.stride;
#pragma unroll
            for (int q = 0; q < PPT; ++q) {
                const int ih = vh + dh[q], iw = vw + dw[q];
                const bool ok = pin & pv[q] & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
                xv[u][q] = bload1(rx, ok ? (unsigned)((((n * a.H + ih) * a.W + iw) * a.C + coff[q]) * 4) : OOB);
            }
            ow += a.G;
            while (ow >= a.OW) {
                ow -= a.OW;
                if (++oh == a.OH) { oh = 0; ++n; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < PPT; ++q)
#pragma unroll
                for (int k = 0; k < KK; ++k) acc[q][k] = fmaf(xv[u][q], dv[u][k], acc[q][k]);
    }
    const int nout = a.npairs * K;
    float* outp = a.part + (size_t)blockIdx.x * nout;
    if (a.G > 1) {          // PPT == 1
        if (active) {
#pragma unroll
            for (int k = 0; k < KK; ++k)
                if (k < K) red[g * nout + j0 * K + k] = acc[0][k];
        }
        __syncthreads();
        for (int e = t; e < nout; e += 256) {
            float sum = 0.f;
            for (int gg = 0; gg < a.G; ++gg) sum += red[gg * nout + e];
            outp[e] = sum;
        }
    } else {
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            if (pv[q]) {
                const int j = j0 + q * 256;
#pragma unroll
                for (int k = 0; k < KK; ++k)
                    if (k < K) outp[j * K + k] = acc[q][k];
            }
        }
    }
}

// Same for C % 4 == 0 and many pairs (the 40->5 logits conv: 1000 pairs): a thread owns QPT quads of 4 consecutive channels of one
// tap and fetches each with ONE 16-byte load — with one dword per pair the 4 loads per lane and pixel kept the texture-address unit
// busy for the whole 0.41 ms of the kernel.  One pixel group (uniform pixel): dy through the scalar cache.
template <int KK, int QPT, bool EXACT>
__global__ void __launch_bounds__(256) wgrad_direct4_kernel(WgdArgs a) {
    const int t = threadIdx.x;
    const int nquads = a.npairs >> 2;
    const int K = EXACT ? KK : a.K;
    int coff[QPT], dh[QPT], dw[QPT];
    bool pv[QPT];
#pragma unroll
    for (int q = 0; q < QPT; ++q) {
        const int i = t + q * 256;
        pv[q] = i < nquads;
        const int j = pv[q] ? 4 * i : 0;
        const int tap = j / a.C;
        coff[q] = j - tap * a.C;
        const int r = tap / a.S;
        dh[q] = r * a.dil - a.pad_t;
        dw[q] = (tap - r * a.S) * a.dil - a.pad_l;
    }
    float acc[QPT][4][KK];
#pragma unroll
    for (int q = 0; q < QPT; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < KK; ++k) acc[q][e][k] = 0.f;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.x_bytes);
    pnp_cfloat* dyc = (pnp_cfloat*)(uintptr_t)a.dy;
    const int p0 = blockIdx.x * a.ppb;
    const int p1 = (p0 + a.ppb < a.P) ? p0 + a.ppb : a.P;
    const int OHW = a.OH * a.OW;
    int n = p0 / OHW;
    int rem = p0 - n * OHW;
    int oh = rem / a.OW;
    int ow = rem - oh * a.OW;
    constexpr int U = 4;
    for (int p = p0; p < p1; p += U) {
        float dv[U][KK];
        f32x4 xv[U][QPT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pu = p + u;
            const bool pin = pu < p1;
            const size_t base = (size_t)(pin ? pu : p) * K;
#pragma unroll
            for (int k = 0; k < KK; ++k) dv[u][k] = (k < K) ? dyc[base + k] : 0.f;
            const int vh = oh * a.stride, vw = ow * a.stride;
#pragma unroll
            for (int q = 0; q < QPT; ++q) {
                const int ih = vh + dh[q], iw = vw + dw[q];
                const bool ok = pin & pv[q] & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
                xv[u][q] = bload4(rx, ok ? (unsigned)((((n * a.H + ih) * a.W + iw) * a.C + coff[q]) * 4) : OOB);
            }
            if (++ow == a.OW) {
                ow = 0;
                if (++oh == a.OH) { oh = 0; ++n; }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < QPT; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int k = 0; k < KK; ++k) acc[q][e][k] = fmaf(xv[u][q][e], dv[u][k], acc[q][e][k]);
    }
    float* outp = a.part + (size_t)blockIdx.x * a.npairs * K;
#pragma unroll
    for (int q = 0; q < QPT; ++q) {
        if (pv[q]) {
            const int j = 4 * (t + q * 256);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k = 0; k < KK; ++k)
                    if (k < K) outp[(j + e) * K + k] = acc[q][e][k];
        }
    }
}

// ---- direct forward for K <= 8 (conv_fwd_narrow_kernel): applicability + launch -------------------------------------------------
// (pnpconv::narrow_fwd_ok is this predicate; the launch also takes the LDS patch it sized)
bool narrow_patch_ok(const pnp_conv_geom* g, NarrowArgs* na) {
    static const int off = getenv("PNP_CONV_NONARROW") ? 1 : 0;
    if (off || g->K > 16 || g->stride != 1 || g->pad_mode != PNP_PAD_ZERO || (g->C & 3) != 0 || g->C < 8) return false;
    if ((long long)g->N * g->OH * g->OW < 8192) return false;
    // launch_narrow puts the images on the grid's z extent.  hipGetDeviceProperties on an MI355X (ROCm 7.2) reports maxGridSize =
    // (2147483647, 65536, 65536), and hipDeviceAttributeMaxGridDimZ 65536: a launch past that is outside what HIP promises, so such a
    // batch of tiny maps runs on the implicit GEMM.  The figure is a constant here because the route query must answer on hosts without
    // a device.  n16_geom_ok (conv_small.hip) stops one short, at the 65535 of the CUDA-style limit it was written against; both are safe,
    // and (65536, 1, 1, 16 -> 16) is the row of tests/test_gpu_igemm_domain.py that runs this kernel at the bound.
    if (g->N > 65536) return false;
    // 9..16 outputs: the MFMA tile is half full, the vector ALUs only win while the work per pixel is small (16->16 3x3: 0.154 -> 0.130 ms;
    // 32->16 3x3, twice the work: 0.062 -> 0.071)
    if (g->K > 8 && (long long)g->R * g->S * g->C * g->K > 2304) return false;
    const int PH = 8 + (g->R - 1) * g->dil, PW = 32 + (g->S - 1) * g->dil;
    const int CP = ((g->C >> 2) & 1) ? g->C : g->C + 4;
    if ((size_t)PH * PW * CP * sizeof(float) > 150 * 1024) return false;
    if (na) { na->PH = PH; na->PW = PW; na->CP = CP; }
    return true;
}

template <int KK, bool EXACT>
int launch_narrow_inst(const NarrowArgs& na, dim3 grid, size_t lds, hipStream_t st) {
    PNP_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(conv_fwd_narrow_kernel<KK, EXACT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                "conv_fwd_narrow_kernel: cannot reserve %zu bytes of LDS", lds);
    const double npx = (double)na.N * na.OH * na.OW, red = (double)na.R * na.S * na.C;
    PnpProfScope ps(PNP_PROF_CONV_DIRECT, st, 2.0 * npx * red * na.K, 4.0 * ((double)na.N * na.H * na.W * na.C + npx * na.K + red * na.K),
                    "conv_fwd_narrow_kernel<%d, %s>", KK, EXACT ? "true" : "false");
    hipLaunchKernelGGL((conv_fwd_narrow_kernel<KK, EXACT>), grid, dim3(256), lds, st, na);
    PNP_CHECK_LAUNCH("conv_fwd_narrow_kernel");
    return PNP_OK;
}

}  // namespace

namespace pnpconv {

bool narrow_fwd_ok(const pnp_conv_geom* g) { return narrow_patch_ok(g, nullptr); }

// x, w, y and geometry of a stride-1 zero-padded conv with K <= 16 (forward, or a data gradient expressed as one); dropout from `a`
int launch_narrow(const float* x, const float* w, float* y, const pnp_conv_geom* g, const ConvArgs& a, hipStream_t st) {
    NarrowArgs na{};
    narrow_patch_ok(g, &na);
    na.x = x; na.w = w; na.y = y;
    na.N = g->N; na.H = g->H; na.W = g->W; na.C = g->C; na.K = g->K; na.R = g->R; na.S = g->S; na.OH = g->OH; na.OW = g->OW;
    na.dil = g->dil; na.pad_t = g->pad_t; na.pad_l = g->pad_l;
    na.do_drop = a.do_drop; na.drop_keep = a.drop_keep; na.drop_thresh = a.drop_thresh; na.drop_key = a.drop_key;
    na.sp = a.sp; na.drop_sid = a.drop_sid;
    na.x_bytes = a.x_bytes;
    const size_t lds = (size_t)na.PH * na.PW * na.CP * sizeof(float);
    dim3 grid((unsigned)pnp_cdiv(g->OW, 32), (unsigned)pnp_cdiv(g->OH, 8), (unsigned)g->N);
    if (g->K == 5) return launch_narrow_inst<5, true>(na, grid, lds, st);
    if (g->K == 16) return launch_narrow_inst<16, true>(na, grid, lds, st);
    if (g->K <= 8) return launch_narrow_inst<8, false>(na, grid, lds, st);
    return launch_narrow_inst<16, false>(na, grid, lds, st);
}

}  // namespace pnpconv

namespace {

// ---- direct (vector-ALU) filter gradient for K <= 16: plan shared by the workspace query and the launch -------------------------
struct WgdPlan { int use, nblk, ppb, G, ppt; size_t ws_bytes; };

WgdPlan wgd_plan(const pnp_conv_geom* g) {
    static const int off = getenv("PNP_CONV_NODIRECT") ? 1 : 0;
    WgdPlan pl{};
    const long long P = (long long)g->N * g->OH * g->OW;
    const int npairs = g->R * g->S * g->C;
    if (off || g->K > 16 || g->pad_mode != PNP_PAD_ZERO || npairs > 1024 || P < 8192) return pl;
    pl.use = 1;
    pl.ppt = npairs <= 256 ? 1 : pnp_cdiv(npairs, 256);
    pl.G = pl.ppt == 1 ? 256 / npairs : 1;
    if (pl.G > 16) pl.G = 16;
    long long nblk = P / 128;
    if (nblk > 2048) nblk = 2048;
    pl.ppb = (int)pnp_cdiv(P, nblk);
    pl.nblk = (int)pnp_cdiv(P, pl.ppb);
    pl.ws_bytes = (size_t)pl.nblk * npairs * g->K * sizeof(float);
    return pl;
}

template <int KK, bool EXACT>
int launch_wgd_inst(const WgdArgs& a, const WgdPlan& pl, hipStream_t st) {
    const size_t lds = pl.G > 1 ? (size_t)pl.G * a.npairs * a.K * sizeof(float) : 0;
    dim3 grid((unsigned)pl.nblk), blk(256);
    const int nquads = a.npairs / 4;
    PnpProfScope ps(PNP_PROF_CONV_DIRECT, st, 2.0 * (double)a.P * a.npairs * a.K,
                    4.0 * ((double)a.N * a.H * a.W * a.C + (double)a.P * a.K + (double)a.npairs * a.K), "wgrad_direct_kernel<%d> (all variants)", KK);
    // quads: one 16-byte x load per 4 pairs, one quad per thread (wgd_plan stops at 1024 pairs = 256 quads)
    if ((a.C % 4) == 0 && nquads >= 128 && nquads <= 256 && KK <= 8) hipLaunchKernelGGL((wgrad_direct4_kernel<KK, 1, EXACT>), grid, blk, 0, st, a);
    else if (pl.ppt == 1 && pl.G > 1) hipLaunchKernelGGL((wgrad_direct_kernel<KK, 1, EXACT, false>), grid, blk, lds, st, a);
    else if (pl.ppt == 1) hipLaunchKernelGGL((wgrad_direct_kernel<KK, 1, EXACT, true>), grid, blk, lds, st, a);
    else if (pl.ppt == 2) hipLaunchKernelGGL((wgrad_direct_kernel<KK, 2, EXACT, true>), grid, blk, lds, st, a);
    else if (pl.ppt == 3) hipLaunchKernelGGL((wgrad_direct_kernel<KK, 3, EXACT, true>), grid, blk, lds, st, a);
    else hipLaunchKernelGGL((wgrad_direct_kernel<KK, 4, EXACT, true>), grid, blk, lds, st, a);
    PNP_CHECK_LAUNCH("wgrad_direct_kernel");
    return PNP_OK;
}

}  // namespace

namespace pnpconv {

bool wgd_ok(const pnp_conv_geom* g) { return wgd_plan(g).use != 0; }
size_t wgd_workspace_bytes(const pnp_conv_geom* g) { return wgd_plan(g).ws_bytes; }
int wgd_blocks(const pnp_conv_geom* g) { return wgd_plan(g).nblk; }

// a = make_args(x, dy, -, g) of the forward geometry with a.w_bytes = the bytes of dy; part: wgd_workspace_bytes(g)
int launch_wgd(const float* x, const float* dy, float* part, const pnp_conv_geom* g, const ConvArgs& a, hipStream_t st) {
    const WgdPlan pl = wgd_plan(g);
    WgdArgs d{};
    d.x = x; d.dy = dy; d.part = part;
    d.N = g->N; d.H = g->H; d.W = g->W; d.C = g->C; d.K = g->K; d.R = g->R; d.S = g->S; d.OH = g->OH; d.OW = g->OW;
    d.stride = g->stride; d.dil = g->dil; d.pad_t = g->pad_t; d.pad_l = g->pad_l;
    d.P = a.M; d.npairs = a.Kred; d.G = pl.G; d.ppb = pl.ppb;
    d.x_bytes = a.x_bytes; d.dy_bytes = a.w_bytes;
    if (g->K == 16) return launch_wgd_inst<16, true>(d, pl, st);
    if (g->K == 5) return launch_wgd_inst<5, true>(d, pl, st);
    if (g->K <= 8) return launch_wgd_inst<8, false>(d, pl, st);
    return launch_wgd_inst<16, false>(d, pl, st);
}

}  // namespace pnpconv
