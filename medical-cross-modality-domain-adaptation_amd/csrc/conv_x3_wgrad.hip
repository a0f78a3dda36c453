// conv_x3_wgrad.hip — FILTER GRADIENT of the narrow stride-1 3x3 layers (32 / 64 input channels, 64 filters) on the bf16 matrix pipe with
// split operands: the third member of conv_x3_direct.hip's family (forward, data gradient), DESIGN §10.2.
//
//   dW[r][s][c][k] = sum over (n, h, w) of x[n][h + r - pad][w + s - pad][c] * dy[n][h][w][k]
//
// The reduction index is the PIXEL and both operands are pixel-major in memory, so both are activations that have to be split (an fp32 value
// IS the sum of three bf16 planes hi / mid / lo; six plane products, smallest first, reproduce the fp32 product to 2^-26) on their way in:
//   * work unit = 4 rows x 16 columns of one 16 x 16 output tile (64 pixels = four MFMA k-slabs of 16).  Four loader waves fetch the unit's
//     6 x 18 halo patch of x (all channels) and its 64 pixels x 64 filters of dy as fp32, split them in registers and store the planes as LDS
//     rows of 64 bytes per pixel (32 channels / filters of one plane): [channel half][plane][108 pixels], [filter half][plane][64 pixels].
//     Two such buffers (2 x 66 048 B for 64 channels): while unit v is contracted the loaders request unit v + 2 from memory (two register
//     sets) and then split and store unit v + 1; ONE workgroup barrier per unit.  The nine taps are LDS address offsets into the one patch.
//     (A whole 16 x 16 tile does not fit twice: 124 KB of patch planes + 96 KB of dy planes.  Staging by 32 channels would idle half of the
//     consumer waves, whose blocks are split by channel half; staging by rows keeps all four busy.  The price is the vertical halo: 6 patch
//     rows per 4 output rows, 1.69x instead of 1.27x of x through L2 -> CU.)
//   * the MFMA wants 8 consecutive reduction elements (pixels) per lane, LDS rows are pixels: ds_read_b64_tr_b16 transposes on the way out
//     (conv_bf16r.hip's filter gradient).  The four rows of a 16-lane group's block are four CONSECUTIVE pixels of 64 bytes: a 32-lane half
//     reads 256 contiguous bytes, every bank once, so the image needs no swizzle and every fragment address is one lane base + an immediate.
//     The consumer waves have no memory loads in flight, so the builtin is used and the compiler counts the waits.
//   * four consumer waves; wave (cm, kn) owns the 32 channels x 32 filters block (cm, kn) of ALL nine taps: nine accumulators = 144
//     registers, in registers for the whole launch.  A unit is walked by patch row, so every x fragment (3 planes) is read once and serves
//     up to three taps, and the dy fragments of a k-slab are read once for its nine taps: 132 reads per 216 v_mfma_f32_32x32x16_bf16.  With 32
//     input channels there are only two such blocks: the waves pair up on one block and take two of the four k-slabs each (two partial
//     sums per workgroup).
//   * persistent workgroups (at most one per CU) over a STATIC contiguous share of the tiles; each writes its partial [9 C 64] once, and
//     split_sum.h's sliced_kernel<4> sums the partials in a fixed order (two deterministic levels: 16 interleaved chains per value, then the 16 in order)
//     and adds into dW for the accumulating entry point.  No atomics: two runs are bit-identical.
// Entry: plan_wgrad (conv_igemm.hip) asks x3w_chosen() after the Winograd filter-gradient planner and before the fp32-pipe ring kernel;
// x3w_workspace_bytes() is what wgrad_ws() reports for the layers the predicate takes.  PNP_X3_WGRAD / pnp_conv2d_x3_wgrad(): 0 off, 1 on,
// under PNP_X3_DIRECT's mode (0 there: off; 1: layers with >= 256 tiles; 2: wherever the shapes allow).
#include "conv_x3_common.h"
#include "split_sum.h"

using namespace pnpconv;

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int TH = 16, TW = 16;                    // the tile of the planner and of the static shares (conv_x3_direct.hip's)
constexpr int UH = 4, UPT = TH / UH;               // output rows per unit, units per tile
constexpr int PW = TW + 2, UPH = UH + 2, NPXU = UPH * PW;       // 6 x 18 = 108 patch pixels per unit
constexpr int ROWB = 64;                           // bytes per LDS row: 32 channels (filters) of one plane
constexpr int XPL = NPXU * ROWB;                   // 6 912 B per (channel half, plane) of the patch
constexpr int DPL = UH * TW * ROWB;                // 4 096 B per (filter half, plane) of the dy unit
constexpr int KF = 64;                             // filters
constexpr int DYB = 2 * 3 * DPL;                   // 24 576 B
constexpr int NLD = 256;                           // loader lanes (4 waves)
constexpr int ND4 = UH * TW * (KF / 4);            // float4 of a dy unit: 1 024
constexpr int NDI = ND4 / NLD;                     // 4 per loader lane

struct X3wArgs {
    const float* x;               // [N][H][W][C]
    const float* dy;              // [N][OH][OW][64]
    float* part;                  // [parts][9][C][64]
    int N, H, W, C, OH, OW, pad_t, pad_l;
    int ntiles;
};

// Timing ablations (`make variant NAME=.. EXTRA=-DPNP_X3W_ABLATE=n`; results are WRONG, never the shipped library): 1 = no split arithmetic in
// the loaders (three copies of the rounded value), 2 = no memory loads after the first unit, 4 = no LDS fragment reads after the first unit
#ifndef PNP_X3W_ABLATE
#define PNP_X3W_ABLATE 0
#endif

// the shared split, with the ablation hook.  (The three plane stores behind it stay spelled out in the loaders: through store3() the kernel
// came out with another register allocation, 1.3 % slower at NH = 1 — profiles/x3_shared_pieces_ab.txt)
__device__ __forceinline__ void split3a(const f32x4 v, bf16x4& hi, bf16x4& mi, bf16x4& lo) {
    if (PNP_X3W_ABLATE & 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) hi[c] = mi[c] = lo[c] = (__bf16)v[c];
    } else {
        split3(v, hi, mi, lo);
    }
}

__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p) {
    // rows p and p + 4 ROWB: pixels 0..3 and 4..7 of the lane's 8 (+ 8 for the upper half-wave, in the lane base)
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * ROWB));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// NH = C / 32 channel halves (1 or 2)
template <int NH>
__global__ void __launch_bounds__(512, 1) conv_x3_wgrad_kernel(X3wArgs a) {
    constexpr int XB = NH * 3 * XPL;               // patch planes of a unit
    constexpr int BUF = XB + DYB;                  // 66 048 B (NH = 2), 45 312 B (NH = 1)
    constexpr int NX4 = NPXU * NH * 8;             // float4 of a patch
    constexpr int NXI = (NX4 + NLD - 1) / NLD;     // per loader lane: 7 (4)
    constexpr int C = NH * 32;
    __shared__ __attribute__((aligned(256))) unsigned char lds[2 * BUF];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tiles_x = a.OW / TW, tiles_y = a.OH / TH;
    // static contiguous share of the tiles (grid <= ntiles: never empty)
    const int t0 = (int)(((long long)blockIdx.x * a.ntiles) / gridDim.x);
    const int t1 = (int)(((long long)(blockIdx.x + 1) * a.ntiles) / gridDim.x);
    const int nu = (t1 - t0) * UPT;

    if (wave >= 4) {
        // ============================ loaders: global fp32 -> three bf16 planes -> LDS ============================
        const int pl = (wave - 4) * 64 + lane;
        // two register sets: the loads of unit v + 2 are issued right behind the barrier of unit v, in FRONT of the split and LDS stores of unit
        // v + 1, so they have a whole unit of MFMA work to land in (issued behind the stores they had what the stores left of it, and the
        // loaders were the last at the barrier: DESIGN 10.2).  Every load is unconditional (clamped address, zeroed when it is stored), so the
        // number in flight behind a set is known: s_waitcnt vmcnt(NLOADS).
        constexpr int NLOADS = NXI + NDI;
        f32x4 sxa[NXI], sda[NDI], sxb[NXI], sdb[NDI];
        unsigned oka = 0, okb = 0;                   // bit i: patch load i of the set lies inside the image
        auto load = [&](int v, f32x4 (&sx)[NXI], f32x4 (&sd)[NDI], unsigned& okm) {
            const int tile = t0 + v / UPT, u = v % UPT;
            const int n = tile / (tiles_x * tiles_y);
            const int r = tile - n * tiles_x * tiles_y;
            const int oh0 = (r / tiles_x) * TH + u * UH, ow0 = (r % tiles_x) * TW;
            okm = 0;
#pragma unroll
            for (int i = 0; i < NXI; ++i) {
                const int e = pl + i * NLD;
                const int q = e / (8 * NH), j = e % (8 * NH);
                const int pr = q / PW, pc = q - pr * PW;
                const int ih = oh0 - a.pad_t + pr, iw = ow0 - a.pad_l + pc;
                const bool ok = (e < NX4) & ((unsigned)ih < (unsigned)a.H) & ((unsigned)iw < (unsigned)a.W);
                okm |= ok ? (1u << i) : 0u;
                const int ihc = min(max(ih, 0), a.H - 1), iwc = min(max(iw, 0), a.W - 1);
                sx[i] = *reinterpret_cast<const f32x4*>(a.x + (((size_t)n * a.H + ihc) * a.W + iwc) * C + j * 4);
            }
#pragma unroll
            for (int i = 0; i < NDI; ++i) {         // (the tile lies inside the output: no mask)
                const int e = pl + i * NLD;
                const int q = e >> 4, j = e & 15;
                sd[i] = *reinterpret_cast<const f32x4*>(a.dy + (((size_t)n * a.OH + oh0 + (q >> 4)) * a.OW + ow0 + (q & 15)) * KF + j * 4);
            }
        };
        auto store = [&](int v, const f32x4 (&sx)[NXI], const f32x4 (&sd)[NDI], unsigned okm) {
            unsigned char* xb = lds + (v & 1) * BUF;
            unsigned char* db = xb + XB;
#pragma unroll
            for (int i = 0; i < NXI; ++i) {
                const int e = pl + i * NLD;
                if (e >= NX4) continue;
                const int q = e / (8 * NH), j = e % (8 * NH);
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                bf16x4 hi, mi, lo;
                split3a(((okm >> i) & 1u) ? sx[i] : zero, hi, mi, lo);
                unsigned char* p = xb + (j >> 3) * (3 * XPL) + q * ROWB + (j & 7) * 8;
                *reinterpret_cast<bf16x4*>(p) = hi;
                *reinterpret_cast<bf16x4*>(p + XPL) = mi;
                *reinterpret_cast<bf16x4*>(p + 2 * XPL) = lo;
            }
#pragma unroll
            for (int i = 0; i < NDI; ++i) {
                const int e = pl + i * NLD;
                const int q = e >> 4, j = e & 15;
                bf16x4 hi, mi, lo;
                split3a(sd[i], hi, mi, lo);
                unsigned char* p = db + (j >> 3) * (3 * DPL) + q * ROWB + (j & 7) * 8;
                *reinterpret_cast<bf16x4*>(p) = hi;
                *reinterpret_cast<bf16x4*>(p + DPL) = mi;
                *reinterpret_cast<bf16x4*>(p + 2 * DPL) = lo;
            }
        };
        // unit v: barrier; request unit v + 2 into the set unit v came from; split and store unit v + 1 from the other set
        auto unit = [&](int v, f32x4 (&sx)[NXI], f32x4 (&sd)[NDI], unsigned& okm, const f32x4 (&nx)[NXI], const f32x4 (&nd)[NDI], unsigned nok) {
            wait_lgkm0();                            // unit v is in LDS
            __builtin_amdgcn_s_barrier();            // ... and every consumer is past unit v - 1, whose buffer unit v + 1 takes
            const bool more = v + 2 < nu && (!(PNP_X3W_ABLATE & 2) || v < 2);
            if (more) load(v + 2, sx, sd, okm);
            if (v + 1 < nu) {
                if (more) wait_vm<NLOADS>();
                else wait_vm0();
                store(v + 1, nx, nd, nok);
            }
        };
        load(0, sxa, sda, oka);
        if (nu > 1) {
            load(1, sxb, sdb, okb);
            wait_vm<NLOADS>();
        } else {
            wait_vm0();
        }
        store(0, sxa, sda, oka);
        for (int v = 0; v < nu; v += 2) {
            unit(v, sxa, sda, oka, sxb, sdb, okb);
            if (v + 1 < nu) unit(v + 1, sxb, sdb, okb, sxa, sda, oka);
        }
        wait_vm0();
        return;
    }
    // ============================ consumers: block (cm, kn) of all nine taps per wave ============================
    // MFMA: A = x (rows = channels), B = dy (columns = filters), k = pixels: D[channel][filter], lane = filter (lane & 31) of block kn,
    // channels (i & 3) + 8 (i >> 2) + 4 (lane >> 5) of block cm.  Transposing read: lane (g = lane >> 4, e = (lane >> 2) & 3, q = lane & 3)
    // points at pixel 8 (g >> 1) + e of the slab, bytes 32 (g & 1) + 8 q of its row, and receives 4 consecutive pixels of channel lane & 31.
    const int cm = NH == 2 ? wave >> 1 : 0, kn = wave & 1;
    constexpr int NS = NH == 2 ? UH : UH / 2;        // k-slabs of a unit this wave contracts: all four, or (NH = 1) the wave pair's two
    const int sl = NH == 2 ? 0 : NS * (wave >> 1);
    const int g16 = lane >> 4, e4 = (lane >> 2) & 3, q4 = lane & 3;
    const int lbase = ((g16 >> 1) * 8 + e4) * ROWB + (g16 & 1) * 32 + q4 * 8;
    const int xoff = lbase + cm * (3 * XPL) + sl * (PW * ROWB);
    const int doff = lbase + XB + kn * (3 * DPL) + sl * (TW * ROWB);
    f32x16 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tap][e] = 0.f;
    // A unit is walked by PATCH row: the x fragments of patch row rho shifted by ts columns serve the taps (tr, ts) of the slabs rho - tr
    // (up to three of them), so every fragment is read once: NS + 2 rows x 3 shifts = 18 (12) steps of 6 reads and 6 .. 18 MFMAs per unit,
    // plus the dy fragments of each slab once.  The reads of step s + 1 (and of the next slab's dy fragments) are issued in front of the
    // MFMAs of step s; a scheduling barrier per step keeps the compiler from gathering them into bursts that the next MFMA waits on
    // (its own schedule of the plain tap loop: 30 exposed waits per unit; 0.410 -> 0.396 ms on 64 -> 64).
    constexpr int NSTEP = (NS + 2) * 3;
    bf16x8 df[NS][3], xf[2][3];
    for (int v = 0; v < nu; ++v) {
        wait_lgkm0();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const unsigned char* X = lds + (v & 1) * BUF + xoff;
        const unsigned char* D = lds + (v & 1) * BUF + doff;
        auto dread = [&](int r) {
            if ((PNP_X3W_ABLATE & 4) && v > 0) return;
#pragma unroll
            for (int p = 0; p < 3; ++p) df[r][p] = tr_frag(D + p * DPL + r * (TW * ROWB));
        };
        auto xread = [&](int step) {
            if ((PNP_X3W_ABLATE & 4) && v > 0) return;
#pragma unroll
            for (int p = 0; p < 3; ++p) xf[step & 1][p] = tr_frag(X + p * XPL + ((step / 3) * PW + step % 3) * ROWB);
        };
        dread(0);
        xread(0);
#pragma unroll
        for (int step = 0; step < NSTEP; ++step) {
            const int rho = step / 3, ts = step % 3;
            if (step + 1 < NSTEP) xread(step + 1);
            if (ts == 0 && rho + 1 < NS) dread(rho + 1);
#pragma unroll
            for (int tr = 0; tr < 3; ++tr) {
                const int r = rho - tr;
                if (r < 0 || r >= NS) continue;
#pragma unroll
                for (int trm = 0; trm < 6; ++trm)
                    acc[tr * 3 + ts] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[step & 1][kTermX[trm]], df[r][kTermW[trm]], acc[tr * 3 + ts], 0, 0, 0);
            }
            // three reads behind each of the step's first MFMAs, the rest of the MFMAs behind them
            const int nrd = (step + 1 < NSTEP ? 6 : 0) + (ts == 0 && rho + 1 < NS ? 6 : 0);
#pragma unroll
            for (int i = 0; i < nrd / 3; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---------------- the workgroup's partial sum(s): [tap][C][64], 128 contiguous bytes per channel row and wave-instruction
    const int pz = NH == 2 ? (int)blockIdx.x : (int)blockIdx.x * 2 + (wave >> 1);      // (NH = 1: one partial per wave pair)
    const int l31 = lane & 31, hh = lane >> 5;
    const __amdgpu_buffer_rsrc_t rp = make_rsrc(a.part + (size_t)pz * (9 * C * KF), (unsigned)(9 * C * KF * 4));
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = (i & 3) + 8 * (i >> 2) + 4 * hh;
            bstore1(rp, (unsigned)(((tap * C + cm * 32 + m) * KF + kn * 32 + l31) * 4), acc[tap][i]);
        }
}

ModeSwitch x3w_switch{"PNP_X3_WGRAD", 1, 1, true};

int x3w_grid(const pnp_conv_geom* g) {
    const long long ntiles = (long long)g->N * (g->OH / TH) * (g->OW / TW);
    return (int)(ntiles > 256 ? 256 : ntiles);
}
int x3w_parts(const pnp_conv_geom* g) { return x3w_grid(g) * (g->C == 32 ? 2 : 1); }

}  // namespace

namespace pnpconv {

// the one predicate of the workspace query and the launch.  Mode 1 (PNP_X3_DIRECT): layers with at least one tile per CU; both shapes the
// joint step has (32 -> 64 and 64 -> 64 at 256^2) measured faster than the fp32-pipe ring kernel.  Mode 2: wherever the
// shapes allow (tests)
bool x3w_chosen(const pnp_conv_geom* g) {
    const int mode = x3d_route_mode();
    if (mode <= 0 || x3w_switch.get() <= 0 || g->dtype != PNP_DTYPE_F32 || g->pad_mode != PNP_PAD_ZERO) return false;
    if (!(g->R == 3 && g->S == 3 && g->stride == 1 && g->dil == 1 && (g->C == 32 || g->C == 64) && g->K == KF)) return false;
    if (g->OH <= 0 || g->OW <= 0 || (g->OH % TH) != 0 || (g->OW % TW) != 0) return false;
    const long long M = (long long)g->N * g->OH * g->OW;
    if (M * KF >= (1ll << 30) || (long long)g->N * g->H * g->W * g->C >= (1ll << 30)) return false;
    return mode >= 2 || M / (TH * TW) >= 256;
}

size_t x3w_workspace_bytes(const pnp_conv_geom* g) { return (size_t)x3w_parts(g) * 9 * g->C * KF * sizeof(float); }

int launch_x3_wgrad(const float* x, const float* dy, float* dw, const pnp_conv_geom* g, int accumulate, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!x3w_chosen(g)) {
        pnp_set_error("launch_x3_wgrad: layer not on this route");
        return PNP_EINVAL;
    }
    const size_t need = x3w_workspace_bytes(g);
    if (!ws || ws_bytes < need) {
        pnp_set_error("launch_x3_wgrad: workspace too small (%zu < %zu)", ws_bytes, need);
        return PNP_EWORKSPACE;
    }
    X3wArgs a{};
    a.x = x; a.dy = dy; a.part = (float*)ws;
    a.N = g->N; a.H = g->H; a.W = g->W; a.C = g->C; a.OH = g->OH; a.OW = g->OW; a.pad_t = g->pad_t; a.pad_l = g->pad_l;
    a.ntiles = g->N * (g->OH / TH) * (g->OW / TW);
    const dim3 grid((unsigned)x3w_grid(g));
    const double M = (double)g->N * g->OH * g->OW;
    const int nout = 9 * g->C * KF, nparts = x3w_parts(g);
    {
        // flops = the bf16 MFMA flops the kernel EXECUTES (six plane products per fp32 multiply-add): its roof is the dense bf16 peak
        PnpProfScope ps(PNP_PROF_CONV_WGRAD, st, 6.0 * 2.0 * M * nout, 4.0 * ((double)g->N * g->H * g->W * g->C + M * KF + (double)nparts * nout),
                        "conv_x3_wgrad_kernel<%d>", g->C / 32);
        if (g->C == 32) hipLaunchKernelGGL((conv_x3_wgrad_kernel<1>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((conv_x3_wgrad_kernel<2>), grid, dim3(512), 0, st, a);
        PNP_CHECK_LAUNCH("conv_x3_wgrad_kernel");
    }
    // dW (+)= the partials in a fixed order, 16 bytes per lane (nout % 64 == 0, the workspace and dW 16-byte aligned)
    PnpProfScope ps(PNP_PROF_CONV_WGRAD, st, 0.0, 4.0 * ((double)nparts * nout + (accumulate ? 2.0 : 1.0) * nout), "%s", split_sum::Lane<4>::label);
    return split_sum::launch_sliced<4>((const float*)ws, dw, nout, nparts, accumulate, st);
}

}  // namespace pnpconv

// the filter gradients' share of the direct split-bf16 route (PNP_X3_WGRAD): 0 off, 1 on (where pnp_conv2d_x3_direct's mode allows)
extern "C" int32_t pnp_conv2d_x3_wgrad(int32_t mode) { return x3w_switch.set(mode); }
