// conv_mma.h — the register-pipelined fragment set and the slice schedule macros of the fp32 MFMA main loops
// (conv_igemm.hip: convolutions; conv_wino.hip: the batched GEMM of the Winograd path).
#pragma once
#include "conv_common.h"

namespace pnpconv {

// ---- register-pipelined fragments: one 8-k slice (kq) of a stage ---------------------------------
// The main loops keep two Frag sets: while the 4*TM*TN MFMAs of slice kq run, the ds_reads of slice kq+1 are in
// flight, the global loads of the next stage are issued (slice 0) and stored to the other LDS buffer (slice 3).
// The only LDS latency a wave exposes per stage is the first slice's reads right after the barrier.
template <int TM, int TN, bool A_MMAJOR, int LDA, int LDB>
struct Frag {
    f32x4 a[TM];
    float b[4][TN];
    __device__ __forceinline__ void load(const float* __restrict__ As, const float* __restrict__ Bs, int kq, int wm0, int wn0,
                                         int lane) {
        const int l31 = lane & 31;
        const int kb = kq * 8 + 4 * (lane >> 5);
        if constexpr (A_MMAJOR) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) a[tm] = *reinterpret_cast<const f32x4*>(As + (wm0 + tm * 32 + l31) * LDA + kb);
        } else {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[tm][j] = As[(kb + j) * LDA + wm0 + tm * 32 + l31];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) b[j][tn] = Bs[(kb + j) * LDB + wn0 + tn * 32 + l31];
    }
    __device__ __forceinline__ void mma(Acc<TM, TN>& acc) const {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc.v[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][j], b[j][tn], acc.v[tm][tn], 0, 0, 0);
    }
};
}  // namespace pnpconv

#define PNP_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// Slices 1..3 of a stage (two Frag sets: the fragment reads of the NEXT slice and the MFMAs of THIS slice are independent).  A slice is its
// fragment reads, then its MFMAs; the next stage's LDS stores go behind the second half of the LAST slice's MFMAs.  Measured A/B/A/B on the
// 512-channel layers at B=16 against stores after the last slice (round 1): 512->512 forward +2.4 %, g10 forward +3.2 % / wgrad +4.6 %,
// segmenter step 422 -> 434 slices/s, joint GAN step 147.4 -> 151.1 — the stores (and the vmcnt wait in front of them) left the exposed
// chain [last MFMA -> stores -> barrier -> first fragment reads -> first MFMA] that the co-resident workgroup has to cover.  Fragment reads
// interleaved behind single MFMAs, stores behind the first half of the last slice or behind slice 2 were no better (tools/experiments/).
#define PNP_SLICE(LOAD, MMA) \
    {                        \
        LOAD;                \
        PNP_SCHED_FENCE();   \
        MMA;                 \
        PNP_SCHED_FENCE();   \
    }
#define PNP_LAST_SLICE(MMA, STORE, NMFMA)                                \
    {                                                                    \
        MMA;                                                             \
        STORE;                                                           \
        __builtin_amdgcn_sched_group_barrier(0x008, (NMFMA) / 2, 0);     \
        _Pragma("unroll") for (int i_ = 0; i_ < (NMFMA) / 2; ++i_) {     \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);           \
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);           \
        }                                                                \
        PNP_SCHED_FENCE();                                               \
    }
// One whole stage of the two-buffer, four-slice pipeline, barrier included (conv_igemm.hip: conv_taps_kernel, conv_wgrad_kernel,
// conv_wgrad_ring_kernel; conv_wino.hip: wino_gemm_kernel, wino_wgrad_gemm_kernel).  It names the caller's locals: Frag sets f0 / f1 (f0
// holds slice 0 on entry), acc, this stage's LDS tiles As / Bs, wm0 / wn0 / lane.  FETCH issues the next stage's global loads, STORE writes
// them to the other LDS buffer.  Slice 0 puts the slice-1 fragment reads first (NDS0 ds_reads), then per MFMA (NMFMA of them) NVALU
// address VALU / SALU instructions and one buffer_load, so that the next stage's address arithmetic rides in the MFMAs' shadow.  The two
// counts follow the kernel's fetch and A layout: NVALU is the address work per load — 4 for tap-unrolled or precomputed scalar-offset rows
// (taps, wino_gemm), 6 for wino_wgrad_gemm's row test, 12 for the filter gradients' per-row pixel walk / divisions; NDS0 covers one
// slice's fragments — TM + 4*TN <= 10 reads for an M-major A tile (8 passed), 4*TM + 4*TN <= 16 for a k-major one (16, or the ring
// kernel's exact count).  conv_fwd_body keeps a stage of its own: its stores come after ALL MFMAs of the last slice, a different schedule.
#define PNP_MMA_STAGE(NVALU, NDS0, NMFMA, FETCH, STORE)                               \
    {                                                                                 \
        f1.load(As, Bs, 1, wm0, wn0, lane);                                           \
        FETCH;                                                                        \
        f0.mma(acc);                                                                  \
        __builtin_amdgcn_sched_group_barrier(0x100, (NDS0), 0);                       \
        _Pragma("unroll") for (int i_ = 0; i_ < (NMFMA); ++i_) {                      \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        \
            __builtin_amdgcn_sched_group_barrier(0x006, (NVALU), 0);                  \
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                        \
        }                                                                             \
        PNP_SCHED_FENCE();                                                            \
        PNP_SLICE(f0.load(As, Bs, 2, wm0, wn0, lane), f1.mma(acc))                    \
        PNP_SLICE(f1.load(As, Bs, 3, wm0, wn0, lane), f0.mma(acc))                    \
        PNP_LAST_SLICE(f1.mma(acc), STORE, NMFMA)                                     \
        __syncthreads();                                                              \
    }
