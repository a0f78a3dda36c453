// pseudo_label.hip — class-balanced self-training on the network's own confident predictions (CBST, Zou et al., ECCV 2018; DESIGN.md
// §29; not in the reference): the loss term of the generator step and the update of its per-class confidence thresholds.
//
//   k_i = argmax_j z_ij (lowest index on ties),  s_i = sum_j exp(z_ij - max),  c_i = 1 / s_i  (the softmax of class k_i: its own
//   exponential is exactly 1).  Pixel i is SELECTED iff class k_i is in the class mask and c_i >= tau[k_i].
//   L = (1/P) sum_selected log s_i  (= -log p_{i,k_i}, from the log-softmax),  dL/dz_ij = (p_ij - [j == k_i]) / P, 0 when not selected
//
//   loss     stream   pixel_loss::stream_kernel<PseudoLabelTerm, ., .>, the streaming pass of the per-pixel skeleton (pixel_loss.h): gradient
//                     and per-block partial of the loss sum as for every term; the class | selected byte and the confidence are the
//                     skeleton's side outputs; thresholds and counters are the term's per-thread state, whose block_end writes the
//                     per-block integer partials of the pixels predicted as / selected as every class
//            final    the term's own second launch: one block adds the loss partials in a fixed order (block_sum.h), one block per
//                     counter adds its integer partials
//   update   init     zero the 4 x [ncls][256] histograms and the per-class selection state
//            hist x 4 per block: LDS histograms of the round's 8-bit digit of the confidence's bit pattern (a positive float orders as
//                     its unsigned integer), one per class, over the pixels whose key shares their class's prefix; integer atomics of
//                     the non-empty bins into the round's global histograms
//            pick x 4 one block per class scans its 256 bins for the digit that holds the rank (pre_pick_kernel of augment.hip walks
//                     them); the first round takes n_k from the bins and turns the portion into a rank, the last one writes q_k and
//                     tau_k <- q_k + beta (tau_k - q_k)
//
// The thresholds are read from device memory by the loss and rewritten in place by the update, so a captured step sees them move.  No
// float atomics: every result is bit-identical from run to run.
#include "pixel_loss.h"

#include <algorithm>
#include <cmath>

namespace {

using pixel_loss::NT;

// ---- the loss ------------------------------------------------------------------------------------------------------------------------

// the term of the per-pixel skeleton (pixel_loss.h), with all three of its options: thresholds and counters per thread, a class byte and
// a confidence per pixel, integer partials per block
struct PseudoLabelTerm {
    static constexpr int NEXTRA = 0;
    static constexpr bool SIDE = true;
    struct Args : pixel_loss::Extra<0> {
        const float* thresholds;      // [ncls], device memory
        uint8_t* labels;              // [P]
        float* conf;                  // [P]
        int* part_cnt;                // [2 ncls][gridDim.x]: every counter's partials are one contiguous list
        uint32_t cmask;
    };

    // tau: the thresholds, in registers; cnt[j]: the pixels this thread saw predicted as class j in the low half, selected as class j in
    // the high half (P < 2^31 over 2 048 x 256 threads at the cap: at most 4 096 pixels a thread, so neither half overflows)
    template <int C>
    struct Lane {
        float tau[C];
        uint32_t cnt[C] = {};
        uint32_t cmask;
        __device__ __forceinline__ Lane(const Args& a, int ncls) : cmask(a.cmask) {
#pragma unroll
            for (int j = 0; j < C; ++j) tau[j] = j < ncls ? a.thresholds[j] : 0.f;
        }
        // the block's counts: a shuffle tree per wave, the four wave sums through LDS.  Integers: any order gives the same number
        __device__ __forceinline__ void block_end(const Args& a, int ncls) {
            __shared__ int wcnt[4][2 * MAXC];
#pragma unroll
            for (int j = 0; j < 2 * C; ++j) {
                int v = j < C ? cnt[j] & 0xffffu : cnt[j - C] >> 16;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
                if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6][j < C ? j : MAXC + j - C] = v;
            }
            __syncthreads();
            if ((int)threadIdx.x < 2 * ncls) {
                const int j = threadIdx.x, l = j < ncls ? j : MAXC + j - ncls;
                a.part_cnt[(long long)j * gridDim.x + blockIdx.x] = (wcnt[0][l] + wcnt[1][l]) + (wcnt[2][l] + wcnt[3][l]);
            }
        }
    };

    // one pixel: z[0..C) -> log s when selected, else 0; lab = k | selected << 7, conf = 1 / s; g[0..C) = gk (p - onehot(k)) or 0 when GRAD
    template <int C, bool GRAD>
    static __device__ __forceinline__ float pixel(const float* z, const float* const*, int ncls, float gk, float* g, Lane<C>& lane, uint32_t& lab,
                                                  float& conf) {
        float e[C], m;
        const float s = pixel_loss::softmax_exp<C>(z, ncls, e, m);
        int k = 0;
#pragma unroll
        for (int j = C - 1; j > 0; --j)
            if (j < ncls && z[j] == m) k = j;
        if (z[0] == m) k = 0;
        conf = 1.0f / s;
        bool sel = false;      // conf >= tau[k] without indexing tau by k: the thresholds stay in registers
#pragma unroll
        for (int j = 0; j < C; ++j) sel |= (j == k) & (conf >= lane.tau[j]);
        sel &= (lane.cmask >> k) & 1u;
        lab = (uint32_t)k | (sel ? 0x80u : 0u);
#pragma unroll
        for (int j = 0; j < C; ++j) lane.cnt[j] += j == k ? (sel ? 0x10001u : 1u) : 0u;
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < C; ++j) g[j] = sel ? gk * (e[j] * conf - (j == k ? 1.f : 0.f)) : 0.f;
        }
        return sel ? logf(s) : 0.f;
    }
};

// 1 + 2 ncls blocks, so that no list waits for another: block 1 + j adds counter j's partials -> counts[j] (counts[0..ncls) = n_k,
// counts[ncls..2 ncls) = m_k); block 0 adds the loss partials through the fixed-order tree in double -> out[0] = L, and all the selected
// counts -> out[1] = the selected share.  The counts are integers: any order of additions gives the same number
__global__ void __launch_bounds__(NT) pl_final_kernel(const float* __restrict__ part, const int* __restrict__ part_cnt, int nblk, int ncls,
                                                      double inv_P, float* __restrict__ out, int32_t* __restrict__ counts) {
    __shared__ double red[NT];
    __shared__ long long wtot[4];
    const int j = (int)blockIdx.x - 1;
    const int* __restrict__ list = part_cnt + (long long)(j < 0 ? ncls : j) * nblk;
    const int len = j < 0 ? ncls * nblk : nblk;
    long long v = 0;
#pragma unroll 4
    for (int i = threadIdx.x; i < len; i += NT) v += list[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = v;
    __syncthreads();
    const long long total = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
    if (j >= 0) {
        if (threadIdx.x == 0) counts[j] = (int32_t)total;
        return;
    }
    const double sum = block_sum_of_list<NT>(part, nblk, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(sum * inv_P);
        out[1] = (float)((double)total * inv_P);
    }
}

struct LossLayout {
    size_t part, cnt, total;
};
LossLayout loss_layout(long long P, int ncls) {
    const size_t nblk = (size_t)pixel_loss::blocks(P);
    LossLayout L;
    L.part = 0;
    L.cnt = nblk * sizeof(float);
    L.total = L.cnt + nblk * 2 * (size_t)(ncls > 0 ? ncls : 0) * sizeof(int);
    return L;
}

// ---- the threshold update --------------------------------------------------------------------------------------------------------------

constexpr int kUpdMaxBlocks = 256;      // one histogram block per CU: zeroing and flushing a block's LDS bins costs more than its share of the pixels

struct SelState {
    uint32_t prefix;    // the key bits fixed by the rounds done so far
    uint32_t k;         // ascending rank of the wanted element among the class's keys that share the prefix
    uint32_t n;         // pixels predicted as the class (set by the first pick)
};

struct UpdLayout {
    size_t hist, state, total;
};
UpdLayout upd_layout() {
    UpdLayout L;
    L.hist = 0;
    L.state = (size_t)4 * MAXC * 256 * sizeof(unsigned int);
    L.total = L.state + MAXC * sizeof(SelState);
    return L;
}

__global__ void __launch_bounds__(NT) pl_init_kernel(unsigned int* __restrict__ hist, SelState* __restrict__ st) {
    for (int i = threadIdx.x; i < 4 * MAXC * 256; i += NT) hist[i] = 0u;
    if (threadIdx.x < MAXC) st[threadIdx.x] = SelState{0u, 0u, 0u};
}

// hist: this round's [MAXC][256].  A confident batch shares its top digits: in the first round almost every key of a class falls into
// one bin, so the lanes that agree with the wave's first lane are counted by one LDS atomic; the others add their own.
__global__ void __launch_bounds__(NT) pl_hist_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ conf, long long n, int ncls,
                                                     int shift, uint32_t mask, const SelState* __restrict__ st, unsigned int* __restrict__ hist) {
    __shared__ unsigned int h[MAXC * 256];
    __shared__ uint32_t pre[MAXC];
    for (int i = threadIdx.x; i < ncls * 256; i += NT) h[i] = 0u;
    if (threadIdx.x < MAXC) pre[threadIdx.x] = st[threadIdx.x].prefix;
    __syncthreads();
    const long long gs = (long long)gridDim.x * NT;
    for (long long base = (long long)blockIdx.x * NT; base < n; base += gs) {      // (block-uniform trip count: the ballot sees whole waves)
        const long long i = base + threadIdx.x;
        int b = -1;
        if (i < n) {
            const int c = labels[i] & 0x7f;
            const uint32_t key = __float_as_uint(conf[i]);
            if (c < ncls && (key & mask) == pre[c]) b = c * 256 + (int)((key >> shift) & 255u);
        }
        const int b0 = __shfl(b, 0, 64);
        const unsigned long long peers = __ballot(b == b0);
        if (b == b0) {
            if ((threadIdx.x & 63) == 0 && b0 >= 0) atomicAdd(&h[b0], (unsigned int)__popcll(peers));
        } else if (b >= 0) {
            atomicAdd(&h[b], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ncls * 256; i += NT) {
        const unsigned int c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// block c < ncls, thread b = bin b of the class's histogram: an inclusive scan over the 256 bins (shuffles per wave, the four wave totals
// through LDS) finds the digit whose bin holds the rank, as the walk of pre_pick_kernel (augment.hip) does serially.  FIRST takes n_c from
// the total and sets the ascending rank n_c - ceil(portion n_c) of the r-th largest; every round fixes one digit; LAST writes q_c and
// the threshold.  A class without pixels keeps its threshold, q_c = NaN
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) pl_pick_kernel(const unsigned int* __restrict__ hist, int shift, double portion, float beta,
                                                      SelState* __restrict__ st, float* __restrict__ thresholds, float* __restrict__ q_out) {
    __shared__ uint32_t wsum[4];
    const int c = blockIdx.x, b = threadIdx.x, lane = b & 63, wave = b >> 6;
    const uint32_t cnt = hist[c * 256 + b];
    SelState s = st[c];      // (every thread reads the state before the barrier, the one that rewrites it does so behind it)
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) incl += wsum[w];
        total += wsum[w];
    }
    if (FIRST) {
        long long r = (long long)ceil(portion * (double)total);
        r = r < 1 ? 1 : (r > (long long)total ? (long long)total : r);
        s.n = total;
        s.k = total ? total - (uint32_t)r : 0u;
    }
    // the one bin with excl <= k < incl (k < total whenever the class has pixels); a class without pixels: thread 0 passes the state on
    const bool mine = s.n ? (cnt > 0u && incl - cnt <= s.k && s.k < incl) : b == 0;
    if (!mine) return;
    if (s.n) {
        s.prefix |= (uint32_t)b << shift;
        s.k -= incl - cnt;
    }
    st[c] = s;
    if (LAST) {
        const float q = s.n ? __uint_as_float(s.prefix) : __uint_as_float(0x7fc00000u);
        if (s.n && beta != 1.f) {      // (beta == 1 keeps the bits: q + (tau - q) rounds twice)
            const float t = thresholds[c];
            thresholds[c] = fmaf(beta, t - q, q);
        }
        if (q_out) q_out[c] = q;
    }
}

template <bool FIRST, bool LAST>
void launch_pick(const unsigned int* hist, int ncls, int shift, double portion, float beta, SelState* st, float* thresholds, float* q_out,
                 hipStream_t stream) {
    hipLaunchKernelGGL((pl_pick_kernel<FIRST, LAST>), dim3(ncls), dim3(256), 0, stream, hist, shift, portion, beta, st, thresholds, q_out);
}

}  // namespace

extern "C" {

size_t pnp_pseudo_label_loss_workspace_bytes(int64_t P, int32_t ncls) { return loss_layout((long long)P, ncls).total; }

int pnp_pseudo_label_loss(const float* logits, const float* thresholds, int64_t P, int32_t ncls, uint32_t class_mask, float coef,
                          float* dlogits, uint8_t* labels, float* conf, float* out, int32_t* counts, void* workspace, size_t workspace_bytes,
                          void* stream) {
    const char* who = "pnp_pseudo_label_loss";
    PNP_REQUIRE(logits && thresholds && labels && conf && out && counts && workspace && P > 0 && ncls > 0, "%s: bad argument", who);
    PNP_REQUIRE(ncls <= MAXC, "%s: ncls = %d, at most %d classes are served", who, (int)ncls, MAXC);
    PNP_REQUIRE(P < (1ll << 31), "%s: P = %lld is not below 2^31 (the counts are int32)", who, (long long)P);
    const LossLayout L = loss_layout((long long)P, ncls);
    PNP_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = pixel_loss::blocks((long long)P);
    float* part = (float*)((char*)workspace + L.part);
    int* part_cnt = (int*)((char*)workspace + L.cnt);
    const float gk = (float)((double)coef / (double)P);
    const PseudoLabelTerm::Args args{{}, thresholds, labels, conf, part_cnt, class_mask};
    if (const int rc = pixel_loss::run_stream<PseudoLabelTerm>(who, logits, args, (long long)P, ncls, gk, dlogits, part, st)) return rc;
    hipLaunchKernelGGL(pl_final_kernel, dim3(1 + 2 * ncls), dim3(NT), 0, st, (const float*)part, (const int*)part_cnt, nblk, (int)ncls, 1.0 / (double)P,
                       out, counts);
    return pixel_loss::launch_failed(who, "pl_final_kernel") ? PNP_ELAUNCH : PNP_OK;
}

size_t pnp_pseudo_label_update_workspace_bytes(int64_t P, int32_t ncls) {
    (void)P, (void)ncls;
    return upd_layout().total;
}

int pnp_pseudo_label_update(const uint8_t* labels, const float* conf, int64_t P, int32_t ncls, double portion, float momentum,
                            float* thresholds, float* q_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pnp_pseudo_label_update";
    PNP_REQUIRE(labels && conf && thresholds && workspace && P > 0 && ncls > 0, "%s: bad argument", who);
    PNP_REQUIRE(ncls <= MAXC, "%s: ncls = %d, at most %d classes are served", who, (int)ncls, MAXC);
    PNP_REQUIRE(P < (1ll << 31), "%s: P = %lld is not below 2^31", who, (long long)P);
    PNP_REQUIRE(portion > 0.0 && portion <= 1.0, "%s: portion %g outside (0, 1]", who, portion);
    PNP_REQUIRE(momentum >= 0.f && momentum <= 1.f, "%s: momentum %g outside [0, 1]", who, (double)momentum);
    const UpdLayout L = upd_layout();
    PNP_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    unsigned int* hist = (unsigned int*)((char*)workspace + L.hist);
    SelState* state = (SelState*)((char*)workspace + L.state);
    const unsigned nb = (unsigned)std::min<long long>(((long long)P + NT - 1) / NT, kUpdMaxBlocks);

    hipLaunchKernelGGL(pl_init_kernel, dim3(1), dim3(NT), 0, st, hist, state);
    if (pixel_loss::launch_failed(who, "pl_init_kernel")) return PNP_ELAUNCH;
    uint32_t mask = 0u;
    for (int r = 0; r < 4; ++r) {
        const int shift = 24 - 8 * r;
        unsigned int* hr = hist + r * MAXC * 256;
        hipLaunchKernelGGL(pl_hist_kernel, dim3(nb), dim3(NT), 0, st, labels, conf, (long long)P, (int)ncls, shift, mask, state, hr);
        if (pixel_loss::launch_failed(who, "pl_hist_kernel")) return PNP_ELAUNCH;
        if (r == 0)
            launch_pick<true, false>(hr, ncls, shift, portion, momentum, state, thresholds, q_out, st);
        else if (r == 3)
            launch_pick<false, true>(hr, ncls, shift, portion, momentum, state, thresholds, q_out, st);
        else
            launch_pick<false, false>(hr, ncls, shift, portion, momentum, state, thresholds, q_out, st);
        if (pixel_loss::launch_failed(who, "pl_pick_kernel")) return PNP_ELAUNCH;
        mask |= 255u << shift;
    }
    return PNP_OK;
}

}  // extern "C"
