/*
 * pnp_hip.h — C-ABI of libpnp_hip.so: the MI355X (gfx950) kernels behind the PnP-AdaNet
 * training hot path (dilated-residual segmenter fwd/bwd + Wasserstein critics).
 *
 * The reference (carrenD/Medical-Cross-Modality-Domain-Adaptation) has NO FFI of its own: every op is
 * a TensorFlow-1.4 graph op created in layers.py / ops.py / source_segmenter.py / adversarial.py.
 * Each entry point below therefore names the reference call site whose TF op it replaces
 * (file:line into /root/reference).  The Python host side binds these with ctypes
 * (see INTEGRATION.md); nothing in the signatures is a torch type.
 *
 * Conventions
 *   - tensors: dense float32, activations NHWC, filters HWIO (exactly the reference layout)
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated inside;
 *     scratch comes from a caller-provided workspace (size from pnp_*_workspace_bytes)
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous w.r.t. the host
 *   - return 0 on success, <0 on error (PNP_E*), message via pnp_last_error(); never throws
 */
#ifndef PNP_HIP_H
#define PNP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNP_OK 0
#define PNP_EINVAL (-1)   /* bad argument / unsupported geometry */
#define PNP_ELAUNCH (-2)  /* hip launch error */
#define PNP_EWORKSPACE (-3) /* workspace too small */
#define PNP_ECOMM (-4)    /* RCCL missing or an RCCL call failed */

/* element types named at the ABI (convolution operand storage, collectives) */
#define PNP_DTYPE_F32 0
#define PNP_DTYPE_BF16 1
#define PNP_DTYPE_F64 2

#define PNP_PAD_ZERO 0      /* tf.nn.conv2d(padding='SAME') zero padding, layers.py:18,67 */
#define PNP_PAD_SYMMETRIC 1 /* tf.pad(x, k//2, 'SYMMETRIC') + VALID conv, layers.py:19-24,68-73 */

int pnp_abi_version(void);
const char* pnp_last_error(void);
/* cu_count, max clock (kHz), LDS bytes per CU, gcn arch name (<=63 chars) of `device` */
int pnp_device_info(int device, int* cu_count, int* clock_khz, int* lds_bytes, char* arch, int arch_len);

/* Kernel-level timing for the roofline figures of bench.py: while a class is enabled, the library records HIP events on the
 * launch stream around every launch of that class's main kernel (not around its helper kernels: filter flips, partial sums).
 * pnp_prof_summary waits for the events, returns one row per kernel symbol (named as rocprofv3 --kernel-trace prints it) with the
 * launch count, the summed duration and the summed ALGORITHMIC flops / bytes (2*N*OH*OW*R*S*C*K; 4*(|x|+|y|+|w|)), and clears
 * the records.  Returns the number of distinct symbols (may exceed max_rows; only max_rows are written). */
#define PNP_PROF_CONV_FWD 1   /* MFMA forward convolutions */
#define PNP_PROF_CONV_DGRAD 2 /* MFMA data gradients */
#define PNP_PROF_CONV_WGRAD 4 /* MFMA filter gradients */
#define PNP_PROF_CONV_DIRECT 8 /* vector-ALU convolutions for K <= 16 */
typedef struct pnp_prof_row {
    char name[128];
    int64_t launches;
    double ms, flops, bytes;
} pnp_prof_row;
int pnp_prof_enable(int32_t mask);
int pnp_prof_summary(pnp_prof_row* rows, int32_t max_rows);

/* Geometry shared by the three conv entry points (all describe the FORWARD convolution):
 *   x [N,H,W,C]  w [R,S,C,K]  y [N,OH,OW,K]
 *   y[n,oh,ow,k] = sum_{r,s,c} xpad[n, oh*stride - pad_t + r*dil, ow*stride - pad_l + s*dil, c] * w[r,s,c,k]
 *   pad_mode PNP_PAD_ZERO: out-of-range taps read 0 (TF SAME; pad_t/pad_l = the TF "pad before" amounts)
 *   pad_mode PNP_PAD_SYMMETRIC: out-of-range taps mirror including the edge (tf.pad SYMMETRIC), pad_t=pad_l=k//2
 * Dropout (tf.nn.dropout, layers.py:25,74,93) is fused in the forward epilogue:
 *   y *= mask(seed, stream_id, flat_index) / keep_prob    (keep_prob >= 1 disables it)
 * mask is the counter-hash stream documented at pnp_dropout (below). */
typedef struct pnp_conv_geom {
    int32_t N, H, W, C;     /* input */
    int32_t K, R, S;        /* filter count and size */
    int32_t OH, OW;         /* output spatial size */
    int32_t stride, dil;    /* same in both spatial dims (reference only uses square) */
    int32_t pad_t, pad_l;   /* pad before (top / left) */
    int32_t pad_mode;       /* PNP_PAD_* */
    int32_t dtype;          /* PNP_DTYPE_F32: the reference's arithmetic.  PNP_DTYPE_BF16 (BASELINE configs[4]): both operands of the
                             * contraction are rounded to bfloat16 (nearest-even) as they are staged, products accumulate in fp32;
                             * x / w / y / gradients stay float32 in memory (w = the fp32 master weights).  Layers off the MFMA fast
                             * paths (C not a multiple of 32, K <= 16, strided filter gradients) compute in fp32 either way. */
} pnp_conv_geom;

/* replaces tf.nn.conv2d (layers.py:18,24,67,73) and tf.nn.atrous_conv2d (layers.py:86,92) + tf.nn.dropout */
int pnp_conv2d_fwd(const float* x, const float* w, float* y, const pnp_conv_geom* g,
                   float keep_prob, uint64_t seed, uint32_t stream_id, void* stream);
/* Same with a workspace: layers with few output pixels (the critics' 4x4 / 2x2 maps, small batches) leave most of the 256 CUs
 * without a tile; given pnp_conv2d_fwd_workspace_bytes(g) bytes the reduction over R*S*C is split across workgroups and the
 * partial sums (fixed order: deterministic) pass through the workspace; dropout is then applied by the summing kernel.
 * workspace may be NULL / 0 bytes (== pnp_conv2d_fwd). */
size_t pnp_conv2d_fwd_workspace_bytes(const pnp_conv_geom* g);
int pnp_conv2d_fwd_ws(const float* x, const float* w, float* y, const pnp_conv_geom* g,
                      float keep_prob, uint64_t seed, uint32_t stream_id,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Training-mode conv -> dropout -> batch norm: the forward convolution leaves per-(pixel tile, wave row) partial sums of (y - shift[k])
 * and (y - shift[k])^2 over its output rows, so that the batch statistics cost no second pass over the activation
 * (pnp_bn_stats_finish combines them in double).  shift [K] (nullable = 0): any per-channel constant near the mean, e.g. the moving
 * mean — it only conditions the variance.  pnp_conv2d_fwd_stats_parts(g) = number of partial rows, 0 when this geometry's forward
 * cannot provide them (vector-ALU narrow-output kernels, reduction-split tiny layers): run pnp_bn_stats on the output instead.
 * parts: [parts][2][K] floats. */
int32_t pnp_conv2d_fwd_stats_parts(const pnp_conv_geom* g);
int pnp_conv2d_fwd_stats(const float* x, const float* w, float* y, const pnp_conv_geom* g,
                         float keep_prob, uint64_t seed, uint32_t stream_id,
                         const float* shift /*nullable*/, float* parts, size_t parts_bytes, void* stream);
/* The same with a workspace of pnp_conv2d_fwd_workspace_bytes(g) bytes.  Wide stride-1 3x3 layers (the segmenter's 256- / 512-channel
 * groups, source_segmenter.py:140-200) may be given to the Winograd F(2x2, 3x3) route (csrc/conv_wino.hip: 2.25x fewer multiplications,
 * transformed tensors through the workspace; same result up to fp32 rounding, ~1e-6 relative); its partial rows are the tile slabs of its
 * output transform, so the count comes from pnp_conv2d_fwd_stats_ws_parts(g).  Every other layer: identical to pnp_conv2d_fwd_stats.
 * pnp_conv2d_wino_chosen(g, kind) tells which route a layer takes (kind 0: forward; 1: data gradient; 2: filter gradient — g = the FORWARD geometry);
 * environment PNP_WINOGRAD = 0 never / 1 where the cost model says it pays / 2 wherever the geometry allows. */
int32_t pnp_conv2d_fwd_stats_ws_parts(const pnp_conv_geom* g);
int pnp_conv2d_fwd_stats_ws(const float* x, const float* w, float* y, const pnp_conv_geom* g,
                            float keep_prob, uint64_t seed, uint32_t stream_id,
                            const float* shift /*nullable*/, float* parts, size_t parts_bytes,
                            void* workspace, size_t workspace_bytes, void* stream);
int32_t pnp_conv2d_wino_chosen(const pnp_conv_geom* g, int32_t kind);   /* 0: direct kernels; else the route's output tile edge (2 or 4) */
/* Which kernel family serves a layer, given the workspace its query asks for (kind 0: forward with the plain epilogue; 1: data gradient;
 * 2: filter gradient — g = the FORWARD geometry): the first candidate of the plan the entry points launch from (csrc/conv_igemm.hip:
 * plan_fwd / plan_dgrad / plan_wgrad).  pnp_conv2d_wino_chosen stays the Winograd planner's tile, which also sizes the workspace of the
 * narrow layers that PNP_ROUTE_X3D then runs.  -1: bad geometry. */
#define PNP_ROUTE_IGEMM 0        /* implicit-GEMM MFMA tiles (forward; data gradient as a convolution of dy, zero-upsampled when strided) */
#define PNP_ROUTE_N16 1          /* 16-filter 16x16x4-MFMA kernels (conv_small.hip) */
#define PNP_ROUTE_NARROW 2       /* narrow-output vector-ALU kernel */
#define PNP_ROUTE_WINO 3         /* Winograd F(2x2) / F(4x4) (conv_wino.hip) */
#define PNP_ROUTE_X3D 4          /* direct split-bf16, stride 1 (conv_x3_direct.hip) */
#define PNP_ROUTE_X3S 5          /* direct split-bf16, strided */
#define PNP_ROUTE_PHASES 6       /* strided data gradient on the fp32 stride-phase kernels */
#define PNP_ROUTE_WINO_WGRAD 7   /* filter gradient: Winograd */
#define PNP_ROUTE_X3W 8          /* filter gradient: direct split-bf16 (conv_x3_wgrad.hip) */
#define PNP_ROUTE_N16_WGRAD 9    /* filter gradient: 16x16x4-MFMA kernel */
#define PNP_ROUTE_WGD 10         /* filter gradient: vector-ALU kernel */
#define PNP_ROUTE_RING 11        /* filter gradient: MFMA ring kernel */
#define PNP_ROUTE_X3N 12         /* direct split-bf16, the 5x5 40 -> 5 logits layer: forward and data gradient (conv_x3_narrow.hip) */
int32_t pnp_conv2d_route(const pnp_conv_geom* g, int32_t kind);
/* sets the route policy at run time (0 / 1 / 2 as PNP_WINOGRAD; < 0: read only) and returns the previous one */
int32_t pnp_conv2d_wino_mode(int32_t mode);
/* Round 5: the route has two output tiles.  F(4x4, 3x3) — 36 multiplications per 4x4 output tile instead of the direct sum's 144
 * (F(2x2): 64), transformed tensors 2.25x the activations (F(2x2): 4x) — on the interpolation points (0, 1, -1, 1/2, -2, inf), whose
 * float32 error against the float64 convolution is the direct kernel's (3e-6..5e-6 of max|y| on the 256- / 512-channel layers;
 * profiles/r05_wino_f43_tolerance.txt).  tile = 2: F(2x2) only; 4 (the default, environment PNP_WINOGRAD_TILE): F(4x4) where its planner
 * takes the layer, else F(2x2), else the direct kernels; tile < 2: read only.  Returns the previous value. */
int32_t pnp_conv2d_wino_tile(int32_t tile);
/* Round 6: arithmetic of the route's forward / data-gradient GEMMs.  0: the fp32 matrix pipe (v_mfma_f32_32x32x2_f32).  1 (the default,
 * environment PNP_WINOGRAD_X3) where it pays (reductions over >= 256 channels), 2 wherever the shapes allow (C % 64 == 0): split-bf16 operands — every transformed value is stored as three bf16 planes whose sum IS the fp32 value, six of the
 * nine plane products (all terms above 2^-26 of the product) run on v_mfma_f32_32x32x16_bf16 (16x the fp32 pipe's rate) with fp32
 * accumulation in 64-channel chunks (csrc/conv_wino_x3.hip; tools/wino_bf16x3_study.py -> profiles/r06_wino_bf16x3_tolerance.txt: the
 * whole layer's error against float64 falls from 4e-6..6e-6 to 1e-6..2e-6, because the chunked chain is shorter than the fp32 pipe's).
 * mode < 0: read only.  Returns the previous mode.  Workspace queries and the transformed-filter cache follow the mode in force. */
int32_t pnp_conv2d_wino_x3(int32_t mode);
/* Round 6: the narrow layers of the route (3x3, stride 1, 32 or 64 input channels, 64 or 128 filters, output a multiple of 16 x 16) as DIRECT
 * split-bf16 convolutions (csrc/conv_x3_direct.hip): no transforms — a tile's halo patch is split into three bf16 planes once and the nine
 * taps are LDS offsets; six plane products per fragment pair on v_mfma_f32_32x32x16_bf16, one fp32 chain of 9 C terms (8e-7 of max|ref|).
 * Replaces, for those layers, the F(4x4) route that is bound by its 2.25x transformed tensors there (reference adversarial.py:337-366, the
 * critics' 64-channel blocks at 256^2 / 128^2).  0: off, 1 (default): where a launch fills the chip (>= 256 tile x filter-block items), 2: wherever the
 * shapes allow (environment PNP_X3_DIRECT); mode < 0: read only.  Returns the previous mode. */
int32_t pnp_conv2d_x3_direct(int32_t mode);
/* The strided layers on the same kernels (stride 2..4, zero padding, dilation 1, C % 32 == 0 input and K % 64 == 0 output channels of the
 * computed convolution, every output or stride-phase grid a multiple of 16 x 16, sub-filters of at most 3 x 3): the forward as a sum of
 * stride-1 convolutions over the input's stride phases, the data gradient as all output stride phases in one persistent launch.  Taken under
 * pnp_conv2d_x3_direct's mode (1: >= 256 items) while this switch is 1 (default; environment PNP_X3_STRIDED); 0: off.  Returns the previous value. */
int32_t pnp_conv2d_x3_strided(int32_t mode);
/* The FILTER GRADIENT of the stride-1 layers on the same arithmetic (csrc/conv_x3_wgrad.hip: 3x3, dilation 1, zero padding, fp32 geometry, 32
 * or 64 input channels, 64 filters, output a multiple of 16 x 16): x patches and dy tiles split into three bf16 planes in the loaders,
 * transposed on the way out of LDS, six plane products per fragment pair, the whole [9][C][64] gradient in registers for the launch; one
 * partial sum per persistent workgroup (two with 32 channels) through pnp_conv2d_wgrad_workspace_bytes(g) of workspace, summed in a fixed
 * order (deterministic; pnp_conv2d_wgrad_acc adds into dw there).  Asked after the Winograd filter-gradient planner, before the fp32-pipe
 * kernels.  Taken under pnp_conv2d_x3_direct's mode (1: >= 256 tiles) while this switch is 1 (default; environment PNP_X3_WGRAD); 0: off.
 * Returns the previous value (mode < 0: read only). */
int32_t pnp_conv2d_x3_wgrad(int32_t mode);
/* The segmenter head's logits layer on the same arithmetic (csrc/conv_x3_narrow.hip: 5x5, stride 1, dilation 1, 40 -> 5 channels, fp32
 * geometry, zero or no padding), forward (output a multiple of 8 x 16; dropout as the vector-ALU kernel's, same masks) and data gradient
 * (any extent; honours the residual of pnp_conv2d_dgrad_add): the 5-channel side is the 16-row operand of v_mfma_f32_16x16x32_bf16, the
 * taps are LDS offsets of one split patch, the split filter image goes through pnp_conv2d_{fwd,dgrad}_workspace_bytes(g) of workspace.
 * Route PNP_ROUTE_X3N.  0: off, 1 (default; environment PNP_X3_NARROW): where a launch fills the chip (>= 256 tiles) and the direction
 * measured faster at B = 16, 2: wherever the shapes allow; pnp_conv2d_x3_direct(0) turns it off as well.  Frozen-BN forwards, bf16
 * geometries and the filter gradient keep their kernels.  Returns the previous mode (mode < 0: read only). */
int32_t pnp_conv2d_x3_narrow(int32_t mode);
/* Transformed-filter cache of the route.  U = G g G^T (36 C K values per filter and pass: fp32, or three bf16 planes) only changes when the filter does: the caller
 * lends one buffer per (filter, pass) and reports weight writes; a launch whose filter has a valid entry skips wino_filter_kernel (the
 * frozen source segmenter / shared half of adversarial.py:839-882 never pay it again, a trained layer once per update instead of once per
 * pass).  pnp_conv2d_wino_filter_bytes(C, K): size of an entry that serves either tile (0: this shape never takes the route).
 * pnp_conv2d_wino_filter_bind(w, kind, U, bytes): kind 0 forward / 1 data gradient; U = null withdraws the entry, w = null all of them;
 * the buffer must outlive the binding.  pnp_weights_changed(lo, hi): the floats in [lo, hi) were (or are queued to be) written —
 * entries of filters inside are stale; lo = null: every entry.  Launches recorded into a hipGraph never touch the cache.
 * pnp_conv2d_wino_filter_stats: transforms skipped / run into an entry since the last reset. */
size_t pnp_conv2d_wino_filter_bytes(int32_t C, int32_t K);
int pnp_conv2d_wino_filter_bind(const float* w, int32_t kind, float* U, size_t bytes);
void pnp_weights_changed(const void* lo, const void* hi);
void pnp_conv2d_wino_filter_stats(int64_t* hits, int64_t* fills, int32_t reset);
/* the filter gradient (pnp_conv2d_wgrad / _wgrad_acc, given pnp_conv2d_wgrad_workspace_bytes) has its own switch (PNP_WINOGRAD_WGRAD,
 * same values); pnp_conv2d_wino_chosen(g, 2) tells its route */
int32_t pnp_conv2d_wino_wgrad_mode(int32_t mode);

/* Inference-mode conv -> dropout -> batch norm -> (+ shortcut) -> leaky-ReLU in ONE kernel (the monitoring forwards of
 * source_segmenter.py:525-570 / adversarial.py:948-991, every frozen-BN forward of the GAN steps, Trainer.test_eval):
 *   y = act( drop(conv(x,w)) * scale[k] + shift[k] + pad_channels(shortcut) ),  scale / shift from pnp_bn_fold.
 * shortcut [N*OH*OW, Cs] is zero-padded (K-Cs)/2 channels on each side (layers.py:159-165); alpha < 0: no activation. */
int pnp_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float* scale, float* shift,
                int32_t C, float eps, void* stream);
int pnp_conv2d_fwd_bn(const float* x, const float* w, float* y, const pnp_conv_geom* g,
                      float keep_prob, uint64_t seed, uint32_t stream_id,
                      const float* scale, const float* shift, const float* shortcut /*nullable*/, int32_t Cs, float alpha,
                      void* stream);
/* the same with a workspace of pnp_conv2d_fwd_workspace_bytes(g) bytes (nullable / too small: == pnp_conv2d_fwd_bn): the layers the
 * planner gives to the Winograd route take it, epilogue included */
int pnp_conv2d_fwd_bn_ws(const float* x, const float* w, float* y, const pnp_conv_geom* g,
                         float keep_prob, uint64_t seed, uint32_t stream_id,
                         const float* scale, const float* shift, const float* shortcut /*nullable*/, int32_t Cs, float alpha,
                         void* workspace, size_t workspace_bytes, void* stream);

/* gradient w.r.t. the conv input (TF autodiff of the ops above; Conv2DBackpropInput).
 * dy is the gradient w.r.t. the conv accumulator (i.e. AFTER the dropout mask has been applied by the caller).
 * workspace: pnp_conv2d_dgrad_workspace_bytes(g). */
size_t pnp_conv2d_dgrad_workspace_bytes(const pnp_conv_geom* g);
int pnp_conv2d_dgrad(const float* dy, const float* w, float* dx, const pnp_conv_geom* g,
                     void* workspace, size_t workspace_bytes, void* stream);
/* dx = data gradient + residual (residual [N,H,W,C], not aliasing dx): the gradient that reaches the conv input a second way — the
 * shortcut of layers.residual_block / DR_block (layers.py:145-189), where TF's autodiff emits an AddN.  Added in the epilogue of the
 * stride-1 MFMA kernels; other geometries add it with one more pass. */
int pnp_conv2d_dgrad_add(const float* dy, const float* w, const float* residual, float* dx, const pnp_conv_geom* g,
                         void* workspace, size_t workspace_bytes, void* stream);

/* gradient w.r.t. the filter (Conv2DBackpropFilter). dw [R,S,C,K] is overwritten. */
size_t pnp_conv2d_wgrad_workspace_bytes(const pnp_conv_geom* g);
int pnp_conv2d_wgrad(const float* x, const float* dy, float* dw, const pnp_conv_geom* g,
                     void* workspace, size_t workspace_bytes, void* stream);
/* dw += filter gradient: written straight into a gradient buffer that may already hold a contribution (filters shared by two
 * passes, adversarial.py:196,235; TF's AddN of the per-use gradients) — no separate accumulation kernel */
int pnp_conv2d_wgrad_acc(const float* x, const float* dy, float* dw, const pnp_conv_geom* g,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Naive one-thread-per-output direct convolution (fp32 fmaf chain in r,s,c order). On-device
 * cross-check for the MFMA kernels at sizes the CPU oracle cannot reach; not used by the product path. */
int pnp_conv2d_fwd_naive(const float* x, const float* w, float* y, const pnp_conv_geom* g, void* stream);

/* tf.nn.dropout (layers.py:25,74,93): y = x * keep_mask / keep.  TF's own RNG stream is not reproducible outside TF, so the
 * mask stream is specified here (csrc/pnp_common.h; restated in numpy in oracle/tf_ops.py):
 *   keep_mask(idx) = (fmix32((idx * 0xCC9E2D51) ^ key(seed, stream_id)) >> 8) >= round((1 - keep) * 2^24)
 * with fmix32 = the murmur3 finaliser and idx the flat element index.  Also used for the backward of the fused epilogue. */
int pnp_dropout(const float* x, float* y, size_t n, float keep_prob, uint64_t seed, uint32_t stream_id, void* stream);

/* tf.contrib.layers.batch_norm(decay=.9, eps=1e-3, updates_collections=None) (layers.py:95-100), fused batch-norm semantics.
 * x,y: [P,C] (P = N*H*W).  stats: mean[C], var[C] (biased).  ws: pnp_bn_workspace_bytes(P,C). */
size_t pnp_bn_workspace_bytes(int64_t P, int32_t C);
int pnp_bn_stats(const float* x, float* mean, float* var, int64_t P, int32_t C,
                 void* workspace, size_t workspace_bytes, void* stream);
/* pnp_bn_stats + pnp_bn_update_moving in one pass (the per-replica training-mode forward: one launch less per BN layer) */
int pnp_bn_stats_update(const float* x, float* mean, float* var, float* moving_mean, float* moving_var, int64_t P, int32_t C,
                        float decay, void* workspace, size_t workspace_bytes, void* stream);
/* mean / biased variance from the partials of pnp_conv2d_fwd_stats (same shift), optionally followed by the moving-average update
 * (moving_mean / moving_var nullable together; shift may alias moving_mean).  `parts` is CONSUMED: long lists (>= 512 partials) are
 * first compacted in place by many workgroups (double sums written back as float high/low pairs), then combined. */
int pnp_bn_stats_finish(float* parts, int32_t nparts, const float* shift, float* mean, float* var,
                        float* moving_mean, float* moving_var, int64_t P, int32_t C, float decay, void* stream);
/* moving_mean -= (1-decay)*(moving_mean-mean); moving_var likewise with var*P/(P-1) (Bessel) */
int pnp_bn_update_moving(float* moving_mean, float* moving_var, const float* mean, const float* var,
                         int64_t P, int32_t C, float decay, void* stream);
/* y = act( gamma*(x-mean)*rsqrt(var+eps) + beta + shortcut_padded ), act = leaky-ReLU(alpha) if alpha>=0 else identity.
 * shortcut (optional, may be NULL) has Cs channels, zero-padded (C-Cs)/2 on each side of the channel axis
 * (layers.py:159-165 residual_block: tf.pad(x,[..,[C/2,C/2]]) + add + leaky_relu). */
int pnp_bn_apply(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                 const float* shortcut, int32_t Cs, float* y, int64_t P, int32_t C, float eps, float alpha,
                 void* stream);
/* backward of pnp_bn_apply.  dz = dout * (out>0 ? 1 : alpha).  dbeta = sum dz, dgamma = sum dz*xhat.
 * out == NULL (allowed when no shortcut entered the activation and `beta` is given): the sign of `out` is RECOMPUTED from x as
 * fmaf(x-mean, gamma*rstd, beta) > 0 — bit for bit the value pnp_bn_apply activated — which saves one full read of the activation in
 * the reduction and in the apply pass (these kernels sit on the HBM roof).
 * training=1 : dx = gamma*rstd*(dz - dbeta/P - xhat*dgamma/P);  training=0 (frozen stats): dx = gamma*rstd*dz
 * dx is then multiplied by the dropout mask of the producing conv when keep_prob<1 (layers.py:25: conv->dropout->BN).
 * dshortcut (optional) receives dz restricted to the Cs un-padded channels. */
int pnp_bn_bwd(const float* dout, const float* out /*nullable*/, const float* x, const float* mean, const float* var,
               const float* gamma, const float* beta /*nullable unless out == NULL*/, float* dx, float* dgamma, float* dbeta, float* dshortcut, int32_t Cs,
               int64_t P, int32_t C, float eps, float alpha, int32_t training,
               float keep_prob, uint64_t seed, uint32_t stream_id,
               void* workspace, size_t workspace_bytes, void* stream);
/* Same, and the sums are ALSO added into dgamma_acc / dbeta_acc [C] (both or neither; e.g. the parameters' slots of a flat gradient
 * arena that may already hold another use's contribution) — no separate accumulation kernel per parameter.  dgamma / dbeta still
 * receive this call's own sums (the apply half needs them). */
int pnp_bn_bwd_acc(const float* dout, const float* out /*nullable*/, const float* x, const float* mean, const float* var,
                   const float* gamma, const float* beta /*nullable unless out == NULL*/, float* dx, float* dgamma, float* dbeta, float* dgamma_acc, float* dbeta_acc,
                   float* dshortcut, int32_t Cs, int64_t P, int32_t C, float eps, float alpha, int32_t training,
                   float keep_prob, uint64_t seed, uint32_t stream_id,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The two halves of pnp_bn_bwd, for synchronised batch statistics under data parallelism: reduce the local
 * sums, all-reduce dgamma / dbeta across ranks (caller, RCCL), then apply with P_norm = the GLOBAL row count behind them.
 * pnp_bn_bwd == reduce followed by apply with P_norm = P. */
int pnp_bn_bwd_reduce(const float* dout, const float* out /*nullable*/, const float* x, const float* mean, const float* var,
                      const float* gamma /*nullable unless out == NULL*/, const float* beta /*nullable unless out == NULL*/, float* dgamma, float* dbeta, int64_t P, int32_t C, float eps, float alpha,
                      void* workspace, size_t workspace_bytes, void* stream);
int pnp_bn_bwd_apply(const float* dout, const float* out /*nullable*/, const float* x, const float* mean, const float* var,
                     const float* gamma, const float* beta /*nullable unless out == NULL*/, const float* dgamma, const float* dbeta, float* dx, float* dshortcut, int32_t Cs,
                     int64_t P, int64_t P_norm, int32_t C, float eps, float alpha, int32_t training,
                     float keep_prob, uint64_t seed, uint32_t stream_id, void* stream);

/* relu/leaky-relu of (a + shortcut) with no BN (not on the reference path; kept for the dead helpers) — omitted. */

/* tf.nn.max_pool(ksize 2, stride 2, SAME) (layers.py:102-103); H,W even. */
int pnp_maxpool2_fwd(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int pnp_maxpool2_bwd(const float* x, const float* dy, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

/* ops.PS (ops.py:3-27) closed form: out[n, i*r+u, j*r+v, c] = x[n, i, j, c*r*r + v*r + u];  x [N,A,B,nc*r*r] */
int pnp_ps_fwd(const float* x, float* y, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, void* stream);
int pnp_ps_bwd(const float* dy, float* dx, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, void* stream);

/* tf.pad(x, [[0,0],[p,p],[p,p],[0,0]], 'SYMMETRIC') (layers.py:23,72,91): xp[N,H+2p,W+2p,C], mirror including the edge.
 * The host path pre-pads SYMMETRIC convolutions with this and runs them as VALID convolutions on the tap-unrolled kernel
 * (pnp_conv2d_* also accept PNP_PAD_SYMMETRIC directly and fold the mirror into the gather). */
int pnp_sympad_fwd(const float* x, float* xp, int32_t N, int32_t H, int32_t W, int32_t C, int32_t p, void* stream);
/* backward of tf.pad(x, p, 'SYMMETRIC') in H and W: dx[N,H,W,C] from dxp[N,H+2p,W+2p,C] */
int pnp_sympad_bwd(const float* dxp, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t p, void* stream);

/* pnp_sympad_fwd(pnp_ps_fwd(x)) in one pass (the segmenter head: PS(r = 8), then the mirror pad of the 5x5 logits convolution):
 * x [N,A,B,nc*r*r] -> xp [N,A*r+2p,B*r+2p,nc]; and its backward pnp_ps_bwd(pnp_sympad_bwd(dxp)), summed in pnp_sympad_bwd's order.
 * Both are bit-identical to the two-kernel sequence.  Needs nc*r*r <= 4096 and p <= r. */
int pnp_ps_pad_fwd(const float* x, float* xp, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, int32_t p, void* stream);
int pnp_ps_pad_bwd(const float* dxp, float* dx, int32_t N, int32_t A, int32_t B, int32_t r, int32_t nc, int32_t p, void* stream);

/* Segmentation loss of source_segmenter.py:211-273 (weighted cross-entropy + soft Dice), 5..8 classes.
 * logits, y (one-hot float, lib._label_decomp) : [P, ncls].
 * out[0]=miu_cross*xent + miu_dice*dice, out[1]=xent, out[2]=dice ; dlogits = d out[0] / d logits * gscale.
 * ws: pnp_seg_loss_workspace_bytes(P, ncls).  The per-class sums land in ws and are reused by the bwd call. */
size_t pnp_seg_loss_workspace_bytes(int64_t P, int32_t ncls);
int pnp_seg_loss_fwd(const float* logits, const float* y, float* out, int64_t P, int32_t ncls,
                     float miu_cross, float miu_dice, void* workspace, size_t workspace_bytes, void* stream);
int pnp_seg_loss_bwd(const float* logits, const float* y, float* dlogits, int64_t P, int32_t ncls,
                     float miu_cross, float miu_dice, float gscale,
                     const void* workspace, size_t workspace_bytes, void* stream);
/* Same with the pixel-mean normaliser given explicitly: under data parallelism with batch-global loss normalisers the caller
 * all-reduces the 32 double sums at the head of the workspace (class counts, Dice sums) and passes P_norm = global pixel count. */
int pnp_seg_loss_bwd_norm(const float* logits, const float* y, float* dlogits, int64_t P, int64_t P_norm, int32_t ncls,
                          float miu_cross, float miu_dice, float gscale,
                          const void* workspace, size_t workspace_bytes, void* stream);
/* pixel_wise_softmax_2 + tf.argmax (layers.py:134-138, source_segmenter.py:80-81): exp(z)/sum exp(z), lowest index on ties */
int pnp_softmax_argmax(const float* logits, float* prob /*nullable*/, int64_t* label, int64_t P, int32_t ncls, void* stream);
/* lib._dice_eval (lib.py:96-110): out[0]=mean dice, out[1..ncls]=per class; label = argmax map, y one-hot */
int pnp_dice_eval(const int64_t* label, const float* y, float* out, int64_t P, int32_t ncls,
                  void* workspace, size_t workspace_bytes, void* stream);

/* lib._label_decomp (lib.py:75-92): integer-valued float label map [P] -> one-hot float32 [P, ncls]; labels >= ncls give an all-zero
 * row.  (The reference does this on the host per dequeued batch; here it runs behind the H2D copy of the feeder.) */
int pnp_label_decomp(const float* label, float* onehot, int64_t P, int32_t ncls, void* stream);
/* compact_y = tf.argmax(y, 3) of the one-hot labels (lowest index on ties; source_segmenter.py:83) and
 * tf.confusion_matrix(compact_y, compact_pred, num_classes) (source_segmenter.py:85; rows = ground truth, columns = prediction) in one
 * pass.  compact_y [P] (nullable), pred [P] / cm [ncls*ncls] int64 (both or neither). */
int pnp_confusion_matrix(const float* y, const int64_t* pred, int64_t* compact_y, int64_t* cm, int64_t P, int32_t ncls, void* stream);
/* Surface distances of label volumes for volume evaluation (the reference's README points to SIFA's evaluate.py, which scores with
 * medpy.metric.binary asd / assd / hd / hd95; connectivity 1).  Volumes [X, Y, Z] int32, z fastest, each extent in [1, 1024];
 * (sx, sy, sz) = spacing per array axis, finite and > 0.  border(A) = voxels of A with a face neighbour outside A (outside the volume
 * counts as outside A); a label outside [0, ncls) is in no class.
 * pnp_edt3d_sq: exact squared Euclidean distance (physical units) to the nearest voxel with mask != 0, +inf everywhere if there is
 * none; bit-exact for unit spacing; no workspace.
 * pnp_surface_distances: out [ncls, 7] double = n_border_pred, n_border_gt, sum pred->gt, sum gt->pred, max pred->gt, max gt->pred,
 * hd95 (numpy.percentile 95, linear, of the pooled distances of both directions).  Row 0 (background) is NaN; a class whose border is
 * empty on either side keeps its counts and has NaN distances.  2 <= ncls <= 32.  Run-to-run bitwise deterministic.
 * workspace: pnp_surface_workspace_bytes (0 for unsupported arguments). */
int pnp_edt3d_sq(const uint8_t* mask, float* dist_sq, int64_t X, int64_t Y, int64_t Z, float sx, float sy, float sz, void* stream);
size_t pnp_surface_workspace_bytes(int64_t X, int64_t Y, int64_t Z, int32_t ncls);
int pnp_surface_distances(const int32_t* pred, const int32_t* gt, int64_t X, int64_t Y, int64_t Z, int32_t ncls, float sx, float sy,
                          float sz, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* WGAN-GP gradient penalty of the critics (gradient_penalty.py).  Per sample i of a [B, n] pair of critic inputs:
 * pnp_gp_interpolate: out = eps_i * a + (1 - eps_i) * b with eps_i in [0, 1) drawn from (seed, stream_id, i) by the dropout counter hash;
 * eps [B] receives the values used.
 * pnp_gp_penalty: norms[i] = |g_i| (fp64 accumulation), penalty[0] = coef * mean_i (|g_i| - 1)^2, then g is scaled IN PLACE into the
 * penalty's adjoint gscale * dP/dg (zero for a sample with |g_i| = 0).  workspace: pnp_gp_workspace_bytes (0 for bad arguments).
 * pnp_bn_dbl_bwd: double backward of conv -> dropout(keep, seed, stream_id) -> BN(train, eps) [-> + pad(shortcut)] -> leaky(alpha; < 0:
 * none) with respect to its input-gradient pass.  In: gc_bar = adjoint of the conv-accumulator gradient, d = BN input (post dropout),
 * y = unit output (sign of the activation), gy = gradient at the unit output, the batch mean / biased var, gamma; sc_bar [P, Cs] = adjoint
 * arriving at the shortcut gradient (Cs = 0: none; zero-padded (C - Cs) / 2 each side).  Out: gy_bar [P, C], xc_bar [P, C] = adjoint of d
 * times mask / keep, gamma_bar [C] += (nullable).  workspace: pnp_bn_dbl_bwd_workspace_bytes.  All three run-to-run deterministic. */
int pnp_gp_interpolate(const float* a, const float* b, float* out, float* eps, int64_t B, int64_t n, uint64_t seed, uint32_t stream_id,
                       void* stream);
size_t pnp_gp_workspace_bytes(int64_t B, int64_t n);
int pnp_gp_penalty(float* g, int64_t B, int64_t n, float coef, float gscale, float* norms, float* penalty, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t pnp_bn_dbl_bwd_workspace_bytes(int64_t P, int32_t C);
int pnp_bn_dbl_bwd(const float* gc_bar, const float* d, const float* y, const float* gy, const float* mean, const float* var,
                   const float* gamma, const float* sc_bar, int32_t Cs, float* gy_bar, float* xc_bar, float* gamma_bar, int64_t P, int32_t C,
                   float eps, float alpha, float keep, uint64_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes,
                   void* stream);
/* Synchronised batch statistics (data-parallel replicas of equally many rows): moments[0..C) = mean, moments[C..2C) = var + mean^2 in
 * double; the caller sums `moments` over the replicas (pnp_comm_allreduce, PNP_DTYPE_F64) and converts back with the replica count. */
int pnp_bn_moments(const float* mean, const float* var, double* moments, int32_t C, void* stream);
int pnp_bn_from_moments(const double* moments, int32_t world, float* mean, float* var, int32_t C, void* stream);

/* Optimisers over ONE flat fp32 arena.  The arena is cut in chunks of PNP_OPT_CHUNK elements; chunk_l2[c] is the
 * L2 coefficient (reg_coeff * multiplicity, source_segmenter.py:132-135,237) applied to that chunk: g += l2 * w.
 * chunk_mask[c]==0 skips the chunk (frozen variables).  Either table may be NULL. */
#define PNP_OPT_CHUNK 1024
/* tf.train.AdamOptimizer (source_segmenter.py:378): lr_t = lr*sqrt(1-b2^t)/(1-b1^t); w -= lr_t*m/(sqrt(v)+eps) */
int pnp_adam_step(float* w, const float* g, float* m, float* v, size_t n, const float* chunk_l2,
                  const uint8_t* chunk_mask, float lr, float beta1, float beta2, float eps, int32_t t, void* stream);
/* tf.train.RMSPropOptimizer(decay .9, momentum 0, eps 1e-10) (adversarial.py:643-652): ms=.9ms+.1g^2; w-=lr*g/sqrt(ms+eps) */
int pnp_rmsprop_step(float* w, const float* g, float* ms, size_t n, const float* chunk_l2, const uint8_t* chunk_mask,
                     float lr, float decay, float eps, void* stream);
/* tf.train.MomentumOptimizer (source_segmenter.py:370): acc = mom*acc + g ; w -= lr*acc */
int pnp_momentum_step(float* w, const float* g, float* acc, size_t n, const float* chunk_l2, const uint8_t* chunk_mask,
                      float lr, float momentum, void* stream);
/* tf.clip_by_value weight clipping (adversarial.py:654), chunk_mask selects the clipped chunks */
int pnp_clip(float* w, size_t n, const uint8_t* chunk_mask, float lo, float hi, void* stream);
/* sum over chunks of chunk_l2[c] * sum(w^2)/2  (tf.nn.l2_loss, source_segmenter.py:237) -> out[0] */
int pnp_l2_loss(const float* w, size_t n, const float* chunk_l2, float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t pnp_reduce_workspace_bytes(size_t n);

/* Critic input assembly (adversarial.py:325-335): concat on C of [tile(a,3) | b | c | d | logits | float(argmax logits)] */
int pnp_critic_input_fwd(const float* a, int32_t Ca, int32_t tile_a, const float* b, int32_t Cb, const float* c, int32_t Cc,
                         const float* d, int32_t Cd, const float* logits, int32_t ncls, float* out, int64_t P, void* stream);
int pnp_critic_input_bwd(const float* dout, float* da, int32_t Ca, int32_t tile_a, float* db, int32_t Cb, float* dc, int32_t Cc,
                         float* dd, int32_t Cd, float* dlogits, int32_t ncls, int64_t P, void* stream);
/* The same from the COARSE tensors: a..d are [N,A,B,C*r*r] and are read through pnp_ps_fwd's permutation, logits and out are
 * [N,A*r,B*r,.]; C* are the channel counts after PS.  Bit-identical to four pnp_ps_fwd + pnp_critic_input_fwd, and to
 * pnp_critic_input_bwd + four pnp_ps_bwd (da..dd come out coarse; NULL outputs are skipped).
 * Needs (Ca+Cb+Cc+Cd)*r*r <= 4096 and, backward, r*(r*(Ctot+8)+1) <= 6144 with Ctot = Ca*tile_a+Cb+Cc+Cd+ncls+1. */
int pnp_critic_input_ps_fwd(const float* a, int32_t Ca, int32_t tile_a, const float* b, int32_t Cb, const float* c, int32_t Cc,
                            const float* d, int32_t Cd, const float* logits, int32_t ncls, float* out, int32_t N, int32_t A, int32_t B,
                            int32_t r, void* stream);
int pnp_critic_input_ps_bwd(const float* dout, float* da, int32_t Ca, int32_t tile_a, float* db, int32_t Cb, float* dc, int32_t Cc,
                            float* dd, int32_t Cd, float* dlogits, int32_t ncls, int32_t N, int32_t A, int32_t B, int32_t r, void* stream);

/* WGAN critic losses (adversarial.py:455-459): out[0] = sum_i coef[i] * mean(logit_i[0..B)) over the (up to 4) non-NULL
 * critic-logit vectors  {ct_cls, mr_cls, ct_mask, mr_mask};  e.g. dis_loss: coef = {+miu, -miu, +lambda*miu, -lambda*miu}. */
int pnp_wgan_loss(const float* ct_cls, const float* mr_cls, const float* ct_mask, const float* mr_mask, int32_t B,
                  float c_ct_cls, float c_mr_cls, float c_ct_mask, float c_mr_mask, float* out, void* stream);
/* Entropy minimisation on unlabelled predictions (csrc/entropy.hip; not in the reference).  logits [P, ncls], fp32,
 * 1 <= ncls <= 8:  out[0] = L = sum_i H_i / (P ln ncls),  H_i = -sum_k p_ik log p_ik of p_i = softmax(logits_i)  (0 for ncls == 1);
 * dlogits (nullable: value only) = coef * dL/dlogits = -coef * p_ij (log p_ij + H_i) / (P ln ncls)  — fold 1/world_size into coef.
 * out[0] is NOT scaled by coef.  log p is taken from the log-softmax, so rows with margins of hundreds give finite values.  One
 * streaming pass plus a one-block sum of its per-block partials in a fixed order, in double: stream-ordered, capturable, bit-identical
 * from run to run.  ws: pnp_softmax_entropy_workspace_bytes(P, ncls). */
size_t pnp_softmax_entropy_workspace_bytes(int64_t P, int32_t ncls);
int pnp_softmax_entropy(const float* logits, int64_t P, int32_t ncls, float coef, float* dlogits, float* out, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Boundary loss of Kervadec et al. (MIDL 2019) on the segmenter's logits (csrc/boundary.hip; not in the reference).
 * pnp_signed_distance_2d: onehot [B, H, W, ncls] fp32 (a pixel is in class c iff its entry is > 0.5) -> phi [B, H, W, ncls].  For a class
 * whose bit is set in class_mask, per slice: d = Euclidean distance in pixels to the nearest pixel of the slice whose membership in c
 * differs; phi = d outside the class, -(d - 1) inside it (one_hot2dist of the paper's code), 0 on a slice the class is absent from or
 * fills.  phi = 0 for a class whose bit is clear.  Exact: integer squared distances, one sqrtf.  1 <= H, W <= 1024, 1 <= ncls <= 8, B >= 1,
 * no bit of class_mask at or above ncls; anything else is refused before any launch.  Two launches, no atomics, no host read:
 * stream-ordered, capturable, bit-identical from run to run.  ws: pnp_signed_distance_2d_workspace_bytes(B, H, W, ncls, class_mask)
 * (one int16 per pixel and selected class; may be NULL when that is 0). */
size_t pnp_signed_distance_2d_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t ncls, uint32_t class_mask);
int pnp_signed_distance_2d(const float* onehot, int32_t B, int32_t H, int32_t W, int32_t ncls, uint32_t class_mask, float* phi,
                           void* workspace, size_t workspace_bytes, void* stream);
/* pnp_boundary_loss: logits, phi [P, ncls], fp32, 1 <= ncls <= 8, 0 <= nsel <= ncls (the number of selected classes: it only enters the
 * normaliser):  out[0] = L = sum_i s_i / (P nsel),  s_i = sum_k p_ik phi_ik of p_i = softmax(logits_i);  dlogits (nullable: value only,
 * bit-identical) = coef * dL/dlogits = coef * p_ij (phi_ij - s_i) / (P nsel)  — fold 1/world_size into coef.  out[0] is NOT scaled by
 * coef.  nsel == 0: value and gradient are 0.  One streaming pass plus a one-block sum of its per-block partials in a fixed order, in
 * double.  ws: pnp_boundary_loss_workspace_bytes(P, ncls). */
size_t pnp_boundary_loss_workspace_bytes(int64_t P, int32_t ncls);
int pnp_boundary_loss(const float* logits, const float* phi, int64_t P, int32_t ncls, int32_t nsel, float coef, float* dlogits, float* out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Class-balanced pseudo-label self-training on unlabelled predictions (csrc/pseudo_label.hip; not in the reference).
 * pnp_pseudo_label_loss: logits [P, ncls], fp32, 1 <= ncls <= 8, P < 2^31; thresholds [ncls] in DEVICE memory (read by the kernel, never
 * by the host).  k_i = argmax_j logits_ij (lowest index on ties), s_i = sum_j exp(logits_ij - max), c_i = 1 / s_i; pixel i is selected
 * iff bit k_i of class_mask is set and c_i >= thresholds[k_i].  out[0] = L = sum_selected log s_i / P (NOT scaled by coef), out[1] = the
 * selected share of the pixels; counts[0..ncls) = pixels predicted as each class, counts[ncls..2 ncls) = pixels selected as each class;
 * labels[i] = k_i | selected << 7; conf[i] = c_i; dlogits (nullable: value only, bit-identical) = coef * (p_ij - [j == k_i]) / P on the
 * selected pixels, 0 elsewhere — fold 1/world_size into coef.  One streaming pass plus a one-block sum of its per-block partials in a
 * fixed order; no float atomics, no host read, capturable.  ws: pnp_pseudo_label_loss_workspace_bytes(P, ncls).
 * pnp_pseudo_label_update: for every class k with n_k >= 1 pixels (labels & 0x7f == k), q_k = the r-th largest conf among them,
 * r = ceil(portion * n_k), EXACT (radix selection over the bit patterns, 4 rounds of 8 bits), then in place on the device
 * thresholds[k] = fmaf(momentum, thresholds[k] - q_k, q_k)  (momentum == 1: untouched).  A class without pixels keeps its threshold bit
 * for bit.  q_out (nullable) [ncls] = q_k, NaN for a class without pixels.  0 < portion <= 1, 0 <= momentum <= 1.  conf must be positive
 * finite floats (what pnp_pseudo_label_loss writes).  ws: pnp_pseudo_label_update_workspace_bytes(P, ncls). */
size_t pnp_pseudo_label_loss_workspace_bytes(int64_t P, int32_t ncls);
int pnp_pseudo_label_loss(const float* logits, const float* thresholds, int64_t P, int32_t ncls, uint32_t class_mask, float coef,
                          float* dlogits, uint8_t* labels, float* conf, float* out, int32_t* counts, void* workspace, size_t workspace_bytes,
                          void* stream);
size_t pnp_pseudo_label_update_workspace_bytes(int64_t P, int32_t ncls);
int pnp_pseudo_label_update(const uint8_t* labels, const float* conf, int64_t P, int32_t ncls, double portion, float momentum,
                            float* thresholds, float* q_out, void* workspace, size_t workspace_bytes, void* stream);
/* Fourier domain adaptation (csrc/fda.hip; not in the reference; Yang & Soatto, CVPR 2020).
 * src [B, H, W, C], tgt [Bt, H, W, C], fp32 NHWC in device memory; band, pair: HOST int32 arrays of length B (they travel in the kernel
 * argument block).  Per sample i and channel c, S = DFT2(src[i, :, :, c]), T = DFT2(tgt[pair[i], :, :, c]), b = band[i]:
 * out[i, :, :, c] = src[i, :, :, c] + Re IDFT2(D), D(u, v) = (|T| - |S|) S / |S| on |u| <= b, |v| <= b (|S| = 0: |T|), 0 elsewhere —
 * the source keeps its phase and takes the target's amplitude on the band.  band[i] = -1: sample i is copied bit for bit.
 * 1 <= B, Bt <= 256, 1 <= H, W <= 1024, 1 <= C <= 4, -1 <= band[i] <= (min(H, W) - 1) / 2, 0 <= pair[i] < Bt; out may be src itself
 * (in place), no other overlap of out with src or tgt.  Separable truncated DFT, fp32 FMAs, no atomics: bit-identical from run to run.
 * ws: pnp_fda_workspace_bytes(B, Bt, H, W, C, max over i of band[i]) (0, and ws may be NULL, when every band is -1). */
size_t pnp_fda_workspace_bytes(int32_t B, int32_t Bt, int32_t H, int32_t W, int32_t C, int32_t max_band);
int pnp_fda_amplitude_swap(const float* src, int32_t B, const float* tgt, int32_t Bt, int32_t H, int32_t W, int32_t C, const int32_t* band,
                           const int32_t* pair, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* p[0..n) = value  (constant gradient of a mean: coef / B) */
int pnp_fill(float* p, size_t n, float value, void* stream);

/* ---- bf16-RESIDENT convolutions (BASELINE.json configs[4]: bf16 mixed precision; csrc/conv_bf16r.hip) ------------------------------
 * The same convolutions as pnp_conv2d_fwd / _dgrad (layers.py:18,24,67,73,86,92) with BOTH MFMA operands stored as bfloat16 in HBM:
 *   xh / dyh : bf16 copy [N,H,W,C] of an activation / upstream gradient, written by the kernel that produced the tensor (the `yh` /
 *              `dxh` outputs below, pnp_bn_apply_h, pnp_bn_bwd_apply_h) or by pnp_cast_bf16,
 *   w_oi     : bf16 shadow [R*S][K][C] of the fp32 master filter [R,S,C,K]  (forward: reduction index C contiguous),
 *   w_io     : bf16 shadow [R*S][C][K]                                      (data gradient: reduction index K contiguous; the kernel
 *              walks the taps in reverse — no flip / transpose launch),
 * both from pnp_filter_bf16 (either pointer nullable).  fp32 accumulation; y / dx are float32 as everywhere else, `yh` / `dxh`
 * (nullable) receive the same values rounded to bf16 (nearest-even) from the same epilogue.  Arithmetic: exactly "both operands of
 * every product rounded to bf16, products summed in fp32" — what PNP_DTYPE_BF16 means for the staged-rounding kernels too.
 * pnp_conv2d_bf16r_served(g, kind) (kind 0 forward, 1 data gradient): 1 when these kernels serve the geometry (zero padding, 3x3 /
 * forward 5x5, reduction channels % 32 == 0, output channels % 64 == 0, >= 4096 output pixels; data gradients of stride 1 directly, of
 * strided layers one launch per stride phase with the phase's sub-filter read out of the full shadow); everything else stays on the
 * fp32-storage entry points above. */
int pnp_cast_bf16(const float* x, void* y_bf16, size_t n, void* stream);
int pnp_filter_bf16(const float* w, void* w_io /*nullable*/, void* w_oi /*nullable*/, int32_t R, int32_t S, int32_t C, int32_t K,
                    void* stream);
int32_t pnp_conv2d_bf16r_served(const pnp_conv_geom* g, int32_t kind);
/* number of BN-statistics partial rows the resident forward leaves (its own tiles: not pnp_conv2d_fwd_stats_parts) */
int32_t pnp_conv2d_fwd_bf16r_stats_parts(const pnp_conv_geom* g);
/* forward + dropout, optionally (stat_parts != NULL) the BN statistics partials of pnp_conv2d_fwd_stats, optionally (scale != NULL) the
 * fused inference-mode BN + shortcut + leaky-ReLU of pnp_conv2d_fwd_bn */
int pnp_conv2d_fwd_bf16r(const void* xh, const void* w_oi, float* y, void* yh /*nullable*/, const pnp_conv_geom* g,
                         float keep_prob, uint64_t seed, uint32_t stream_id,
                         const float* stat_shift /*nullable*/, float* stat_parts /*nullable*/, size_t stat_parts_bytes,
                         const float* scale /*nullable*/, const float* shift, const float* shortcut /*nullable*/, int32_t Cs, float alpha,
                         void* stream);
/* dx = data gradient (+ residual, nullable, as pnp_conv2d_dgrad_add) */
int pnp_conv2d_dgrad_bf16r(const void* dyh, const void* w_io, const float* residual /*nullable*/, float* dx, void* dxh /*nullable*/,
                           const pnp_conv_geom* g, void* stream);

/* The elementwise producers with a bf16 SIDE OUTPUT (`yh` / `dxh`, nullable): the same values as the float32 output rounded to bf16, from
 * the same launch — what the next resident convolution reads.  Otherwise identical to pnp_bn_apply / pnp_bn_bwd_acc / pnp_bn_bwd_apply /
 * pnp_dropout (pnp_dropout_h: y may be NULL when only the bf16 copy is wanted). */
int pnp_bn_apply_h(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                   const float* shortcut /*nullable*/, int32_t Cs, float* y, void* yh, int64_t P, int32_t C, float eps, float alpha,
                   void* stream);
int pnp_bn_bwd_acc_h(const float* dout, const float* out, const float* x, const float* mean, const float* var, const float* gamma,
                     const float* beta, float* dx, void* dxh, float* dgamma, float* dbeta, float* dgamma_acc, float* dbeta_acc,
                     float* dshortcut, int32_t Cs, int64_t P, int32_t C, float eps, float alpha, int32_t training, float keep_prob,
                     uint64_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream);
int pnp_bn_bwd_apply_h(const float* dout, const float* out, const float* x, const float* mean, const float* var, const float* gamma,
                       const float* beta, const float* dgamma, const float* dbeta, float* dx, void* dxh, float* dshortcut, int32_t Cs,
                       int64_t P, int64_t P_norm, int32_t C, float eps, float alpha, int32_t training, float keep_prob, uint64_t seed,
                       uint32_t stream_id, void* stream);
int pnp_dropout_h(const float* x, float* y /*nullable*/, void* yh, size_t n, float keep_prob, uint64_t seed, uint32_t stream_id,
                  void* stream);

/* filter gradient from bf16 x [N,H,W,C] and bf16 dy [N,OH,OW,K] (pnp_conv2d_bf16r_served(g, 2)): dw [R,S,C,K] float32 is overwritten
 * (accumulate = 0) or added to (accumulate != 0, as pnp_conv2d_wgrad_acc); workspace: pnp_conv2d_wgrad_bf16r_workspace_bytes(g) */
size_t pnp_conv2d_wgrad_bf16r_workspace_bytes(const pnp_conv_geom* g);
int pnp_conv2d_wgrad_bf16r(const void* xh, const void* dyh, float* dw, int32_t accumulate, const pnp_conv_geom* g,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- step capture (one hipGraph launch per training step instead of ~1 400 kernel launches from the host) ---------------------------------
 * A captured step replays its launches with every by-value argument frozen.  Two scalars change every step: the dropout seed
 * (tf.nn.dropout's per-run mask, layers.py:25,74,93) and Adam's bias-corrected learning rate (tf.train.AdamOptimizer, source_segmenter.py:378).
 * With a 16-byte DEVICE block bound (pnp_step_params_bind(block); NULL unbinds: the default), every dropout-carrying entry point takes
 * its seed from the block instead of its `seed` argument — the mask stream is the same function of (seed, stream_id) either way — and
 * pnp_adam_step takes lr * sqrt(1 - beta2^t) / (1 - beta1^t) from the block instead of computing it from (lr, t).
 * pnp_step_params_set enqueues the write of the block on `stream` (ordered before the graph launch that follows it).
 * The binding is process-global state of the library (one training loop per process). */
int pnp_step_params_bind(const void* dev_block /*16 bytes, or NULL*/);
int pnp_step_params_set(void* dev_block, uint64_t drop_seed, float adam_lr_t, void* stream);

/* Data-parallel exchange step (new with respect to the single-GPU reference, train_segmenter.py:20 / train_gan.py:18): in-place
 * SUM all-reduce over RCCL (xGMI), one communicator per process / GPU.  librccl.so is resolved at run time: pnp_comm_load(path)
 * names the copy to bind (NULL: the one already mapped in this process, else the default search path); the other calls load it
 * on first use.  Bring-up: rank 0 calls pnp_comm_unique_id and ships the PNP_COMM_ID_BYTES to every rank out of band (the host
 * side uses the torchrun rendezvous store); then EVERY rank calls pnp_comm_init (collective; binds the current HIP device).
 * pnp_comm_allreduce enqueues on `stream` and returns; ordering against producers / consumers of `buf` is the caller's business
 * (events on that stream).  buf: n elements of dtype PNP_DTYPE_F32 or PNP_DTYPE_F64. */
#define PNP_COMM_ID_BYTES 128
int pnp_comm_load(const char* librccl_path /*nullable*/);
int pnp_comm_version(int* version);
int pnp_comm_unique_id(uint8_t* id /*[PNP_COMM_ID_BYTES]*/);
int pnp_comm_init(int32_t rank, int32_t world, const uint8_t* id, void** comm_out);
int pnp_comm_allreduce(void* comm, void* buf, size_t n, int32_t dtype, void* stream);
int pnp_comm_destroy(void* comm);

/* y = a*x + b*y elementwise (gradient fan-in adds) */
int pnp_axpby(const float* x, float* y, size_t n, float a, float b, void* stream);
/* out = x + y (out may alias neither): the gradient sum of a tensor that feeds two branches of the graph (TF autodiff's AddN) */
int pnp_add(const float* x, const float* y, float* out, size_t n, void* stream);

/* ---- training input from resident volumes (csrc/augment.hip; no counterpart in the reference, whose README only names
 * the steps that produced its tfrecords: crop, cut the top 2 % of the intensity histogram, z-score, sample augmented 2-D slices) ----------
 *
 * pnp_volume_preprocess: one stream-ordered call, no host synchronisation.  v: n finite float32 voxels (NaN is unsupported: the caller's
 * error); out (may be v itself): (min(v, clip) - mean) / std in float32, all zeros when std == 0.
 *   clip  = the exact order statistic sorted(v)[k], k = (percentile * (n - 1) + 99) / 100 in integer arithmetic (percentile in [0, 100];
 *           98 = "top 2 % cut off", numpy's method="higher" without a float index) — radix selection over the order-preserving uint32 key
 *           of the float, 4 rounds of 8 bits, integer atomics only;
 *   mean, std (population, ddof 0) of min(v, clip): float64 per-block partials summed in a fixed order, two passes (sum, then squared
 *           deviations from the mean) — bit-identical from run to run;
 *   stats[4] (device, float64): clip, mean, std, the normalised minimum (= the smallest value of `out`; the default fill of pnp_aug_slices).
 * Refused on the host before any HIP call: n < 1, n >= 2^31, percentile outside [0, 100], null pointers, a short workspace. */
size_t pnp_volume_preprocess_workspace_bytes(int64_t n);
int pnp_volume_preprocess(const float* v, float* out, int64_t n, int32_t percentile, double* stats, void* workspace,
                          size_t workspace_bytes, void* stream);

/* one resident volume: image [X, Y, Z] float32 and label [X, Y, Z] uint8, both C order (z fastest: the array order of a NIfTI reader);
 * `fill` is what an image corner outside [0, X) x [0, Y) contributes */
typedef struct pnp_aug_volume {
    const float* image;
    const uint8_t* label;
    int32_t X, Y, Z;
    float fill;
} pnp_aug_volume;
/* one output slice: volume index, centre frame z in [1, Z - 2] and the affine map of output pixel (i, j) to source coordinates
 *   sx = fmaf(m[0], i, fmaf(m[1], j, m[2])),  sy = fmaf(m[3], i, fmaf(m[4], j, m[5]))      (this order is part of the contract) */
typedef struct pnp_aug_sample {
    int32_t volume, frame;
    float m[6];
} pnp_aug_sample;
/* x [B, H, W, 3]: channels = frames z-1, z, z+1, each bilinear between the four corners around (sx, sy), a corner outside the slice
 *   contributing `fill` (scipy map_coordinates order=1, mode="grid-constant", cval=fill);
 * label [B, H, W]: the label voxel at (floor(sx + 0.5), floor(sy + 0.5), z) as float32, 0 outside (order=0, grid-constant, cval=0);
 * onehot [B, H, W, ncls] (nullable): the rows pnp_label_decomp gives for `label` (a label >= ncls: an all-zero row), same pass.
 * vols_host / vols_dev: the same nvol descriptors in host memory (checked here, before any launch: X, Y in [1, 4096], Z >= 3, non-null
 * pointers) and in device memory (read by the kernel).  A sample whose volume index or frame is out of range is not an error of the
 * call: it is written as fill / 0 (0 / 0 when the volume index itself is bad) and counted once in *errors (device uint32, added to, never
 * reset here).  x, label and onehot must be 16-byte aligned. */
int pnp_aug_slices(const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol, const pnp_aug_sample* samples_dev,
                   int32_t B, int32_t H, int32_t W, float* x, float* label, float* onehot /*nullable*/, int32_t ncls,
                   uint32_t* errors, void* stream);

/* ---- sampling on a millimetre grid (csrc/augment.hip): the outer channels at a fractional frame distance ---------------------
 *
 * one output slice of pnp_aug_slices_z: volume index, centre frame in [0, Z - 1], the frame step dz >= 0 (frames per channel: the wanted
 * millimetres between channels over the volume's frame spacing) and pnp_aug_sample's map */
typedef struct pnp_aug_sample_z {
    int32_t volume, frame;
    float dz;
    float m[6];
} pnp_aug_sample_z;
/* pnp_aug_slices with these differences (everything else, the lane layout and the 16-byte alignment included, is pnp_aug_slices'):
 *   volumes need Z >= 1 (checked on the host); `frame` may be any of 0 .. Z - 1;
 *   channel 1 is frame `frame`; channels 0 / 2 read at zf = fminf(fmaxf((float)frame -+ dz, 0), Z - 1) (the clamp replicates the first and
 *   the last frame): with z0 = floorf(zf), z1 = min(z0 + 1, Z - 1), t = zf - z0 an in-slice corner contributes
 *   fmaf(t, v[z1] - v[z0], v[z0]) — the lerp along z comes FIRST — and an out-of-slice corner `fill`; then pnp_aug_slices' bilinear chain
 *   (this order is part of the contract);
 *   label and one-hot: at (floor(sx + 0.5), floor(sy + 0.5), frame), unchanged.
 * With dz == 1 and frame in [1, Z - 2] image, label and one-hot equal pnp_aug_slices' bit for bit (t = 0 returns v[z0]); with dz == 1 at
 * frame 0 or Z - 1 the missing neighbour is the edge frame itself.  A sample whose volume index or frame is out of range, or whose dz is
 * NaN, infinite or negative, is written as fill / 0 and counted once in *errors; dz is compared before it enters any arithmetic and no
 * unchecked float is converted to an integer. */
int pnp_aug_slices_z(const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol, const pnp_aug_sample_z* samples_dev,
                     int32_t B, int32_t H, int32_t W, float* x, float* label, float* onehot /*nullable*/, int32_t ncls,
                     uint32_t* errors, void* stream);

/* ---- elastic deformation and intensity augmentation in the gather (csrc/augment.hip) ------------------------------------------
 *
 * one output slice of pnp_aug_slices_warp: pnp_aug_sample_z's fields, then the intensity map out = gain * v + bias + noise * n of the image
 * channels, the seed of the sample's noise stream and whether the sample is displaced by its control table (warp != 0) */
typedef struct pnp_aug_sample_w {
    int32_t volume, frame;
    float dz;
    float m[6];
    float gain, bias, noise;
    uint32_t seed;
    int32_t warp;
} pnp_aug_sample_w;
/* pnp_aug_slices_z (frames, clamp, refusals, lane layout, alignment: all its own) with two additions.
 * ctrl_dev [B][G + 3][G + 3][2] float32 (device, 8-byte aligned): per sample the control points (dx, dy) of a uniform cubic B-spline over
 *   the output plane, in SOURCE-VOXEL units; 1 <= G <= 16 cells per axis, or G == 0 with ctrl_dev == NULL (then a sample with warp != 0 is
 *   refused: fill / 0, counted once in *errors, as a bad frame is).
 * Coordinates of output pixel (i, j): (sx, sy) by pnp_aug_sample's fmaf chain; if warp != 0, in float32 and in this order (the order is
 *   part of the contract; no operation is contracted other than the fmaf written here):
 *     rh = (float)G / (float)H;  gi = ((float)i + 0.5f) * rh;  ci = max(min((int)floorf(gi), G - 1), 0);  t = gi - (float)ci;
 *     rw, gj, cj, s likewise from j and W;
 *     weights of t (and of s):  u = 1 - t,  k = 1.f / 6.f,
 *       B0 = ((u * u) * u) * k,  B1 = fmaf(t * t, fmaf(3, t, -6), 4) * k,  B2 = fmaf(t, fmaf(t, fmaf(-3, t, 3), 3), 1) * k,  B3 = ((t * t) * t) * k;
 *     per column c = 0 .. 3, with P_a = ctrl[ci + a][cj + c] (each component):  R_c = fmaf(B3(t), P_3, fmaf(B2(t), P_2, fmaf(B1(t), P_1, B0(t) * P_0)));
 *     d = fmaf(B3(s), R_3, fmaf(B2(s), R_2, fmaf(B1(s), R_1, B0(s) * R_0)));   sx = sx + d.x;  sy = sy + d.y.
 *   Image (bilinear with fill) and label (nearest) are both read at the displaced coordinates.  A NaN, infinite or huge displacement ends
 *   in pnp_aug_slices' comparison "outside -> fill / label 0", which comes before any conversion to an integer.
 * Intensity of every image value v of an accepted sample (fill pixels included; the label is untouched):
 *     v = (gain == 1 && bias == 0) ? v : fmaf(gain, v, bias);      if (noise != 0)  v = fmaf(noise, n, v)
 *     e  = 3 * (i * W + j) + channel;   h1 = fmix32((2 e) * 0xCC9E2D51 ^ seed),  h2 = fmix32((2 e + 1) * 0xCC9E2D51 ^ seed)   (uint32, pnp_dropout's hash)
 *     u1 = ((h1 >> 8) + 1) * 2^-24,  u2 = (h2 >> 8) * 2^-24;   n = sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2)
 *   With noise == 0 no random number is computed.  Refused samples are written as plain fill / 0.
 * With warp == 0, gain == 1, bias == 0, noise == 0 the outputs equal pnp_aug_slices_z's bit for bit (and pnp_aug_slices' when dz == 1).
 * Refused on the host before any HIP call: everything pnp_aug_slices_z refuses; G outside [0, 16]; ctrl_dev null with G >= 1 or non-null
 * with G == 0; ctrl_dev not 8-byte aligned; 6 * H * W >= 2^32. */
int pnp_aug_slices_warp(const pnp_aug_volume* vols_host, const pnp_aug_volume* vols_dev, int32_t nvol, const pnp_aug_sample_w* samples_dev,
                        const float* ctrl_dev /*nullable*/, int32_t G, int32_t B, int32_t H, int32_t W, float* x, float* label,
                        float* onehot /*nullable*/, int32_t ncls, uint32_t* errors, void* stream);

/* ---- volume inference, the way back (csrc/paste.hip): labels of a batch of logits written onto the scan's own grid --------
 *
 * logits [B, H, W, ncls] float32 (device, finite: anything else is the caller's error), 1 <= ncls <= 8; slice b < nb <= B is frame z0 + b.
 * For every x < X, y < Y, b < nb one label byte is written at vol[origin + x * sx + y * sy + (z0 + b) * sz] (element strides of any sign:
 * one launch writes the array order of the NIfTI file, the double flip, the axis move and a crop offset folded into origin and strides);
 * nothing else of `vol` is touched.  The label of voxel column (x, y):
 *   pi = fmaf(inv[0], x, fmaf(inv[1], y, inv[2])),  pj = fmaf(inv[3], x, fmaf(inv[4], y, inv[5]))     (this order is part of the contract;
 *        inv: six HOST floats, the map from a source voxel to output-plane coordinates)
 *   each clamped into [0, H - 1] / [0, W - 1] (NaN -> 0, before any integer conversion);
 *   every class's logit bilinear between the four corners (scipy map_coordinates order=1, mode="nearest"; a fractional part of 0 returns
 *   the corner's value bit for bit); the label is the lowest index among the strictly largest interpolated logits.
 * Refused on the host before any HIP call: null pointers; B, H, W, X, Y < 1; H, W, X, Y > 4096; ncls outside [1, 8]; nb outside [1, B];
 * z0 < 0; vol_elems < 1; an addressed element outside [0, vol_elems) (from the extreme corners of the box); strides under which two
 * voxels of the box collide (sorted by magnitude, each must be at least the one before it times that axis' extent). */
int pnp_paste_labels(const float* logits, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0, const float* inv,
                     int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                     void* stream);

/* ---- ensemble inference (csrc/paste.hip): M members' logits -> label, mean probabilities, normalised entropy ------------------
 *
 * logits: HOST array of M device pointers (1 <= M <= 8; a pointer may repeat), each [B, H, W, ncls] float32, finite; inv: HOST array of
 * 6 * M floats, member m's map from a source voxel to its output plane.  The box, vol, origin and strides are pnp_paste_labels'.  Per voxel
 * (x, y, frame b), with e = origin + x * sx + y * sy + (z0 + b) * sz:
 *   for m ascending: r_m[c] exactly as pnp_paste_labels interpolates with inv_m (a map that leaves the plane contributes the clamped edge
 *     value); mx = max_c r_m[c]; e_c = expf(r_m[c] - mx); s = sum of e_c over ascending c; p_c = e_c / s;
 *   acc_c = (p_c of members 0 .. 3 summed ascending) + (those of members 4 .. 7 summed ascending; absent for M <= 4);
 *   P_c = acc_c * (1.0f / M) (exact for M = 1, 2, 4, 8; M equal members give P = p bit for bit for those M);
 *   vol[e] = the lowest c with the strictly largest acc_c;
 *   prob[c * vol_elems + e] = P_c (nullable; class-major planes of vol_elems floats);
 *   entropy[e] = -sum_c fmaf-accumulated P_c * logf(P_c) / logf(ncls), a term with P_c == 0 contributing 0; 0 for ncls == 1 (nullable).
 * Nothing else of vol, prob or entropy is touched.  Refused on the host before any HIP call: all that pnp_paste_labels refuses; M outside
 * [1, 8]; a null member pointer; a null inv; ncls * vol_elems overflowing int64. */
int pnp_paste_ensemble(int32_t M, const float* const* logits, const float* inv, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb,
                       int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                       float* prob /*nullable*/, float* entropy /*nullable*/, void* stream);

/* ---- paste inside the field of view only (csrc/paste.hip) -----------------------------------------------------------------------
 *
 * The arguments, the checks and the arithmetic of pnp_paste_labels / pnp_paste_ensemble.  A voxel column (x, y) is COVERED iff for every
 * member m (one for pnp_paste_labels_fov) the unclamped plane coordinates — the same two fmaf chains, before the clamp — satisfy
 *   -0.5 <= pi <= H - 0.5  and  -0.5 <= pj <= W - 0.5        (a NaN coordinate is not covered).
 * For a covered column the entry writes exactly the bytes / floats the entry without _fov writes, bit for bit; for an uncovered column
 * nothing of vol, prob or entropy is touched.  Coverage does not depend on the frame: still one writer per element, no atomics. */
int pnp_paste_labels_fov(const float* logits, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb, int32_t z0, const float* inv,
                         int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy, int64_t sz,
                         void* stream);
int pnp_paste_ensemble_fov(int32_t M, const float* const* logits, const float* inv, int32_t B, int32_t H, int32_t W, int32_t ncls, int32_t nb,
                           int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy,
                           int64_t sz, float* prob /*nullable*/, float* entropy /*nullable*/, void* stream);

/* ---- tiled inference: overlapping planes blended over their union (csrc/paste.hip) ----------------------------------------------
 *
 * The arguments and checks of pnp_paste_ensemble_fov with 1 <= M <= 64 members and one more float, `ramp` >= 1 (plane pixels).  A member
 * COVERS the voxel column (x, y) iff its unclamped plane coordinates (pi, pj) — the two fmaf chains — satisfy pnp_paste_labels_fov's rule.
 * A column that no member covers is written in none of vol, prob, entropy.  For a covered column and frame b, over the covering members in
 * ascending m:
 *   w_m = g(pi; H) * g(pj; W),  g(p; n) = fminf(1, fmaxf(d, 0.5f) * (1.0f / ramp)),  d = fminf(p + 0.5f, (n - 0.5f) - p)
 *   p_c as pnp_paste_ensemble computes member m's softmax;  acc_c += w_m * p_c (the product rounded, then the sum);  wsum += w_m;
 *   vol[e] = the lowest c with the strictly largest acc_c;  prob[c * vol_elems + e] = P_c = acc_c / wsum;  entropy[e] from P as
 *   pnp_paste_ensemble's.  A member given twice (same pointer, same map) leaves all three outputs as with that member given once, bit for bit.
 * Refused on the host before any HIP call: all that pnp_paste_ensemble refuses (M outside [1, 64]); ramp not finite or < 1. */
int pnp_paste_tiles(int32_t M, const float* const* logits, const float* inv, float ramp, int32_t B, int32_t H, int32_t W, int32_t ncls,
                    int32_t nb, int32_t z0, int32_t X, int32_t Y, uint8_t* vol, int64_t vol_elems, int64_t origin, int64_t sx, int64_t sy,
                    int64_t sz, float* prob /*nullable*/, float* entropy /*nullable*/, void* stream);

/* ---- multi-planar fusion: several probability volumes of one grid -> label, mean probabilities, entropy (csrc/paste.hip) -----
 *
 * probs: HOST array of n_views device pointers (1 <= n_views <= 8), each ncls class-major planes of vol_elems float32 — class c of
 * element e at probs[v][c * vol_elems + e], the layout pnp_paste_ensemble writes; weights: HOST array of n_views positive finite floats,
 * NULL = all 1.  Per element e, in this order:
 *   for v ascending: s_v = sum of probs[v][c][e] over ascending c (each step rounded); view v COVERS e iff s_v > 0.5 (a view's
 *     probabilities sum to 1 within rounding where it predicted, and are exactly 0 where it did not; a NaN sum does not cover);
 *   no covering view: label[e] = 0, prob[c][e] = 0 for every c, entropy[e] = 0;
 *   otherwise, over the covering views in ascending v: acc_c += w_v * probs[v][c][e] (the product rounded, then the sum), wsum += w_v;
 *     P_c = acc_c / wsum;  label[e] = the lowest c with the strictly largest P_c;  prob[c * vol_elems + e] = P_c (nullable);
 *     entropy[e] from P as pnp_paste_ensemble's (nullable).
 * EVERY element of label, prob and entropy is written (they may be uninitialised).  One view without weights reproduces its probabilities
 * bit for bit.  prob may be probs[0] itself (every element's inputs are read before it is written); no atomics, bit-identical from run
 * to run.  Bases aligned to 4 bytes only are served (16-byte accesses are used where all float bases share one phase of the 16-byte grid
 * and ncls == 1 or vol_elems % 4 == 0).
 * Refused on the host before any HIP call: n_views outside [1, 8]; ncls outside [1, 8]; vol_elems < 1; 4 * ncls * vol_elems overflowing
 * int64; a null probs, view or label; a weight that is not positive and finite; a float pointer not aligned to 4 bytes; any overlap
 * among the views, prob, entropy and label other than prob == probs[0]. */
int pnp_fuse_views(int32_t n_views, const float* const* probs, const float* weights /*host, nullable*/, int32_t ncls, int64_t vol_elems,
                   uint8_t* label, float* prob /*nullable*/, float* entropy /*nullable*/, void* stream);

/* ---- connected components of label volumes (csrc/components.hip): keep the largest 3-D component of every structure -------
 *
 * vol: uint8 labels [D0, D1, D2], C order (D2 fastest: what pnp_paste_labels writes and a NIfTI reader returns), each extent in [1, 4096],
 * n = D0 * D1 * D2 < 2^31; 2 <= ncls <= 8; a label >= ncls counts as background (0).  A component is a maximal set of voxels of ONE non-zero
 * label joined by steps of the 6 / 18 / 26 neighbourhood (connectivity 1 / 2 / 3: scipy's generate_binary_structure(3, connectivity)); all
 * classes in one pass, voxels of different classes are never joined.
 * pnp_label_components: roots [n] int32 = -1 for background, otherwise the smallest flat index among the voxels of the voxel's component.
 *   Union-find, three launches whatever the data, no host read in between; bit-identical from run to run.
 * pnp_filter_components: out [n] uint8 (may be vol itself) from vol and the roots of the SAME vol, ncls and connectivity.  A component of a
 *   class c in [1, ncls) whose bit is set in class_mask survives when its size is >= min_size and, if keep > 0, it is among the `keep`
 *   largest of its class, ties going to the lower root (the key (size << 32) | ~root, largest first); its voxels keep their label, those of
 *   a removed component become 0.  Classes outside the mask pass through unchanged; labels >= ncls become 0.
 *   stats [ncls, 4] int64 = components found, voxels before, voxels kept, size of the largest component; row 0 is all zero; classes outside
 *   the mask report kept = before.  3 + max(keep, 1) launches.
 * Workspace: pnp_components_workspace_bytes (0 for unsupported extents), one size for both calls.  Its first two uint32 are device error
 * counters the caller reads after the call(s): [0], zeroed and written by pnp_label_components only, counts union-find loops that reached
 * their cap of n steps (they cannot: a non-zero value means the result is not to be used); [1], zeroed and written by
 * pnp_filter_components, counts waves that met a roots entry >= n (roots that are not pnp_label_components' output).
 * Refused on the host before any HIP call: null pointers; an extent outside [1, 4096]; n >= 2^31; ncls outside [2, 8]; connectivity outside
 * {1, 2, 3}; keep outside [0, 8]; min_size < 0; class_mask with bit 0 or a bit >= ncls; a short workspace. */
size_t pnp_components_workspace_bytes(int64_t D0, int64_t D1, int64_t D2);
int pnp_label_components(const uint8_t* vol, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, int32_t connectivity, int32_t* roots,
                         void* workspace, size_t workspace_bytes, void* stream);
int pnp_filter_components(const uint8_t* vol, const int32_t* roots, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, uint32_t class_mask,
                          int32_t keep, int64_t min_size, uint8_t* out, int64_t* stats, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- hole filling of label volumes (csrc/components.hip): close the enclosed background holes of every structure -----------
 *
 * vol, the extents and ncls as above.  A voxel is BACKGROUND when its label is 0 or >= ncls.  A CAVITY is a maximal set of background voxels
 * joined by face steps (6 neighbours) without a voxel at index 0 or D - 1 of any axis: scipy.ndimage.binary_fill_holes with its default
 * structure fills exactly the union of the cavities (a volume with an extent <= 2 has none).  For a cavity and a class c in [1, ncls) the
 * contacts are the pairs (v in the cavity, u a face neighbour of v) with label(u) == c; the WINNER is the class with the most contacts,
 * ties going to the lower class.  A cavity is filled with its winner when the winner's bit is set in class_mask and max_size == 0 or its
 * size <= max_size; otherwise it is left (the mask never redirects a cavity to a runner-up).
 *   out [n] uint8 (may be vol itself) = the winner on filled cavities, 0 on every other background voxel (labels >= ncls included), vol
 *   elsewhere: only background is ever rewritten, a class enclosed by another class is never touched.
 *   stats [ncls, 4] int64: row c >= 1 = cavities filled with c, voxels filled with c, size of the largest cavity filled with c, cavities
 *   won by c and left; row 0 = cavities found, voxels in them, cavities left, voxels left.
 * Integers only, bit-identical from run to run; 10 launches whatever the data, no host read.
 * Workspace: pnp_fill_holes_workspace_bytes (0 for unsupported extents or ncls) = 2 048 + 4 n + 4 n + n + 4 n (ncls - 1) bytes, every block
 * rounded up to 256.  Its first two uint32 are the labelling's and the size count's error counters (see above), the uint32 at byte 1 024
 * counts cavities without a contact and cavity voxels on a face (neither can happen); all are zeroed by the call and read by the caller.
 * Refused on the host before any HIP call: null pointers; an extent outside [1, 4096]; n >= 2^31; ncls outside [2, 8]; class_mask with bit 0
 * or a bit >= ncls; max_size < 0; a short workspace; a workspace address that is no multiple of 16 (the kernels read it in 16-byte loads and
 * keep 64-bit sums in it); an out that is neither vol itself nor disjoint from vol's n bytes (a partial overlap). */
size_t pnp_fill_holes_workspace_bytes(int64_t D0, int64_t D1, int64_t D2, int32_t ncls);
int pnp_fill_holes(const uint8_t* vol, int64_t D0, int64_t D1, int64_t D2, int32_t ncls, uint32_t class_mask, int64_t max_size, uint8_t* out,
                   int64_t* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- anti-alias prefilter of a resident volume (csrc/smooth.hip) ---------------------------------------------------------------
 *
 * pnp_volume_smooth: dst = the separable filter of src, both float32 [X, Y, Z] in C order (z fastest), borders replicated (the index of
 * every tap clamped into [0, n - 1] per axis: scipy.ndimage's mode="nearest").  wx / wy / wz: HOST pointers to 2 r + 1 float32 weights
 * (tap k multiplies the voxel at index + k - r), null exactly when that r == 0; they are read during the call and travel to the kernels by
 * value, so the caller may free them at once.  One stream-ordered call, no host synchronisation.
 *   An axis with r == 0 is not filtered at all (no multiplication by 1: its values pass through bit for bit).  All radii 0: nothing is
 *   launched when dst == src, a device-to-device copy otherwise.
 *   dst == src (in place) and disjoint buffers are both served; the passes themselves run between src, dst and the workspace.
 *   Every output of a pass is fmaf(w[2r], v[2r], ... fmaf(w[1], v[1], fmaf(w[0], v[0], 0))) in float32; the passes run in the order X, Y, Z.
 *   No atomics: bit-identical from run to run, and in place equals out of place bit for bit.
 * Workspace: pnp_volume_smooth_workspace_bytes (0 for unsupported arguments, and when no intermediate volume is needed): at most one volume,
 *   rounded up to 256 bytes, unless all three axes are filtered and Z > 2048 (two).
 * Refused on the host before any HIP call: null src / dst; an extent below 1; X or Y above 4096; X * Y * Z >= 2^31; a radius outside
 * [0, 32]; null weights with r > 0; a weight that is not finite; src and dst overlapping partially; a short workspace. */
size_t pnp_volume_smooth_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t rx, int32_t ry, int32_t rz);
int pnp_volume_smooth(const float* src, float* dst, int32_t X, int32_t Y, int32_t Z, const float* wx /*host, nullable*/, int32_t rx,
                      const float* wy /*host, nullable*/, int32_t ry, const float* wz /*host, nullable*/, int32_t rz, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- per-frame class statistics of a resident label volume (csrc/frame_stats.hip): where the classes are ---------------------
 *
 * pnp_label_frame_stats: label uint8 [X, Y, Z] in C order (z fastest: pnp_aug_volume's label), at ANY byte address (a misaligned base or a
 * Z that is no multiple of 4 takes byte loads, anything else 4-, 8- or 16-byte loads).  stats [Z, ncls, 5] int32:
 *   stats[z][c] = (count, xmin, xmax, ymin, ymax) over the voxels of frame z whose label equals c, c in [0, ncls); a label >= ncls counts
 *   nowhere (as it gives an all-zero one-hot row in pnp_aug_slices); a class absent from a frame is (0, X, -1, Y, -1).
 * The call initialises the table itself: stats may be uninitialised memory.  One stream-ordered call (two launches), no host
 * synchronisation, no workspace.  int32 add / min / max atomics only: bit-identical from run to run.
 * Refused on the host before any HIP call: null pointers; X or Y outside [1, 4096]; Z < 1; X * Y * Z >= 2^31; ncls outside [1, 8]; stats not
 * 4-byte aligned. */
int pnp_label_frame_stats(const uint8_t* label, int32_t X, int32_t Y, int32_t Z, int32_t ncls, int32_t* stats /* [Z, ncls, 5] */,
                          void* stream);

/* ---- label-free body crop of a resident volume (csrc/body.hip): histogram between min and max, mask of the upper bins --------
 *
 * The bin of a voxel x of a volume with minimum lo and maximum hi, lo < hi, is
 *   bin(x) = min(nbins - 1, (int)((x - lo) * scale)),   scale = (float)nbins / (hi - lo),
 * every operation one float32 IEEE round-to-nearest operation, nothing contracted or reassociated; both calls compute it with the same
 * device function, so they never disagree about a voxel on a bin edge.  2 <= nbins <= 1024.
 * pnp_volume_histogram: v = n finite float32 voxels at ANY 4-byte address (a base that is no multiple of 16 costs up to three scalar loads
 *   at either end, the rest are 16-byte loads).  range [2] float32 <- (lo, hi) = (min v, max v), bit-exact; hist [nbins] uint32 <- the voxel
 *   count per bin, sum = n.  hi == lo (a constant volume): hist[0] = n, every other bin 0.  The call initialises range and hist itself;
 *   one stream-ordered call (four launches), no host synchronisation, no workspace.  Integer atomics only (min / max of the order-preserving
 *   uint32 key of a float, one pair per workgroup; LDS histograms, one global add per non-empty bin and workgroup): bit-identical from run
 *   to run.
 * pnp_volume_threshold_mask: mask [n] uint8 (any address) <- bin(v[i]) > k ? 1 : 0 with (lo, hi) read from `range` ON THE DEVICE (what
 *   pnp_volume_histogram wrote for the same v) — the threshold is a bin index, a float threshold is never compared.  hi == lo: all zeros.
 *   One launch, no host synchronisation.
 * Refused on the host before any HIP call: null pointers; n < 1; n >= 2^31; nbins outside [2, 1024]; k outside [0, nbins - 1]; v, range or
 * hist not 4-byte aligned; mask overlapping v. */
int pnp_volume_histogram(const float* v, int64_t n, int32_t nbins, float* range /* [2] */, uint32_t* hist /* [nbins] */, void* stream);
int pnp_volume_threshold_mask(const float* v, int64_t n, const float* range /* [2], device */, int32_t nbins, int32_t k, uint8_t* mask,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PNP_HIP_H */
