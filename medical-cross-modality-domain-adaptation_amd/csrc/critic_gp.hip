// critic_gp.hip — WGAN-GP gradient penalty of the two critics (gradient_penalty.py): the interpolation between the two
// domains' critic inputs, the per-sample gradient norms / penalty / penalty adjoint, and the double backward of the critics' unit
// conv -> dropout -> BN(train) [-> + channel-zero-padded shortcut] -> leaky-ReLU with respect to its input-gradient pass.
// Tensors are [P][C] fp32 with C contiguous; 16 B per lane where C % 4 == 0, one channel per lane otherwise.
// Every reduction is two-level in a fixed order (no atomics): run-to-run bitwise deterministic.  Nothing here synchronises.
#include "block_sum.h"
#include "pnp_common.h"

namespace {

constexpr int NT = 256;
constexpr int GP_BLOCKS = 64;        // partial sums per sample of the norm reduction
constexpr int DBL_SUMS = 5;          // sum v, sum v*xhat, sum v*gz, sum gz, sum gz*xhat
constexpr int DBL_COEF = 8;          // per-channel coefficients handed from the combine to the apply kernel

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// uniform [0, 1) per sample from the dropout counter hash: 24 bits of fmix32((i * 0xCC9E2D51) ^ key(seed, stream id))
__device__ __forceinline__ float gp_uniform(uint32_t i, uint32_t key) {
    return (float)(pnp_fmix32((i * 0xCC9E2D51u) ^ key) >> 8) * (1.0f / 16777216.0f);
}

// ---- interpolation x_hat = eps_i * a + (1 - eps_i) * b ------------------------------------------------------------------------------
// grid (blocks per sample, B)
__global__ void __launch_bounds__(NT) gp_interp_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                       float* __restrict__ eps_out, long long n, uint32_t key) {
    const int s = blockIdx.y;
    const float e = gp_uniform((uint32_t)s, key), f = 1.0f - e;
    if (blockIdx.x == 0 && threadIdx.x == 0) eps_out[s] = e;
    const size_t base = (size_t)s * n;
    const size_t gs = (size_t)gridDim.x * NT;
    if ((n & 3) == 0) {
        const size_t n4 = (size_t)n >> 2;
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += gs) {
            const f32x4 av = ld4(a + base + i * 4), bv = ld4(b + base + i * 4);
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = fmaf(e, av[k], f * bv[k]);
            st4(out + base + i * 4, r);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < (size_t)n; i += gs) out[base + i] = fmaf(e, a[base + i], f * b[base + i]);
    }
}

// ---- per-sample squared norms: GP_BLOCKS double partials per sample (grid (GP_BLOCKS, B)), fixed lane order and tree -------------
__global__ void __launch_bounds__(NT) gp_norm_partial_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
    __shared__ double red[NT];
    const int s = blockIdx.y;
    const float* gs_ = g + (size_t)s * n;
    const size_t stride = (size_t)GP_BLOCKS * NT;
    double acc = 0.0;
    if ((n & 3) == 0) {
        const size_t n4 = (size_t)n >> 2;
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += stride) {
            const f32x4 v = ld4(gs_ + i * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma((double)v[k], (double)v[k], acc);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < (size_t)n; i += stride) acc = fma((double)gs_[i], (double)gs_[i], acc);
    }
    const double sum = block_tree<NT>(acc, red);
    if (threadIdx.x == 0) part[(size_t)s * GP_BLOCKS + blockIdx.x] = sum;
}

// one workgroup: norms, per-sample adjoint scale, penalty = coef * mean_i (|g_i| - 1)^2
__global__ void __launch_bounds__(NT) gp_final_kernel(const double* __restrict__ part, int B, float coef, float gscale,
                                                      float* __restrict__ norms, float* __restrict__ scale, float* __restrict__ penalty) {
    __shared__ double red[NT];
    double acc = 0.0;
    for (int s = threadIdx.x; s < B; s += NT) {
        double q = 0.0;
        for (int j = 0; j < GP_BLOCKS; ++j) q += part[(size_t)s * GP_BLOCKS + j];
        const double nrm = sqrt(q);
        norms[s] = (float)nrm;
        // dP/dg_i = coef * 2 / B * (|g_i| - 1) * g_i / |g_i|; a zero gradient has no direction: zero adjoint, not NaN
        scale[s] = nrm > 0.0 ? (float)((double)coef * (double)gscale * 2.0 / (double)B * (nrm - 1.0) / nrm) : 0.0f;
        acc += (nrm - 1.0) * (nrm - 1.0);
    }
    const double sum = block_tree<NT>(acc, red);
    if (threadIdx.x == 0) penalty[0] = (float)((double)coef * sum / (double)B);
}

// g <- scale_i * g in place (the penalty's adjoint with respect to the input gradient); grid (blocks per sample, B)
__global__ void __launch_bounds__(NT) gp_scale_kernel(float* __restrict__ g, long long n, const float* __restrict__ scale) {
    const int s = blockIdx.y;
    const float k = scale[s];
    float* gs_ = g + (size_t)s * n;
    const size_t gs = (size_t)gridDim.x * NT;
    if ((n & 3) == 0) {
        const size_t n4 = (size_t)n >> 2;
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n4; i += gs) {
            f32x4 v = ld4(gs_ + i * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= k;
            st4(gs_ + i * 4, v);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < (size_t)n; i += gs) gs_[i] *= k;
    }
}

// ---- BN double backward ---------------------------------------------------------------------------------------------------------------
// Unit: c = conv(x), d = c * mask / keep, z = (d - mean) * gamma / sigma + beta [+ pad(shortcut)], y = leaky(z).  Its input-gradient pass
// is g_z = g_y * leaky'(z), g_d = (gamma/sigma) (g_z - m_g - xhat m_gx), g_c = g_d * mask / keep.  Given the adjoint gcb of g_c:
//   v = gcb * mask / keep;  m_* = per-channel means over the P rows
//   gzb = (gamma/sigma) (v - m_v - xhat m_vx) [+ pad(adjoint at the shortcut)],  gyb = gzb * leaky'(z)
//   gamma_bar += P (m_vg - m_v m_g - m_vx m_gx) / sigma
//   xd = -(gamma/sigma^2) [xhat (m_vg - m_v m_g - 3 m_vx m_gx) + m_gx (v - m_v) + m_vx (g_z - m_g)],  xcb = xd * mask / keep
// leaky'(z) is read from the sign of y (y > 0 <=> z > 0; slope alpha at z == 0, like the forward kernels' backward passes).
struct DblArgs {
    const float *gcb, *d, *y, *gy, *mean, *var, *gamma, *scb;
    float *gyb, *xcb, *gamma_bar;
    double* part;        // [nblk][DBL_SUMS][C]
    float* coef;         // [C][DBL_COEF]
    long long P;
    int C, Cs, rows_per_block, nblk;
    float eps, alpha, keep;
    int do_drop;
    uint32_t key, thresh;
};

template <int V>
__device__ __forceinline__ void ldv(const float* p, float* v) {
    if constexpr (V == 4) {
        const f32x4 t = ld4(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void stv(float* p, const float* v) {
    if constexpr (V == 4) {
        f32x4 t = {v[0], v[1], v[2], v[3]};
        st4(p, t);
    } else {
        p[0] = v[0];
    }
}

// channel-group mapping shared by the reduce and apply kernels: blockIdx.y = slice of NT groups of V channels; a thread owns one group
// and walks rows (rpi rows per pass)
struct GroupMap {
    int c, cgs, rpi, rsub;
    bool active;
};

template <int V>
__device__ __forceinline__ GroupMap group_map(int C) {
    const int CG = C / V;
    const int g0 = blockIdx.y * NT;
    const int CGs = (CG - g0) < NT ? (CG - g0) : NT;
    GroupMap m;
    m.cgs = CGs;
    m.rpi = NT / CGs;
    m.rsub = threadIdx.x / CGs;
    m.active = m.rsub < m.rpi;
    m.c = (g0 + (int)(threadIdx.x % CGs)) * V;
    return m;
}

// level 1: per row slab (blockIdx.x) and channel, the five sums as fp32 per lane, combined over the slab's lanes in double, fixed order
template <int V>
__global__ void __launch_bounds__(NT) bn_dbl_reduce_kernel(DblArgs a) {
    __shared__ float red[NT * DBL_SUMS * V];
    const GroupMap gm = group_map<V>(a.C);
    const int t = threadIdx.x;
    float s[DBL_SUMS][V];
#pragma unroll
    for (int q = 0; q < DBL_SUMS; ++q)
#pragma unroll
        for (int e = 0; e < V; ++e) s[q][e] = 0.f;
    if (gm.active) {
        float m[V], rs[V], vv[V];
        ldv<V>(a.mean + gm.c, m);
        ldv<V>(a.var + gm.c, vv);
#pragma unroll
        for (int e = 0; e < V; ++e) rs[e] = 1.0f / sqrtf(vv[e] + a.eps);
        const long long r0 = (long long)blockIdx.x * a.rows_per_block;
        const long long r1 = r0 + a.rows_per_block < a.P ? r0 + a.rows_per_block : a.P;
        for (long long r = r0 + gm.rsub; r < r1; r += gm.rpi) {
            const size_t off = (size_t)r * a.C + gm.c;
            float gc[V], xv[V], gy[V], yv[V] = {};
            ldv<V>(a.gcb + off, gc);
            ldv<V>(a.d + off, xv);
            ldv<V>(a.gy + off, gy);
            if (a.alpha >= 0.f) ldv<V>(a.y + off, yv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float xh = (xv[e] - m[e]) * rs[e];
                const float gz = a.alpha >= 0.f ? (yv[e] > 0.f ? gy[e] : gy[e] * a.alpha) : gy[e];
                float v = gc[e];
                if (a.do_drop) v = pnp_drop_keep((uint32_t)(off + e), a.key, a.thresh) ? v / a.keep : 0.f;
                s[0][e] += v;
                s[1][e] = fmaf(v, xh, s[1][e]);
                s[2][e] = fmaf(v, gz, s[2][e]);
                s[3][e] += gz;
                s[4][e] = fmaf(gz, xh, s[4][e]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < DBL_SUMS; ++q)
#pragma unroll
        for (int e = 0; e < V; ++e) red[(t * DBL_SUMS + q) * V + e] = s[q][e];
    __syncthreads();
    if (!gm.active || gm.rsub != 0) return;
    for (int q = 0; q < DBL_SUMS; ++q) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double acc = 0.0;
            for (int j = 0; j < gm.rpi; ++j) acc += (double)red[((j * gm.cgs + t) * DBL_SUMS + q) * V + e];
            a.part[((size_t)blockIdx.x * DBL_SUMS + q) * a.C + gm.c + e] = acc;
        }
    }
}

// level 2: 32 channels x 8 slices of the slab list per workgroup, fixed order; then the per-channel coefficients and gamma_bar
__global__ void __launch_bounds__(NT) bn_dbl_combine_kernel(DblArgs a) {
    __shared__ double red[DBL_SUMS][8][33];
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    double s[DBL_SUMS] = {0, 0, 0, 0, 0};
    if (c < a.C) {
        for (int b = sl; b < a.nblk; b += 8)
#pragma unroll
            for (int q = 0; q < DBL_SUMS; ++q) s[q] += a.part[((size_t)b * DBL_SUMS + q) * a.C + c];
    }
#pragma unroll
    for (int q = 0; q < DBL_SUMS; ++q) red[q][sl][cl] = s[q];
    __syncthreads();
    if (sl != 0 || c >= a.C) return;
#pragma unroll
    for (int q = 0; q < DBL_SUMS; ++q) {
        s[q] = 0.0;
        for (int j = 0; j < 8; ++j) s[q] += red[q][j][cl];
    }
    const double N = (double)a.P;
    const double m_v = s[0] / N, m_vx = s[1] / N, m_vg = s[2] / N, m_g = s[3] / N, m_gx = s[4] / N;
    const double sig2 = (double)a.var[c] + (double)a.eps, sig = sqrt(sig2), ga = (double)a.gamma[c];
    const double ka = ga / sig, kb = -ga / sig2;
    float* k = a.coef + (size_t)c * DBL_COEF;
    k[0] = (float)(-ka * m_v);                                    // gzb = k0 + k1 xhat + k2 v
    k[1] = (float)(-ka * m_vx);
    k[2] = (float)ka;
    k[3] = (float)(kb * (-m_gx * m_v - m_vx * m_g));              // xd = k3 + k4 xhat + k5 v + k6 gz
    k[4] = (float)(kb * (m_vg - m_v * m_g - 3.0 * m_vx * m_gx));
    k[5] = (float)(kb * m_gx);
    k[6] = (float)(kb * m_vx);
    k[7] = 0.f;
    if (a.gamma_bar) a.gamma_bar[c] += (float)(N * (m_vg - m_v * m_g - m_vx * m_gx) / sig);
}

// level 3: elementwise gyb / xcb; a workgroup streams one contiguous slab of rows
template <int V>
__global__ void __launch_bounds__(NT) bn_dbl_apply_kernel(DblArgs a) {
    const GroupMap gm = group_map<V>(a.C);
    if (!gm.active) return;
    const int cpad = (a.C - a.Cs) / 2;
    float m[V], rs[V], vv[V], k[DBL_COEF][V];
    ldv<V>(a.mean + gm.c, m);
    ldv<V>(a.var + gm.c, vv);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        rs[e] = 1.0f / sqrtf(vv[e] + a.eps);
#pragma unroll
        for (int j = 0; j < DBL_COEF; ++j) k[j][e] = a.coef[(size_t)(gm.c + e) * DBL_COEF + j];
    }
    const long long per = ((a.P + gridDim.x - 1) / gridDim.x + gm.rpi - 1) / gm.rpi * gm.rpi;
    const long long rend = ((long long)blockIdx.x + 1) * per < a.P ? ((long long)blockIdx.x + 1) * per : a.P;
    for (long long row = (long long)blockIdx.x * per + gm.rsub; row < rend; row += gm.rpi) {
        const size_t off = (size_t)row * a.C + gm.c;
        float gc[V], xv[V], gy[V], yv[V] = {}, gyb[V], xcb[V];
        ldv<V>(a.gcb + off, gc);
        ldv<V>(a.d + off, xv);
        ldv<V>(a.gy + off, gy);
        if (a.alpha >= 0.f) ldv<V>(a.y + off, yv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float xh = (xv[e] - m[e]) * rs[e];
            const float lk = a.alpha >= 0.f ? (yv[e] > 0.f ? 1.0f : a.alpha) : 1.0f;
            const float gz = gy[e] * lk;
            const bool kept = a.do_drop ? pnp_drop_keep((uint32_t)(off + e), a.key, a.thresh) : true;
            const float v = a.do_drop ? (kept ? gc[e] / a.keep : 0.f) : gc[e];
            float gzb = fmaf(k[2][e], v, fmaf(k[1][e], xh, k[0][e]));
            const int cs = gm.c + e - cpad;
            if (a.scb && cs >= 0 && cs < a.Cs) gzb += a.scb[(size_t)row * a.Cs + cs];
            gyb[e] = gzb * lk;
            const float xd = fmaf(k[6][e], gz, fmaf(k[5][e], v, fmaf(k[4][e], xh, k[3][e])));
            xcb[e] = a.do_drop ? (kept ? xd / a.keep : 0.f) : xd;
        }
        stv<V>(a.gyb + off, gyb);
        stv<V>(a.xcb + off, xcb);
    }
}

void dbl_plan(long long P, int* nblk, int* rpb) {
    long long b = (P + 63) / 64;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    const long long r = (P + b - 1) / b;
    *rpb = (int)r;
    *nblk = (int)((P + r - 1) / r);
}

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

int gp_blocks_per_sample(long long n) {
    long long b = (n / 4 + NT * 8 - 1) / (NT * 8);
    if (b > 256) b = 256;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

extern "C" {

int pnp_gp_interpolate(const float* a, const float* b, float* out, float* eps, int64_t B, int64_t n, uint64_t seed, uint32_t stream_id,
                       void* stream) {
    PNP_REQUIRE(B >= 1 && B <= 65535 && n >= 1, "pnp_gp_interpolate: B %lld (1..65535) / n %lld (>= 1)", (long long)B, (long long)n);
    PNP_REQUIRE(a && b && out && eps, "pnp_gp_interpolate: null pointer");
    hipLaunchKernelGGL(gp_interp_kernel, dim3(gp_blocks_per_sample(n), (unsigned)B), dim3(NT), 0, (hipStream_t)stream, a, b, out, eps,
                       (long long)n, pnp_drop_key(seed, stream_id));
    PNP_CHECK_LAUNCH("gp_interp_kernel");
    return PNP_OK;
}

size_t pnp_gp_workspace_bytes(int64_t B, int64_t n) {
    if (B < 1 || B > 65535 || n < 1) return 0;
    return align_up((size_t)B * GP_BLOCKS * sizeof(double)) + align_up((size_t)B * sizeof(float));
}

int pnp_gp_penalty(float* g, int64_t B, int64_t n, float coef, float gscale, float* norms, float* penalty, void* workspace,
                   size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(B >= 1 && B <= 65535 && n >= 1, "pnp_gp_penalty: B %lld (1..65535) / n %lld (>= 1)", (long long)B, (long long)n);
    PNP_REQUIRE(g && norms && penalty && workspace, "pnp_gp_penalty: null pointer");
    const size_t need = pnp_gp_workspace_bytes(B, n);
    PNP_REQUIRE(workspace_bytes >= need, "pnp_gp_penalty: workspace %zu bytes < %zu (pnp_gp_workspace_bytes)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    float* scale = (float*)((char*)workspace + align_up((size_t)B * GP_BLOCKS * sizeof(double)));
    hipLaunchKernelGGL(gp_norm_partial_kernel, dim3(GP_BLOCKS, (unsigned)B), dim3(NT), 0, st, (const float*)g, (long long)n, part);
    PNP_CHECK_LAUNCH("gp_norm_partial_kernel");
    hipLaunchKernelGGL(gp_final_kernel, dim3(1), dim3(NT), 0, st, (const double*)part, (int)B, coef, gscale, norms, scale, penalty);
    PNP_CHECK_LAUNCH("gp_final_kernel");
    hipLaunchKernelGGL(gp_scale_kernel, dim3(gp_blocks_per_sample(n), (unsigned)B), dim3(NT), 0, st, g, (long long)n, (const float*)scale);
    PNP_CHECK_LAUNCH("gp_scale_kernel");
    return PNP_OK;
}

size_t pnp_bn_dbl_bwd_workspace_bytes(int64_t P, int32_t C) {
    if (P < 1 || C < 1 || C > 65535) return 0;
    int nblk, rpb;
    dbl_plan(P, &nblk, &rpb);
    return align_up((size_t)nblk * DBL_SUMS * C * sizeof(double)) + align_up((size_t)C * DBL_COEF * sizeof(float));
}

int pnp_bn_dbl_bwd(const float* gc_bar, const float* d, const float* y, const float* gy, const float* mean, const float* var,
                   const float* gamma, const float* sc_bar, int32_t Cs, float* gy_bar, float* xc_bar, float* gamma_bar, int64_t P, int32_t C,
                   float eps, float alpha, float keep, uint64_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes,
                   void* stream) {
    PNP_REQUIRE(P >= 1 && C >= 1 && C <= 65535, "pnp_bn_dbl_bwd: P %lld (>= 1) / C %d (1..65535)", (long long)P, (int)C);
    PNP_REQUIRE((unsigned long long)P * (unsigned long long)C <= 0xFFFFFFFFull, "pnp_bn_dbl_bwd: P*C %lld beyond the 32-bit mask index",
                (long long)P * C);
    PNP_REQUIRE(gc_bar && d && gy && mean && var && gamma && gy_bar && xc_bar && workspace, "pnp_bn_dbl_bwd: null pointer");
    PNP_REQUIRE(alpha < 0.f || y, "pnp_bn_dbl_bwd: the activation's sign is read from y (null)");
    PNP_REQUIRE(Cs == 0 || (Cs > 0 && Cs <= C && (C - Cs) % 2 == 0 && sc_bar), "pnp_bn_dbl_bwd: shortcut %d channels into %d", (int)Cs,
                (int)C);
    PNP_REQUIRE(keep > 0.f && keep <= 1.f, "pnp_bn_dbl_bwd: keep %g outside (0, 1]", keep);
    PNP_REQUIRE(eps > 0.f, "pnp_bn_dbl_bwd: eps %g must be > 0", eps);
    const size_t need = pnp_bn_dbl_bwd_workspace_bytes(P, C);
    PNP_REQUIRE(workspace_bytes >= need, "pnp_bn_dbl_bwd: workspace %zu bytes < %zu (pnp_bn_dbl_bwd_workspace_bytes)", workspace_bytes,
                need);
    hipStream_t st = (hipStream_t)stream;
    DblArgs a;
    a.gcb = gc_bar; a.d = d; a.y = y; a.gy = gy; a.mean = mean; a.var = var; a.gamma = gamma; a.scb = Cs ? sc_bar : nullptr;
    a.gyb = gy_bar; a.xcb = xc_bar; a.gamma_bar = gamma_bar;
    int nblk, rpb;
    dbl_plan(P, &nblk, &rpb);
    a.part = (double*)workspace;
    a.coef = (float*)((char*)workspace + align_up((size_t)nblk * DBL_SUMS * C * sizeof(double)));
    a.P = P; a.C = C; a.Cs = Cs; a.rows_per_block = rpb; a.nblk = nblk;
    a.eps = eps; a.alpha = alpha; a.keep = keep;
    a.do_drop = keep < 1.f;
    a.key = pnp_drop_key(seed, stream_id);
    a.thresh = pnp_drop_thresh(keep);
    const bool vec = (C & 3) == 0;
    const int CG = vec ? C / 4 : C;
    const unsigned ny = (unsigned)((CG + NT - 1) / NT);
    if (vec) hipLaunchKernelGGL(bn_dbl_reduce_kernel<4>, dim3(nblk, ny), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(bn_dbl_reduce_kernel<1>, dim3(nblk, ny), dim3(NT), 0, st, a);
    PNP_CHECK_LAUNCH("bn_dbl_reduce_kernel");
    hipLaunchKernelGGL(bn_dbl_combine_kernel, dim3((C + 31) / 32), dim3(NT), 0, st, a);
    PNP_CHECK_LAUNCH("bn_dbl_combine_kernel");
    // apply: like bn_bwd_apply's grid — row slabs up to 2048 workgroups over all channel slices
    const int CGs = CG < NT ? CG : NT;
    const int rpi = NT / CGs;
    long long bx = (P + rpi - 1) / rpi;
    const long long cap = 2048 / ny > 0 ? 2048 / ny : 1;
    if (bx > cap) bx = cap;
    if (bx < 1) bx = 1;
    if (vec) hipLaunchKernelGGL(bn_dbl_apply_kernel<4>, dim3((unsigned)bx, ny), dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(bn_dbl_apply_kernel<1>, dim3((unsigned)bx, ny), dim3(NT), 0, st, a);
    PNP_CHECK_LAUNCH("bn_dbl_apply_kernel");
    return PNP_OK;
}

}  // extern "C"
