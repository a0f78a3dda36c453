// entropy.hip — normalised mean Shannon entropy of the softmax of a logits tensor and its gradient, in one streaming pass
// (entropy minimisation on the unlabelled target's predictions; not in the reference).
//
//   p_i = softmax(z_i),  H_i = -sum_k p_ik log p_ik,  L = sum_i H_i / (P ln C),  dL/dz_ij = -p_ij (log p_ij + H_i) / (P ln C)
//
// log p comes from the log-softmax (z - max - log sum exp), never from logf(p): a class hundreds of logits behind has p == 0 and a
// finite log p, its term is 0 * finite = 0.  The two launches are the per-pixel skeleton's (pixel_loss.h); this file is the term.
#include "pixel_loss.h"

#include <cmath>

namespace {

// one pixel: z[0..C) -> H (returned); g[0..C) = -gk * p (log p + H) when GRAD
struct EntropyTerm : pixel_loss::Plain<0> {
    template <int C, bool GRAD>
    static __device__ __forceinline__ float pixel(const float* z, const float* const*, int ncls, float gk, float* g, Lane<C>&, uint32_t&, float&) {
        float e[C], m;
        const float s = pixel_loss::softmax_exp<C>(z, ncls, e, m);
        const float ls = logf(s), inv = 1.0f / s;
        float lp[C], H = 0.f;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            lp[j] = j < ncls ? (z[j] - m) - ls : 0.f;
            e[j] *= inv;
            H = fmaf(-e[j], lp[j], H);
        }
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < C; ++j) g[j] = -gk * e[j] * (lp[j] + H);
        }
        return H;
    }
};

}  // namespace

extern "C" {

size_t pnp_softmax_entropy_workspace_bytes(int64_t P, int32_t ncls) {
    (void)ncls;
    return pixel_loss::workspace_bytes(P);
}

int pnp_softmax_entropy(const float* logits, int64_t P, int32_t ncls, float coef, float* dlogits, float* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
    PNP_REQUIRE(logits && out && workspace && P > 0 && ncls > 0, "pnp_softmax_entropy: bad argument");
    PNP_REQUIRE(ncls <= MAXC, "pnp_softmax_entropy: ncls = %d, at most %d classes are served", (int)ncls, MAXC);
    PNP_REQUIRE(workspace_bytes >= pnp_softmax_entropy_workspace_bytes(P, ncls), "pnp_softmax_entropy: workspace too small (%zu < %zu bytes)",
                workspace_bytes, pnp_softmax_entropy_workspace_bytes(P, ncls));
    // 1 / (P ln C); a single class has entropy 0 and no normaliser (soft_entropy of paste.hip): value and gradient are 0
    const double scale = ncls > 1 ? 1.0 / ((double)P * std::log((double)ncls)) : 0.0;
    const float gk = (float)((double)coef * scale);
    return pixel_loss::run<EntropyTerm>("pnp_softmax_entropy", logits, {}, (long long)P, ncls, scale, gk, dlogits, out, workspace,
                                        (hipStream_t)stream);
}

}  // extern "C"
