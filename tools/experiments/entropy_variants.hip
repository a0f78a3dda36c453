// Timing experiment behind DESIGN.md §27: launch shapes of the entropy pass at P = 16*256*256, C = 5 — the shipped direct float4 kernel
// (pixel_loss::stream_kernel<EntropyTerm, true, .> of csrc/pixel_loss.h) at several grid sizes against a variant that stages 1 024-pixel
// tiles through LDS (coalesced 16-byte loads and stores) around the same EntropyTerm::pixel.  Not part of the library.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../include -o entropy_variants entropy_variants.hip
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
void pnp_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
#include "../../medical-cross-modality-domain-adaptation_amd/csrc/entropy.hip"

namespace {
constexpr int NT = pixel_loss::NT;

template <bool GRAD>
__global__ void __launch_bounds__(NT) ent_lds_kernel(const float* __restrict__ logits, float* __restrict__ dlogits, float* __restrict__ part,
                                                     long long ntile, float gk) {
    __shared__ float4 tile[5 * NT];
    __shared__ float lds[4];
    const float4* __restrict__ in = reinterpret_cast<const float4*>(logits);
    float4* __restrict__ out = reinterpret_cast<float4*>(dlogits);
    float acc = 0.f, conf;      // (the term has no per-thread state and no side outputs: lane, lab and conf are the signature's only)
    uint32_t lab;
    EntropyTerm::Lane<5> lane({}, 5);
    for (long long t = blockIdx.x; t < ntile; t += gridDim.x) {
        const long long base = t * (5 * NT);
#pragma unroll
        for (int k = 0; k < 5; ++k) tile[threadIdx.x + NT * k] = in[base + threadIdx.x + NT * k];
        __syncthreads();
        float f[20];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float4 v = tile[threadIdx.x * 5 + k];
            f[4 * k] = v.x, f[4 * k + 1] = v.y, f[4 * k + 2] = v.z, f[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc += EntropyTerm::pixel<5, GRAD>(f + 5 * r, nullptr, 5, gk, f + 5 * r, lane, lab, conf);
        if (GRAD) {
#pragma unroll
            for (int k = 0; k < 5; ++k) tile[threadIdx.x * 5 + k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 5; ++k) out[base + threadIdx.x + NT * k] = tile[threadIdx.x + NT * k];
        }
        __syncthreads();
    }
    float x = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
}  // namespace

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    const long long P = 16ll * 256 * 256;
    const int C = 5, NB = 8, REPS = 64;
    const size_t n = (size_t)P * C;
    std::vector<float> h(n);
    unsigned s = 12345u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = ((int)(s >> 8) % 2000 - 1000) * 0.006f; }
    float *z[NB], *g[NB], *part, *ref;
    for (int b = 0; b < NB; ++b) {
        CK(hipMalloc(&z[b], n * 4)); CK(hipMalloc(&g[b], n * 4));
        CK(hipMemcpy(z[b], h.data(), n * 4, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&part, 8192 * 4)); CK(hipMalloc(&ref, n * 4));
    const float gk = 0.01f / ((float)P * logf(5.f));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    struct V { const char* name; int kind; int blocks; };
    const long long ngrp = P / 4, ntile = P / 1024;
    V vs[] = {{"direct 8px/thread (shipped)", 0, (int)(P / (256 * 8))}, {"direct 4px/thread", 0, (int)(ngrp / 256)},
              {"direct 16px/thread", 0, (int)(P / (256 * 16))}, {"direct 2048 blocks cap=ngrp/128", 0, 2048},
              {"lds tile, 1 tile/block", 1, (int)ntile}, {"lds tile, 2 tiles/block", 1, (int)(ntile / 2)}, {"lds tile, 4 tiles/block", 1, (int)(ntile / 4)}};
    std::vector<float> a(n), bb(n);
    for (auto& v : vs) {
        for (int grad = 1; grad >= 0; --grad) {
            auto launch = [&](int b) {
                if (v.kind == 0) {
                    const EntropyTerm::Args none{};
                    if (grad)
                        hipLaunchKernelGGL((pixel_loss::stream_kernel<EntropyTerm, true, true>), dim3(v.blocks), dim3(NT), 0, 0, z[b], g[b], part, P,
                                           C, gk, none);
                    else
                        hipLaunchKernelGGL((pixel_loss::stream_kernel<EntropyTerm, true, false>), dim3(v.blocks), dim3(NT), 0, 0, z[b], g[b], part, P,
                                           C, gk, none);
                } else {
                    if (grad) hipLaunchKernelGGL((ent_lds_kernel<true>), dim3(v.blocks), dim3(NT), 0, 0, z[b], g[b], part, ntile, gk);
                    else hipLaunchKernelGGL((ent_lds_kernel<false>), dim3(v.blocks), dim3(NT), 0, 0, z[b], g[b], part, ntile, gk);
                }
            };
            for (int b = 0; b < NB; ++b) launch(b);
            CK(hipDeviceSynchronize());
            float best[2] = {1e30f, 1e30f};
            for (int mode = 0; mode < 2; ++mode)
                for (int rep = 0; rep < 5; ++rep) {
                    CK(hipEventRecord(e0, 0));
                    for (int r = 0; r < REPS; ++r) launch(mode ? r % NB : 0);
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                    if (ms < best[mode]) best[mode] = ms;
                }
            CK(hipGetLastError());
            const double bytes = (grad ? 2.0 : 1.0) * n * 4;
            printf("%-34s grad=%d blocks=%5d  one buffer %7.2f us %6.0f GB/s | rotating %7.2f us %6.0f GB/s\n", v.name, grad, v.blocks,
                   best[0] / REPS * 1e3, bytes / (best[0] / REPS * 1e-3) / 1e9, best[1] / REPS * 1e3, bytes / (best[1] / REPS * 1e-3) / 1e9);
            if (grad) {
                CK(hipMemcpy((&v == &vs[0] ? a : bb).data(), g[0], n * 4, hipMemcpyDeviceToHost));
                if (&v != &vs[0]) printf("    gradient %s the first variant's\n", memcmp(a.data(), bb.data(), n * 4) ? "DIFFERS from" : "bit-equal to");
            }
        }
    }
    return 0;
}
