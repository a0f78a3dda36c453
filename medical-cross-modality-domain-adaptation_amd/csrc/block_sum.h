// block_sum.h — the project's deterministic reduction: no atomics, one fixed order of additions in double, the same
// bits from run to run.  One block of NT threads (a power of two); sh is NT doubles of LDS.  Both functions end with a barrier and
// return the sum to EVERY thread, so sh can be handed to the next call at once; a caller that stores from thread 0 alone may do so.
#pragma once
#include <hip/hip_runtime.h>

// thread t brings a; level by level (NT / 2, NT / 4, ... 1) thread t < h adds the value of thread t + h to its own
template <int NT>
__device__ __forceinline__ double block_tree(double a, double* sh) {
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// sum of a partial list (float or double entries): thread t adds entries t, t + NT, ... in ascending order, then the tree
template <int NT, typename T>
__device__ __forceinline__ double block_sum_of_list(const T* __restrict__ p, int np, double* sh) {
    double a = 0.0;
    for (int i = threadIdx.x; i < np; i += NT) a += (double)p[i];
    return block_tree<NT>(a, sh);
}
