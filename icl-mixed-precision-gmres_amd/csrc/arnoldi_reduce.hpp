// Reductions of the fused Arnoldi cycle. Global sums are two-stage and
// deterministic (per-workgroup fp64 partials, then k_reduce_partials in a
// fixed order), which is also the seam where a multi-GPU caller all-reduces
// across ranks.
#pragma once

#include "arnoldi_plan.hpp"
#include "panel.hpp"

namespace {

// Combine in the last arriver: sums[c] = sum over g of partial[c*G + g] for
// c < ncols <= BS/32; 32 lanes per column, each a strided run in g order,
// then a 32-lane xor tree (fixed order).
template <int BS, class A = double>
__device__ __forceinline__ void combine_columns(const double* __restrict__ partial, int G, int ncols,
                                                double* __restrict__ sums) {
    const int c = threadIdx.x / 32, sub = threadIdx.x % 32;
    A v = A(0);
    if (c < ncols)
        for (int g = sub; g < G; g += 32) v += (A)partial[(size_t)c * G + g];
#pragma unroll
    for (int mask = 16; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask, kWave);
    if (c < ncols && sub == 0) sums[c] = (double)v;
}

// ---------------------------------------------------------------- reductions
// sum of G partials in a fixed order (identical in every workgroup that
// calls it with the same G); result valid in thread 0. A: the accumulation
// class (fp32: the partials are fp32 values, every add rounds to fp32)
template <int BS, class A = double>
__device__ __forceinline__ A sum_partials(const double* __restrict__ p, int G, A* scratch) {
    A v0 = A(0), v1 = A(0);
    int g = threadIdx.x;
    for (; g + BS < G; g += 2 * BS) {
        v0 += (A)p[g];
        v1 += (A)p[g + BS];
    }
    if (g < G) v0 += (A)p[g];
    return block_sum<BS>(v0 + v1, scratch);
}

template <int BS, class A = double>
__global__ __launch_bounds__(BS) void k_reduce_partials(int G, const double* __restrict__ partial,
                                                        double* __restrict__ sums) {
    __shared__ A scratch[BS / kWave];
    const A s = sum_partials<BS, A>(partial + (size_t)blockIdx.x * G, G, scratch);
    if (threadIdx.x == 0) sums[blockIdx.x] = (double)s;
}

// ||w||^2 partials again (column 1 of the prologue's partials, same grid)
// after a preconditioner applied outside the prologue kernel (ILU)
template <class T>
__global__ __launch_bounds__(kBlock) void k_wnorm_partials(int n, const T* __restrict__ w, double* __restrict__ partial) {
    double acc[1] = {0.0};
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) acc[0] += (double)w[i] * (double)w[i];
    store_partials<1>(acc, 1, partial + gridDim.x);
}

}  // namespace
