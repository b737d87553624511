// Block-Jacobi preconditioner for node-ordered matrices (bs = 2, 3 or 4
// unknowns per node): M = blockdiag(D_r)^-1, D_r the rows and columns
// [bs r, bs r + bs) of A.
//
// Set-up: one lane per block scans the block's CSR rows for its bs columns
// (a missing entry is 0, the first occurrence of a column wins), widens the
// values to fp64 and inverts in registers by Gauss-Jordan on [D | I] with
// partial pivoting (largest |entry| of the column, lowest row on a tie), in
// one fixed operation order with contraction off, then rounds the inverse
// once to the preconditioner precision P: bs*bs values per block, row-major,
// blocks contiguous.
//
// Apply (in place on a vector of T): y_i = sum_j Dinv[i][j] * x_j in P, each
// product rounded, summed left to right in j, contraction off; x is cast
// T -> P before and P -> T after. One lane per row. A workgroup owns
// R = 256 / bs * bs consecutive rows (a whole number of blocks), so every
// global access is one contiguous run per wave: the rows go through LDS (a
// lane reads its block's bs inputs from there), and so do the workgroup's
// R * bs inverse entries, loaded with consecutive lanes on consecutive words
// and read back at stride bs words (conflict-free for bs = 3).
// Bytes per row: 2 sizeof(T) + bs sizeof(P).
#include <cfloat>
#include <climits>
#include <cmath>

#include "internal.hpp"

namespace {

using namespace mpg;

template <class P, int BS>
__global__ __launch_bounds__(kBlock) void k_bjacobi_setup(int32_t nblk, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col,
                                                          const P* __restrict__ val, P* __restrict__ dinv,
                                                          int32_t* __restrict__ first_bad) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= nblk) return;
    const int64_t base = r * BS;
    double M[BS][2 * BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) {
#pragma unroll
        for (int j = 0; j < BS; ++j) {
            M[i][j] = 0.0;
            M[i][BS + j] = i == j ? 1.0 : 0.0;
        }
        unsigned seen = 0;
        const int32_t k1 = rowptr[base + i + 1];
        for (int32_t k = rowptr[base + i]; k < k1; ++k) {
            const int64_t c = (int64_t)col[k] - base;
            if (c < 0 || c >= BS || (seen >> c & 1u)) continue;
            seen |= 1u << c;
            const double v = (double)val[k];
#pragma unroll
            for (int j = 0; j < BS; ++j)
                if (j == c) M[i][j] = v;
        }
    }
    bool bad = false;
#pragma unroll
    for (int c = 0; c < BS; ++c) {
        int p = c;
        double best = fabs(M[c][c]);
#pragma unroll
        for (int q = c + 1; q < BS; ++q) {
            const double a = fabs(M[q][c]);
            if (a > best) {
                best = a;
                p = q;
            }
        }
        if (!(best > 0.0) || !(best <= DBL_MAX)) bad = true;  // zero, NaN or Inf pivot
#pragma unroll
        for (int q = c + 1; q < BS; ++q) {
            if (p == q) {
#pragma unroll
                for (int j = 0; j < 2 * BS; ++j) {
                    const double t = M[c][j];
                    M[c][j] = M[q][j];
                    M[q][j] = t;
                }
            }
        }
        const double piv = M[c][c];
#pragma unroll
        for (int j = 0; j < 2 * BS; ++j) M[c][j] = M[c][j] / piv;
#pragma unroll
        for (int q = 0; q < BS; ++q) {
            if (q == c) continue;
            const double f = M[q][c];
#pragma unroll
            for (int j = 0; j < 2 * BS; ++j) {
                const double t = f * M[c][j];
                M[q][j] = M[q][j] - t;
            }
        }
    }
    if (bad) atomicMin(first_bad, (int32_t)r);
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) dinv[r * (BS * BS) + i * BS + j] = (P)M[i][BS + j];
}

template <class T, class P, int BS>
__global__ __launch_bounds__(kBlock) void k_bjacobi_apply(int64_t n, const P* __restrict__ dinv, T* x) {
#pragma clang fp contract(off)
    constexpr int R = kBlock / BS * BS;
    __shared__ P xs[R];
    __shared__ P ds[R * BS];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * R;
    const int64_t left = n - base;
    const int rows = left < R ? (int)left : R;  // a multiple of BS (n is)
    if (t < rows) xs[t] = (P)x[base + t];
#pragma unroll
    for (int j = 0; j < BS; ++j) {
        const int q = t + j * kBlock;
        if (q < rows * BS) ds[q] = dinv[base * BS + q];
    }
    __syncthreads();
    if (t >= rows) return;
    const int b0 = t / BS * BS;
    P acc = ds[t * BS] * xs[b0];
#pragma unroll
    for (int j = 1; j < BS; ++j) {
        const P p = ds[t * BS + j] * xs[b0 + j];
        acc = acc + p;
    }
    x[base + t] = (T)acc;
}

template <class P, int BS>
void launch_setup(mpg_ctx* ctx, mpg_csr* A, const P* vals, P* dinv, int32_t* bad) {
    const int32_t nblk = A->rows / BS;
    const int grid = (nblk + kBlock - 1) / kBlock;
    k_bjacobi_setup<P, BS><<<grid, kBlock, 0, ctx->stream>>>(nblk, A->rowptr, A->col, vals, dinv, bad);
}

template <class P>
int setup_impl(mpg_ctx* ctx, mpg_csr* A, const P* vals, int32_t bs, P* dinv, int32_t* first_bad_block) {
    if (first_bad_block) *first_bad_block = -1;
    if (!ctx || !A || bs < 2 || bs > 4 || A->rows % bs != 0) return MPG_ERR_ARG;
    if (A->rows == 0) return MPG_OK;
    if (!vals || !dinv) return MPG_ERR_ARG;
    int32_t* bad = reinterpret_cast<int32_t*>(ctx->red_ws);
    int32_t h = INT32_MAX;
    MPG_HIP(ctx, hipMemcpyAsync(bad, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
    MPG_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (h is on the stack)
    if (bs == 2) launch_setup<P, 2>(ctx, A, vals, dinv, bad);
    else if (bs == 3) launch_setup<P, 3>(ctx, A, vals, dinv, bad);
    else launch_setup<P, 4>(ctx, A, vals, dinv, bad);
    MPG_LAUNCH_CHECK(ctx);
    MPG_HIP(ctx, hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    MPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h != INT32_MAX) {
        if (first_bad_block) *first_bad_block = h;
        ctx->last_error = "block Jacobi: diagonal block " + std::to_string(h) + " (rows " +
                          std::to_string((int64_t)h * bs) + ".." + std::to_string((int64_t)h * bs + bs - 1) +
                          ") is singular or not finite (zero or non-finite pivot)";
        return MPG_ERR_BREAKDOWN;
    }
    return MPG_OK;
}

template <class T, class P>
int apply_impl(mpg_ctx* ctx, int64_t n, int32_t bs, const P* dinv, T* x) {
    if (!ctx || n < 0 || bs < 2 || bs > 4 || n % bs != 0) return MPG_ERR_ARG;
    if (n == 0) return MPG_OK;
    if (!dinv || !x) return MPG_ERR_ARG;
    const int R = kBlock / bs * bs;
    const int64_t grid = (n + R - 1) / R;
    if (grid > INT32_MAX) return MPG_ERR_ARG;
    const dim3 g((unsigned)grid), b(kBlock);
    if (bs == 2) k_bjacobi_apply<T, P, 2><<<g, b, 0, ctx->stream>>>(n, dinv, x);
    else if (bs == 3) k_bjacobi_apply<T, P, 3><<<g, b, 0, ctx->stream>>>(n, dinv, x);
    else k_bjacobi_apply<T, P, 4><<<g, b, 0, ctx->stream>>>(n, dinv, x);
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

}  // namespace

extern "C" {

int mpg_bjacobi_setup_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, int32_t bs, double* dinv_out,
                          int32_t* first_bad_block) {
    return setup_impl<double>(c, A, vals, bs, dinv_out, first_bad_block);
}
int mpg_bjacobi_setup_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, int32_t bs, float* dinv_out,
                          int32_t* first_bad_block) {
    return setup_impl<float>(c, A, vals, bs, dinv_out, first_bad_block);
}
int mpg_bjacobi_apply_f64(mpg_ctx_t c, int64_t n, int32_t bs, const double* dinv, double* x) {
    return apply_impl<double, double>(c, n, bs, dinv, x);
}
int mpg_bjacobi_apply_f32(mpg_ctx_t c, int64_t n, int32_t bs, const float* dinv, float* x) {
    return apply_impl<float, float>(c, n, bs, dinv, x);
}
int mpg_bjacobi_apply_f64_p32(mpg_ctx_t c, int64_t n, int32_t bs, const float* dinv, double* x) {
    return apply_impl<double, float>(c, n, bs, dinv, x);
}

}  // extern "C"
