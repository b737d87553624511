// CSR SpMV on gfx950 (replaces mkl_sparse_?_mv, kernels_mkl.cpp:326-352, and
// legacy cusparse?csrmv, kernels_cuda.cpp:576-614) + Jacobi setup
// (types.hpp:393-431).
//
// CSR-adaptive schedule. mpg_csr_create splits the rows into "row blocks":
// consecutive rows whose total nnz fits kNnzCap (streamed through LDS), or a
// single row (long-row mode: the whole workgroup reduces it). One 256-lane
// workgroup per row block:
//   stream mode: lanes load (val, col) contiguously — every wave instruction
//     touches 64 consecutive nonzeros — gather x[col], form the fp64 product
//     and stage it in LDS; then one lane per row sums its LDS segment in
//     column order (a segmented reduction with no cross-lane traffic);
//   row mode: strided fp64 partial sums, wave64 shuffle + LDS tree.
// Products and sums are fp64 for every precision (exact products for fp32
// and fp16 values); the row sum is rounded once to the vector type, then
// y = alpha*sum (+ beta*y when beta != 0).
#include "csr_tile.hpp"
#include "internal.hpp"

#include <cfloat>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace mpg;


namespace {

template <class V, class X>
__global__ __launch_bounds__(kBlock) void k_csr_adaptive(const int32_t* __restrict__ blocks,
                                                         const int32_t* __restrict__ bnnz,
                                                         const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const V* __restrict__ val, int64_t nnz,
                                                         const X* __restrict__ x, X alpha, X beta,
                                                         X* __restrict__ y) {
    __shared__ double prod[kNnzCap];
    __shared__ double scratch[kBlock / kWave];
    const int b = blockIdx.x;
    csr_row_block(
        blocks[b], blocks[b + 1], bnnz[b], bnnz[b + 1], rowptr, col, val, nnz, [&](int c) { return (double)x[c]; },
        [&](int i) { return beta == X(0) ? X(0) : y[i]; },
        [&](int i, double sum, X yi) {
            const X t = (X)sum;
            y[i] = spmv_axpby(alpha, t, beta, yi);
        },
        prod, scratch);
}

// fp16 values scaled per row (mpg_csr_half_values): the row sum times 2^-e_i
template <class X>
__global__ __launch_bounds__(kBlock) void k_csr_adaptive_scaled(const int32_t* __restrict__ blocks,
                                                                const int32_t* __restrict__ bnnz,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const uint16_t* __restrict__ val, int64_t nnz,
                                                                const int8_t* __restrict__ rexp,
                                                                const X* __restrict__ x, X alpha, X beta,
                                                                X* __restrict__ y) {
    __shared__ double prod[kNnzCap];
    __shared__ double scratch[kBlock / kWave];
    struct Pre {
        X yi;
        int e;
    };
    const int b = blockIdx.x;
    csr_row_block(
        blocks[b], blocks[b + 1], bnnz[b], bnnz[b + 1], rowptr, col, val, nnz, [&](int c) { return (double)x[c]; },
        [&](int i) { return Pre{beta == X(0) ? X(0) : y[i], (int)rexp[i]}; },
        [&](int i, double sum, const Pre& p) {
            const X t = (X)ldexp(sum, -p.e);
            y[i] = spmv_axpby(alpha, t, beta, p.yi);
        },
        prod, scratch);
}

template <class V, class X>
int spmv_impl(mpg_ctx* ctx, mpg_csr* A, X alpha, const V* vals, const X* x, X beta, X* y,
              const int8_t* rexp = nullptr) {
    if (!ctx || !A) return MPG_ERR_ARG;
    if (A->rows == 0) return MPG_OK;
    if constexpr (std::is_same_v<V, uint16_t>) {
        if (rexp) {
            k_csr_adaptive_scaled<X><<<A->nblocks, kBlock, 0, ctx->stream>>>(
                A->blocks, A->bnnz, A->rowptr, A->col, vals, A->nnz, rexp, x, alpha, beta, y);
            MPG_LAUNCH_CHECK(ctx);
            return MPG_OK;
        }
    }
    k_csr_adaptive<V, X><<<A->nblocks, kBlock, 0, ctx->stream>>>(A->blocks, A->bnnz, A->rowptr, A->col, vals, A->nnz, x,
                                                                 alpha, beta, y);
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

// ---------------- fp16 values with power-of-two row scaling ----------------
// One thread per row: the row's largest finite |a|, its exponent e (0 when
// the row is in range), then half(float(a * 2^e)) for each entry, counting
// what the cast loses (stats: rows scaled, flushed to 0, overflowed, e out
// of int8). mpg_csr_half_values, capi.h.
constexpr int kHalfRowLo = -2, kHalfRowHi = 14, kHalfRowTop = 14;

__global__ __launch_bounds__(kBlock) void k_half_rows(int32_t rows, const int32_t* __restrict__ rowptr,
                                                      const double* __restrict__ val, int scale,
                                                      uint16_t* __restrict__ out, int8_t* __restrict__ rexp,
                                                      unsigned long long* __restrict__ stats) {
    unsigned long long cnt[4] = {0, 0, 0, 0};
    const int stride = gridDim.x * kBlock;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        const int j0 = rowptr[i], j1 = rowptr[i + 1];
        double m = 0.0;
        for (int j = j0; j < j1; ++j) {
            const double a = fabs(val[j]);
            if (a <= DBL_MAX && a > m) m = a;
        }
        int e = 0;
        if (scale && m > 0.0) {
            const int E = ilogb(m);
            if (E < kHalfRowLo || E > kHalfRowHi) e = kHalfRowTop - E;
            if (e < -127 || e > 127) {
                ++cnt[3];
                e = 0;
            }
        }
        cnt[0] += e != 0;
        if (rexp) rexp[i] = (int8_t)e;
        for (int j = j0; j < j1; ++j) {
            const double a = val[j];
            // fp64 -> fp32 -> fp16, two roundings as mpg_copy_f64f16 (and
            // numpy's astype chain); the empty asm keeps the compiler from
            // folding the pair into one fp64 -> fp16 rounding, which it did
            // here (66 of BAND-100k's 1M entries differed)
            float f = (float)ldexp(a, e);
            asm volatile("" : "+v"(f));
            const uint16_t h = __half_as_ushort(__float2half_rn(f));
            if (fabs(a) <= DBL_MAX) {
                cnt[1] += a != 0.0 && (h & 0x7fffu) == 0;
                cnt[2] += (h & 0x7fffu) == 0x7c00u;
            }
            out[j] = h;
        }
    }
    for (int q = 0; q < 4; ++q)
        if (cnt[q]) atomicAdd(stats + q, cnt[q]);
}

// The scaled fp16 values back as fp32, one thread per row: float(half) 2^-e,
// exact unless it leaves fp32's range (counted when it overflows).
// mpg_csr_half_dequant_f32, capi.h.
__global__ __launch_bounds__(kBlock) void k_half_dequant(int32_t rows, const int32_t* __restrict__ rowptr,
                                                         const uint16_t* __restrict__ val,
                                                         const int8_t* __restrict__ rexp, float* __restrict__ out,
                                                         unsigned long long* __restrict__ bad) {
    unsigned long long cnt = 0;
    const int stride = gridDim.x * kBlock;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        const int e = rexp[i];
        for (int j = rowptr[i], j1 = rowptr[i + 1]; j < j1; ++j) {
            const float h = to_float(val[j]);
            const float f = ldexpf(h, -e);
            cnt += fabsf(h) <= FLT_MAX && !(fabsf(f) <= FLT_MAX);
            if (out) out[j] = f;
        }
    }
    if (cnt) atomicAdd(bad, cnt);
}

// ---------------- Jacobi setup (types.hpp:393-431) ----------------
template <class T>
__global__ __launch_bounds__(kBlock) void k_rowabs_max(int32_t rows, const int32_t* __restrict__ rowptr,
                                                       const T* __restrict__ val, double* __restrict__ partial) {
    __shared__ double scratch[kBlock / kWave];
    double m = 0.0;
    const int stride = gridDim.x * kBlock;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        T sum = 0;  // summed in the values' precision, as the Kokkos lambda does
        for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) sum += fabs(val[k]);
        m = (double)sum > m ? (double)sum : m;
    }
    double bm = block_max<kBlock>(m, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = bm;
}

__global__ __launch_bounds__(1024) void k_rowmax_final(int nparts, const double* __restrict__ partial,
                                                       double* __restrict__ out) {
    __shared__ double scratch[1024 / kWave];
    double v = threadIdx.x < nparts ? partial[threadIdx.x] : 0.0;
    double m = block_max<1024>(v, scratch);
    if (threadIdx.x == 0) *out = m;  // exact: one of the row sums
}

// rows are the local rows; columns >= rows are halo entries (row-partitioned
// matrix), which sort before the own columns when their global id is lower
template <class T>
__global__ __launch_bounds__(kBlock) void k_jacobi_diag(int32_t rows, int64_t nnz, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, const T* __restrict__ val,
                                                        const double* __restrict__ rowmax, T* __restrict__ diag) {
    T alpha = (T)*rowmax;
    alpha *= (T)FLT_EPSILON;  // alpha *= numeric_limits<float>::epsilon() (types.hpp:417)
    const int stride = gridDim.x * kBlock;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        int64_t j = rowptr[i];
        // `while (inds(j) < i) ++j;` (types.hpp:422-425), bounded so a row
        // without a diagonal cannot run off the arrays; a leading run of
        // lower-numbered halo columns is skipped first
        while (j < nnz - 1 && j < rowptr[i + 1] - 1 && col[j] >= rows) ++j;
        while (j < nnz - 1 && col[j] < i) ++j;
        const T v = val[j];
        if (v >= T(0)) diag[i] = T(1) / ((v < alpha) ? alpha : v);
        else diag[i] = T(1) / ((v > -alpha) ? -alpha : v);
    }
}

template <class T>
int rowmax_impl(mpg_ctx* ctx, mpg_csr* A, const T* vals, double* out) {
    if (!ctx || !A || !out) return MPG_ERR_ARG;
    int g = grid_for(A->rows > 0 ? A->rows : 1, 1, kMaxRedBlocks);
    k_rowabs_max<T><<<g, kBlock, 0, ctx->stream>>>(A->rows, A->rowptr, vals, ctx->red_ws);
    MPG_LAUNCH_CHECK(ctx);
    k_rowmax_final<<<1, 1024, 0, ctx->stream>>>(g, ctx->red_ws, out);
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

template <class T>
int jdiag_impl(mpg_ctx* ctx, mpg_csr* A, const T* vals, const double* rowmax, T* diag) {
    if (!ctx || !A || !rowmax) return MPG_ERR_ARG;
    if (A->rows == 0) return MPG_OK;
    k_jacobi_diag<T><<<grid_for(A->rows, 1), kBlock, 0, ctx->stream>>>(A->rows, A->nnz, A->rowptr, A->col, vals,
                                                                      rowmax, diag);
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

template <class T>
int jacobi_impl(mpg_ctx* ctx, mpg_csr* A, const T* vals, T* diag) {
    if (!ctx || !A) return MPG_ERR_ARG;
    if (A->rows == 0) return MPG_OK;
    double* rowmax = ctx->red_ws + (size_t)kMaxRedBlocks * kGemvMaxCols + 16;
    int st = rowmax_impl<T>(ctx, A, vals, rowmax);
    if (st) return st;
    return jdiag_impl<T>(ctx, A, vals, rowmax, diag);
}

}  // namespace

extern "C" {

int mpg_csr_create(mpg_ctx_t ctx, int32_t rows, int32_t cols, int64_t nnz, const int32_t* rowptr_host,
                   const int32_t* rowptr_dev, const int32_t* col_dev, mpg_csr_t* out) {
    if (!ctx || !out || rows < 0 || cols < 0 || nnz < 0 || nnz > INT32_MAX || !rowptr_host) return MPG_ERR_ARG;
    *out = nullptr;
    if (rowptr_host[0] != 0 || rowptr_host[rows] != nnz) return MPG_ERR_ARG;
    std::vector<int32_t> starts;
    starts.reserve(rows / 64 + 2);
    int32_t r = 0;
    while (r < rows) {
        starts.push_back(r);
        const int64_t base = rowptr_host[r];
        int32_t q = r + 1;
        if (rowptr_host[q] - base <= kNnzCap) {
            while (q < rows && q - r < kRowCap && rowptr_host[q + 1] - base <= kNnzCap) ++q;
        }
        r = q;
    }
    starts.push_back(rows);
    mpg_csr* A = new (std::nothrow) mpg_csr();
    if (!A) return MPG_ERR_ALLOC;
    A->ctx = ctx;
    A->rows = rows;
    A->cols = cols;
    A->nnz = nnz;
    A->rowptr = rowptr_dev;
    A->col = col_dev;
    A->nblocks = (int)starts.size() - 1;
    const size_t nb = starts.size();
    for (size_t b = 0; b < nb; ++b) starts.push_back(rowptr_host[starts[b]]);  // nnz start of each block
    hipError_t e = hipMalloc(&A->blocks, starts.size() * sizeof(int32_t));
    if (e == hipSuccess)
        e = hipMemcpy(A->blocks, starts.data(), starts.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    A->bnnz = A->blocks + nb;
    if (e != hipSuccess) {
        if (A->blocks) (void)hipFree(A->blocks);
        delete A;
        return set_hip_error(ctx, e, "mpg_csr_create");
    }
    *out = A;
    return MPG_OK;
}

int mpg_csr_destroy(mpg_csr_t A) {
    if (!A) return MPG_OK;
    if (A->ctx) (void)hipStreamSynchronize(A->ctx->stream);
    if (A->blocks) (void)hipFree(A->blocks);
    delete A;
    return MPG_OK;
}

int mpg_csr_num_blocks(mpg_csr_t A) { return A ? A->nblocks : -1; }

int mpg_csr_spmv_f64(mpg_ctx_t c, mpg_csr_t A, double alpha, const double* vals, const double* x, double beta, double* y) {
    return spmv_impl<double, double>(c, A, alpha, vals, x, beta, y);
}
int mpg_csr_spmv_f32(mpg_ctx_t c, mpg_csr_t A, float alpha, const float* vals, const float* x, float beta, float* y) {
    return spmv_impl<float, float>(c, A, alpha, vals, x, beta, y);
}
int mpg_csr_spmv_f16f32(mpg_ctx_t c, mpg_csr_t A, float alpha, const uint16_t* vals, const float* x, float beta, float* y) {
    return spmv_impl<uint16_t, float>(c, A, alpha, vals, x, beta, y);
}
int mpg_csr_spmv_f16f32_scaled(mpg_ctx_t c, mpg_csr_t A, float alpha, const uint16_t* vals, const int8_t* row_exp,
                               const float* x, float beta, float* y) {
    if (!row_exp) return MPG_ERR_ARG;
    return spmv_impl<uint16_t, float>(c, A, alpha, vals, x, beta, y, row_exp);
}

int mpg_csr_half_values(mpg_ctx_t c, mpg_csr_t A, const double* vals, int32_t scale, uint16_t* out, int8_t* row_exp,
                        int64_t* stats) {
    if (!c || !A || (A->nnz > 0 && (!vals || !out)) || (scale && !row_exp)) return MPG_ERR_ARG;
    int64_t h[4] = {0, 0, 0, 0};
    if (A->rows > 0) {
        unsigned long long* d = reinterpret_cast<unsigned long long*>(c->red_ws);
        if (hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), c->stream) != hipSuccess) return MPG_ERR_HIP;
        k_half_rows<<<grid_for(A->rows, 1), kBlock, 0, c->stream>>>(A->rows, A->rowptr, vals, scale ? 1 : 0, out,
                                                                    row_exp, d);
        MPG_LAUNCH_CHECK(c);
        if (hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return MPG_ERR_HIP;
    }
    if (stats)
        for (int q = 0; q < 4; ++q) stats[q] = h[q];
    if (h[2] || h[3] || (!scale && h[1])) {
        c->last_error = "fp16 values: " + std::to_string(h[2]) + " entries overflow, " + std::to_string(h[1]) +
                        " nonzero entries round to 0, " + std::to_string(h[3]) + " row exponents out of range" +
                        (scale ? "" : " (row scaling off)");
        return MPG_ERR_RANGE;
    }
    return MPG_OK;
}

int mpg_csr_half_dequant_f32(mpg_ctx_t c, mpg_csr_t A, const uint16_t* vals, const int8_t* row_exp, float* out,
                             int64_t* nonfinite) {
    if (!c || !A || !nonfinite || (A->nnz > 0 && !vals) || (A->rows > 0 && !row_exp)) return MPG_ERR_ARG;
    *nonfinite = 0;
    if (A->rows == 0) return MPG_OK;
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c->red_ws);
    unsigned long long h = 0;
    if (hipMemsetAsync(d, 0, sizeof h, c->stream) != hipSuccess) return MPG_ERR_HIP;
    k_half_dequant<<<grid_for(A->rows, 1), kBlock, 0, c->stream>>>(A->rows, A->rowptr, vals, row_exp, out, d);
    MPG_LAUNCH_CHECK(c);
    if (hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return MPG_ERR_HIP;
    *nonfinite = (int64_t)h;
    return MPG_OK;
}

int mpg_jacobi_rowmax_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, double* out) { return rowmax_impl<double>(c, A, vals, out); }
int mpg_jacobi_rowmax_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, double* out) { return rowmax_impl<float>(c, A, vals, out); }
int mpg_jacobi_diag_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, const double* rm, double* d) { return jdiag_impl<double>(c, A, vals, rm, d); }
int mpg_jacobi_diag_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, const double* rm, float* d) { return jdiag_impl<float>(c, A, vals, rm, d); }
int mpg_jacobi_setup_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, double* diag) { return jacobi_impl<double>(c, A, vals, diag); }
int mpg_jacobi_setup_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, float* diag) { return jacobi_impl<float>(c, A, vals, diag); }

}  // extern "C"
