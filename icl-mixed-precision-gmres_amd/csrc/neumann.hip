// Jacobi sweeps on A z = r: the truncated Neumann series
//
//   M^-1 = sum_{j < s} (I - D A)^j D,    D the Jacobi inverse diagonal,
//
// applied as z_1 = D r (mpg_gdmv_*) and z_{j+1} = z_j + D (r - A z_j). One
// launch per sweep: for every row i
//
//   z_out[i] = z_in[i] + d[i] * (r[i] - s_i),   s_i = T(sum_j a_ij z_in[j])
//
// The row sum is the SpMV's of the same storage, value type and accumulation
// class (csr_tile.hpp / sell_tile.hpp: the bits of mpg_csr_spmv_* /
// mpg_sell_spmv_* at alpha = 1, beta = 0, and of the Arnoldi SpMV under the
// fp32 class); the epilogue is three separately rounded operations in T.
// z_out may alias r (row i's lane alone reads r[i], before its store), never
// z_in (other rows gather it).
//
// The SELL form runs one slice per wave and gathers z_in from memory for
// every copy (int32, int16, stepped and implicit columns, sorted rows, the
// stepped form's CSR-summed slices), in XCD slice order: the row sum's order
// does not depend on the SpMV's window or pair forms, so the bits are theirs.
#include "arnoldi_kernels.hpp"

#include <type_traits>

using namespace mpg;

namespace {

// t = r - s; u = d * t; z + u: each rounded to T
template <class T>
__device__ __forceinline__ T sweep_update(T s, T r, T d, T z) {
#pragma clang fp contract(off)
    const T t = r - s;
    const T u = d * t;
    return z + u;
}

template <class T>
struct SweepOps {
    T r, d, z;
};

// (r and z_out carry no __restrict__: they may be one vector)
template <class T, class A>
__global__ __launch_bounds__(kBlock) void k_csr_sweep(const int32_t* __restrict__ blocks, int nblocks,
                                                      const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const T* __restrict__ val,
                                                      int64_t nnz, const T* __restrict__ dinv, const T* r,
                                                      const T* __restrict__ z_in, T* z_out) {
    __shared__ double prod[kNnzCap];
    __shared__ double scratch[kBlock / kWave];
    for_rows<false, false, A>(
        blocks, nblocks, rowptr, col, val, nnz, [&](int c) { return (double)z_in[c]; },
        [&](int i) { return SweepOps<T>{r[i], dinv[i], z_in[i]}; },
        [&](int i, A sum, const SweepOps<T>& o) { z_out[i] = sweep_update((T)sum, o.r, o.d, o.z); }, prod, scratch);
}

template <class T, class CI, int W, bool UNI, class A>
__global__ __launch_bounds__(kBlock) void k_sell_sweep(int n, int nslices, const int64_t* __restrict__ off,
                                                       const CI* __restrict__ col, const T* __restrict__ val,
                                                       const int32_t* __restrict__ sbase,
                                                       const int32_t* __restrict__ spat,
                                                       const int64_t* __restrict__ coff, const CI* __restrict__ pat,
                                                       const int32_t* __restrict__ xrp,
                                                       const int32_t* __restrict__ xcol, const T* __restrict__ xval,
                                                       const T* __restrict__ dinv, const T* r,
                                                       const T* __restrict__ z_in, T* z_out, int64_t ustride, int xcd,
                                                       const int32_t* __restrict__ rows) {
    const int lane = threadIdx.x & (kWave - 1), wid = wave_id();
    const int s = (xcd ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x) * (kBlock / kWave) + wid;
    if (s >= nslices) return;  // (no workgroup barrier below)
    const int row0 = s * kWave;
    SellRow<T, CI, W> row;
    if constexpr (UNI) row.init_uniform(s, ustride, spat, coff);
    else row.init_load(s, off, spat, coff);
    __builtin_amdgcn_sched_barrier(0);
    // the lane's row (a sorted copy's rows[]) and its epilogue operands, issued ahead of the slice
    const int i = rows ? rows[row0 + lane] : row0 + lane;
    const int ic = i < n ? i : 0;
    const SweepOps<T> o{r[ic], dinv[ic], z_in[ic]};
    __builtin_amdgcn_sched_barrier(0);
    row.init_finish(lane, col, val, sbase, pat);
    row.load(0);
    __builtin_amdgcn_sched_barrier(0);
    auto xv = [&](int c) { return (double)z_in[c]; };
    A sum = A(0);
    if (SellCol<CI>::stepped && row.exc) {
        sum = csr_row_sum<A>(i < n ? row.xrow : -1, xrp, xcol, xval, xv);
    } else {
        row.sum(0, xv, sum);
        for (int q = row.U; q < row.steps; q += row.U) {
            row.load(q);
            row.sum(q, xv, sum);
        }
    }
    if (i < n) z_out[i] = sweep_update((T)sum, o.r, o.d, o.z);
}

template <class T, class A>
int csr_sweep(mpg_ctx* ctx, const mpg_csr* M, int grid, const T* vals, const T* dinv, const T* r, const T* z_in,
              T* z_out) {
    if (M->rows == 0) return MPG_OK;
    k_csr_sweep<T, A><<<grid, kBlock, 0, ctx->stream>>>(M->blocks, M->nblocks, M->rowptr, M->col, vals, M->nnz, dinv, r,
                                                        z_in, z_out);
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

template <class T, class A>
int sell_sweep(mpg_ctx* ctx, const SellCopy& S, const T* dinv, const T* r, const T* z_in, T* z_out) {
    if (S.nslices == 0) return MPG_OK;
    const int grid = (S.nslices + kBlock / kWave - 1) / (kBlock / kWave);
    const char* xe = std::getenv("MPG_SELL_XCD");
    const int xcd = xe && *xe == '0' ? 0 : 1;
    int st = sell_dispatch(S, [&](auto ci, auto wc) {
        using CI = decltype(ci);
        constexpr int Wc = decltype(wc)::value;
        auto go = [&](auto kern) {
            kern<<<grid, kBlock, 0, ctx->stream>>>(S.n, S.nslices, S.off, static_cast<const CI*>(S.col),
                                                   static_cast<const T*>(S.val), S.sbase, S.spat, S.coff,
                                                   static_cast<const CI*>(S.pat), S.xrp, S.xcol,
                                                   static_cast<const T*>(S.xval), dinv, r, z_in, z_out, S.ustride, xcd,
                                                   S.rows);
            return (int)MPG_OK;
        };
        return sell_uniform(S) ? go(k_sell_sweep<T, CI, Wc, true, A>) : go(k_sell_sweep<T, CI, Wc, false, A>);
    });
    if (st) return st;
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

template <class T>
int csr_sweep_api(mpg_ctx* ctx, mpg_csr* M, const T* vals, const T* dinv, const T* r, const T* z_in, T* z_out) {
    if (!ctx || !M || M->rows != M->cols || (M->nnz > 0 && !vals)) return MPG_ERR_ARG;
    if (M->rows > 0 && (!dinv || !r || !z_in || !z_out || z_out == z_in)) return MPG_ERR_ARG;
    return csr_sweep<T, double>(ctx, M, M->nblocks, vals, dinv, r, z_in, z_out);
}

template <class T, int VT>
int sell_sweep_api(mpg_ctx* ctx, mpg_sell* M, const T* dinv, const T* r, const T* z_in, T* z_out) {
    if (!ctx || !M || M->S.vtype != VT || M->cols != M->S.n) return MPG_ERR_ARG;
    if (M->S.n > 0 && (!dinv || !r || !z_in || !z_out || z_out == z_in)) return MPG_ERR_ARG;
    return sell_sweep<T, double>(ctx, M->S, dinv, r, z_in, z_out);
}

template <class T>
int gdmv_t(mpg_ctx* ctx, int64_t n, const T* d, const T* x, T* y) {
    if constexpr (std::is_same_v<T, double>) return mpg_gdmv_f64(ctx, n, 1.0, d, x, 0.0, y);
    else return mpg_gdmv_f32(ctx, n, 1.0f, d, x, 0.0f, y);
}

// z_1 = D w (into w for one step, else into work0), then the sweeps between
// the work vectors with w as r; the last one stores into w
template <class T, class A>
int neumann_run(mpg_arnoldi* a, int steps, T* w, T* work0, T* work1) {
    mpg_ctx* ctx = a->ctx;
    const T* d = static_cast<const T*>(a->d.diag);
    const int n = a->d.n;
    if (int st = gdmv_t<T>(ctx, n, d, w, steps == 1 ? w : work0)) return st;
    T* bufs[2] = {work0, work1};
    for (int j = 1; j < steps; ++j) {
        const T* z_in = bufs[(j - 1) & 1];
        T* z_out = j == steps - 1 ? w : bufs[j & 1];
        const int st = a->sell.nslices > 0
                           ? sell_sweep<T, A>(ctx, a->sell, d, w, z_in, z_out)
                           : csr_sweep<T, A>(ctx, a->d.A, a->Grb, static_cast<const T*>(a->d.val_inner), d, w, z_in,
                                             z_out);
        if (st) return st;
    }
    return MPG_OK;
}

}  // namespace

extern "C" {

int mpg_csr_jacobi_sweep_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, const double* dinv, const double* r,
                             const double* z_in, double* z_out) {
    return csr_sweep_api<double>(c, A, vals, dinv, r, z_in, z_out);
}
int mpg_csr_jacobi_sweep_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, const float* dinv, const float* r,
                             const float* z_in, float* z_out) {
    return csr_sweep_api<float>(c, A, vals, dinv, r, z_in, z_out);
}
int mpg_sell_jacobi_sweep_f64(mpg_ctx_t c, mpg_sell_t A, const double* dinv, const double* r, const double* z_in,
                              double* z_out) {
    return sell_sweep_api<double, MPG_F64>(c, A, dinv, r, z_in, z_out);
}
int mpg_sell_jacobi_sweep_f32(mpg_ctx_t c, mpg_sell_t A, const float* dinv, const float* r, const float* z_in,
                              float* z_out) {
    return sell_sweep_api<float, MPG_F32>(c, A, dinv, r, z_in, z_out);
}

int mpg_arnoldi_neumann_apply(mpg_arnoldi_t a, int32_t steps, void* w, void* work0, void* work1) {
    if (!a || !a->ctx || steps < 1 || steps > 64 || !w || (steps >= 2 && !work0) || (steps >= 3 && !work1) ||
        (steps >= 2 && work0 == w) || (steps >= 3 && (work1 == w || work1 == work0)) || !a->d.diag)
        return MPG_ERR_ARG;
    // an fp32 or fp64 Arnoldi on values of its own type, preconditioner precision = T, one GPU's rows
    if ((a->combo != 0 && a->combo != 2 && a->combo != 3) || a->front != 0 || a->d.n_ext != a->d.n)
        return MPG_ERR_UNSUPPORTED;
    if (a->d.n == 0) return MPG_OK;
    if (a->combo == 0)
        return neumann_run<double, double>(a, steps, static_cast<double*>(w), static_cast<double*>(work0),
                                           static_cast<double*>(work1));
    if (a->acc32)
        return neumann_run<float, float>(a, steps, static_cast<float*>(w), static_cast<float*>(work0),
                                         static_cast<float*>(work1));
    return neumann_run<float, double>(a, steps, static_cast<float*>(w), static_cast<float*>(work0),
                                      static_cast<float*>(work1));
}

}  // extern "C"
