// The prologue of a restart cycle (true residual + preconditioner + norms)
// on CSR row blocks, node blocks and SELL-64 slices, and the row-block walk
// (for_rows) and preconditioner application the SpMV kernels share with it.
#pragma once

#include "arnoldi_reduce.hpp"
#include "csr_tile.hpp"
#include "node_tile.hpp"
#include "sell_tile.hpp"
#include "panel.hpp"

namespace {

// Jacobi / identity preconditioner in precision P applied to a T value:
// typesafe_apply (gmres.cpp:12-22) + gdmv(1, d, w, 0, w) (kernels.hpp:141-144).
template <class T, class P>
__device__ __forceinline__ T precond(T w, const P* __restrict__ d, int64_t i) {
    P p = (P)w;
    if (d) p = P(0) * p + P(1) * d[i] * p;
    return (T)p;
}

// This workgroup's contiguous run of row blocks [rb0, rb1) — contiguous so
// that its rows form one range [blocks[rb0], blocks[rb1]) for the dot pass.
__device__ __forceinline__ void my_blocks(int nblocks, int& rb0, int& rb1, bool xcd = false) {
    const int b = xcd ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    rb0 = (int)((int64_t)b * nblocks / gridDim.x);
    rb1 = (int)((int64_t)(b + 1) * nblocks / gridDim.x);
}

// For every row of this workgroup's row blocks: fp64 sum of val * xval(col)
// (csr_tile.hpp), then epi(row, sum) on one lane. NT: non-temporal matrix
// loads (a pass that runs once per restart cycle).
// XCD (round 5): workgroups take their runs of row blocks in XCD order
// (xcd_block), so each XCD's L2 holds the neighbourhood of x that its own
// contiguous eighth of the rows gathers (the SELL kernels' placement).
template <bool NT = false, bool XCD = false, class A = double, class V, class XF, class PF, class EPI>
__device__ __forceinline__ void for_rows(const int32_t* __restrict__ blocks, int nblocks,
                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                         const V* __restrict__ val, int64_t nnz, XF xval, PF pre, EPI epi,
                                         double* prod, double* scratch) {
    const int32_t* __restrict__ bnnz = blocks + nblocks + 1;  // mpg_csr's nnz starts follow the row starts
    int rb0, rb1;
    my_blocks(nblocks, rb0, rb1, XCD);
    for (int b = rb0; b < rb1; ++b)
        csr_row_block<NT, A>(blocks[b], blocks[b + 1], bnnz[b], bnnz[b + 1], rowptr, col, val, nnz, xval, pre, epi,
                             prod, scratch);
}

// ---------------------------------------------------------------- prologue
// r = b - A x (X), w = M(T(r)); partials: ||T(r)||^2, ||w||^2, ||x||^2
template <class T, class X, class P>
__global__ __launch_bounds__(kBlock) void k_prologue(const int32_t* __restrict__ blocks, int nblocks,
                                                     const int32_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col, const X* __restrict__ val,
                                                     int64_t nnz, const X* __restrict__ x, const X* __restrict__ b,
                                                     const P* __restrict__ diag, T* __restrict__ w,
                                                     double* __restrict__ partial) {
    __shared__ double prod[kNnzCap];
    __shared__ double scratch[kBlock / kWave];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    struct Ops {
        X b, x;
        P d;
    };
    for_rows<true>(  // once per cycle: keep V and the Arnoldi matrix cached
        blocks, nblocks, rowptr, col, val, nnz, [&](int c) { return (double)x[c]; },
        [&](int i) { return Ops{b[i], x[i], diag ? diag[i] : P(0)}; },
        [&](int i, double sum, const Ops& o) {
            const X bi = o.b, xi = o.x;
            const P di = o.d;
            const X t = (X)sum;
            const X r = bi - t;  // copy(b, w); spmv(-1, A, x, 1, w)
            T wi = (T)r;
            acc[0] += (double)wi * (double)wi;
            P pw = (P)wi;  // = precond<T, P> (typesafe_apply's rounding to P included)
            if (diag) pw = P(0) * pw + P(1) * di * pw;
            wi = (T)pw;
            acc[1] += (double)wi * (double)wi;
            acc[2] += (double)xi * (double)xi;
            w[i] = wi;
        },
        prod, scratch);
    store_partials<4>(acc, 3, partial);
}

// The residual prologue on node blocks (round 6), in two launches whose
// arithmetic is k_prologue's: k_node_rowsums forms every row's fp64 sum of
// A x on the node copy of the outer values (the CSR tile's products in CSR
// storage order, node_tile.hpp), then k_prologue_rows runs k_prologue's
// epilogue on those sums with k_prologue's grid, row blocks and lane-to-row
// map (for_rows / csr_row_block: lane t takes rows r0 + t, r0 + t + 256, ...
// of each of its workgroup's blocks), so every lane's three norm partials
// add the same terms in the same order and the cycle keeps the CSR bits.
// (A single row past kNnzCap, csr_row_block's tree-summed row mode, cannot
// occur: a node row holds at most kNodeCap blocks.) fem27 / C4: 8.9 B per
// nonzero of fp64 records against CSR's 12.
template <class X>
__global__ __launch_bounds__(kBlock) void k_node_rowsums(const int32_t* __restrict__ tiles,
                                                         const int32_t* __restrict__ bptr,
                                                         const char* __restrict__ recs, int ntiles, int64_t nblk,
                                                         int tpw, int xcd, const X* __restrict__ x,
                                                         double* __restrict__ rsum) {
    __shared__ double prod[kNodeProd];
    const int g = xcd ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int t0 = g * tpw, t1 = t0 + tpw < ntiles ? t0 + tpw : ntiles;
    node_tiles<X>(
        t0, t1, tiles, tiles + ntiles + 1, bptr, recs, nblk, [&](int c) { return x[c]; },
        [&](X v) { return (double)v; }, [&](int) { return 0; }, [&](int i, double sum, int) { rsum[i] = sum; },
        prod);
}

// BJ: `diag` holds the 3 x 3 inverses of the nodes' diagonal blocks (block
// Jacobi, mpg_bjacobi_setup_*) and w = Dinv T(r): each lane forms T(r) of its
// node's three rows from the same sums and applies its own row of the
// inverse with mpg_bjacobi_apply_*'s arithmetic (products rounded, summed
// left to right), so w has the bits of that launch run on the plain prologue.
template <class T, class X, class P, bool BJ = false>
__global__ __launch_bounds__(kBlock) void k_prologue_rows(const int32_t* __restrict__ blocks, int nblocks,
                                                          const double* __restrict__ rsum,
                                                          const X* __restrict__ x, const X* __restrict__ b,
                                                          const P* __restrict__ diag, T* __restrict__ w,
                                                          double* __restrict__ partial) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    auto epi = [&](int i) {  // k_prologue's epilogue, on the same sum
        const X t = (X)rsum[i];
        const X r = b[i] - t;
        T wi = (T)r;
        acc[0] += (double)wi * (double)wi;
        P pw = (P)wi;
        if constexpr (BJ) {
#pragma clang fp contract(off)
            const int q = i / kNodeDof * kNodeDof, kk = i - q;
            const P* d = diag + (int64_t)q * kNodeDof + kNodeDof * kk;
            const P own = pw;
            auto tr = [&](int j) { return j == i ? own : (P)(T)(X)(b[j] - (X)rsum[j]); };
            pw = d[0] * tr(q);
            const P p1 = d[1] * tr(q + 1);
            pw = pw + p1;
            const P p2 = d[2] * tr(q + 2);
            pw = pw + p2;
        } else {
            if (diag) pw = P(0) * pw + P(1) * diag[i] * pw;
        }
        wi = (T)pw;
        acc[1] += (double)wi * (double)wi;
        acc[2] += (double)x[i] * (double)x[i];
        w[i] = wi;
    };
    int rb0, rb1;
    my_blocks(nblocks, rb0, rb1);
    for (int bk = rb0; bk < rb1; ++bk) {
        const int r0 = blocks[bk], r1 = blocks[bk + 1];
        for (int r = threadIdx.x; r < r1 - r0; r += kBlock) epi(r0 + r);
    }
    store_partials<4>(acc, 3, partial);
}

// The same prologue on a SELL-64 copy of the outer-precision values (one
// wave per slice, one lane per row; loads issued in need order as in
// k_step_sell): r = b - A x (X), w = M(T(r)), partials ||T(r)||^2,
// ||w||^2, ||x||^2 per workgroup.
template <class T, class X, class P, class CI, int W, bool WIN, bool UNI = false>
__global__ __launch_bounds__(kBlock) void k_prologue_sell(int n, int n_lo, int n_ext, int nslices, const int64_t* __restrict__ off,
                                                          const CI* __restrict__ col, const X* __restrict__ val,
                                                          const X* __restrict__ x, const X* __restrict__ b,
                                                          const P* __restrict__ diag, T* __restrict__ w,
                                                          double* __restrict__ partial,
                                                          const int32_t* __restrict__ sbase,
                                                          const int32_t* __restrict__ spat, const int64_t* __restrict__ coff, const CI* __restrict__ pat,
                                                          const int32_t* __restrict__ xrp,
                                                          const int32_t* __restrict__ xcol,
                                                          const X* __restrict__ xval, int64_t ustride, int xcd,
                                                          const int32_t* __restrict__ rows) {
    constexpr int NQ = kWinLen / kWave;
    __shared__ X win[WIN ? kBlock / kWave : 1][WIN ? kWinLen : 1];
    const int lane = threadIdx.x & (kWave - 1), wid = wave_id();
    const int s = (xcd ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x) * (kBlock / kWave) + wid;
    const bool live = s < nslices;  // a dead wave still joins the partials' barrier
    const int row0 = s * kWave;
    // the lane's row (a sorted SELL-C-sigma copy: rows[], padding lanes n)
    const int i = rows ? rows[live ? row0 + lane : 0] : row0 + lane;
    const bool own = live && i < n;
    SellRow<X, CI, W, true> row;  // once per cycle: non-temporal slices
    if constexpr (UNI) row.init_uniform(live ? s : 0, ustride, spat, coff);
    else row.init_load(live ? s : 0, off, spat, coff);
    __builtin_amdgcn_sched_barrier(0);
    X xr[WIN ? NQ : 1];
    if constexpr (WIN) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = row0 - kWinLo + q * kWave + lane;
            xr[q] = x[c >= n_lo && c < n_ext ? c : 0];
        }
    }
    const int ic = own ? i : 0;
    const X bi = b[ic], xi = x[ic];
    const P di = diag ? diag[ic] : P(0);
    __builtin_amdgcn_sched_barrier(0);
    row.init_finish(lane, col, val, sbase, pat);
    row.load(0);
    __builtin_amdgcn_sched_barrier(0);
    double sum = 0.0;
    if (live) {
        if constexpr (WIN) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = row0 - kWinLo + q * kWave + lane;
                win[wid][q * kWave + lane] = (c >= n_lo && c < n_ext) ? xr[q] : X(0);
            }
            wave_lds_sync();
            auto xv = [&](int c) { return (double)win[wid][c - row0 + kWinLo]; };
            row.sum(0, xv, sum);
            for (int q = row.U; q < row.steps; q += row.U) {
                row.load(q);
                row.sum(q, xv, sum);
            }
        } else {
            auto xv = [&](int c) { return (double)x[c]; };
            if (SellCol<CI>::stepped && row.exc) {
                sum = csr_row_sum(own ? row.xrow : -1, xrp, xcol, xval, xv);
            } else {
                row.sum(0, xv, sum);
                for (int q = row.U; q < row.steps; q += row.U) {
                    row.load(q);
                    row.sum(q, xv, sum);
                }
            }
        }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (own) {
        const X t = (X)sum;
        const X r = bi - t;  // copy(b, w); spmv(-1, A, x, 1, w)
        T wi = (T)r;
        acc[0] = (double)wi * (double)wi;
        P pw = (P)wi;  // = precond<T, P>
        if (diag) pw = P(0) * pw + P(1) * di * pw;
        wi = (T)pw;
        acc[1] = (double)wi * (double)wi;
        acc[2] = (double)xi * (double)xi;
        w[i] = wi;
    }
    store_partials<4>(acc, 3, partial);
}

template <class T, class X>
__global__ void k_prologue_finish(const double* __restrict__ sums, int m, T* __restrict__ s, T* __restrict__ inv,
                                  double* __restrict__ report) {
    const T r_norm = (T)sqrt(sums[0]);
    const T beta = (T)sqrt(sums[1]);
    const X x_norm = (X)sqrt(sums[2]);
    const T iv = beta != T(0) ? T(1) / beta : T(0);  // first_vector: zero fill when beta == 0
    if (threadIdx.x == 0) {
        report[0] = (double)r_norm;
        report[1] = (double)beta;
        report[2] = (double)x_norm;
        report[3] = (double)iv;
        *inv = iv;
    }
    for (int i = threadIdx.x; i <= m; i += blockDim.x) s[i] = i == 0 ? beta : T(0);
}

// k_reduce_partials of the prologue's 3 columns + k_prologue_finish in one
// workgroup (one GPU: nothing to all-reduce between them): each column is
// summed by sum_partials<BS>, as its k_reduce_partials workgroup would, so
// the sums and everything formed from them have the same bits.
// stage != nullptr: also hcol[0..m] = stage[0..m] (see UpdateTail)
template <class T, class X, int BS>
__global__ __launch_bounds__(BS) void k_prologue_finish_parts(int G, const double* __restrict__ partial,
                                                              double* __restrict__ sums, int m, T* __restrict__ s,
                                                              T* __restrict__ inv, double* __restrict__ report,
                                                              const T* __restrict__ stage, T* __restrict__ hcol) {
    __shared__ double scratch[BS / kWave];
    __shared__ double sm[3];
    // the cycle's last launch: the column H(0..m, m-1) that k_update_tail_nc
    // rotated and could not store in place (its other workgroups read it)
    if (stage)
        for (int i = threadIdx.x; i <= m; i += BS) hcol[i] = stage[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = sum_partials<BS>(partial + (size_t)c * G, G, scratch);
        if (threadIdx.x == 0) {
            sm[c] = v;
            sums[c] = v;
        }
    }
    __syncthreads();
    const T r_norm = (T)sqrt(sm[0]);
    const T beta = (T)sqrt(sm[1]);
    const X x_norm = (X)sqrt(sm[2]);
    const T iv = beta != T(0) ? T(1) / beta : T(0);  // first_vector: zero fill when beta == 0
    if (threadIdx.x == 0) {
        report[0] = (double)r_norm;
        report[1] = (double)beta;
        report[2] = (double)x_norm;
        report[3] = (double)iv;
        *inv = iv;
    }
    for (int i = threadIdx.x; i <= m; i += blockDim.x) s[i] = i == 0 ? beta : T(0);
}

}  // namespace
