// Plan object, constants and type-combination dispatch of the fused Arnoldi
// cycle (gfx950), shared by arnoldi.hip (the C-ABI, fp64 accumulation),
// arnoldi_acc32.hip (the fp32-accumulation instantiations of the fp32-Arnoldi
// kernels) and neumann.hip. The kernels live in one header per phase:
// arnoldi_reduce.hpp, arnoldi_givens.hpp, arnoldi_prologue.hpp,
// arnoldi_spmv.hpp, arnoldi_dots.hpp, arnoldi_orth.hpp (with lds_ring.hpp)
// and arnoldi_update.hpp.
//
// One restart cycle of GMRES(m) becomes a fixed program of phase kernels
// with no host round trip: the prologue (true residual + preconditioner +
// norms), per step an SpMV that normalises the previous vector on the fly
// and emits the Gram-Schmidt dot partials, the CGS/MGS update kernels that
// emit the next partials, a one-lane Givens kernel, and the solution update.
//
// Numerics follow the operator surface exactly where the reference fixes
// an order (reciprocal-then-multiply normalisation, y = alpha*t + beta*y
// forms, Givens on rounded products). Accumulation class (template parameter
// A of the dot/norm/gemv/SpMV kernels): A = double (default) sums fp32
// products in fp64 and rounds once to the working precision — the same
// rounding the stand-alone kernels (blas1/blas2/spmv) apply, so the fused
// engine and the operator-surface driver agree to the last bit in most
// steps; A = float (fp32 Arnoldi only, mpg_arnoldi_set_accum) keeps every
// partial sum in fp32, the class of the reference's cblas_sdot / snrm2 /
// sgemv and mkl_sparse_s_mv (kernels_mkl.cpp:82,94,104,284,348) and of
// cublasSdot / Sgemv / cusparseScsrmv (kernels_cuda.cpp:132,160,530,609).
//
// The floating-point contraction state is part of the kernels' text: the
// Givens header ends with `#pragma clang fp contract(on)`, and the reduce and
// prologue kernels are compiled ahead of it, in the compiler's default state.
// Every header that needs both includes them in that order.
#pragma once

#include "internal.hpp"
#include "node_tile.hpp"
#include "sell_tile.hpp"
#include "mpgmres/arnoldi.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

using namespace mpg;

namespace {

constexpr int kNC = 32;        // dot columns carried in registers per pass
constexpr int kGroups = 1024;  // max workgroups of the row-block phase kernels
constexpr int kCombineBlock = 1024;  // threads per workgroup of the combining panel dots
constexpr int kCombineGroups = 256;  // its workgroups: one per CU
constexpr int kOrthMGS = 1, kOrthCGSR = 2;  // mpg_orth_t (include/mpgmres/solve.h)
constexpr int kFoldMaxM = 128;  // GMRES(100), the reference's published restart length
constexpr int kWideMax = 128;

// f(integral_constant<int, C>) for C = 0 .. N - 1, in order
template <int C, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (C < N) {
        f(std::integral_constant<int, C>{});
        static_for<C + 1, N>(f);
    }
}

// f(integral_constant<int, nc>) for 1 <= nc <= N
template <int N, class F>
int with_nc(int nc, F&& f) {
    if constexpr (N == 0) {
        return MPG_ERR_ARG;
    } else {
        if (nc == N) return f(std::integral_constant<int, N>());
        return with_nc<N - 1>(nc, f);
    }
}

// f(std::true_type) or f(std::false_type): a runtime flag that only selects a
// template argument, spelled once (both instances are built, as by `b ? k<true> : k<false>`)
template <class F>
int with_flag(bool b, F&& f) {
    return b ? f(std::true_type()) : f(std::false_type());
}

// f(integral_constant<int, v>) for 0 <= v <= N (any other v: 0)
template <int N, class F>
int with_int(int v, F&& f) {
    if constexpr (N == 0) {
        return f(std::integral_constant<int, 0>());
    } else {
        if (v == N) return f(std::integral_constant<int, N>());
        return with_int<N - 1>(v, f);
    }
}

}  // namespace

// ---------------------------------------------------------------- plan object
struct mpg_arnoldi {
    mpg_ctx* ctx = nullptr;
    mpg_arnoldi_desc d{};
    int combo = 0;    // type combination (see dispatch below)
    int G = 1;        // workgroups of the row-parallel panel kernels
    int Grb = 1;      // workgroups of the row-block (SpMV) kernels: one per row block
    int last_G = 1;   // partial count per column written by the last producer
    double* last_part = nullptr;  // ... and the buffer it wrote (partial or dpart)
    // ... which hold the residual prologue's fp64 sums (set by mpg_arnoldi_prologue, cleared by every
    // other producer): mpg_arnoldi_reduce adds them in fp64 in either accumulation class
    bool last_prologue = false;
    int64_t ld = 0;   // leading dimension of V (elements)
    size_t tsize = 8;
    void* V = nullptr;
    void* H = nullptr;      // (m+1) x m
    void* small = nullptr;  // cs, sn, s (m+1 each), inv, corr (m+1), coef scratch
    void* w[2] = {nullptr, nullptr};      // row 0 of each w buffer
    void* wbase[2] = {nullptr, nullptr};  // the allocations: `front` entries before row 0
    int front = 0;                        // MPG_FRONT_PAD(d.n_front)
    double* partial = nullptr;  // (kNC + 4) x G
    double* dpart = nullptr;    // kNC x Gd: one-panel dots partials (read by the CGS update that writes `partial`)
    double* sums = nullptr;     // m + 4
    double* report = nullptr;   // 4 + m
    unsigned* counters = nullptr;  // last-arriver tickets: [0] dots, [32] CGS + Givens (zeroed at create)
    int Gd = 1;                    // workgroups (kCombineBlock threads) of the combining panel dots
    int cgs_pref = -1;             // MPG_CGS_PREFETCH as read at create: 0 / 1, -1 unset (the CGS update's form)
    SellCopy sell;  // sliced-ELL copy of the Arnoldi matrix (nslices == 0: CSR row blocks)
    SellCopy sell_outer;        // ... of the outer-precision values, for the residual prologue
    NodeCopy node;              // node-block copy of the Arnoldi matrix (nblk > 0: the Arnoldi SpMV uses it)
    // the residual prologue on node blocks (round 6): an fp64 node copy of the
    // outer values (or `node` itself when it holds them) and the fp64 row sums
    // A x it writes for k_prologue_rows; nullptr / empty: the CSR prologue
    NodeCopy node_outer;
    const NodeCopy* node_res = nullptr;
    double* rsum = nullptr;
    bool outer_is_inner = false;  // the prologue runs on `sell` (baseline / single modes)
    // SELL SpMV with the panel dots fused (SellDots): per-workgroup partials,
    // group tickets, group size and count
    double* fd_part = nullptr;
    unsigned* fd_cnt = nullptr;
    int fd_gs = 0, fd_ng = 0;
    // the SpMV in the dots' launch (k_step_dots): the ||w||^2 partials step
    // sd_k's launch folded, so that a repeat of that launch right behind it
    // (the duplicate of a measurement) folds the same ones, not its own dots'
    int sd_k = -1, sd_G = 0;
    double* sd_part = nullptr;
    // fp32 Arnoldi with fp32 accumulation (mpg_arnoldi_set_accum): the
    // launches go through arnoldi_acc32.hip's A = float instantiations
    bool acc32 = false;
    // the basis' storage (mpg_arnoldi_set_basis; basis.hpp): MPG_BASIS_F32,
    // _F16 (V holds fp16_rne(2^14 v), ld a multiple of 128 entries) or _F16EMU
    // (the same values as fp32). Other than F32: the plain launch forms only.
    int basis = 0;
    // the copy of A the polynomial preconditioners' sweeps read instead of the
    // Arnoldi matrix (mpg_arnoldi_set_prec_copy; neumann.hip): MPG_PREC_VALUES_F32
    // none, _F16 fp16 bits with row exponents, as a SELL copy (prec_sell) or
    // in CSR order (prec_vals), _F16EMU the same values as fp32 in CSR order.
    // The caller's memory: the workspace reads it and frees none of it.
    int prec_kind = 0;
    const void* prec_vals = nullptr;
    const int8_t* prec_rexp = nullptr;
    const mpg_sell* prec_sell = nullptr;
    // the cycle's tail in one launch (k_update_tail_nc): where it keeps the x
    // it read (mpg_arnoldi_set_x_snapshot), and whether its rotated column
    // H(:, m-1) still waits in tail_stage() for the finish launch
    void* x_snap = nullptr;
    bool tail_staged = false;

    char* small_at(int slot) const { return static_cast<char*>(small) + (size_t)slot * (d.m + 1) * tsize; }
    void* cs() const { return small_at(0); }
    void* sn() const { return small_at(1); }
    void* s() const { return small_at(2); }
    void* corr() const { return small_at(3); }
    void* inv() const { return small_at(4); }
    void* tail_stage() const { return small_at(6); }
};

namespace {

// block Jacobi applied inside the node kernels (desc.block_dinv): 3 x 3
// blocks on the node-block copy, one GPU's rows (no halo)
inline bool bj_fused(const mpg_arnoldi* a) {
    return a->d.block_dinv && a->d.prec_block == kNodeDof && a->node.nblk > 0 && a->d.n % kNodeDof == 0 &&
           a->front == 0 && a->d.n_ext == a->d.n;
}

// combos: 0 baseline <d,d,d,d>; 1 single-prec <d,d,f,d>; 2 single <f,f,f,f>;
//         3 mixed <f,d,f,f>; 4 mixed-half <f,d,f,h>
int combo_of(const mpg_arnoldi_desc& d) {
    if (d.vec_type == MPG_F64 && d.outer_type == MPG_F64 && d.inner_val == MPG_F64)
        return d.prec_type == MPG_F64 ? 0 : (d.prec_type == MPG_F32 ? 1 : -1);
    if (d.vec_type == MPG_F32 && d.prec_type == MPG_F32) {
        if (d.outer_type == MPG_F32 && d.inner_val == MPG_F32) return 2;
        if (d.outer_type == MPG_F64 && d.inner_val == MPG_F32) return 3;
        if (d.outer_type == MPG_F64 && d.inner_val == MPG_F16) return 4;
    }
    return -1;
}

template <class F>
int dispatch(int combo, F&& f) {
    switch (combo) {
        case 0: return f(double(), double(), double(), double());
        case 1: return f(double(), double(), float(), double());
        case 2: return f(float(), float(), float(), float());
        case 3: return f(float(), double(), float(), float());
        case 4: return f(float(), double(), float(), half_v());
        default: return MPG_ERR_UNSUPPORTED;
    }
}

// MPG_CSR_MODE (the Arnoldi CSR SpMV, k_step_spmv<..., MODE>): bit 0
// non-temporal matrix streams, bit 1 XCD-ordered row blocks
int csr_mode() {
    const char* e = std::getenv("MPG_CSR_MODE");
    return e && *e >= '0' && *e <= '4' ? *e - '0' : 0;
}

// Tiles per workgroup of the node-block SpMV (MPG_NODE_TPW: 1 one tile
// each, N > 1 a pipelined walk of N tiles; default 2; 0: as many as keep
// the grid at kNodeGroups workgroups, so the Givens step folds in).
// Measured (profiles/r05_node_ab.jsonl): fem27 248 / 218 / 215-228 / 223-238
// / 255 us at 1 / 2 / 4 / 8 / 16 (auto, folded: 247), C4's stencil 341 /
// 295-312 / 300 / 306-334 / 345 (auto 355): longer walks leave the grid's
// tail to fewer workgroups, two tiles in flight is the gain.
constexpr int kNodeGroups = 2048;
int node_tpw(const NodeCopy& S) {
    const int v = node_tpw_default();
    if (v >= 1) return v;
    return std::max(2, (S.ntiles + kNodeGroups - 1) / kNodeGroups);
}

int row_grid(const mpg_arnoldi* a) { return a->G; }
int rb_grid(const mpg_arnoldi* a) { return a->Grb; }

}  // namespace
