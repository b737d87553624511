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
//
// The Chebyshev polynomial on [a, b] (theta = (a + b) / 2, delta = (b - a) / 2)
// runs through the same launches with another epilogue (the template
// parameter E): z_1 = (1 / theta) D r, then
//
//   z_out[i] = z_in[i] + alpha (z_in[i] - z_prev[i]) + beta d[i] (r[i] - s_i)
//
// in seven separately rounded operations (sweep_update below), alpha and beta from
// mpg_cheb_coeffs. The fourth epilogue operand z_prev[i] is loaded with the
// other three; z_out may alias it too. mpg_csr_jacobi_bound_* is the
// Gershgorin bound of D A that gives b.
//
// The GMRES polynomial (roots theta_i, residual polynomial prod (1 - x / theta_i))
// is applied in product form through four more epilogues (kPoly*): with
// B = D A, the running product p and the result z, a real root's step is
// p <- p - (1 / theta) B p, z <- z + (1 / theta_next) p; a pair a +- b i takes
// t = 2 a p - B p, z <- z + c t and then p <- p - c B t, c = 1 / (a^2 + b^2)
// (poly_update below; capi.h states each operation). There z is read and
// written by row i's lane alone, so it is one vector; the gathered vector may
// differ from the lane's own operand p (a pair's second half gathers t), and
// the second output may be p, never the gathered vector. mpg_gmres_poly_roots
// gives the roots in the order the product is stable in.
//
// The sweeps on an fp16 copy of A (the value type VI = half_v beside the
// vectors' T = float; mpg_*_sweep_f16f32, mpg_arnoldi_set_prec_copy): the values
// are mpg_csr_half_values' with scale = 1, row i's entries times 2^e_i, and
//
//   s_i = T(ldexp(sum_j half(a_ij) z_in[j], -e_i))
//
// summed in the same class and order, the unscale (exact: a power of two)
// applied once to the finished sum and the epilogues unchanged. Row i's
// exponent is one more epilogue operand, loaded with the others.
#include "arnoldi_prologue.hpp"
#include "mpgmres/solve.h"

#include <cmath>

#include <type_traits>

using namespace mpg;

namespace {

// The sweep's epilogue: the Neumann step, the Chebyshev step, and the first
// Chebyshev step (z_prev = 0: no fourth operand); the GMRES polynomial's step
// and pair (the first half of a pair), each also in the form that reads no z
enum : int {
    kNeumann = 0,
    kCheb = 1,
    kChebFirst = 2,
    kPolyStep = 4,
    kPolyStepFirst = 5,
    kPolyPair = 6,
    kPolyPairFirst = 7
};
constexpr bool poly_form(int e) { return e >= kPolyStep; }
constexpr bool poly_pair(int e) { return e == kPolyPair || e == kPolyPairFirst; }
constexpr bool poly_first(int e) { return e == kPolyStepFirst || e == kPolyPairFirst; }

// what the Chebyshev epilogues take besides the Neumann operands (z_prev
// carries no __restrict__: z_out may be that vector)
template <class T>
struct ChebArgs {
    const T* z_prev;
    T alpha, beta;
};

// ... and what a sweep on a scaled fp16 copy takes besides those: the row exponents
template <class T>
struct HalfArgs : ChebArgs<T> {
    const int8_t* rexp;
};
template <class T, class VI>
struct SweepArgs {
    using type = ChebArgs<T>;
};
template <class T>
struct SweepArgs<T, half_v> {
    using type = HalfArgs<T>;
};
template <class T, class VI>
__host__ __device__ inline typename SweepArgs<T, VI>::type sweep_args(const ChebArgs<T>& ch, const int8_t* rexp) {
    if constexpr (std::is_same_v<VI, half_v>) return {ch, rexp};
    else return ch;
}

// row i's exponent of a scaled fp16 copy, an epilogue operand like the others;
// unscale(sum) = sum 2^-e. A value type of the vectors' own carries nothing.
template <class VI>
struct RowExp {
    template <class AR> __device__ __forceinline__ void load(const AR&, int) {}
    template <class A> __device__ __forceinline__ A unscale(A sum) const { return sum; }
};
template <>
struct RowExp<half_v> {
    int e;
    template <class AR> __device__ __forceinline__ void load(const AR& ar, int i) { e = ar.rexp[i]; }
    template <class A> __device__ __forceinline__ A unscale(A sum) const { return ldexp(sum, -e); }
};

template <class T, int E>
struct SweepOps {
    T r, d, z;
};
template <class T>
struct SweepOps<T, kCheb> {
    T r, d, z, zp;
};

// row i's epilogue operands (i clamped by the caller)
template <int E, class T>
__device__ __forceinline__ SweepOps<T, E> sweep_ops(const T* r, const T* dinv, const T* z_in, const T* z_prev, int i) {
    if constexpr (E == kCheb) return {r[i], dinv[i], z_in[i], z_prev[i]};
    else if constexpr (poly_first(E)) return {r[i], dinv[i], T(0)};  // (the first form reads no z)
    else if constexpr (poly_form(E)) return {r[i], dinv[i], z_prev[i]};  // p (passed as r), d, z (passed as z_prev)
    else return {r[i], dinv[i], z_in[i]};
}

// Neumann: t = r - s; u = d * t; z + u. Chebyshev: t, u, then v = beta * u;
// p = z - z_prev (z for the first step); q = alpha * p; y = z + q; y + v.
// Each rounded to T.
template <int E, class T>
__device__ __forceinline__ T sweep_update(T s, const SweepOps<T, E>& o, T alpha, T beta) {
#pragma clang fp contract(off)
    const T t = o.r - s;
    const T u = o.d * t;
    if constexpr (E == kNeumann) {
        return o.z + u;
    } else {
        const T v = beta * u;
        T p = o.z;
        if constexpr (E == kCheb) p = o.z - o.zp;
        const T q = alpha * p;
        const T y = o.z + q;
        return y + v;
    }
}

// The GMRES polynomial's forms, o.r the lane's own operand p and o.z its z
// (the first forms: z = w0 p, w0 = c0 for a step, 0 for a pair). Step, c0 =
// omega, c1 = omega_next: u = d s; v = c0 u; o = p - v; y = c1 o. Pair's first
// half, c0 = 2 a, c1 = 1 / (a^2 + b^2): u = d s; q = c0 p; t = q - u; y = c1 t.
// Then z + y and the second output (o or t). Each rounded to T.
template <int E, class T>
__device__ __forceinline__ void poly_update(T s, const SweepOps<T, E>& o, T c0, T c1, T& z, T& out) {
#pragma clang fp contract(off)
    const T u = o.d * s;
    T zin = o.z;
    if constexpr (poly_first(E)) zin = (poly_pair(E) ? T(0) : c0) * o.r;
    T y;
    if constexpr (poly_pair(E)) {
        const T q = c0 * o.r;
        out = q - u;
        y = c1 * out;
    } else {
        const T v = c0 * u;
        out = o.r - v;
        y = c1 * out;
    }
    z = zin + y;
}

// row i's stores: z_out of the Neumann and Chebyshev steps; z (in place) and,
// unless it is the last form (no z_out), the second output of the GMRES
// polynomial's
template <int E, class T>
__device__ __forceinline__ void sweep_store(int i, T s, const SweepOps<T, E>& o, T* z_out, const ChebArgs<T>& ch) {
    if constexpr (poly_form(E)) {
        T z, out;
        poly_update<E>(s, o, ch.alpha, ch.beta, z, out);
        const_cast<T*>(ch.z_prev)[i] = z;
        if (z_out) z_out[i] = out;
    } else {
        z_out[i] = sweep_update<E>(s, o, ch.alpha, ch.beta);
    }
}

// (r and z_out carry no __restrict__: they may be one vector)
// VI: the matrix values' type, T or (T = float) half_v with its row exponents in ch
template <class T, class A, int E, class VI = T>
__global__ __launch_bounds__(kBlock) void k_csr_sweep(const int32_t* __restrict__ blocks, int nblocks,
                                                      const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const VI* __restrict__ val,
                                                      int64_t nnz, const T* __restrict__ dinv, const T* r,
                                                      const T* __restrict__ z_in, T* z_out,
                                                      typename SweepArgs<T, VI>::type ch) {
    __shared__ double prod[kNnzCap];
    __shared__ double scratch[kBlock / kWave];
    struct Pre {
        SweepOps<T, E> o;
        RowExp<VI> x;
    };
    for_rows<false, false, A>(
        blocks, nblocks, rowptr, col, val, nnz, [&](int c) { return (double)z_in[c]; },
        [&](int i) {
            Pre p{sweep_ops<E>(r, dinv, z_in, ch.z_prev, i), {}};
            p.x.load(ch, i);
            return p;
        },
        [&](int i, A sum, const Pre& p) { sweep_store<E>(i, (T)p.x.unscale(sum), p.o, z_out, ch); }, prod, scratch);
}

// (SV: the slices' and the CSR-summed rows' stored values, raw fp16 bits for VI = half_v)
template <class T, class CI, int W, bool UNI, class A, int E, class VI = T, class SV = typename SellStore<VI>::type>
__global__ __launch_bounds__(kBlock) void k_sell_sweep(int n, int nslices, const int64_t* __restrict__ off,
                                                       const CI* __restrict__ col, const SV* __restrict__ val,
                                                       const int32_t* __restrict__ sbase,
                                                       const int32_t* __restrict__ spat,
                                                       const int64_t* __restrict__ coff, const CI* __restrict__ pat,
                                                       const int32_t* __restrict__ xrp,
                                                       const int32_t* __restrict__ xcol, const SV* __restrict__ xval,
                                                       const T* __restrict__ dinv, const T* r,
                                                       const T* __restrict__ z_in, T* z_out, int64_t ustride, int xcd,
                                                       const int32_t* __restrict__ rows,
                                                       typename SweepArgs<T, VI>::type ch) {
    const int lane = threadIdx.x & (kWave - 1), wid = wave_id();
    const int s = (xcd ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x) * (kBlock / kWave) + wid;
    if (s >= nslices) return;  // (no workgroup barrier below)
    const int row0 = s * kWave;
    SellRow<SV, CI, W> row;
    if constexpr (UNI) row.init_uniform(s, ustride, spat, coff);
    else row.init_load(s, off, spat, coff);
    __builtin_amdgcn_sched_barrier(0);
    // the lane's row (a sorted copy's rows[]) and its epilogue operands, issued ahead of the slice
    const int i = rows ? rows[row0 + lane] : row0 + lane;
    const int ic = i < n ? i : 0;
    const SweepOps<T, E> o = sweep_ops<E>(r, dinv, z_in, ch.z_prev, ic);
    RowExp<VI> rx;
    rx.load(ch, ic);
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
    if (i < n) sweep_store<E>(i, (T)rx.unscale(sum), o, z_out, ch);
}

template <class T, class A, int E, class VI = T>
int csr_sweep(mpg_ctx* ctx, const mpg_csr* M, int grid, const VI* vals, const T* dinv, const T* r, const T* z_in,
              T* z_out, ChebArgs<T> ch = {}, const int8_t* rexp = nullptr) {
    if (M->rows == 0) return MPG_OK;
    k_csr_sweep<T, A, E, VI><<<grid, kBlock, 0, ctx->stream>>>(M->blocks, M->nblocks, M->rowptr, M->col, vals, M->nnz,
                                                               dinv, r, z_in, z_out, sweep_args<T, VI>(ch, rexp));
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

template <class T, class A, int E, class VI = T>
int sell_sweep(mpg_ctx* ctx, const SellCopy& S, const T* dinv, const T* r, const T* z_in, T* z_out,
               ChebArgs<T> ch = {}, const int8_t* rexp = nullptr) {
    using SV = typename SellStore<VI>::type;
    if (S.nslices == 0) return MPG_OK;
    const int grid = (S.nslices + kBlock / kWave - 1) / (kBlock / kWave);
    const char* xe = std::getenv("MPG_SELL_XCD");
    const int xcd = xe && *xe == '0' ? 0 : 1;
    int st = sell_dispatch(S, [&](auto ci, auto wc) {
        using CI = decltype(ci);
        constexpr int Wc = decltype(wc)::value;
        auto go = [&](auto kern) {
            kern<<<grid, kBlock, 0, ctx->stream>>>(S.n, S.nslices, S.off, static_cast<const CI*>(S.col),
                                                   static_cast<const SV*>(S.val), S.sbase, S.spat, S.coff,
                                                   static_cast<const CI*>(S.pat), S.xrp, S.xcol,
                                                   static_cast<const SV*>(S.xval), dinv, r, z_in, z_out, S.ustride, xcd,
                                                   S.rows, sweep_args<T, VI>(ch, rexp));
            return (int)MPG_OK;
        };
        return sell_uniform(S) ? go(k_sell_sweep<T, CI, Wc, true, A, E, VI>)
                               : go(k_sell_sweep<T, CI, Wc, false, A, E, VI>);
    });
    if (st) return st;
    MPG_LAUNCH_CHECK(ctx);
    return MPG_OK;
}

// The matrix a sweep reads: a SELL copy (S), else CSR row blocks (M, grid,
// vals). rexp: its values are fp16 bits scaled per row, with these exponents
// (T = float only); NULL: values of the vectors' type.
struct SweepMat {
    const SellCopy* S;
    const mpg_csr* M;
    int grid;
    const void* vals;
    const int8_t* rexp;
};

template <class T, class A, int E>
int sweep(mpg_ctx* ctx, const SweepMat& m, const T* dinv, const T* r, const T* z_in, T* z_out, ChebArgs<T> ch = {}) {
    if constexpr (std::is_same_v<T, float>) {
        if (m.rexp)
            return m.S ? sell_sweep<T, A, E, half_v>(ctx, *m.S, dinv, r, z_in, z_out, ch, m.rexp)
                       : csr_sweep<T, A, E, half_v>(ctx, m.M, m.grid, static_cast<const half_v*>(m.vals), dinv, r,
                                                    z_in, z_out, ch, m.rexp);
    }
    if (m.rexp) return MPG_ERR_UNSUPPORTED;
    return m.S ? sell_sweep<T, A, E>(ctx, *m.S, dinv, r, z_in, z_out, ch)
               : csr_sweep<T, A, E>(ctx, m.M, m.grid, static_cast<const T*>(m.vals), dinv, r, z_in, z_out, ch);
}

// the Chebyshev step on either storage: the first-step form when there is no z_prev
template <class T, class A>
int cheb_sweep(mpg_ctx* ctx, const SweepMat& m, const T* dinv, const T* r, const T* z_in, const T* z_prev, T* z_out,
               T alpha, T beta) {
    const ChebArgs<T> ch{z_prev, alpha, beta};
    return z_prev ? sweep<T, A, kCheb>(ctx, m, dinv, r, z_in, z_out, ch)
                  : sweep<T, A, kChebFirst>(ctx, m, dinv, r, z_in, z_out, ch);
}

// The stand-alone entries' matrix (vals: T values, or with row_exp fp16 bits;
// row_exp of a SELL copy: it must be an MPG_F16 one). false: MPG_ERR_ARG.
bool api_mat(mpg_ctx* ctx, const mpg_csr* M, const void* vals, const int8_t* row_exp, bool half, SweepMat& m) {
    if (!ctx || !M || M->rows != M->cols || (M->nnz > 0 && !vals) || (half && !row_exp)) return false;
    m = SweepMat{nullptr, M, M->nblocks, vals, half ? row_exp : nullptr};
    return true;
}
bool api_mat(mpg_ctx* ctx, const mpg_sell* M, int vtype, const int8_t* row_exp, SweepMat& m) {
    if (!ctx || !M || M->S.vtype != vtype || M->cols != M->S.n || (vtype == MPG_F16 && !row_exp)) return false;
    m = SweepMat{&M->S, nullptr, 0, nullptr, vtype == MPG_F16 ? row_exp : nullptr};
    return true;
}
int mat_rows(const SweepMat& m) { return m.S ? m.S->n : m.M->rows; }

template <class T>
int sweep_api(mpg_ctx* ctx, const SweepMat& m, const T* dinv, const T* r, const T* z_in, T* z_out) {
    if (mat_rows(m) > 0 && (!dinv || !r || !z_in || !z_out || z_out == z_in)) return MPG_ERR_ARG;
    if (mat_rows(m) == 0) return MPG_OK;
    return sweep<T, double, kNeumann>(ctx, m, dinv, r, z_in, z_out);
}

template <class T>
int cheb_api(mpg_ctx* ctx, const SweepMat& m, const T* dinv, const T* r, const T* z_in, const T* z_prev, T* z_out,
             T alpha, T beta) {
    if (mat_rows(m) > 0 && (!dinv || !r || !z_in || !z_out || z_out == z_in)) return MPG_ERR_ARG;
    if (mat_rows(m) == 0) return MPG_OK;
    return cheb_sweep<T, double>(ctx, m, dinv, r, z_in, z_prev, z_out, alpha, beta);
}

// one sweep of the GMRES polynomial on either storage: g gathered, p the
// lane's own operand, z in place, out the second output (NULL: the last form)
template <class T, class A>
int poly_sweep(mpg_ctx* ctx, const SweepMat& m, const T* dinv, const T* g, const T* p, T* z, T* out, bool pair,
               bool first, T c0, T c1) {
    const ChebArgs<T> ch{z, c0, c1};
    auto go = [&](auto e) {
        constexpr int E = decltype(e)::value;
        return sweep<T, A, E>(ctx, m, dinv, p, g, out, ch);
    };
    if (pair)
        return first ? go(std::integral_constant<int, kPolyPairFirst>{}) : go(std::integral_constant<int, kPolyPair>{});
    return first ? go(std::integral_constant<int, kPolyStepFirst>{}) : go(std::integral_constant<int, kPolyStep>{});
}

// the vectors of one sweep: out is absent exactly in the last form and is
// never the gathered vector; z is nobody else's
template <class T>
bool poly_vectors_ok(const T* dinv, const T* g, const T* p, const T* z, const T* out, int form, int last) {
    if (!dinv || !g || !p || !z || (form != MPG_POLY_STEP && form != MPG_POLY_PAIR)) return false;
    if (last ? out != nullptr : out == nullptr) return false;
    return out != g && z != g && z != p && z != out;
}

template <class T>
int poly_api(mpg_ctx* ctx, const SweepMat& m, const T* dinv, const T* g, const T* p, T* z, T* out, int form, int first,
             int last, T c0, T c1) {
    if (mat_rows(m) > 0 && !poly_vectors_ok(dinv, g, p, z, out, form, last)) return MPG_ERR_ARG;
    if (mat_rows(m) == 0) return MPG_OK;
    return poly_sweep<T, double>(ctx, m, dinv, g, p, z, out, form == MPG_POLY_PAIR, first != 0, c0, c1);
}

// The matrix a workspace's sweeps read: the copy of mpg_arnoldi_set_prec_copy
// when one is set, else the Arnoldi matrix in the storage the SpMV runs on
SweepMat run_mat(const mpg_arnoldi* a) {
    if (a->prec_kind == MPG_PREC_VALUES_F16)
        return {a->prec_sell ? &a->prec_sell->S : nullptr, a->d.A, a->Grb, a->prec_vals, a->prec_rexp};
    if (a->prec_kind == MPG_PREC_VALUES_F16EMU) return {nullptr, a->d.A, a->Grb, a->prec_vals, nullptr};
    return {a->sell.nslices > 0 ? &a->sell : nullptr, a->d.A, a->Grb, a->d.val_inner, nullptr};
}

template <class T>
int gdmv_t(mpg_ctx* ctx, int64_t n, T alpha, const T* d, const T* x, T* y) {
    if constexpr (std::is_same_v<T, double>) return mpg_gdmv_f64(ctx, n, alpha, d, x, 0.0, y);
    else return mpg_gdmv_f32(ctx, n, alpha, d, x, 0.0f, y);
}

// z_1 = D w (into w for one step, else into work0), then the sweeps between
// the work vectors with w as r; the last one stores into w
template <class T, class A>
int neumann_run(mpg_arnoldi* a, int steps, T* w, T* work0, T* work1) {
    mpg_ctx* ctx = a->ctx;
    const T* d = static_cast<const T*>(a->d.diag);
    const int n = a->d.n;
    if (int st = gdmv_t<T>(ctx, n, T(1), d, w, steps == 1 ? w : work0)) return st;
    T* bufs[2] = {work0, work1};
    const SweepMat mat = run_mat(a);
    for (int j = 1; j < steps; ++j) {
        const T* z_in = bufs[(j - 1) & 1];
        T* z_out = j == steps - 1 ? w : bufs[j & 1];
        if (int st = sweep<T, A, kNeumann>(ctx, mat, d, w, z_in, z_out)) return st;
    }
    return MPG_OK;
}

// z_1 = (1 / theta) D w as neumann_run forms D w, then sweep j reads z_j from
// bufs[(j - 1) & 1] and z_{j-1} from bufs[j & 1] (none at j = 1) and stores
// z_{j+1} over z_{j-1} (row i's lane alone reads z_{j-1}[i], before its store);
// the last one stores into w. Two work vectors serve any count.
template <class T, class A>
int cheb_run(mpg_arnoldi* a, int steps, double theta, double delta, T* w, T* work0, T* work1) {
    mpg_ctx* ctx = a->ctx;
    const T* d = static_cast<const T*>(a->d.diag);
    const int n = a->d.n;
    double alpha[64], beta[64];
    if (int st = mpg_cheb_coeffs(steps, theta, delta, alpha, beta)) return st;
    if (int st = gdmv_t<T>(ctx, n, (T)alpha[0], d, w, steps == 1 ? w : work0)) return st;
    T* bufs[2] = {work0, work1};
    const SweepMat mat = run_mat(a);
    for (int j = 1; j < steps; ++j) {
        const T* z_in = bufs[(j - 1) & 1];
        const T* z_prev = j == 1 ? nullptr : bufs[j & 1];
        T* z_out = j == steps - 1 ? w : bufs[j & 1];
        if (int st = cheb_sweep<T, A>(ctx, mat, d, w, z_in, z_prev, z_out, (T)alpha[j], (T)beta[j])) return st;
    }
    return MPG_OK;
}

// a root list mpg_arnoldi_poly_apply takes: finite, nonzero, every member with
// im > 0 followed by its conjugate (the same bits of re, the opposite im)
bool poly_roots_ok(int count, const double* re, const double* im) {
    if (count < 1 || count > 64 || !re || !im) return false;
    for (int k = 0; k < count; ++k) {
        if (!std::isfinite(re[k]) || !std::isfinite(im[k]) || (re[k] == 0.0 && im[k] == 0.0)) return false;
        if (im[k] < 0.0) return false;  // (a conjugate is consumed with its partner below)
        if (im[k] > 0.0) {
            if (k + 1 >= count || re[k + 1] != re[k] || im[k + 1] != -im[k]) return false;
            ++k;
        }
    }
    return true;
}

// The product form on the workspace's storage. p_0 = D w into work0, z in w
// from the first sweep on; a real root's step gathers p from `cur` and stores
// the new p into the other work vector; a pair's first half stores t there and
// its second half gathers t and stores the new p over `cur`. The coefficients
// are formed in fp64 and rounded once to T. A final real root's term came with
// the sweep before it (omega_next); a final pair runs its first half alone.
template <class T, class A>
int poly_run(mpg_arnoldi* a, int count, const double* re, const double* im, T* w, T* work0, T* work1) {
#pragma clang fp contract(off)
    mpg_ctx* ctx = a->ctx;
    const T* d = static_cast<const T*>(a->d.diag);
    const int n = a->d.n;
    if (count == 1) return gdmv_t<T>(ctx, n, (T)(1.0 / re[0]), d, w, w);
    if (int st = gdmv_t<T>(ctx, n, T(1), d, w, work0)) return st;
    const SweepMat mat = run_mat(a);
    auto sweep = [&](const T* g, const T* p, T* out, bool pair, bool first, double c0, double c1) {
        return poly_sweep<T, A>(ctx, mat, d, g, p, w, out, pair, first, (T)c0, (T)c1);
    };
    // the coefficient that adds root k's own term ahead of its sweep (0: a pair adds its own)
    auto omega_at = [&](int k) { return im[k] != 0.0 ? 0.0 : 1.0 / re[k]; };
    T *cur = work0, *oth = work1;
    bool first = true;
    for (int k = 0; k < count;) {
        const bool pair = im[k] != 0.0;
        const int kn = k + (pair ? 2 : 1);
        const bool next_ends = kn == count - 1 && im[kn] == 0.0;  // the next root is the final real one
        if (!pair) {
            if (kn >= count) break;
            if (int st = sweep(cur, cur, next_ends ? nullptr : oth, false, first, 1.0 / re[k], omega_at(kn))) return st;
            T* t = cur;
            cur = oth;
            oth = t;
        } else {
            const double aa = re[k] * re[k], bb = im[k] * im[k];
            const double c = 1.0 / (aa + bb);
            const bool ends = kn >= count;
            if (int st = sweep(cur, cur, ends ? nullptr : oth, true, first, 2.0 * re[k], c)) return st;
            if (ends) break;
            if (int st = sweep(oth, cur, next_ends ? nullptr : cur, false, false, c, omega_at(kn))) return st;
        }
        first = false;
        k = kn;
    }
    return MPG_OK;
}

// ---- the harmonic Ritz values: eigenvalues of an upper Hessenberg matrix ----
// Shifted QR with Francis double steps on a (n x n, row-major, overwritten),
// the classical EISPACK organisation: deflate on a negligible subdiagonal
// entry, take 1 x 1 and 2 x 2 blocks off the bottom, exceptional shifts at
// iterations 10 and 20 of a block. A 2 x 2 block with discriminant >= 0 gives
// two real values, else a pair: equal bits of re, im = -+ sqrt(-disc), the
// member with im < 0 at the lower index. Returns the index whose block did not
// converge in 60 iterations, or -1.
int hessenberg_eigenvalues(int n, double* a, double* wr, double* wi) {
#pragma clang fp contract(off)
    auto at = [&](int i, int j) -> double& { return a[(size_t)i * n + j]; };
    double anorm = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = i > 0 ? i - 1 : 0; j < n; ++j) anorm += std::fabs(at(i, j));
    int nn = n - 1;
    double t = 0.0, p = 0.0, q = 0.0, r = 0.0;
    while (nn >= 0) {
        int its = 0, l;
        do {
            for (l = nn; l >= 1; --l) {
                double s = std::fabs(at(l - 1, l - 1)) + std::fabs(at(l, l));
                if (s == 0.0) s = anorm;
                if (std::fabs(at(l, l - 1)) + s == s) {
                    at(l, l - 1) = 0.0;
                    break;
                }
            }
            double x = at(nn, nn);
            if (l == nn) {  // one value
                wr[nn] = x + t;
                wi[nn--] = 0.0;
            } else {
                double y = at(nn - 1, nn - 1), w = at(nn, nn - 1) * at(nn - 1, nn);
                if (l == nn - 1) {  // a 2 x 2 block
                    p = 0.5 * (y - x);
                    q = p * p + w;
                    double z = std::sqrt(std::fabs(q));
                    x += t;
                    if (q >= 0.0) {
                        z = p + std::copysign(z, p);
                        wr[nn - 1] = wr[nn] = x + z;
                        if (z != 0.0) wr[nn] = x - w / z;
                        wi[nn - 1] = wi[nn] = 0.0;
                    } else {
                        wr[nn - 1] = wr[nn] = x + p;
                        wi[nn] = z;
                        wi[nn - 1] = -z;
                    }
                    nn -= 2;
                } else {
                    if (its == 60) return nn;
                    if (its == 10 || its == 20) {  // an exceptional shift
                        t += x;
                        for (int i = 0; i <= nn; ++i) at(i, i) -= x;
                        const double s = std::fabs(at(nn, nn - 1)) + std::fabs(at(nn - 1, nn - 2));
                        y = x = 0.75 * s;
                        w = -0.4375 * s * s;
                    }
                    ++its;
                    int m;
                    for (m = nn - 2; m >= l; --m) {  // two consecutive small subdiagonal entries
                        const double z = at(m, m);
                        r = x - z;
                        double s = y - z;
                        p = (r * s - w) / at(m + 1, m) + at(m, m + 1);
                        q = at(m + 1, m + 1) - z - r - s;
                        r = at(m + 2, m + 1);
                        s = std::fabs(p) + std::fabs(q) + std::fabs(r);
                        p /= s;
                        q /= s;
                        r /= s;
                        if (m == l) break;
                        const double u = std::fabs(at(m, m - 1)) * (std::fabs(q) + std::fabs(r));
                        const double v =
                            std::fabs(p) * (std::fabs(at(m - 1, m - 1)) + std::fabs(z) + std::fabs(at(m + 1, m + 1)));
                        if (u + v == v) break;
                    }
                    for (int i = m + 2; i <= nn; ++i) {
                        at(i, i - 2) = 0.0;
                        if (i != m + 2) at(i, i - 3) = 0.0;
                    }
                    for (int k = m; k <= nn - 1; ++k) {  // the double QR step on rows l .. nn, columns m .. nn
                        if (k != m) {
                            p = at(k, k - 1);
                            q = at(k + 1, k - 1);
                            r = k != nn - 1 ? at(k + 2, k - 1) : 0.0;
                            x = std::fabs(p) + std::fabs(q) + std::fabs(r);
                            if (x != 0.0) {
                                p /= x;
                                q /= x;
                                r /= x;
                            }
                        }
                        const double s = std::copysign(std::sqrt(p * p + q * q + r * r), p);
                        if (s == 0.0) continue;
                        if (k == m) {
                            if (l != m) at(k, k - 1) = -at(k, k - 1);
                        } else {
                            at(k, k - 1) = -s * x;
                        }
                        p += s;
                        x = p / s;
                        y = q / s;
                        const double z = r / s;
                        q /= p;
                        r /= p;
                        for (int j = k; j <= nn; ++j) {
                            p = at(k, j) + q * at(k + 1, j);
                            if (k != nn - 1) {
                                p += r * at(k + 2, j);
                                at(k + 2, j) -= p * z;
                            }
                            at(k + 1, j) -= p * y;
                            at(k, j) -= p * x;
                        }
                        const int mmin = nn < k + 3 ? nn : k + 3;
                        for (int i = l; i <= mmin; ++i) {
                            p = x * at(i, k) + y * at(i, k + 1);
                            if (k != nn - 1) {
                                p += z * at(i, k + 2);
                                at(i, k + 2) -= p * r;
                            }
                            at(i, k + 1) -= p * q;
                            at(i, k) -= p;
                        }
                    }
                }
            }
        } while (l < nn - 1);
    }
    return -1;
}

// ---- the Gershgorin bound of D A: max_i |d_i| sum_j |a_ij| ----
// (a NaN row stays in the maximum: the caller refuses a non-finite bound)
__device__ __forceinline__ double max_keep_nan(double a, double b) { return (a != a || a > b) ? a : b; }

__device__ __forceinline__ double block_max_keep_nan(double v, double* scratch) {
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = max_keep_nan(v, __shfl_down(v, off, kWave));
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    double m = scratch[0];
    for (int q = 1; q < (int)blockDim.x / kWave; ++q) m = max_keep_nan(m, scratch[q]);
    __syncthreads();
    return m;  // the same value in every lane
}

// one lane per row: the fp64 sum of |a_ij| in storage order, times |d_i| in fp64
template <class T>
__global__ __launch_bounds__(kBlock) void k_jacobi_bound_rows(int n, const int32_t* __restrict__ rowptr,
                                                              const T* __restrict__ val, const T* __restrict__ dinv,
                                                              double* __restrict__ partial) {
    __shared__ double scratch[kBlock / kWave];
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double sum = 0.0;
        for (int k = rowptr[i], e = rowptr[i + 1]; k < e; ++k) sum += fabs((double)val[k]);
        m = max_keep_nan(m, fabs((double)dinv[i]) * sum);
    }
    m = block_max_keep_nan(m, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// the finishing workgroup: the maximum of the partials (any order gives the same value)
__global__ __launch_bounds__(kMaxRedBlocks) void k_jacobi_bound_finish(int nparts, const double* __restrict__ partial,
                                                                       double* out) {
    __shared__ double scratch[kMaxRedBlocks / kWave];
    const double v = (int)threadIdx.x < nparts ? partial[threadIdx.x] : 0.0;
    const double m = block_max_keep_nan(v, scratch);
    if (threadIdx.x == 0) __hip_atomic_store(out, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <class T>
int jacobi_bound(mpg_ctx* ctx, mpg_csr* M, const T* vals, const T* dinv, double* b_host) {
    if (!ctx || !M || !b_host || M->rows != M->cols || (M->nnz > 0 && !vals) || (M->rows > 0 && !dinv))
        return MPG_ERR_ARG;
    *b_host = 0.0;
    if (M->rows == 0) return MPG_OK;
    const int g = grid_for(M->rows, 1, kMaxRedBlocks);
    k_jacobi_bound_rows<T><<<g, kBlock, 0, ctx->stream>>>(M->rows, M->rowptr, vals, dinv, ctx->red_ws);
    MPG_LAUNCH_CHECK(ctx);
    if (ctx->host_ws_dev) {  // into the pinned block, read after the stream has drained
        k_jacobi_bound_finish<<<1, kMaxRedBlocks, 0, ctx->stream>>>(g, ctx->red_ws,
                                                                    static_cast<double*>(ctx->host_ws_dev));
        MPG_LAUNCH_CHECK(ctx);
        MPG_HIP(ctx, spin_wait(ctx->stream));
        *b_host = *static_cast<volatile double*>(ctx->host_ws);
        return MPG_OK;
    }
    double* tmp = ctx->red_ws + kMaxRedBlocks * kGemvMaxCols;
    k_jacobi_bound_finish<<<1, kMaxRedBlocks, 0, ctx->stream>>>(g, ctx->red_ws, tmp);
    MPG_LAUNCH_CHECK(ctx);
    return mpg_memcpy_d2h(ctx, b_host, tmp, sizeof(double));
}

}  // namespace

extern "C" {

int mpg_csr_jacobi_sweep_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, const double* dinv, const double* r,
                             const double* z_in, double* z_out) {
    SweepMat m;
    return api_mat(c, A, vals, nullptr, false, m) ? sweep_api<double>(c, m, dinv, r, z_in, z_out) : MPG_ERR_ARG;
}
int mpg_csr_jacobi_sweep_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, const float* dinv, const float* r,
                             const float* z_in, float* z_out) {
    SweepMat m;
    return api_mat(c, A, vals, nullptr, false, m) ? sweep_api<float>(c, m, dinv, r, z_in, z_out) : MPG_ERR_ARG;
}
int mpg_csr_jacobi_sweep_f16f32(mpg_ctx_t c, mpg_csr_t A, const uint16_t* vals_half, const int8_t* row_exp,
                                const float* dinv, const float* r, const float* z_in, float* z_out) {
    SweepMat m;
    return api_mat(c, A, vals_half, row_exp, true, m) ? sweep_api<float>(c, m, dinv, r, z_in, z_out) : MPG_ERR_ARG;
}
int mpg_sell_jacobi_sweep_f64(mpg_ctx_t c, mpg_sell_t A, const double* dinv, const double* r, const double* z_in,
                              double* z_out) {
    SweepMat m;
    return api_mat(c, A, MPG_F64, nullptr, m) ? sweep_api<double>(c, m, dinv, r, z_in, z_out) : MPG_ERR_ARG;
}
int mpg_sell_jacobi_sweep_f32(mpg_ctx_t c, mpg_sell_t A, const float* dinv, const float* r, const float* z_in,
                              float* z_out) {
    SweepMat m;
    return api_mat(c, A, MPG_F32, nullptr, m) ? sweep_api<float>(c, m, dinv, r, z_in, z_out) : MPG_ERR_ARG;
}
int mpg_sell_jacobi_sweep_f16f32(mpg_ctx_t c, mpg_sell_t A, const int8_t* row_exp, const float* dinv, const float* r,
                                 const float* z_in, float* z_out) {
    SweepMat m;
    return api_mat(c, A, MPG_F16, row_exp, m) ? sweep_api<float>(c, m, dinv, r, z_in, z_out) : MPG_ERR_ARG;
}

int mpg_csr_cheb_sweep_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, const double* dinv, const double* r,
                           const double* z_in, const double* z_prev, double* z_out, double alpha, double beta) {
    SweepMat m;
    return api_mat(c, A, vals, nullptr, false, m) ? cheb_api<double>(c, m, dinv, r, z_in, z_prev, z_out, alpha, beta)
                                                  : MPG_ERR_ARG;
}
int mpg_csr_cheb_sweep_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, const float* dinv, const float* r,
                           const float* z_in, const float* z_prev, float* z_out, float alpha, float beta) {
    SweepMat m;
    return api_mat(c, A, vals, nullptr, false, m) ? cheb_api<float>(c, m, dinv, r, z_in, z_prev, z_out, alpha, beta)
                                                  : MPG_ERR_ARG;
}
int mpg_csr_cheb_sweep_f16f32(mpg_ctx_t c, mpg_csr_t A, const uint16_t* vals_half, const int8_t* row_exp,
                              const float* dinv, const float* r, const float* z_in, const float* z_prev, float* z_out,
                              float alpha, float beta) {
    SweepMat m;
    return api_mat(c, A, vals_half, row_exp, true, m) ? cheb_api<float>(c, m, dinv, r, z_in, z_prev, z_out, alpha, beta)
                                                      : MPG_ERR_ARG;
}
int mpg_sell_cheb_sweep_f64(mpg_ctx_t c, mpg_sell_t A, const double* dinv, const double* r, const double* z_in,
                            const double* z_prev, double* z_out, double alpha, double beta) {
    SweepMat m;
    return api_mat(c, A, MPG_F64, nullptr, m) ? cheb_api<double>(c, m, dinv, r, z_in, z_prev, z_out, alpha, beta)
                                              : MPG_ERR_ARG;
}
int mpg_sell_cheb_sweep_f32(mpg_ctx_t c, mpg_sell_t A, const float* dinv, const float* r, const float* z_in,
                            const float* z_prev, float* z_out, float alpha, float beta) {
    SweepMat m;
    return api_mat(c, A, MPG_F32, nullptr, m) ? cheb_api<float>(c, m, dinv, r, z_in, z_prev, z_out, alpha, beta)
                                              : MPG_ERR_ARG;
}
int mpg_sell_cheb_sweep_f16f32(mpg_ctx_t c, mpg_sell_t A, const int8_t* row_exp, const float* dinv, const float* r,
                               const float* z_in, const float* z_prev, float* z_out, float alpha, float beta) {
    SweepMat m;
    return api_mat(c, A, MPG_F16, row_exp, m) ? cheb_api<float>(c, m, dinv, r, z_in, z_prev, z_out, alpha, beta)
                                              : MPG_ERR_ARG;
}

int mpg_csr_jacobi_bound_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, const double* dinv, double* b_host) {
    return jacobi_bound<double>(c, A, vals, dinv, b_host);
}
int mpg_csr_jacobi_bound_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, const float* dinv, double* b_host) {
    return jacobi_bound<float>(c, A, vals, dinv, b_host);
}

// (host arithmetic; it lives in this library because mpg_arnoldi_cheb_apply
// calls it, and the host library, which links this one, hands it on)
int mpg_cheb_coeffs(int steps, double theta, double delta, double* alpha, double* beta) {
#pragma clang fp contract(off)
    if (steps < 1 || steps > 64 || !alpha || !beta || !std::isfinite(theta) || !std::isfinite(delta) || delta <= 0.0 ||
        theta <= delta)
        return MPG_ERR_ARG;
    const double sigma = theta / delta;
    double rho_prev = 1.0 / sigma;
    alpha[0] = 1.0 / theta;
    beta[0] = 0.0;
    for (int j = 1; j < steps; ++j) {
        const double two_sigma = 2.0 * sigma;
        const double rho = 1.0 / (two_sigma - rho_prev);
        alpha[j] = rho * rho_prev;
        const double two_rho = 2.0 * rho;
        beta[j] = two_rho / delta;
        rho_prev = rho;
    }
    return MPG_OK;
}

int mpg_csr_poly_sweep_f64(mpg_ctx_t c, mpg_csr_t A, const double* vals, const double* dinv, const double* g,
                           const double* p, double* z, double* out, int32_t form, int32_t first, int32_t last,
                           double c0, double c1) {
    SweepMat m;
    return api_mat(c, A, vals, nullptr, false, m) ? poly_api<double>(c, m, dinv, g, p, z, out, form, first, last, c0, c1)
                                                  : MPG_ERR_ARG;
}
int mpg_csr_poly_sweep_f32(mpg_ctx_t c, mpg_csr_t A, const float* vals, const float* dinv, const float* g,
                           const float* p, float* z, float* out, int32_t form, int32_t first, int32_t last, float c0,
                           float c1) {
    SweepMat m;
    return api_mat(c, A, vals, nullptr, false, m) ? poly_api<float>(c, m, dinv, g, p, z, out, form, first, last, c0, c1)
                                                  : MPG_ERR_ARG;
}
int mpg_csr_poly_sweep_f16f32(mpg_ctx_t c, mpg_csr_t A, const uint16_t* vals_half, const int8_t* row_exp,
                              const float* dinv, const float* g, const float* p, float* z, float* out, int32_t form,
                              int32_t first, int32_t last, float c0, float c1) {
    SweepMat m;
    return api_mat(c, A, vals_half, row_exp, true, m)
               ? poly_api<float>(c, m, dinv, g, p, z, out, form, first, last, c0, c1)
               : MPG_ERR_ARG;
}
int mpg_sell_poly_sweep_f64(mpg_ctx_t c, mpg_sell_t A, const double* dinv, const double* g, const double* p, double* z,
                            double* out, int32_t form, int32_t first, int32_t last, double c0, double c1) {
    SweepMat m;
    return api_mat(c, A, MPG_F64, nullptr, m) ? poly_api<double>(c, m, dinv, g, p, z, out, form, first, last, c0, c1)
                                              : MPG_ERR_ARG;
}
int mpg_sell_poly_sweep_f32(mpg_ctx_t c, mpg_sell_t A, const float* dinv, const float* g, const float* p, float* z,
                            float* out, int32_t form, int32_t first, int32_t last, float c0, float c1) {
    SweepMat m;
    return api_mat(c, A, MPG_F32, nullptr, m) ? poly_api<float>(c, m, dinv, g, p, z, out, form, first, last, c0, c1)
                                              : MPG_ERR_ARG;
}
int mpg_sell_poly_sweep_f16f32(mpg_ctx_t c, mpg_sell_t A, const int8_t* row_exp, const float* dinv, const float* g,
                               const float* p, float* z, float* out, int32_t form, int32_t first, int32_t last,
                               float c0, float c1) {
    SweepMat m;
    return api_mat(c, A, MPG_F16, row_exp, m) ? poly_api<float>(c, m, dinv, g, p, z, out, form, first, last, c0, c1)
                                              : MPG_ERR_ARG;
}

int mpg_arnoldi_set_prec_copy(mpg_arnoldi_t a, int32_t kind, const void* vals, const int8_t* row_exp, mpg_sell_t sell) {
    if (!a || kind < MPG_PREC_VALUES_F32 || kind > MPG_PREC_VALUES_F16EMU) return MPG_ERR_ARG;
    if (kind == MPG_PREC_VALUES_F32) {
        if (vals || row_exp || sell) return MPG_ERR_ARG;
    } else {
        // an fp32 Arnoldi on fp32 values of one GPU's rows (mpg_arnoldi_neumann_apply's combinations, less fp64)
        if ((a->combo != 2 && a->combo != 3) || a->d.inner_val != MPG_F32 || a->front != 0 || a->d.n_ext != a->d.n)
            return MPG_ERR_UNSUPPORTED;
        if (kind == MPG_PREC_VALUES_F16EMU ? (sell || row_exp || (a->d.A->nnz > 0 && !vals))
                                           : (!row_exp || (sell ? vals != nullptr : a->d.A->nnz > 0 && !vals)))
            return MPG_ERR_ARG;
        if (sell && (sell->S.vtype != MPG_F16 || sell->S.n != a->d.n || sell->cols != a->d.n || sell->S.nslices == 0))
            return MPG_ERR_ARG;
    }
    a->prec_kind = kind;
    a->prec_vals = vals;
    a->prec_rexp = row_exp;
    a->prec_sell = sell;
    return MPG_OK;
}

int mpg_arnoldi_prec_values(mpg_arnoldi_t a) { return a ? a->prec_kind : MPG_ERR_ARG; }

// (host arithmetic, here for mpg_cheb_coeffs' reason)
int mpg_gmres_poly_roots(int s, const double* H, int ldh, double* re, double* im, int* count) {
#pragma clang fp contract(off)
    if (count) *count = 0;
    if (s < 1 || s > 64 || !H || ldh < s || !re || !im || !count) return MPG_ERR_ARG;
    const int n = s;
    double G[64 * 64], L[64 * 64], f[64], wr[64], wi[64];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) G[i * n + j] = j + 1 >= i ? H[(size_t)i * ldh + j] : 0.0;
    const double h = H[(size_t)n * ldh + (n - 1)];
    if (!std::isfinite(h)) return MPG_ERR_ARG;
    if (h != 0.0) {
        // H_s^T f = e_s by elimination with partial pivoting (L holds H_s^T; ties to the lower row)
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j) L[i * n + j] = G[j * n + i];
            f[i] = i == n - 1 ? 1.0 : 0.0;
        }
        for (int k = 0; k < n; ++k) {
            int piv = k;
            for (int i = k + 1; i < n; ++i)
                if (std::fabs(L[i * n + k]) > std::fabs(L[piv * n + k])) piv = i;
            if (!(std::fabs(L[piv * n + k]) > 0.0) || !std::isfinite(L[piv * n + k])) return MPG_ERR_BREAKDOWN;
            if (piv != k) {
                for (int j = 0; j < n; ++j) std::swap(L[k * n + j], L[piv * n + j]);
                std::swap(f[k], f[piv]);
            }
            for (int i = k + 1; i < n; ++i) {
                const double m = L[i * n + k] / L[k * n + k];
                if (m == 0.0) continue;
                for (int j = k; j < n; ++j) L[i * n + j] -= m * L[k * n + j];
                f[i] -= m * f[k];
            }
        }
        for (int i = n - 1; i >= 0; --i) {
            double v = f[i];
            for (int j = i + 1; j < n; ++j) v -= L[i * n + j] * f[j];
            f[i] = v / L[i * n + i];
        }
        const double h2 = h * h;
        for (int i = 0; i < n; ++i) G[i * n + (n - 1)] += h2 * f[i];
    }
    for (int i = 0; i < n * n; ++i)
        if (!std::isfinite(G[i])) return MPG_ERR_BREAKDOWN;
    const int bad = hessenberg_eigenvalues(n, G, wr, wi);
    if (bad >= 0) {
        *count = bad;
        return MPG_ERR_BREAKDOWN;
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(wr[i]) || !std::isfinite(wi[i]) || (wr[i] == 0.0 && wi[i] == 0.0)) {
            *count = i;
            return MPG_ERR_BREAKDOWN;
        }
    // Leja order over the items (a real value, or a pair taken as its im > 0 member and standing for both)
    int item[64], nitems = 0;
    for (int i = 0; i < n; ++i) {
        item[nitems++] = i;
        if (wi[i] != 0.0) ++i;  // (its conjugate follows)
    }
    bool used[64] = {};
    double pr[64], pi[64];  // the members placed
    int placed = 0;
    while (placed < n) {
        int best = -1;
        double best_score = 0.0;
        for (int q = 0; q < nitems; ++q) {
            if (used[q]) continue;
            const double a = wr[item[q]], b = std::fabs(wi[item[q]]);
            double score = 0.0;
            if (placed == 0) score = std::hypot(a, b);
            else
                for (int j = 0; j < placed; ++j) score += std::log(std::hypot(a - pr[j], b - pi[j]));
            if (best < 0 || score > best_score) {
                best = q;
                best_score = score;
            }
        }
        used[best] = true;
        const double a = wr[item[best]], b = std::fabs(wi[item[best]]);
        pr[placed] = a;
        pi[placed++] = b;
        if (b != 0.0) {
            pr[placed] = a;
            pi[placed++] = -b;
        }
    }
    for (int i = 0; i < n; ++i) {
        re[i] = pr[i];
        im[i] = pi[i];
    }
    *count = n;
    return MPG_OK;
}

int mpg_arnoldi_poly_apply(mpg_arnoldi_t a, int32_t count, const double* re, const double* im, void* w, void* work0,
                           void* work1) {
    if (!a || !a->ctx || count < 1 || count > 64 || !w || (count >= 2 && !work0) || (count >= 3 && !work1) ||
        (count >= 2 && work0 == w) || (count >= 3 && (work1 == w || work1 == work0)) || !a->d.diag ||
        !poly_roots_ok(count, re, im))
        return MPG_ERR_ARG;
    // (mpg_arnoldi_neumann_apply's combinations)
    if ((a->combo != 0 && a->combo != 2 && a->combo != 3) || a->front != 0 || a->d.n_ext != a->d.n)
        return MPG_ERR_UNSUPPORTED;
    if (a->d.n == 0) return MPG_OK;
    if (a->combo == 0)
        return poly_run<double, double>(a, count, re, im, static_cast<double*>(w), static_cast<double*>(work0),
                                        static_cast<double*>(work1));
    if (a->acc32)
        return poly_run<float, float>(a, count, re, im, static_cast<float*>(w), static_cast<float*>(work0),
                                      static_cast<float*>(work1));
    return poly_run<float, double>(a, count, re, im, static_cast<float*>(w), static_cast<float*>(work0),
                                   static_cast<float*>(work1));
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

extern "C" int mpg_arnoldi_cheb_apply(mpg_arnoldi_t a, int32_t steps, double theta, double delta, void* w, void* work0,
                                      void* work1) {
    if (!a || !a->ctx || steps < 1 || steps > 64 || !w || (steps >= 2 && !work0) || (steps >= 3 && !work1) ||
        (steps >= 2 && work0 == w) || (steps >= 3 && (work1 == w || work1 == work0)) || !a->d.diag ||
        !std::isfinite(theta) || !std::isfinite(delta) || delta <= 0.0 || theta <= delta)
        return MPG_ERR_ARG;
    // (mpg_arnoldi_neumann_apply's combinations)
    if ((a->combo != 0 && a->combo != 2 && a->combo != 3) || a->front != 0 || a->d.n_ext != a->d.n)
        return MPG_ERR_UNSUPPORTED;
    if (a->d.n == 0) return MPG_OK;
    if (a->combo == 0)
        return cheb_run<double, double>(a, steps, theta, delta, static_cast<double*>(w), static_cast<double*>(work0),
                                        static_cast<double*>(work1));
    if (a->acc32)
        return cheb_run<float, float>(a, steps, theta, delta, static_cast<float*>(w), static_cast<float*>(work0),
                                      static_cast<float*>(work1));
    return cheb_run<float, double>(a, steps, theta, delta, static_cast<float*>(w), static_cast<float*>(work0),
                                   static_cast<float*>(work1));
}
