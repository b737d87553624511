// The initial-guess store of a live engine: fp64 panels Z and Q
// of n x L, Q = A Z, Q^T Q = I, and the two kernels every operation on them
// is made of.
//
//   k_guess_dots<NC>    one pass over r and NC columns of Q: per-workgroup fp64
//                       partials of Q^T r in columns 0..NC-1 and of ||r||^2 in
//                       column NC (partial[c * G + workgroup]).
//   k_guess_update<NC>  every workgroup sums those partials to c itself, 32
//                       lanes per column, each a strided run over the
//                       workgroups and a fixed xor tree (combine_columns'
//                       order; the same bits in every workgroup), then
//                       y = y_in + alpha Z c for its rows. PAIR: w += alpha Q c
//                       in the same launch, and the partials of Q^T w' and
//                       ||w'||^2 of the rows it has just written, so a second
//                       Gram-Schmidt pass needs no dots launch of its own.
//   k_guess_scale       the update's final form: sums ||w||^2 (nu^2) and the
//                       image's ||A x||^2 (omega^2) from their partials, and
//                       unless the direction is below the threshold stores
//                       Q(:, p) = w / nu, Z(:, p) = d / nu.
//
// No atomics, no reduce launch: a global sum is the per-workgroup partials of
// store_partials (panel.hpp) summed by the consumer in one fixed order, so two
// runs give the same bits. Rows go four per lane with 16-byte loads (the
// panels' leading dimension is even and their base 16-byte aligned); the n % 4
// tail rows are taken one per lane, and nothing at or past row n is read or
// written. The column count is a template parameter: every column index is
// static, a batch of columns issues its loads back to back and the
// accumulators stay in registers (k_dots_nc's reason, arnoldi_dots.hpp).
#include <cmath>

#include "panel.hpp"

namespace {

using namespace mpg;

constexpr int kGuessBlock = 256;
constexpr int kGuessMaxGroups = 512;  // two workgroups per CU: <= 16 partial loads per lane and column
constexpr int kGuessMaxCols = 16;     // MPG_GUESS_MAX_DEPTH
constexpr int kGuessBatch = 4;        // columns per load batch: 32 VGPRs of raw fp64 rows

inline int guess_groups(int64_t n) {
    const int64_t g = (n + 4 * kGuessBlock - 1) / (4 * kGuessBlock);
    return (int)(g < 1 ? 1 : g > kGuessMaxGroups ? kGuessMaxGroups : g);
}

// coef[c] = sum over g of partial[c * G + g], c < ncols, in every workgroup alike
template <int BS>
__device__ __forceinline__ void guess_sum_columns(const double* __restrict__ partial, int G, int ncols,
                                                  double* coef) {
    const int grp = threadIdx.x / 32, sub = threadIdx.x % 32;
    for (int c = grp; c < ncols; c += BS / 32) {
        double v = 0.0;
        for (int g = sub; g < G; g += 32) v += partial[(size_t)c * G + g];
#pragma unroll
        for (int mask = 16; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask, kWave);
        if (sub == 0) coef[c] = v;
    }
    __syncthreads();
}

// NC accumulators and one more to partial columns 0..NC-1 and NC
template <int NC, int BS, int NP>
__device__ __forceinline__ void guess_store(double (&acc)[NP], double last, double* __restrict__ partial) {
    if constexpr (NC > 0) {
        store_partials<NP, BS>(acc, NC, partial);
        __syncthreads();  // (NC == 1 comes through the one-column form twice: its LDS is read above)
    }
    double one[1] = {last};
    store_partials<1, BS>(one, 1, partial + (size_t)NC * gridDim.x);
}

template <int NC, int BS>
__global__ __launch_bounds__(BS) void k_guess_dots(int n, const double* __restrict__ Q, int64_t ld,
                                                   const double* __restrict__ r, double* __restrict__ partial) {
    constexpr int NP = Pow2Ceil<NC>::v;
    constexpr int B = kGuessBatch;
    double acc[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) acc[c] = 0.0;
    double rr = 0.0;
    const int n4 = n & ~3;
    for (int64_t i = 4 * ((int64_t)blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * (int64_t)gridDim.x * BS) {
        double rv[4];
        Row4<double>::load(r + i, rv);
        rr += rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2] + rv[3] * rv[3];
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += B) {
            Raw4<double> v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) v[u].load(Q + (int64_t)(c0 + u) * ld + i);
            __builtin_amdgcn_sched_barrier(0);  // keep the batch's loads issued back to back
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) acc[c0 + u] += v[u][0] * rv[0] + v[u][1] * rv[1] + v[u][2] * rv[2] + v[u][3] * rv[3];
        }
    }
    for (int64_t i = n4 + (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        const double ri = r[i];
        rr += ri * ri;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += Q[(int64_t)c * ld + i] * ri;
    }
    guess_store<NC, BS>(acc, rr, partial);
}

// y = y_in + alpha Z c (y_in == nullptr: zeros; y_in == y: in place), c summed
// from part_in. PAIR: w += alpha Q c too, and part_out takes Q^T w' and ||w'||^2.
// coef_out (may be nullptr): workgroup 0 stores the NC + 1 sums it used.
template <int NC, int BS, bool PAIR>
__global__ __launch_bounds__(BS) void k_guess_update(int n, int64_t ld, const double* __restrict__ part_in, int G,
                                                     double alpha, const double* __restrict__ Z, const double* y_in,
                                                     double* y, const double* __restrict__ Q, double* __restrict__ w,
                                                     double* __restrict__ part_out, double* __restrict__ coef_out) {
    constexpr int NP = Pow2Ceil<NC>::v;
    constexpr int B = kGuessBatch;
    // (the scaled coefficients stay in LDS, read where used: NC = 16 of them in registers beside the
    // accumulators and a batch of rows took the pair form past 256 VGPRs)
    __shared__ double coef[NC + 1], ac[NC];
    guess_sum_columns<BS>(part_in, G, NC + 1, coef);
    if (coef_out && blockIdx.x == 0 && threadIdx.x <= NC) coef_out[threadIdx.x] = coef[threadIdx.x];
    if (threadIdx.x < NC) ac[threadIdx.x] = alpha * coef[threadIdx.x];
    __syncthreads();
    double acc[PAIR ? NP : 1];
#pragma unroll
    for (int c = 0; c < (PAIR ? NP : 1); ++c) acc[c] = 0.0;
    double ww = 0.0;
    // t += P(i..i+3, :) ac, the columns in batches
    auto gemv4 = [&](const double* __restrict__ P, int64_t i, double (&t)[4]) {
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += B) {
            Raw4<double> v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) v[u].load(P + (int64_t)(c0 + u) * ld + i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) t[q] = fma(v[u][q], ac[c0 + u], t[q]);
                }
            // the next batch's loads after this batch's adds (dots_panel_from's reason, arnoldi_dots.hpp)
            asm volatile("" : "+v"(t[0]) : : "memory");
        }
    };
    const int n4 = n & ~3;
    for (int64_t i = 4 * ((int64_t)blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * (int64_t)gridDim.x * BS) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        if (y_in) Row4<double>::load(y_in + i, t);
        gemv4(Z, i, t);
        Row4<double>::store(y + i, t);
        if constexpr (PAIR) {
            double s[4];
            Row4<double>::load(w + i, s);
            gemv4(Q, i, s);
            Row4<double>::store(w + i, s);
            ww += s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3];
            // Q^T w' of these rows: the columns again (this lane's own lines, just read)
#pragma unroll
            for (int c0 = 0; c0 < NC; c0 += B) {
                Raw4<double> v[B];
#pragma unroll
                for (int u = 0; u < B; ++u)
                    if (c0 + u < NC) v[u].load(Q + (int64_t)(c0 + u) * ld + i);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < B; ++u)
                    if (c0 + u < NC)
                        acc[c0 + u] += v[u][0] * s[0] + v[u][1] * s[1] + v[u][2] * s[2] + v[u][3] * s[3];
                asm volatile("" : "+v"(acc[c0]) : : "memory");
            }
        }
    }
    for (int64_t i = n4 + (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double t = y_in ? y_in[i] : 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) t = fma(Z[(int64_t)c * ld + i], ac[c], t);
        y[i] = t;
        if constexpr (PAIR) {
            double s = w[i];
#pragma unroll
            for (int c = 0; c < NC; ++c) s = fma(Q[(int64_t)c * ld + i], ac[c], s);
            w[i] = s;
            ww += s * s;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += Q[(int64_t)c * ld + i] * s;
        }
    }
    if constexpr (PAIR) guess_store<NC, BS>(acc, ww, part_out);
}

// info[0] = nu = sqrt(sum nu2_part), info[1] = omega = sqrt(sum om2_part),
// info[2] = 1 where the column is stored: both finite and nu > thr * omega
template <int BS>
__global__ __launch_bounds__(BS) void k_guess_scale(int n, const double* __restrict__ nu2_part,
                                                    const double* __restrict__ om2_part, int G, double thr,
                                                    const double* __restrict__ w, const double* __restrict__ d,
                                                    double* __restrict__ qcol, double* __restrict__ zcol,
                                                    double* __restrict__ info) {
    __shared__ double s2[2];
    {
        const int grp = threadIdx.x / 32, sub = threadIdx.x % 32;
        if (grp < 2) {
            const double* __restrict__ p = grp == 0 ? nu2_part : om2_part;
            double v = 0.0;
            for (int g = sub; g < G; g += 32) v += p[g];
#pragma unroll
            for (int mask = 16; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask, kWave);
            if (sub == 0) s2[grp] = v;
        }
        __syncthreads();
    }
    const double nu = sqrt(s2[0]), om = sqrt(s2[1]);
    const bool keep = isfinite(nu) && isfinite(om) && nu > thr * om;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = nu;
        info[1] = om;
        info[2] = keep ? 1.0 : 0.0;
    }
    if (!keep) return;
    const int n4 = n & ~3;
    for (int64_t i = 4 * ((int64_t)blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * (int64_t)gridDim.x * BS) {
        double a[4], b[4];
        Row4<double>::load(w + i, a);
        Row4<double>::load(d + i, b);
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = a[q] / nu, b[q] = b[q] / nu;
        Row4<double>::store(qcol + i, a);
        Row4<double>::store(zcol + i, b);
    }
    for (int64_t i = n4 + (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        qcol[i] = w[i] / nu;
        zcol[i] = d[i] / nu;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int NC>
void launch_dots(mpg_ctx* c, int n, int64_t ld, const double* Q, const double* r, double* partial) {
    k_guess_dots<NC, kGuessBlock><<<guess_groups(n), kGuessBlock, 0, c->stream>>>(n, Q, ld, r, partial);
}
template <int NC>
void launch_update(mpg_ctx* c, int n, int64_t ld, const double* part_in, double alpha, const double* Z,
                   const double* y_in, double* y, const double* Q, double* w, double* part_out, double* coef_out) {
    const int G = guess_groups(n);
    if (Q)
        k_guess_update<NC, kGuessBlock, true><<<G, kGuessBlock, 0, c->stream>>>(n, ld, part_in, G, alpha, Z, y_in, y, Q,
                                                                               w, part_out, coef_out);
    else
        k_guess_update<NC, kGuessBlock, false><<<G, kGuessBlock, 0, c->stream>>>(n, ld, part_in, G, alpha, Z, y_in, y,
                                                                                nullptr, nullptr, nullptr, coef_out);
}

// f.template operator()<NC>() for the runtime column count nc in [LO, 16]
template <int LO, class F>
bool for_columns(int nc, F&& f) {
#define MPG_GUESS_CASE(N)                 \
    case N:                               \
        if constexpr (N >= LO) f.template operator()<N>(); \
        return N >= LO;
    switch (nc) {
        MPG_GUESS_CASE(0) MPG_GUESS_CASE(1) MPG_GUESS_CASE(2) MPG_GUESS_CASE(3) MPG_GUESS_CASE(4) MPG_GUESS_CASE(5)
        MPG_GUESS_CASE(6) MPG_GUESS_CASE(7) MPG_GUESS_CASE(8) MPG_GUESS_CASE(9) MPG_GUESS_CASE(10) MPG_GUESS_CASE(11)
        MPG_GUESS_CASE(12) MPG_GUESS_CASE(13) MPG_GUESS_CASE(14) MPG_GUESS_CASE(15) MPG_GUESS_CASE(16)
        default: return false;
    }
#undef MPG_GUESS_CASE
}

struct DotsCall {
    mpg_ctx* c;
    int n;
    int64_t ld;
    const double *Q, *r;
    double* partial;
    template <int NC> void operator()() const { launch_dots<NC>(c, n, ld, Q, r, partial); }
};
struct UpdateCall {
    mpg_ctx* c;
    int n;
    int64_t ld;
    const double* part_in;
    double alpha;
    const double *Z, *y_in;
    double* y;
    const double* Q;
    double *w, *part_out, *coef_out;
    template <int NC> void operator()() const {
        launch_update<NC>(c, n, ld, part_in, alpha, Z, y_in, y, Q, w, part_out, coef_out);
    }
};

}  // namespace

extern "C" {

int mpg_guess_groups(int32_t n) { return n < 1 ? MPG_ERR_ARG : guess_groups(n); }

int mpg_guess_dots_f64(mpg_ctx_t c, int32_t n, int32_t nc, int64_t ld, const double* Q, const double* r,
                       double* partial) {
    if (!c || n < 1 || nc < 0 || nc > kGuessMaxCols || !r || !partial || !aligned16(r)) return MPG_ERR_ARG;
    if (nc > 0 && (!Q || ld < n || (ld & 1) || !aligned16(Q))) return MPG_ERR_ARG;
    if (!for_columns<0>(nc, DotsCall{c, n, ld, Q, r, partial})) return MPG_ERR_ARG;
    MPG_LAUNCH_CHECK(c);
    return MPG_OK;
}

int mpg_guess_update_f64(mpg_ctx_t c, int32_t n, int32_t nc, int64_t ld, const double* partial, double alpha,
                         const double* Z, const double* y_in, double* y, const double* Q, double* w,
                         double* partial_out, double* coef_out) {
    if (!c || n < 1 || nc < 1 || nc > kGuessMaxCols || ld < n || (ld & 1) || !partial || !Z || !y) return MPG_ERR_ARG;
    if (!aligned16(Z) || !aligned16(y) || !aligned16(y_in)) return MPG_ERR_ARG;
    const bool pair = Q != nullptr;
    if (pair != (w != nullptr) || pair != (partial_out != nullptr)) return MPG_ERR_ARG;
    if (pair && (!aligned16(Q) || !aligned16(w) || partial_out == partial || w == y)) return MPG_ERR_ARG;
    if (!for_columns<1>(nc, UpdateCall{c, n, ld, partial, alpha, Z, y_in, y, Q, w, partial_out, coef_out}))
        return MPG_ERR_ARG;
    MPG_LAUNCH_CHECK(c);
    return MPG_OK;
}

int mpg_guess_scale_f64(mpg_ctx_t c, int32_t n, const double* nu2_partial, const double* om2_partial, double thr,
                        const double* w, const double* d, double* qcol, double* zcol, double* info) {
    if (!c || n < 1 || !nu2_partial || !om2_partial || !w || !d || !qcol || !zcol || !info) return MPG_ERR_ARG;
    if (!aligned16(w) || !aligned16(d) || !aligned16(qcol) || !aligned16(zcol)) return MPG_ERR_ARG;
    const int G = guess_groups(n);
    k_guess_scale<kGuessBlock><<<G, kGuessBlock, 0, c->stream>>>(n, nu2_partial, om2_partial, G, thr, w, d, qcol, zcol,
                                                                info);
    MPG_LAUNCH_CHECK(c);
    return MPG_OK;
}

}  // extern "C"
