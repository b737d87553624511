// The Arnoldi SpMV of step k, which normalises the previous vector on the fly
// (v_k = T(w_prev * inv), w = M(A v_k)), in its four storage forms: CSR row
// blocks, node blocks (with and without block Jacobi) and SELL-64 slices, one
// or two per wave.
#pragma once

#include "arnoldi_prologue.hpp"
#include "arnoldi_givens.hpp"
#include "basis.hpp"
#include "handoff.hpp"

namespace {

// ---------------------------------------------------------------- step: SpMV
// v_k = T(w_prev * inv) (local rows stored to V[:,k]); w = M(A v_k).
// inv = 1/h_{k,k-1} from the previous Givens kernel, or formed here with
// that Givens step folded in (fold.norm2 != nullptr). The Gram-Schmidt dots
// follow in k_panel_dots (measured: dots inside this gather-bound launch
// cost more than the separate pass, 71 us vs 30 + 20 us on BAND-10M).
// AT: the accumulation class, or WithBasis<A, B> for a compressed or emulated
// basis (basis.hpp): the operator is then applied to the stored value
// round(T(w_prev * inv)), which is also what V(:,k) receives.
template <class T, class P, class VI, bool FOLD, int MODE = 0, class AT = double>
__global__ __launch_bounds__(kBlock) void k_step_spmv(const int32_t* __restrict__ blocks, int nblocks,
                                                      const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const VI* __restrict__ val,
                                                      int64_t nnz, const T* __restrict__ wprev,
                                                      const T* __restrict__ inv_p, T* __restrict__ V, int64_t ld,
                                                      int k, const P* __restrict__ diag, T* __restrict__ w,
                                                      GivensFold<T> fold, const int8_t* __restrict__ rexp) {
    using A = typename AccOf<AT>::type;
    using Bs = BasisOf<T, AT>;
    __shared__ double prod[kNnzCap];
    __shared__ double scratch[kBlock / kWave];
    const T inv = fold_givens<FOLD, T, A>(fold, inv_p);
    typename Bs::elem* __restrict__ Vk = basis_ptr<Bs>(V) + (int64_t)k * ld;
    struct Ops {
        T wp;
        P d;
        int e;  // row exponent of a scaled fp16 copy (mpg_csr_half_values)
    };
    // MODE bit 0: non-temporal matrix streams; bit 1: XCD-ordered row blocks;
    // bit 2 (measurement only, wrong results): no gathers, x = 1
    for_rows<(MODE & 1) != 0, (MODE & 2) != 0, A>(
        blocks, nblocks, rowptr, col, val, nnz,
        [&](int c) { return (MODE & 4) ? 1.0 + 0.0 * c : (double)Bs::round((T)(wprev[c] * inv)); },
        [&](int i) { return Ops{wprev[i], diag ? diag[i] : P(0), rexp ? (int)rexp[i] : 0}; },
        [&](int i, double sum, const Ops& o) {
            const T t = (T)ldexp(sum, -o.e);  // spmv(1, A, v, 0, w): y = 1*t (exact unscale)
            P pw = (P)t;         // = precond<T, P> with the diagonal loaded ahead
            if (diag) pw = P(0) * pw + P(1) * o.d * pw;
            w[i] = (T)pw;
            const T vk = Bs::round(o.wp * inv);
            Bs::store(&Vk[i], vk);
        },
        prod, scratch);
}

// ---------------------------------------------------------------- step: SpMV (node blocks)
// Same contract as k_step_spmv on the node-block copy (node_tile.hpp): one
// tile of node rows per workgroup, the CSR tile's products and row order.
// WALK: each workgroup walks tpw consecutive tiles, the next tile's records
// in flight during this one's gathers and row sums (node_tiles); else one
// tile per workgroup (node_tile).
template <class T, class P, class VI, bool FOLD, bool WALK = true, class A = double>
__global__ __launch_bounds__(kBlock) void k_step_node(const int32_t* __restrict__ tiles,
                                                      const int32_t* __restrict__ bptr, const char* __restrict__ recs,
                                                      const T* __restrict__ wprev, const T* __restrict__ inv_p,
                                                      T* __restrict__ V, int64_t ld, int k,
                                                      const P* __restrict__ diag, T* __restrict__ w,
                                                      GivensFold<T> fold, const int8_t* __restrict__ rexp,
                                                      int ntiles, int64_t nblk, int tpw, int xcd) {
    __shared__ double prod[kNodeProd];
    const T inv = fold_givens<FOLD, T, A>(fold, inv_p);
    T* __restrict__ Vk = V + (int64_t)k * ld;
    struct Ops {
        T wp;
        P d;
        int e;
    };
    auto xraw = [&](int c) { return wprev[c]; };
    auto xfin = [&](T v) { return (double)(T)(v * inv); };
    auto xval = [&](int c) { return xfin(xraw(c)); };
    auto pre = [&](int i) { return Ops{wprev[i], diag ? diag[i] : P(0), rexp ? (int)rexp[i] : 0}; };
    auto epi = [&](int i, double sum, const Ops& o) {
        const T t = (T)ldexp(sum, -o.e);
        P pw = (P)t;
        if (diag) pw = P(0) * pw + P(1) * o.d * pw;
        w[i] = (T)pw;
        Vk[i] = o.wp * inv;
    };
    // xcd: workgroups take their tiles in XCD order (xcd_block), so each
    // XCD's L2 serves one contiguous eighth of the rows' gathers
    const int g = xcd ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    if constexpr (!WALK) {
        node_tile<VI, A>(g, tiles, bptr, recs, xval, pre, epi, prod);
    } else {
        const int t0 = g * tpw, t1 = t0 + tpw < ntiles ? t0 + tpw : ntiles;
        node_tiles<VI, A>(t0, t1, tiles, tiles + ntiles + 1, bptr, recs, nblk, xraw, xfin, pre, epi, prod);
    }
}

// ---------------------------------------------------------------- step: SpMV (node blocks) + block Jacobi
// k_step_node with w = Dinv (A v_k): the 3 x 3 inverse of each node's
// diagonal block (mpg_bjacobi_setup_*) applied inside the launch. A node's
// three row sums are formed by three lanes, which may sit in two waves or in
// two turns of the rows loop (a tile holds up to 3 * 256 rows): every lane
// keeps P(T(sum)) of its rows in registers until the whole tile has read its
// products, stores them over the products in LDS, and after a second barrier
// forms its own row of Dinv * sums -- mpg_bjacobi_apply_*'s arithmetic
// (products rounded, summed left to right, contraction off) on the values
// the plain launch would have written: the same bits. The walk over the
// tiles, the products and the order of every row sum are node_tiles'.
template <class T, class P, class VI, bool FOLD, class A = double>
__global__ __launch_bounds__(kBlock) void k_step_node_bj(const int32_t* __restrict__ tiles,
                                                         const int32_t* __restrict__ bptr,
                                                         const char* __restrict__ recs,
                                                         const T* __restrict__ wprev, const T* __restrict__ inv_p,
                                                         T* __restrict__ V, int64_t ld, int k,
                                                         const P* __restrict__ dinv, T* __restrict__ w,
                                                         GivensFold<T> fold, const int8_t* __restrict__ rexp,
                                                         int ntiles, int64_t nblk, int tpw, int xcd) {
    constexpr int R = NodeRec<VI>::R;
    constexpr int D = kNodeDof;
    __shared__ double prod[kNodeProd];
    P* xs = reinterpret_cast<P*>(prod);  // (D * kNodeCap values at most: a tile's rows)
    const T inv = fold_givens<FOLD, T, A>(fold, inv_p);
    T* __restrict__ Vk = V + (int64_t)k * ld;
    const int g = xcd ? xcd_block((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int t0 = g * tpw, t1 = t0 + tpw < ntiles ? t0 + tpw : ntiles;
    const int32_t* __restrict__ tb0 = tiles + ntiles + 1;
    const int l = threadIdx.x;
    auto rec = [&](int t) {
        const int b0 = tb0[t], nb = tb0[t + 1] - b0;
        int64_t b = (int64_t)b0 + (l < nb ? l : nb - 1);
        b = b < 0 ? 0 : b >= nblk ? nblk - 1 : b;
        return recs + b * R;
    };
    NodeWords<VI> cur, nxt;
    cur.load(rec(t0));
    for (int t = t0; t < t1; ++t) {
        const int nr0 = tiles[t], nr1 = tiles[t + 1];
        const int b0 = tb0[t], nb = tb0[t + 1] - b0;
        const int rows = D * (nr1 - nr0);  // <= D * kNodeCap (node_build)
        const int c = cur.col();
        const T r0 = wprev[c], r1 = wprev[c + 1], r2 = wprev[c + 2];
        const double x0 = (double)(T)(r0 * inv), x1 = (double)(T)(r1 * inv), x2 = (double)(T)(r2 * inv);
        if (t + 1 < t1) nxt.load(rec(t + 1));
        if (l < nb) {
            double* p = prod + l * (D * D);
#pragma unroll
            for (int q = 0; q < D; ++q) {
                p[3 * q + 0] = cur.val(3 * q + 0) * x0;
                p[3 * q + 1] = cur.val(3 * q + 1) * x1;
                p[3 * q + 2] = cur.val(3 * q + 2) * x2;
            }
        }
        lds_barrier();
        P pw[D], dd[D][D];
        T wp[D];
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int r = l + u * kBlock;
            pw[u] = P(0);
            if (r < rows) {
                const int nr = nr0 + r / D, q = r % D;
                const int i = D * nr0 + r;
                const int a = bptr[nr] - b0, z = bptr[nr + 1] - b0;
                const int e = rexp ? (int)rexp[i] : 0;
                A acc = A(0);
                int b = a;
                for (; b + kNodeSumAhead <= z; b += kNodeSumAhead) {
                    double v[3 * kNodeSumAhead];
#pragma unroll
                    for (int s = 0; s < kNodeSumAhead; ++s) {
                        const double* p = prod + (b + s) * (D * D) + D * q;
                        v[3 * s] = p[0];
                        v[3 * s + 1] = p[1];
                        v[3 * s + 2] = p[2];
                    }
#pragma unroll
                    for (int s = 0; s < 3 * kNodeSumAhead; ++s) add_prod(acc, v[s]);
                }
                for (; b < z; ++b) {
                    const double* p = prod + b * (D * D) + D * q;
                    add_prod(acc, p[0]);
                    add_prod(acc, p[1]);
                    add_prod(acc, p[2]);
                }
                const double sum = acc;
                pw[u] = (P)(T)ldexp(sum, -e);
            }
        }
        lds_barrier();  // every row sum has read its products
        // (the lane's rows of the inverses and of w_prev are loaded here, not
        // held through the row sums, where the registers are needed)
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int r = l + u * kBlock;
            if (r < rows) {
                const int i = D * nr0 + r;
                xs[r] = pw[u];
                wp[u] = wprev[i];
#pragma unroll
                for (int j = 0; j < D; ++j) dd[u][j] = dinv[(int64_t)i * D + j];
            }
        }
        lds_barrier();
#pragma unroll
        for (int u = 0; u < D; ++u) {
#pragma clang fp contract(off)
            const int r = l + u * kBlock;
            if (r < rows) {
                const int q0 = r / D * D;
                const int i = D * nr0 + r;
                P acc = dd[u][0] * xs[q0];
                const P p1 = dd[u][1] * xs[q0 + 1];
                acc = acc + p1;
                const P p2 = dd[u][2] * xs[q0 + 2];
                acc = acc + p2;
                w[i] = (T)acc;
                Vk[i] = wp[u] * inv;
            }
        }
        lds_barrier();  // the next tile's products overwrite xs
        cur = nxt;
    }
}

// ---------------------------------------------------------------- step: SpMV (SELL-64)
// Same contract as k_step_spmv on the sliced-ELL copy (sell_tile.hpp): one
// wave per slice, one lane per row; v_k and w are written coalesced.
// WIN (every column of a slice within [row0 - kWinLo, row0 + 64 + kWinHi),
// checked when the copy is built): the slice's window of v_k is formed once
// in LDS with three coalesced loads per lane and the gathers read LDS —
// 10 scattered global loads per row become LDS reads (-20 % on BAND-10M,
// tools/sell_bench.hip). Values are the same T(w_prev * inv) either way.

//
// Load order (vmcnt retires in order, so what is needed first is issued
// first, and nothing is waited for before everything is in flight): the
// slice's offsets, the folded Givens step's partial (one per lane), the
// window of w_prev (raw,
// clamped addresses), the slice's first batch of (col, val); then the
// partial sum behind LDS-only barriers, the scaled window into LDS, the
// gathers. A guarded load would be widened inside its branch and waited
// for right there — the previous form waited for each window load and each
// step's loads in turn.
// DN > 0 (one GPU, CGS, k + 1 <= DN): the panel dots <v_j, w> for j <= k
// are formed here too, from the lane's own w(i) (no re-read of w and no dots
// launch). Each workgroup block-reduces its products (store_partials); the
// last arriver of each group of `gs` workgroups sums the group's partials
// in workgroup order, so the CGS update (FROM_PARTS) sees <= 256 partials
// per column, as from k_dots_nc. Deterministic: fixed order throughout.
struct SellDots {
    int nc;            // columns: k + 1
    int gs, ng;        // workgroups per group, groups (<= kCombineGroups)
    double* wgpart;    // [c * gridDim.x + blockIdx.x]
    unsigned* cnt;     // one ticket per group (zero between launches)
    double* out;       // [c * ng + g]
};

// AT: the accumulation class, or WithBasis<A, B> for a compressed basis
// (basis.hpp; no fused dots): v_k is rounded wherever it is formed.
template <class T, class P, class VI, class CI, int W, bool WIN, bool FOLD, int DN = 0, int BS = kBlock,
          bool UNI = false, bool PIPE = false, class AT = double>
__global__ __launch_bounds__(BS) void k_step_sell(int n, int n_lo, int n_ext, int nslices, const int64_t* __restrict__ off,
                                                      const CI* __restrict__ col,
                                                      const typename SellStore<VI>::type* __restrict__ val,
                                                      const T* __restrict__ wprev, const T* __restrict__ inv_p,
                                                      T* __restrict__ V, int64_t ld, int k,
                                                      const P* __restrict__ diag, T* __restrict__ w,
                                                      GivensFold<T> fold, SellDots dd,
                                                      const int32_t* __restrict__ sbase,
                                                      const int32_t* __restrict__ spat, const int64_t* __restrict__ coff, const CI* __restrict__ pat,
                                                      const int32_t* __restrict__ xrp,
                                                      const int32_t* __restrict__ xcol,
                                                      const typename SellStore<VI>::type* __restrict__ xval,
                                                      const int8_t* __restrict__ rexp, int64_t ustride, int xcd,
                                                      const int32_t* __restrict__ rows) {
    using A = typename AccOf<AT>::type;
    using Bs = BasisOf<T, AT>;
    static_assert(DN == 0 || BS == kBlock, "the fused dots' partials assume kBlock-thread workgroups");
    static_assert(DN == 0 || std::is_same_v<A, double>, "the fused dots accumulate in fp64");
    static_assert(DN == 0 || std::is_same_v<AT, A>, "the fused dots read an uncompressed basis");
    using S = typename SellStore<VI>::type;
    constexpr int NQ = kWinLen / kWave;
    __shared__ T win[WIN ? BS / kWave : 1][WIN ? kWinLen : 1];
    const int lane = threadIdx.x & (kWave - 1), wid = wave_id();
    const int s = (xcd ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x) * (BS / kWave) + wid;
    const bool live = s < nslices;  // a dead wave still joins the fold's barriers
    const int row0 = s * kWave;
    // the lane's row: row0 + lane, or a sorted (SELL-C-sigma) copy's rows[],
    // loaded behind the slice's first batch (below); nothing before needs it
    int i = row0 + lane;
    // 0. the slice's offsets (UNI: computed) and pattern index
    SellRow<S, CI, W> row;
    if constexpr (UNI) row.init_uniform(live ? s : 0, ustride, spat, coff);
    else row.init_load(live ? s : 0, off, spat, coff);
    __builtin_amdgcn_sched_barrier(0);
    // 1. the fold's ||w||^2 partial (nparts <= kBlock, checked at launch: one per lane)
    // (a workgroup narrower than kBlock loads kBlock / BS per lane: the
    // partials keep their kBlock-lane positions, so the sums below run in
    // the same order whatever BS is)
    constexpr int NPL = BS < kBlock ? kBlock / BS : 1;
    A part[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) part[j] = A(0);
    if constexpr (FOLD) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int t = j * BS + (int)threadIdx.x;
            part[j] = (A)fold.norm2[t < fold.nparts ? t : 0];
            if (t >= fold.nparts) part[j] = A(0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // 2. w_prev window (or this row's own w_prev), raw
    T wr[WIN ? NQ : 1];
    if constexpr (WIN) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = row0 - kWinLo + q * kWave + lane;
            wr[q] = wprev[c >= n_lo && c < n_ext ? c : 0];
        }
    } else {
        if (!rows) wr[0] = wprev[i < n ? i : 0];  // the round-3 order (unsorted copies)
    }
    __builtin_amdgcn_sched_barrier(0);
    // 3. the slice's first batch (UNI: the values before the pattern index
    // is waited for, then the columns)
    if constexpr (UNI) {
        row.init_vals(lane, val);
        row.load_vals(0);
        __builtin_amdgcn_sched_barrier(0);
        row.init_finish(lane, col, val, sbase, pat);
        row.load_cols(0);
    } else {
        row.init_finish(lane, col, val, sbase, pat);
        row.load(0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // 3b. without the window, sorted (SELL-C-sigma) copies: the lane's row and
    // its own w_prev, behind the first batch (needed last)
    if constexpr (!WIN) {
        if (rows) {
            i = rows[live ? row0 + lane : 0];
            wr[0] = wprev[i < n ? i : 0];
        }
    }
    // 4. a scaled fp16 copy's row exponent (needed last, issued last)
    int rex = 0;
    if constexpr (std::is_same_v<VI, half_v>) {
        if (rexp) rex = rexp[live && i < n ? i : 0];
    }
    __builtin_amdgcn_sched_barrier(0);
    // the scale 1/h_{k,k-1}: the folded Givens step, or the Givens kernel's
    T inv;
    // the folded step's ||w||^2; workgroup 0 runs the rotation step with it
    // after its own rows (nothing in this launch reads what the rotation
    // writes, and its serial chain then holds none of the slice's loads live)
    double nrm2sq = 0.0;
    if constexpr (FOLD) {
        constexpr int NG = (BS < kBlock ? kBlock : BS) / kWave;
        __shared__ A scratch[NG];
        __shared__ T inv_s;
        if (fold.nparts > 0) {
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                const A v = wave_sum(part[j] + A(0));  // the same fixed order in every workgroup
                if (lane == 0) scratch[j * (BS / kWave) + wid] = v;
            }
            lds_barrier();
            A r = A(0);
#pragma unroll
            for (int q = 0; q < NG; ++q) r += scratch[q];
            nrm2sq = (double)r;
        } else {
            nrm2sq = fold.norm2[0];
        }
        if (threadIdx.x == 0) inv_s = inv_of_norm2<T>(nrm2sq);
        lds_barrier();
        inv = inv_s;
    } else {
        inv = *inv_p;
    }
    // with dots, a dead wave joins the partials' barriers; with the fold,
    // workgroup 0's waves all join the rotation step's barriers at the end
    if (DN == 0 && !live && !(FOLD && blockIdx.x == 0)) return;
    A sum = A(0);
    T vk = T(0);  // v_k(i) = T(w_prev(i) * inv)
    if (live) {
        if constexpr (WIN) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = row0 - kWinLo + q * kWave + lane;
                win[wid][q * kWave + lane] = (c >= n_lo && c < n_ext) ? Bs::round((T)(wr[q] * inv)) : T(0);
            }
            wave_lds_sync();
            auto xv = [&](int c) { return (double)win[wid][c - row0 + kWinLo]; };
            row.sum(0, xv, sum);
            for (int q = row.U; q < row.steps; q += row.U) {
                row.load(q);
                row.sum(q, xv, sum);
            }
            vk = win[wid][lane + kWinLo];
        } else {
            auto xv = [&](int c) { return (double)Bs::round((T)(wprev[c] * inv)); };
            if (SellCol<CI>::stepped && row.exc) {
                sum = csr_row_sum<A>(i < n ? row.xrow : -1, xrp, xcol, xval, xv);
            } else if constexpr (PIPE) {
                // two batch buffers: batch q's gathers are issued, then batch
                // q + U's loads, so the wait for the gathers leaves the next
                // batch's loads in flight under the sums (one HBM round trip
                // per batch instead of a load round trip then a gather round
                // trip). x is gathered raw and scaled at the sum: the same
                // (T)(w_prev * inv) operand, the same bits.
                using Row = SellRow<S, CI, W>;
                Row rb;
                rb.geom_from(row);
                auto xraw = [&](int c) { return wprev[c]; };
                auto xs = [&](T r) { return (double)Bs::round((T)(r * inv)); };
                T x[Row::U][W];
                for (int q = 0;;) {
                    row.gather(xraw, x);
                    __builtin_amdgcn_sched_barrier(0);
                    rb.load(q + Row::U);
                    __builtin_amdgcn_sched_barrier(0);
                    row.sum_gathered(q, x, xs, sum);
                    q += Row::U;
                    if (q >= row.steps) break;
                    rb.gather(xraw, x);
                    __builtin_amdgcn_sched_barrier(0);
                    row.load(q + Row::U);
                    __builtin_amdgcn_sched_barrier(0);
                    rb.sum_gathered(q, x, xs, sum);
                    q += Row::U;
                    if (q >= row.steps) break;
                }
            } else {
                row.sum(0, xv, sum);
                for (int q = row.U; q < row.steps; q += row.U) {
                    row.load(q);
                    row.sum(q, xv, sum);
                }
            }
            vk = Bs::round((T)(wr[0] * inv));
        }
    }
    T wi = T(0);
    if (live && i < n) {
        if constexpr (std::is_same_v<VI, half_v>) sum = ldexp(sum, -rex);  // exact unscale (0: unchanged)
        const T t = (T)sum;  // spmv(1, A, v, 0, w): y = 1*t
        wi = precond<T, P>(t, diag, i);
        w[i] = wi;
        Bs::store(basis_ptr<Bs>(V) + (int64_t)k * ld + i, vk);
    }
    if constexpr (DN > 0) {
        // the earlier basis columns at this row: clamped, branch-free loads
        // issued together (one latency), then one product per column
        // (n >= 1: spmv_impl refuses the fused dots on an empty block, so row n - 1 exists)
        const bool own_row = live && i < n;
        const int ic = i < n ? i : n - 1;
        const int kc = k > 0 ? k - 1 : 0;
        T vc[DN];
#pragma unroll
        for (int c = 0; c < DN; ++c) vc[c] = V[(int64_t)(c < kc ? c : kc) * ld + ic];
        __builtin_amdgcn_sched_barrier(0);
        const double wd = (double)wi;
        double acc[DN];
        // a lane without a row contributes an exact 0 (not a clamped row's
        // value times 0, which is NaN when that value is Inf or NaN)
#pragma unroll
        for (int c = 0; c < DN; ++c)
            acc[c] = own_row ? (c < k ? (double)vc[c] : c == k ? (double)vk : 0.0) * wd : 0.0;
        store_partials<DN, kBlock, true>(acc, dd.nc, dd.wgpart);
        const int g = blockIdx.x / dd.gs;
        const int m0 = g * dd.gs, m1 = m0 + dd.gs < (int)gridDim.x ? m0 + dd.gs : (int)gridDim.x;
        if (last_arriver_of(dd.cnt + g, (unsigned)(m1 - m0)) && (int)threadIdx.x < dd.nc) {
            const int c = threadIdx.x;
            double v = 0.0;
            for (int m = m0; m < m1; ++m) v += dd.wgpart[(size_t)c * gridDim.x + m];
            dd.out[(size_t)c * dd.ng + g] = v;
        }
    }
    if constexpr (FOLD) {
        __shared__ T col_s[kFoldMaxM + 2], c_s[kFoldMaxM + 2], s_s[kFoldMaxM + 2];
        if (blockIdx.x == 0) givens_block(fold.g, nrm2sq, col_s, c_s, s_s);
    }
}

// k_step_sell with two adjacent slices per wave (lane l owns rows
// 128 s' + l and 128 s' + 64 + l): every load of both slices -- one LDS
// window of 64 + 128 + 64 entries for the pair, both slices' first batches --
// is in flight before the wave waits for any, so each wave carries twice the
// bytes through the same fixed work (the fold's partial sum, the barriers,
// the window). Past the Infinity Cache a slice's loads alone do not keep
// enough bytes in flight per CU (MI355X_MICROARCH.md: ~72 KiB per CU hides
// an HBM miss). Same sums in the same order as k_step_sell: same bits.
// AT: as k_step_sell's.
template <class T, class P, class VI, int W, bool WIN, bool FOLD, int BE, int BS = kBlock, bool PG = true,
          class AT = double>
__global__ __launch_bounds__(BS) void k_step_sell2(int n, int n_lo, int n_ext, int nslices, const int64_t* __restrict__ off,
                                                   const int16_t* __restrict__ col,
                                                   const typename SellStore<VI>::type* __restrict__ val,
                                                   const T* __restrict__ wprev, const T* __restrict__ inv_p,
                                                   T* __restrict__ V, int64_t ld, int k,
                                                   const P* __restrict__ diag, T* __restrict__ w,
                                                   GivensFold<T> fold, SellDots,
                                                   const int32_t* __restrict__ sbase,
                                                   const int32_t* __restrict__ spat, const int64_t* __restrict__ coff, const int16_t* __restrict__ pat,
                                                   const int32_t* __restrict__ xrp,
                                                   const int32_t* __restrict__ xcol,
                                                   const typename SellStore<VI>::type* __restrict__ xval,
                                                   const int8_t* __restrict__ rexp, int64_t ustride, int xcd) {
    using A = typename AccOf<AT>::type;
    using Bs = BasisOf<T, AT>;
    using S = typename SellStore<VI>::type;
    using CI = int16_t;
    constexpr bool UNI = true;
    constexpr int SPW = 2;
    constexpr int WL = kWinLen + (SPW - 1) * kWave;  // the pair's window
    constexpr int NQ = WL / kWave;
    __shared__ T win[WIN ? BS / kWave : 1][WIN ? WL : 1];
    const int lane = threadIdx.x & (kWave - 1), wid = wave_id();
    const int s0 = ((xcd ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x) * (BS / kWave) + wid) * SPW;
    const bool live = s0 < nslices;  // a dead wave still joins the fold's barriers
    bool live_p[SPW];
    const int row0 = s0 * kWave;
    // 0. both slices' offsets (UNI: computed) and pattern indices
    SellRow<S, CI, W, (MPG_SELL_NT != 0), BE> row[SPW];
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        live_p[p] = s0 + p < nslices;
        const int sp = live_p[p] ? s0 + p : 0;
        if constexpr (UNI) row[p].init_uniform(sp, ustride, spat, coff);
        else row[p].init_load(sp, off, spat, coff);
    }
    __builtin_amdgcn_sched_barrier(0);
    // 1. the fold's ||w||^2 partial (one per lane, as k_step_sell)
    constexpr int NPL = BS < kBlock ? kBlock / BS : 1;
    A part[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) part[j] = A(0);
    if constexpr (FOLD) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int t = j * BS + (int)threadIdx.x;
            part[j] = (A)fold.norm2[t < fold.nparts ? t : 0];
            if (t >= fold.nparts) part[j] = A(0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // 2. the pair's w_prev window (or the lane's own rows' w_prev), raw
    T wr[WIN ? NQ : SPW];
    if constexpr (WIN) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = row0 - kWinLo + q * kWave + lane;
            wr[q] = wprev[c >= n_lo && c < n_ext ? c : 0];
        }
    } else {
#pragma unroll
        for (int p = 0; p < SPW; ++p) {
            const int i = row0 + p * kWave + lane;
            wr[p] = wprev[i < n ? i : 0];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // 3. both slices' first batches (UNI: values first, then the columns)
    if constexpr (UNI) {
#pragma unroll
        for (int p = 0; p < SPW; ++p) {
            row[p].init_vals(lane, val);
            row[p].load_vals(0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < SPW; ++p) {
            row[p].init_finish(lane, col, val, sbase, pat);
            row[p].load_cols(0);
        }
    } else {
#pragma unroll
        for (int p = 0; p < SPW; ++p) {
            row[p].init_finish(lane, col, val, sbase, pat);
            row[p].load(0);
        }
    }
    // 4. a scaled fp16 copy's row exponents
    int rex[SPW] = {};
    if constexpr (std::is_same_v<VI, half_v>) {
        if (rexp) {
#pragma unroll
            for (int p = 0; p < SPW; ++p) {
                const int i = row0 + p * kWave + lane;
                rex[p] = rexp[live_p[p] && i < n ? i : 0];
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // 5. PG, no window: the first batch's gathers of w_prev, raw, issued
    // before the scale is known (the fold's sums and barriers), and scaled
    // at the sum: (T)(w_prev * inv), the same operation, the same bits.
    // A dead wave gathers for slice 0 (valid addresses) and returns.
    constexpr bool PRE = PG && !WIN;
    using RowT = SellRow<S, CI, W, (MPG_SELL_NT != 0), BE>;
    T xr[PRE ? SPW : 1][PRE ? RowT::U : 1][PRE ? W : 1];
    if constexpr (PRE) {
#pragma unroll
        for (int p = 0; p < SPW; ++p) row[p].gather([&](int c) { return wprev[c]; }, xr[p]);
    }
    __builtin_amdgcn_sched_barrier(0);
    T inv;
    double nrm2sq = 0.0;
    if constexpr (FOLD) {
        constexpr int NG = (BS < kBlock ? kBlock : BS) / kWave;
        __shared__ A scratch[NG];
        __shared__ T inv_s;
        if (fold.nparts > 0) {
#pragma unroll
            for (int j = 0; j < NPL; ++j) {
                const A v = wave_sum(part[j] + A(0));
                if (lane == 0) scratch[j * (BS / kWave) + wid] = v;
            }
            lds_barrier();
            A r = A(0);
#pragma unroll
            for (int q = 0; q < NG; ++q) r += scratch[q];
            nrm2sq = (double)r;
        } else {
            nrm2sq = fold.norm2[0];
        }
        if (threadIdx.x == 0) inv_s = inv_of_norm2<T>(nrm2sq);
        lds_barrier();
        inv = inv_s;
    } else {
        inv = *inv_p;
    }
    if (!live && !(FOLD && blockIdx.x == 0)) return;
    A sum[SPW] = {};
    T vk[SPW] = {};
    if (live) {
        if constexpr (WIN) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = row0 - kWinLo + q * kWave + lane;
                win[wid][q * kWave + lane] = (c >= n_lo && c < n_ext) ? Bs::round((T)(wr[q] * inv)) : T(0);
            }
            wave_lds_sync();
            auto xv = [&](int c) { return (double)win[wid][c - row0 + kWinLo]; };
#pragma unroll
            for (int p = 0; p < SPW; ++p) row[p].sum(0, xv, sum[p]);
#pragma unroll
            for (int p = 0; p < SPW; ++p) {
                for (int q = row[p].U; q < row[p].steps; q += row[p].U) {
                    row[p].load(q);
                    row[p].sum(q, xv, sum[p]);
                }
                vk[p] = win[wid][p * kWave + lane + kWinLo];
            }
        } else {
            auto xv = [&](int c) { return (double)Bs::round((T)(wprev[c] * inv)); };
#pragma unroll
            for (int p = 0; p < SPW; ++p) {
                const int i = row0 + p * kWave + lane;
                if (SellCol<CI>::stepped && row[p].exc) {
                    sum[p] = csr_row_sum<A>(live_p[p] && i < n ? row[p].xrow : -1, xrp, xcol, xval, xv);
                } else {
                    if constexpr (PRE) row[p].sum_gathered(0, xr[p], [&](T r) { return (double)Bs::round((T)(r * inv)); }, sum[p]);
                    else row[p].sum(0, xv, sum[p]);
                    for (int q = row[p].U; q < row[p].steps; q += row[p].U) {
                        row[p].load(q);
                        row[p].sum(q, xv, sum[p]);
                    }
                }
                vk[p] = Bs::round((T)(wr[p] * inv));
            }
        }
    }
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        const int i = row0 + p * kWave + lane;
        if (live_p[p] && i < n) {
            double sp = sum[p];
            if constexpr (std::is_same_v<VI, half_v>) sp = ldexp(sp, -rex[p]);
            const T t = (T)sp;
            w[i] = precond<T, P>(t, diag, i);
            Bs::store(basis_ptr<Bs>(V) + (int64_t)k * ld + i, vk[p]);
        }
    }
    if constexpr (FOLD) {
        __shared__ T col_s[kFoldMaxM + 2], c_s[kFoldMaxM + 2], s_s[kFoldMaxM + 2];
        if (blockIdx.x == 0) givens_block(fold.g, nrm2sq, col_s, c_s, s_s);
    }
}

}  // namespace
