// The Gram-Schmidt panel dots V^T w of the fused Arnoldi cycle (per-workgroup
// fp64 partials), and the launch that runs step k's SpMV ahead of them
// (k_step_dots).
#pragma once

#include "arnoldi_spmv.hpp"

namespace {

// Tall-skinny panel reduction: partial <v_j, w> for j in [c0, c0 + nc),
// nc <= kNC, over all local rows. Each lane owns 4 consecutive rows per
// iteration (16-B loads of every column: V's leading dimension is padded to
// 256 B), issues all column loads before its FMAs, and keeps one fp64
// accumulator per column; store_partials does the wave64/LDS combine.
// BS threads per workgroup. COMBINE (one GPU, nc <= kNC, c0 == 0): the
// partials go write-through and the last-arriving workgroup sums them into
// sums[0..nc) itself — no separate reduce launch (BS = 1024, so one
// workgroup per CU keeps the partial count at 256 per column).
template <class T, int BS = kBlock, bool COMBINE = false, class A = double>
__global__ __launch_bounds__(BS) void k_panel_dots(int n, const T* __restrict__ V, int64_t ld, int c0, int nc,
                                                   const T* __restrict__ w, double* __restrict__ partial,
                                                   unsigned* __restrict__ cnt, double* __restrict__ sums) {
    A acc[kNC];
#pragma unroll
    for (int c = 0; c < kNC; ++c) acc[c] = A(0);
    const int n4 = n & ~3;
    const T* __restrict__ Vb = V + (int64_t)c0 * ld;
    for (int i = 4 * (blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * gridDim.x * BS) {
        A wv[4];
        Row4<T>::load(w + i, wv);
#pragma unroll
        for (int c = 0; c < kNC; ++c) {
            if (c < nc) {
                A v[4];
                Row4<T>::load(Vb + (int64_t)c * ld + i, v);
                acc[c] += v[0] * wv[0] + v[1] * wv[1] + v[2] * wv[2] + v[3] * wv[3];
            }
        }
    }
    // tail rows (n not a multiple of 4)
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        const A wi = (A)w[i];
#pragma unroll
        for (int c = 0; c < kNC; ++c)
            if (c < nc) acc[c] += (A)Vb[(int64_t)c * ld + i] * wi;
    }
    store_partials<kNC, BS, COMBINE>(acc, nc, partial + (size_t)c0 * gridDim.x);
    if constexpr (COMBINE) {
        if (last_arriver(cnt)) combine_columns<BS, A>(partial, gridDim.x, nc, sums);
    }
}

// The one-panel forms of the dots and the CGS update with the column count
// NC a compile-time constant (the captured cycle knows k at every step):
// every column index is static, so the loads of a batch of columns issue
// back to back and the accumulators stay in registers. With a runtime
// count the compiler guarded each column's load with its own branch and
// waited for it before the next (one memory latency per column: t(k) =
// 8.6 + 0.50 k us for the dots on BAND-10M, tools/per_step.py).
// Where dots_panel_from reads w and the newest column V(:, NC - 1) from. DotsGlobal:
// global memory (k_dots_nc, k_dots_panels). A staged source (k_step_dots,
// DotsStaged) hands out the workgroup's own rows of both from LDS, where the
// SpMV phase of the same launch left them, and may hold the lane's first
// batch of earlier columns, loaded ahead of that phase (kHeld > 0: columns
// 0..kHeld-1 of the lane's first row group, in held[]).
// BT: the basis' storage (basis.hpp): V is read as stored, 4 rows per load
// (8 bytes of a compressed basis, twice the columns per batch), and used as
// Basis<T, BT>::Raw4::at gives it: the same products in the same order.
template <class T, class A, class BT = T>
struct DotsGlobal {
    static constexpr bool kStaged = false;
    static constexpr int kHeld = 0;
    using R4 = typename Basis<T, BT>::Raw4;
    const T* __restrict__ w;
    R4 held[1];
    __device__ __forceinline__ void load_w(int i, A (&wv)[4]) const { Row4<T>::load(w + i, wv); }
    __device__ __forceinline__ R4 newest(int) const { return R4(); }
};

template <class T, int BS, int NC, class A = double, class BT = T, class SRC>
__device__ __forceinline__ void dots_panel_from(int n, const typename Basis<T, BT>::elem* __restrict__ V, int64_t ld,
                                           const SRC& src, double* __restrict__ partial, unsigned G = gridDim.x) {
    static_assert(NC >= 1 && NC <= kNC, "one panel");
    using Bs = Basis<T, BT>;
    constexpr int NP = Pow2Ceil<NC>::v;
    // (a compressed basis doubles the batch in the fp32 class only: with 32 fp64
    // accumulators the 16-column batch spilled, 12 B of scratch per lane)
    constexpr int B = sizeof(A) == 8 ? kColBatch<T> : Bs::kBatch;
    A acc[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) acc[c] = A(0);
    const int n4 = n & ~3;
    bool first = SRC::kHeld > 0;
    for (int i = 4 * (blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * gridDim.x * BS) {
        A wv[4];
        src.load_w(i, wv);
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += B) {
            typename Bs::Raw4 v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) {
                    if (SRC::kStaged && c0 + u == NC - 1) v[u] = src.newest(i);
                    else if (c0 + u < SRC::kHeld && first) v[u] = src.held[c0 + u < SRC::kHeld ? c0 + u : 0];
                    else v[u].load(V + (int64_t)(c0 + u) * ld + i);
                }
            __builtin_amdgcn_sched_barrier(0);  // keep the batch's loads issued back to back
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC)
                    acc[c0 + u] += v[u].template at<A>(0) * wv[0] + v[u].template at<A>(1) * wv[1] +
                                   v[u].template at<A>(2) * wv[2] + v[u].template at<A>(3) * wv[3];
            // the next batch's loads after this batch's adds: without it the
            // fp32 class's NC = 32 form issued all 32 columns' loads first
            // (128 VGPRs, 180 B of scratch per lane)
            asm volatile("" : "+v"(acc[c0]) : : "memory");
        }
        if constexpr (SRC::kHeld > 0) first = false;
    }
    // tail rows (n not a multiple of 4; a staged source runs only where there are none)
    if constexpr (!SRC::kStaged) {
        for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
            const A wi = (A)src.w[i];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += Bs::template get<A>(V + (int64_t)c * ld + i) * wi;
        }
    }
    store_partials<NP, BS>(acc, NC, partial, G);
}

template <class T, int BS, int NC, class A = double, class BT = T>
__device__ __forceinline__ void dots_panel(int n, const typename Basis<T, BT>::elem* __restrict__ V, int64_t ld,
                                           const T* __restrict__ w, double* __restrict__ partial) {
    dots_panel_from<T, BS, NC, A, BT>(n, V, ld, DotsGlobal<T, A, BT>{w, {}}, partial);
}

// AT: the accumulation class, or WithBasis<A, B> for a compressed basis
// (basis.hpp), read as stored through basis_ptr.
template <class T, int BS, int NC, bool STAMP = false, class AT = double>
__global__ __launch_bounds__(BS) void k_dots_nc(int n, const T* __restrict__ V, int64_t ld,
                                                const T* __restrict__ w, double* __restrict__ partial,
                                                unsigned long long* stamp) {
    using A = typename AccOf<AT>::type;
    using Bs = BasisOf<T, AT>;
    stamp_at<STAMP>(stamp, 0);
    dots_panel<T, BS, NC, A, typename AccOf<AT>::template basis<T>>(n, basis_ptr<Bs>(V), ld, w, partial);
    stamp_at<STAMP>(stamp, 1);
}

// ---------------------------------------------------------------- step: SpMV + panel dots
// The Arnoldi SpMV of step k inside the panel dots' launch (fp32 basis and
// values, the uniform pair storage with the v_k window; one pass: n <= 4096
// kCombineGroups, n % 4 == 0). The grid and the row ownership are k_dots_nc's:
// workgroup b (1024 threads) owns rows [4096 b, 4096 b + 4096), lane t the row
// group 4 (1024 b + t) -- 64 whole SELL-64 slices, four per wave. Each wave
// forms v_k = T(w_prev * inv) for its 256 rows and 64 on either side in an
// LDS window of its own (every gather of its slices falls inside; the rows
// beside its own are the neighbouring wave's, scaled again by the same
// operation), runs k_step_sell2's row sums on it, stores w and v_k, and leaves
// its rows of w in LDS. dots_panel then runs on the staged w and v_k and the
// global V(:, 0..k-1): the same products, the same order and the same Gd
// partials per column as k_dots_nc after k_step_sell2, with no second launch
// and no re-read of w and v_k. PF: the lane's first batch of earlier columns
// is issued behind the slices' loads, so its latency runs under the row sums.
// FOLD: every wave sums the <= kBlock ||w||^2 partials itself, with the
// butterflies and in the order of k_step_sell2's waves 0..3.
// The waves of a workgroup do not wait for one another before the partial
// combine at the end (store_partials): with the three workgroup barriers this
// kernel first had (the fold, one shared window, the hand-off to the dots)
// the earliest wave waited for the latest three times over.
constexpr int kStepDotsRows = 4 * kCombineBlock;  // rows of a workgroup

template <class T, class A, int HELD>
struct DotsStaged {
    static constexpr bool kStaged = true;
    static constexpr int kHeld = HELD;
    const T* wst;   // LDS: w of this wave's rows
    const T* vkst;  // LDS: v_k of this wave's rows
    int base;       // its first row
    Raw4<T> held[HELD > 0 ? HELD : 1];
    __device__ __forceinline__ void load_w(int i, A (&wv)[4]) const { Row4<T>::load(wst + (i - base), wv); }
    __device__ __forceinline__ Raw4<T> newest(int i) const {
        Raw4<T> r;
        r.load(vkst + (i - base));
        return r;
    }
};

// LDS written by a wave and read back by other lanes of the same wave: the
// wave's own LDS operations complete (lgkmcnt(0); vmcnt and expcnt untouched,
// so loads issued ahead stay in flight), and neither the compiler nor the
// hardware moves an LDS access across.
__device__ __forceinline__ void wave_lds_handoff() {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    wave_lds_sync();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// FOLD launches one workgroup more than the dots' grid, the rider: the last
// block index runs Givens step k - 1 (givens_block) and nothing else, beside
// the SpMV phase of the others -- on a CU the grid leaves free while it has
// fewer workgroups than the chip has CUs, behind the first workgroup to
// retire otherwise. (At the end of workgroup 0, where the split kernels carry
// the step, it was this launch's tail: one workgroup per CU, all of them
// ending together, and every CU but one waiting for the rotation chain of one
// lane.) The rider stores no partials: the others store G = gridDim.x - 1 per
// column, and nothing they read is written by it.
template <class T, class P, int W, bool FOLD, int BE, int NC, bool PF, class A>
__global__ __launch_bounds__(kCombineBlock) void k_step_dots(int n, int nslices, const int16_t* __restrict__ col,
                                                             const T* __restrict__ val, const T* __restrict__ wprev,
                                                             const T* __restrict__ inv_p, T* __restrict__ V,
                                                             int64_t ld, int k, const P* __restrict__ diag,
                                                             T* __restrict__ w, GivensFold<T> fold,
                                                             const int32_t* __restrict__ spat,
                                                             const int64_t* __restrict__ coff,
                                                             const int16_t* __restrict__ pat, int64_t ustride,
                                                             double* __restrict__ dpart) {
    static_assert(std::is_same_v<T, float>, "fp32 basis and values");
    using CI = int16_t;
    using Row = SellRow<T, CI, W, (MPG_SELL_NT != 0), BE>;
    constexpr int BS = kCombineBlock, SPW = 4, NW = BS / kWave;
    constexpr int RB = kStepDotsRows, RW = SPW * kWave;  // rows of the workgroup, of a wave
    constexpr int WL = kWinLo + RW + kWinHi;             // a wave's window of v_k
    // The wave's four slices are the rows its lanes take in dots_panel_from:
    // wave wid owns slices s0..s0+3 = rows [base + RW wid, base + RW wid + RW),
    // and lane `lane` of that wave reads the row group base + 4 (kWave wid +
    // lane) of w and v_k there. So both go from the SpMV phase to the dots
    // inside one wave, and no wave waits for another before the final combine.
    static_assert(NW * RW == RB, "four slices per wave cover the workgroup's rows");
    static_assert(RW == 4 * kWave, "a wave's slices are its lanes' row groups of dots_panel_from");
    __shared__ __attribute__((aligned(16))) T win[NW][WL];
    __shared__ __attribute__((aligned(16))) T wst[RB];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = wave_id();
    constexpr int NG = kBlock / kWave;
    if constexpr (FOLD) {
        if (blockIdx.x == gridDim.x - 1) {  // the rider
            __shared__ T col_s[kFoldMaxM + 2], c_s[kFoldMaxM + 2], s_s[kFoldMaxM + 2];
            A part[NG];
            fold_parts_load(fold, lane, part);
            givens_block(fold.g, fold_parts_sum(fold, part), col_s, c_s, s_s);
            return;
        }
    }
    const unsigned G = FOLD ? gridDim.x - 1 : gridDim.x;  // workgroups with rows
    const int base = (int)blockIdx.x * RB;
    const int row0 = base + wid * RW;  // the wave's first row
    const int s0 = (int)blockIdx.x * (RB / kWave) + wid * SPW;
    // 0. the slices' offsets (computed) and pattern indices
    Row row[SPW];
    bool live_p[SPW];
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        live_p[p] = s0 + p < nslices;  // (a dead wave runs on slice 0's addresses and reaches the final combine)
        row[p].init_uniform(live_p[p] ? s0 + p : 0, ustride, spat, coff);
    }
    __builtin_amdgcn_sched_barrier(0);
    // 1. the fold's ||w||^2 partials
    A part[NG];
    if constexpr (FOLD) fold_parts_load(fold, lane, part);
    __builtin_amdgcn_sched_barrier(0);
    // 2. the wave's window of w_prev, raw: the lane's own row group and one
    // entry each of the 64 rows below and above the wave's (clamped addresses;
    // n % 4 == 0, so a row group lies inside [0, n) or outside)
    const int i4 = base + 4 * tid;
    const bool in4 = i4 < n;
    Raw4<T> wr;
    wr.load(wprev + (in4 ? i4 : 0));
    const int clo = row0 - kWinLo + lane, chi = row0 + RW + lane;
    const bool lo_in = clo >= 0 && clo < n, hi_in = chi < n;
    const T wlo = wprev[lo_in ? clo : 0];
    const T whi = wprev[hi_in ? chi : 0];
    __builtin_amdgcn_sched_barrier(0);
    // 3. the slices' first batches: values first, then the columns
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        row[p].init_vals(lane, val);
        row[p].load_vals(0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        row[p].init_finish(lane, col, val, nullptr, pat);
        row[p].load_cols(0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // 4. PF: the dots' first batch of earlier columns at the lane's row group
    constexpr int B = kColBatch<T>;
    // (with the fold 6 columns: 8 held across the partial sums spilled, 20-28 B per lane)
    constexpr int HMAX = FOLD ? 6 : B;
    constexpr int HELD = !PF ? 0 : NC - 1 < HMAX ? NC - 1 : HMAX;
    T* const wwin = win[wid];  // the wave's own rows sit at wwin + kWinLo
    DotsStaged<T, A, HELD> src;
    src.wst = wst + wid * RW;
    src.vkst = wwin + kWinLo;
    src.base = row0;
    if constexpr (HELD > 0) {
#pragma unroll
        for (int u = 0; u < HELD; ++u) src.held[u].load(V + (int64_t)u * ld + (in4 ? i4 : 0));
    }
    __builtin_amdgcn_sched_barrier(0);
    T inv;
    if constexpr (FOLD) inv = inv_of_norm2<T>(fold_parts_sum(fold, part));  // (the rider's value, formed per wave)
    else inv = *inv_p;
    // the window of v_k = T(w_prev * inv), zero outside [0, n)
    {
        T vq[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) vq[r] = in4 ? (T)(wr.template at<T>(r) * inv) : T(0);
        Row4<T>::store(wwin + kWinLo + 4 * lane, vq);
        wwin[lane] = lo_in ? (T)(wlo * inv) : T(0);
        wwin[kWinLo + RW + lane] = hi_in ? (T)(whi * inv) : T(0);
    }
    wave_lds_handoff();  // the window is the wave's own
    auto xv = [&](int c) { return (double)wwin[c - row0 + kWinLo]; };
    A sum[SPW] = {};
#pragma unroll
    for (int p = 0; p < SPW; ++p)
        if (live_p[p]) row[p].sum(0, xv, sum[p]);
#pragma unroll
    for (int p = 0; p < SPW; ++p) {
        if (live_p[p])
            for (int q = Row::U; q < row[p].steps; q += Row::U) {
                row[p].load(q);
                row[p].sum(q, xv, sum[p]);
            }
        const int i = (s0 + p) * kWave + lane;
        T wi = T(0);
        if (live_p[p] && i < n) {
            const T t = (T)sum[p];  // spmv(1, A, v, 0, w): y = 1*t
            wi = precond<T, P>(t, diag, i);
            // (plain dword stores: as two 16-B write-through stores per lane behind the
            // hand-off below, which leave the launch's end nothing to flush, the kernel
            // took 0.3 us longer and the bench lost 0.6 %, profiles/r12_step_tail/)
            w[i] = wi;
            V[(int64_t)k * ld + i] = wwin[i - row0 + kWinLo];
        }
        wst[i - base] = wi;  // rows past n: an exact 0, and no row group of theirs is read
    }
    wave_lds_handoff();  // the wave's rows of w and v_k go to its own lanes (the identity above)
    dots_panel_from<T, BS, NC, A>(n, V, ld, src, dpart, G);
}

// V^T w for nc > kNC columns in ONE launch (GMRES(100): the round-3 form ran
// one runtime-count k_panel_dots launch per 32 columns, each re-reading w and
// waiting for every column in turn): blockIdx.y is the 32-column panel,
// the last one holding NCL columns; blockIdx.x a row group. The grid keeps
// about one workgroup per CU in total (gridDim.x = kCombineGroups / panels),
// so each column gets gridDim.x <= 128 partials, [column][gridDim.x], which
// the wide CGS update sums itself (k_cgs_update_wide).
template <class T, int BS, int NCL, class A = double>
__global__ __launch_bounds__(BS) void k_dots_panels(int n, const T* __restrict__ V, int64_t ld,
                                                    const T* __restrict__ w, double* __restrict__ partial) {
    const int c0 = blockIdx.y * kNC;
    double* __restrict__ part = partial + (size_t)c0 * gridDim.x;
    if (blockIdx.y + 1 < gridDim.y) dots_panel<T, BS, kNC, A>(n, V + (int64_t)c0 * ld, ld, w, part);
    else dots_panel<T, BS, NCL, A>(n, V + (int64_t)c0 * ld, ld, w, part);
}

}  // namespace
