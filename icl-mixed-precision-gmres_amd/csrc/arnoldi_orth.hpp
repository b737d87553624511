// The CGS / MGS update kernels of the fused Arnoldi cycle: w = w - T(V coef),
// and the next partials (||w'||^2, or CGSR's second dots).
#pragma once

#include "arnoldi_givens.hpp"
#include "basis.hpp"
#include "lds_ring.hpp"
#include "panel.hpp"

namespace {

// coef = T(sums[0..NC)); w = w - T(V coef); partial ||w'||^2 (the last
// CGS pass; same arithmetic and order as k_cgs_update).
// FROM_PARTS (one GPU): the coefficients are summed here from the one-panel
// dots' part_G <= kCombineGroups partials per column (32 lanes per column,
// each summing its 8 strided partials in g order, then a 32-lane xor tree:
// the same fixed order in every workgroup) instead of a reduce launch. The 8
// loads per lane are branch-free so they issue together: one latency.
// NEXT_DOTS (CGSR's first pass): the partials of <v_j, w'> for j < NC
// instead of ||w'||^2, from a second batched pass over the lane's columns.
// PF (with FROM_PARTS): the lane's first row group -- w and the first batch
// of basis columns, raw and unconditional (clamped row) -- is issued right
// behind the partial loads, so its memory latency runs under the coefficient
// sums; the coefficients are published with an LDS-only barrier
// (__syncthreads would drain those loads). Same operands, same order.
// STREAM (with FROM_PARTS, fp32 basis and class): the lane's first row group
// streams its basis columns through a ring of LDS slots (cgs_stream_*,
// above): w and the first kStreamSlots columns are requested right behind
// the partial loads, a slot is refilled with column c + R as soon as column
// c has been read out of it, and each column is retired by a counted vmcnt,
// so the lane keeps R columns in flight until the last one is requested.
// The partials are loaded outside the compiler's wait bookkeeping (it would
// wait vmcnt(0) at their first use and drain the ring). Same operands, the
// columns added in the same ascending order.
// AT: the accumulation class, or WithBasis<A, B> for a compressed basis
// (basis.hpp), which takes the plain forms only (no PF, no STREAM: both hold
// or stream an fp32 basis), its columns read as stored, 4 rows per 8-byte
// load, twice the columns per batch.
template <class T, int BS, int NC, bool FROM_PARTS = false, bool NEXT_DOTS = false, bool PF = false,
          bool STAMP = false, class AT = double, bool STREAM = false>
__global__ __launch_bounds__(BS) void k_cgs_update_nc(int n, const T* __restrict__ V_, int64_t ld,
                                                      const double* __restrict__ sums, int part_G,
                                                      T* __restrict__ coef_out, T* __restrict__ w,
                                                      double* __restrict__ partial, unsigned long long* stamp) {
    using A = typename AccOf<AT>::type;
    using Bs = BasisOf<T, AT>;
    const typename Bs::elem* __restrict__ V = basis_ptr<Bs>(V_);
    static_assert(NC >= 1 && NC <= kNC, "one panel");
    stamp_at<STAMP>(stamp, 0);
    static_assert(!FROM_PARTS || BS >= 32 * NC, "32 lanes per column");
    static_assert(!PF || (FROM_PARTS && !NEXT_DOTS), "prefetch under the partial sums");
    static_assert(!PF || NC <= kColBatch<T>, "the prefetch form holds one batch of columns (the only form run)");
    static_assert(!STREAM || (FROM_PARTS && !NEXT_DOTS && !PF && !STAMP && sizeof(T) == 4 && sizeof(A) == 4),
                  "the streaming form: the last pass with in-launch sums, fp32 basis, fp32 class");
    static_assert(std::is_same_v<AT, A> || (!PF && !STREAM), "fp32 basis only");
    constexpr int B = Bs::kBatch;
    constexpr int B0 = NC < B ? NC : B;
    constexpr int R = NC < kStreamSlots ? NC : kStreamSlots;  // the ring's depth
    __shared__ A coef[NC];
    const int n4 = n & ~3;
    const int i_first = 4 * (blockIdx.x * BS + threadIdx.x);
    Raw4<T> pw;
    typename Bs::Raw4 pv[PF ? B0 : 1];
    // clamped row of the early requests: every lane reads valid memory
    const int ip = i_first < n4 ? i_first : 0;
    unsigned ring_lane = 0;  // LDS byte address of this lane's 16 bytes of slot 0
    if constexpr (FROM_PARTS) {
        const int j = threadIdx.x / 32, sub = threadIdx.x % 32;
        const int jc = j < NC ? j : NC - 1;
        constexpr int Q = kCombineGroups / 32;
        A pp[Q];
        if constexpr (STREAM) {
            static_assert(Q == 8, "cgs_stream_wait_partials names 8 loads");
            double pd[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int g = sub + 32 * q;
                pd[q] = cgs_stream_load_partial(sums + (size_t)jc * part_G + (g < part_G ? g : 0));
            }
            __builtin_amdgcn_sched_barrier(0);
            pw.load(w + ip);
            __builtin_amdgcn_sched_barrier(0);  // w is older than every column: the counts below say so
            // The image of one slot: lane t's row quad of the slot's column at
            // byte 16 t, which is what one LDS-DMA wave-instruction writes
            // (wave-uniform base + lane * 16 B) when the base is the slot's
            // address of the wave's first lane. A lane only ever reads the 16
            // bytes it requested itself, so no lane waits for another lane's
            // request: the lane's own counted vmcnt orders its read, and the
            // read's lgkmcnt(0) orders the slot's refill. No barrier.
            __shared__ float4 ring[R][BS];
            static_assert(sizeof(float4) == 16 && sizeof(ring[0]) == 16 * BS && BS % kWave == 0 &&
                              sizeof(ring) + sizeof(coef) + 64 <= 160 * 1024,
                          "lane-linear 16-B image, whole waves, inside the CU's LDS");
            const int wave0 = wave_id() * kWave;
            ring_lane = (unsigned)(size_t)(lds_ptr_t)&ring[0][threadIdx.x];
            const unsigned ring_wave0 = (unsigned)(size_t)(lds_ptr_t)&ring[0][wave0];
#pragma unroll
            for (int u = 0; u < R; ++u) cgs_stream_request(V + (int64_t)u * ld + ip, ring_wave0 + u * 16 * BS);
            __builtin_amdgcn_sched_barrier(0);
            // the partials are the oldest requests: w and R columns stay in flight
            cgs_stream_wait_partials<1 + R>(pd);
#pragma unroll
            for (int q = 0; q < Q; ++q) pp[q] = (A)pd[q];
        } else {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int g = sub + 32 * q;
                pp[q] = (A)sums[(size_t)jc * part_G + (g < part_G ? g : 0)];
            }
        }
        if constexpr (PF) {
            __builtin_amdgcn_sched_barrier(0);
            pw.load(w + ip);
#pragma unroll
            for (int u = 0; u < B0; ++u) pv[u].load(V + (int64_t)u * ld + ip);
            __builtin_amdgcn_sched_barrier(0);
        }
        A v = A(0);
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (sub + 32 * q < part_G) v += pp[q];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (j < NC && sub == 0) {
            const T c = (T)v;
            coef[j] = (A)c;
            if (blockIdx.x == 0) coef_out[j] = c;
        }
    } else if (threadIdx.x < NC) {
        const T c = (T)sums[threadIdx.x];
        coef[threadIdx.x] = (A)c;
        if (blockIdx.x == 0) coef_out[threadIdx.x] = c;
    }
    if constexpr (PF || STREAM) lds_barrier();  // (__syncthreads would drain the requests in flight)
    else __syncthreads();
    constexpr int NA = NEXT_DOTS ? Pow2Ceil<NC>::v : 1;
    A acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = A(0);
    // w' = w - T(t) for one row quad, and its share of ||w'||^2
    auto finish_rows = [&](int i, const A (&t)[4], const Raw4<T>& wr, A (&wd)[4]) {
        T wo[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wo[r] = T(-1) * (T)t[r] + T(1) * (T)wr[r];
            wd[r] = (A)wo[r];
            if (!NEXT_DOTS) acc[0] += wd[r] * wd[r];
        }
        Row4<T>::store(w + i, wo);
    };
    int i_loop = i_first;
    if constexpr (STREAM) {
        // every lane runs the ring to its end, so no request outlives the
        // workgroup's LDS; lanes past the last row quad store nothing
        A t[4] = {A(0), A(0), A(0), A(0)};
        const unsigned coef_lds = (unsigned)(size_t)(lds_ptr_t)&coef[0];
        const unsigned ring_wave = __builtin_amdgcn_readfirstlane(ring_lane);
        static_for<0, NC>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            constexpr unsigned slot = (unsigned)((c % R) * 16 * BS);
            // columns c + 1 .. c + R - 1 were requested after column c
            constexpr int behind = NC - 1 - c < R - 1 ? NC - 1 - c : R - 1;
            f32x4_t x;
            A cu;
            cgs_stream_take<behind>(ring_lane + slot, coef_lds + 4u * c, x, cu);
            if constexpr (c + R < NC) cgs_stream_request(V + (int64_t)(c + R) * ld + ip, ring_wave + slot);
            Raw4<T> v;
            v.v = make_float4(x.x, x.y, x.z, x.w);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] += v.template at<A>(r) * cu;
            // the products are formed here: left to the compiler they sink
            // into the row test below, and every column read stays live (spills)
            cgs_stream_pin(t);
        });
        if (i_first < n4) {
            A wd[4];
            finish_rows(i_first, t, pw, wd);
        }
        i_loop = i_first + 4 * gridDim.x * BS;
    }
    bool first = PF;
    for (int i = i_loop; i < n4; i += 4 * gridDim.x * BS) {
        Raw4<T> wr;
        if (first) wr = pw;
        else wr.load(w + i);
        A t[4] = {A(0), A(0), A(0), A(0)};
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += B) {
            typename Bs::Raw4 v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) {
                    if (c0 == 0 && first) v[u] = pv[u < B0 ? u : 0];
                    else v[u].load(V + (int64_t)(c0 + u) * ld + i);
                }
            __builtin_amdgcn_sched_barrier(0);  // keep the batch's loads issued back to back
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) {
                    const A cu = coef[c0 + u];
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] += v[u].template at<A>(r) * cu;
                }
        }
        A wd[4];
        finish_rows(i, t, wr, wd);
        first = false;
        if constexpr (NEXT_DOTS) {
#pragma unroll
            for (int c0 = 0; c0 < NC; c0 += B) {
                typename Bs::Raw4 v[B];
#pragma unroll
                for (int u = 0; u < B; ++u)
                    if (c0 + u < NC) v[u].load(V + (int64_t)(c0 + u) * ld + i);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < B; ++u)
                    if (c0 + u < NC)
                        acc[c0 + u] += v[u].template at<A>(0) * wd[0] + v[u].template at<A>(1) * wd[1] +
                                       v[u].template at<A>(2) * wd[2] + v[u].template at<A>(3) * wd[3];
            }
        }
    }
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        A t = A(0);
#pragma unroll
        for (int j = 0; j < NC; ++j) t += Bs::template get<A>(V + (int64_t)j * ld + i) * coef[j];
        const T wi = T(-1) * (T)t + T(1) * w[i];
        w[i] = wi;
        if constexpr (NEXT_DOTS) {
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += Bs::template get<A>(V + (int64_t)c * ld + i) * (A)wi;
        } else {
            acc[0] += (A)wi * (A)wi;
        }
    }
    store_partials<NA, BS>(acc, NEXT_DOTS ? NC : 1, partial);
    stamp_at<STAMP>(stamp, 1);
}

// The CGS update for kNC < nc <= kWideMax columns (GMRES(100)): the
// coefficients are summed here from k_dots_panels' part_G <= 128 partials per
// column (8 lanes per column, 16 branch-free loads each in g order, then an
// xor tree: the same fixed order in every workgroup; no reduce launch), then
// w = w - T(V coef) with 4 rows per lane, the columns in compile-time batches
// of B (the last batch clamped to column nc - 1 with coefficient 0: +0 terms,
// so t is the j-ordered sum of the real terms), and the ||w'||^2 partials.
template <class T, int BS, class A = double>
__global__ __launch_bounds__(BS) void k_cgs_update_wide(int n, const T* __restrict__ V, int64_t ld, int nc,
                                                        const double* __restrict__ parts, int part_G,
                                                        T* __restrict__ coef_out, T* __restrict__ w,
                                                        double* __restrict__ partial) {
    constexpr int LPC = BS / kWideMax, Q = 128 / LPC, B = kColBatch<T>;
    static_assert(LPC * kWideMax == BS && Q * LPC == 128, "8 lanes per column, <= 128 partials");
    __shared__ A coef[kWideMax];
    {
        const int j = threadIdx.x / LPC, sub = threadIdx.x % LPC;
        const int jc = j < nc ? j : nc - 1;
        A pp[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int g = sub + LPC * q;
            pp[q] = (A)parts[(size_t)jc * part_G + (g < part_G ? g : 0)];
        }
        A v = A(0);
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (sub + LPC * q < part_G) v += pp[q];
#pragma unroll
        for (int o = LPC / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (sub == 0) {
            const T c = (T)v;
            coef[j] = j < nc ? (A)c : A(0);
            if (blockIdx.x == 0 && j < nc) coef_out[j] = c;
        }
    }
    __syncthreads();
    A acc[1] = {A(0)};
    const int n4 = n & ~3;
    const int nb = (nc + B - 1) / B;
    for (int i = 4 * (blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * gridDim.x * BS) {
        Raw4<T> wr;
        wr.load(w + i);
        A t[4] = {A(0), A(0), A(0), A(0)};
        for (int bi = 0; bi < nb; ++bi) {
            const int c0 = bi * B;
            Raw4<T> v[B];
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const int c = c0 + u < nc ? c0 + u : nc - 1;
                v[u].load(V + (int64_t)c * ld + i);
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the batch's loads issued back to back
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const A cu = coef[c0 + u < kWideMax ? c0 + u : kWideMax - 1];
                if (c0 + u < nc)
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] += v[u].template at<A>(r) * cu;
            }
        }
        T wo[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wo[r] = T(-1) * (T)t[r] + T(1) * (T)wr[r];
            const A wd = (A)wo[r];
            acc[0] += wd * wd;
        }
        Row4<T>::store(w + i, wo);
    }
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        A t = A(0);
        for (int j = 0; j < nc; ++j) t += (A)V[(int64_t)j * ld + i] * coef[j];
        const T wi = T(-1) * (T)t + T(1) * w[i];
        w[i] = wi;
        acc[0] += (A)wi * (A)wi;
    }
    store_partials<1, BS>(acc, 1, partial);
}

// ---------------------------------------------------------------- step: CGS
// coef = T(sums[0..k]); w = w - T(V coef) (gemv(-1, V, h, 1, w));
// NEXT_DOTS: partials <v_j, w'> (j <= k) else partial ||w'||^2.
// Each lane owns 4 consecutive rows (16-B loads of every basis column), and
// issues the loads of 8 columns before their FMAs; the row sum t runs over
// j = 0..k in order in fp64, as the scalar form did.
// GIVENS (one GPU, last pass, m <= kFoldMaxM): the ||w'||^2 partials go
// write-through and the last-arriving workgroup sums them and runs the
// Givens step k (givens_block) — no separate Givens launch.
template <class T, bool NEXT_DOTS, bool GIVENS = false, int BS = kBlock, bool FROM_PARTS = false, class A = double>
__global__ __launch_bounds__(BS) void k_cgs_update(int n, const T* __restrict__ V, int64_t ld, int k,
                                                       const double* __restrict__ sums, T* __restrict__ coef_out,
                                                       T* __restrict__ w, double* __restrict__ partial,
                                                       unsigned* __restrict__ cnt, GivensArgs<T> g, int part_G) {
    static_assert(!(NEXT_DOTS && GIVENS), "the Givens step follows the last pass");
    // GIVENS: the last-arriving workgroup's givens_block reads the column workgroup 0 stores here, and the
    // XCDs' L2s are not coherent: a plain store may stay in workgroup 0's L2, where another XCD's acquire does
    // not reach it. Seen once (tests/test_arnoldi_phases_gpu.py::test_cgs_from_sums, cgs_givens at k + 1 = 9):
    // the step had rotated the column's old contents and stored that over the coefficients; the cause is read
    // from the code, not demonstrated. Write-through, as the partials (handoff.hpp; drained ahead of the
    // ticket by last_arriver's vmcnt(0))
    auto store_coef = [](T* p, T c) {
        if constexpr (GIVENS) store_wt(p, c);
        else *p = c;
    };
    __shared__ A coef[256];
    const int nc = k + 1;
    const int n4 = n & ~3;
    const int i_first = 4 * (blockIdx.x * BS + threadIdx.x);
    // part_G > 0: this lane's first row group (the first kPre columns and w)
    // is loaded BEFORE the coefficient sums, so the partial loads below
    // travel with it and their latency hides behind the basis stream
    constexpr int kPre = 8;
    const int npre = nc < kPre ? nc : kPre;
    const bool pre = FROM_PARTS && i_first < n4;
    A pv[kPre][4], pw[4];
    if (pre) {
#pragma unroll
        for (int u = 0; u < kPre; ++u)
            if (u < npre) Row4<T>::load(V + (int64_t)u * ld + i_first, pv[u]);
        Row4<T>::load(w + i_first, pw);
    }
    if (FROM_PARTS) {
        // sums straight from the panel-dots partials (nc <= kNC, part_G per
        // column): LPC lanes per column, each summing part_G / LPC partials
        // (all loads issued first) in g order, then an xor tree — the same
        // fixed order in every workgroup
        constexpr int LPC = BS / kNC;
        const int j = threadIdx.x / LPC, sub = threadIdx.x % LPC;
        const int per = (part_G + LPC - 1) / LPC;
        A v = A(0);
        if (j < nc) {
            const double* src = sums + (size_t)j * part_G + sub;
#pragma unroll 8
            for (int q = 0; q < per; ++q)
                if (q * LPC + sub < part_G) v += (A)src[q * LPC];
        }
#pragma unroll
        for (int o = LPC / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
        if (j < nc && sub == 0) {
            const T c = (T)v;
            coef[j] = (A)c;
            if (blockIdx.x == 0) store_coef(coef_out + j, c);
        }
    } else {
        for (int j = threadIdx.x; j < nc; j += BS) {
            const T c = (T)sums[j];
            coef[j] = (A)c;
            if (blockIdx.x == 0) store_coef(coef_out + j, c);
        }
    }
    __syncthreads();
    constexpr int NA = NEXT_DOTS ? kNC : 1;
    A acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = A(0);
    for (int i = i_first; i < n4; i += 4 * gridDim.x * BS) {
        A t[4] = {A(0), A(0), A(0), A(0)};
        int j = 0;
        const bool use_pre = pre && i == i_first;
        if (use_pre) {
#pragma unroll
            for (int u = 0; u < kPre; ++u)
                if (u < npre)
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] += pv[u][r] * coef[u];
            j = npre;
        }
        for (; j + 8 <= nc; j += 8) {
            A v[8][4];
#pragma unroll
            for (int u = 0; u < 8; ++u) Row4<T>::load(V + (int64_t)(j + u) * ld + i, v[u]);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] += v[u][r] * coef[j + u];
        }
        for (; j < nc; ++j) {
            A v[4];
            Row4<T>::load(V + (int64_t)j * ld + i, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] += v[r] * coef[j];
        }
        A wv[4];
        if (use_pre) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wv[r] = pw[r];
        } else {
            Row4<T>::load(w + i, wv);
        }
        T wo[4];
        A wd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wo[r] = T(-1) * (T)t[r] + T(1) * (T)wv[r];
            wd[r] = (A)wo[r];
        }
        Row4<T>::store(w + i, wo);
        if (NEXT_DOTS) {
#pragma unroll
            for (int c = 0; c < NA; ++c) {
                if (c < nc) {
                    A v[4];
                    Row4<T>::load(V + (int64_t)c * ld + i, v);
                    acc[c] += v[0] * wd[0] + v[1] * wd[1] + v[2] * wd[2] + v[3] * wd[3];
                }
            }
        } else {
            acc[0] += wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2] + wd[3] * wd[3];
        }
    }
    // tail rows (n not a multiple of 4)
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        A t = A(0);
        for (int j = 0; j < nc; ++j) t += (A)V[(int64_t)j * ld + i] * coef[j];
        const T wi = T(-1) * (T)t + T(1) * w[i];
        w[i] = wi;
        if (NEXT_DOTS) {
#pragma unroll
            for (int c = 0; c < NA; ++c)
                if (c < nc) acc[c] += (A)V[(int64_t)c * ld + i] * (A)wi;
        } else {
            acc[0] += (A)wi * (A)wi;
        }
    }
    store_partials<NA, BS, GIVENS>(acc, NEXT_DOTS ? (nc < kNC ? nc : kNC) : 1, partial);
    if constexpr (GIVENS) {
        if (last_arriver(cnt)) {
            __shared__ T col[kFoldMaxM + 2], c_s[kFoldMaxM + 2], s_s[kFoldMaxM + 2];
            __shared__ A scratch[BS / kWave];
            const double nrm2sq = (double)sum_partials<BS, A>(partial, gridDim.x, scratch);
            givens_block(g, nrm2sq, col, c_s, s_s);
        }
    }
}

// ---------------------------------------------------------------- step: MGS
// h_jk = T(sums[0]); w -= h_jk v_j (naxpy); partial <v_{j+1}, w> or ||w||^2.
// src_G > 0: h_jk is summed here from the src_G partials of the previous
// launch (the dots or the previous MGS update, one GPU), in the same fixed
// order in every workgroup — one launch per j instead of reduce + update.
// Each lane owns 4 consecutive rows (16-B loads).
template <class T, int BS, class A = double>
__global__ __launch_bounds__(BS) void k_mgs_update(int n, const T* __restrict__ V, int64_t ld, int j, int k,
                                                   const double* __restrict__ src, int src_G, T* __restrict__ hjk,
                                                   T* __restrict__ w, double* __restrict__ partial) {
    __shared__ A scratch[BS / kWave];
    __shared__ T h_s;
    const T* __restrict__ vj = V + (int64_t)j * ld;
    const T* __restrict__ vn = V + (int64_t)(j + 1) * ld;
    const bool last = j == k;
    const int n4 = n & ~3;
    // this lane's first row group is loaded before h_jk is known, so its
    // latency overlaps the partial sum's instead of following it
    const int i_first = 4 * (blockIdx.x * BS + threadIdx.x);
    const bool pre = i_first < n4;
    // raw and unconditional (a clamped address when this lane has no row
    // group): a guarded load would be widened to fp64 inside its branch,
    // i.e. waited for right here. Column j + 1 <= m exists; unused when last.
    // The partial (src_G <= BS: one per lane) is loaded FIRST: vmcnt retires
    // in order, so waiting for it must not wait for the row group behind it.
    static_assert(BS >= kCombineGroups * 4, "one partial per lane");
    A part = (A)src[threadIdx.x < src_G ? threadIdx.x : 0];
    if (threadIdx.x >= src_G) part = A(0);
    __builtin_amdgcn_sched_barrier(0);
    const int ip = pre ? i_first : 0;
    Raw4<T> pw, pv, pn;
    pw.load(w + ip);
    pv.load(vj + ip);
    pn.load(vn + ip);
    __builtin_amdgcn_sched_barrier(0);
    // LDS-only barriers: the first row group's loads stay in flight. The
    // block sum runs unconditionally so the partial load is not sunk below
    // the row group's loads.
    {
        const A v = wave_sum(part + A(0));  // = sum_partials' order for src_G <= BS
        if ((threadIdx.x & (kWave - 1)) == 0) scratch[threadIdx.x / kWave] = v;
        lds_barrier();
        if (threadIdx.x == 0) {
            A r = A(0);
#pragma unroll
            for (int q = 0; q < BS / kWave; ++q) r += scratch[q];
            h_s = src_G > 0 ? (T)r : (T)src[0];
        }
    }
    lds_barrier();
    const T h = h_s;
    if (blockIdx.x == 0 && threadIdx.x == 0) *hjk = h;
    A acc[1] = {A(0)};
    for (int i = i_first; i < n4; i += 4 * gridDim.x * BS) {
        A wv[4], vv[4], nv[4] = {A(0), A(0), A(0), A(0)};
        if (i == i_first) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                wv[r] = pw.template at<A>(r);
                vv[r] = pv.template at<A>(r);
                nv[r] = last ? A(0) : pn.template at<A>(r);
            }
        } else {
            Row4<T>::load(w + i, wv);
            Row4<T>::load(vj + i, vv);
            if (!last) Row4<T>::load(vn + i, nv);
        }
        T wo[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            T wi = (T)wv[r];
            wi -= h * (T)vv[r];
            wo[r] = wi;
            acc[0] += last ? (A)wi * (A)wi : nv[r] * (A)wi;
        }
        Row4<T>::store(w + i, wo);
    }
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        T wi = w[i];
        wi -= h * vj[i];
        w[i] = wi;
        acc[0] += last ? (A)wi * (A)wi : (A)vn[i] * (A)wi;
    }
    store_partials<1, BS>(acc, 1, partial);
}

}  // namespace
