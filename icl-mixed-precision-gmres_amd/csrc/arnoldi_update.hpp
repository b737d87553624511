// The end of a restart cycle: the upper-triangular solve, the solution update
// x += X(T(V y)), and the cycle's tail in one launch (the last Givens step,
// the solve, the update and the x snapshot: k_update_tail_nc).
#pragma once

#include "arnoldi_givens.hpp"
#include "basis.hpp"
#include "lds_ring.hpp"
#include "panel.hpp"

namespace {

#pragma clang fp contract(off)
// upper-triangular solve y = H(0:k,0:k)^-1 s(0:k), in place on s (one lane per
// row of the axpy sweep; k <= m is small)
template <class T>
__global__ __launch_bounds__(kBlock) void k_trsv_upper(int k, int ldh, const T* __restrict__ H, T* __restrict__ y) {
    __shared__ T ys[1024];
    __shared__ T temp_s;
    for (int i = threadIdx.x; i < k; i += kBlock) ys[i] = y[i];
    __syncthreads();
    for (int j = k - 1; j >= 0; --j) {
        if (threadIdx.x == 0) {
            T yj = ys[j];
            if (yj != T(0)) yj = yj / H[(int64_t)j * ldh + j];
            ys[j] = yj;
            temp_s = yj;
        }
        __syncthreads();
        const T t = temp_s;
        if (t != T(0))
            for (int i = threadIdx.x; i < j; i += kBlock) ys[i] = ys[i] - t * H[(int64_t)j * ldh + i];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < k; i += kBlock) y[i] = ys[i];
}
// The same solve for 64 < k <= 64 * KW by one wave64 (GMRES(100): the
// one-lane-per-step form above took 92.6 us at k = 100, one workgroup barrier
// pair per column). The upper triangle of H(0:k,0:k) is staged in LDS packed
// by columns (column j at j(j+1)/2, dynamic shared memory) with one load
// round; lane l holds y_{l + 64q} in register slot q. The column sweep is
// the netlib order of k_trsv_upper (no contraction): y_j /= H(j,j) (when
// y_j != 0), broadcast by a shuffle, then y_i -= y_j H(i,j) for i < j.
// (kBlock threads stage H, 8 independent loads per lane per round; wave 0 solves)
template <class T, int KW>
__global__ __launch_bounds__(kBlock) void k_trsv_upper_lds(int k, int ldh, const T* __restrict__ H,
                                                           T* __restrict__ y) {
    extern __shared__ char trsv_smem[];
    T* Hp = reinterpret_cast<T*>(trsv_smem);
    const int lane = threadIdx.x;
    const int P = k * (k + 1) / 2;
    constexpr int U = 8;
    for (int base = 0; base < P; base += kBlock * U) {
        T v[U];
        int e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            e[u] = base + kBlock * u + (int)threadIdx.x;
            const int ec = e[u] < P ? e[u] : P - 1;
            // column j of packed entry ec: j(j+1)/2 <= ec < (j+1)(j+2)/2
            int j = (int)((sqrtf(8.0f * (float)ec + 1.0f) - 1.0f) * 0.5f);
            while (j * (j + 1) / 2 > ec) --j;
            while ((j + 1) * (j + 2) / 2 <= ec) ++j;
            v[u] = H[(int64_t)j * ldh + (ec - j * (j + 1) / 2)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e[u] < P) Hp[e[u]] = v[u];
    }
    __syncthreads();
    if (threadIdx.x >= kWave) return;
    T yr[KW];
#pragma unroll
    for (int q = 0; q < KW; ++q) yr[q] = lane + kWave * q < k ? y[lane + kWave * q] : T(0);
    for (int j = k - 1; j >= 0; --j) {
        const int jq = j / kWave, jl = j % kWave;
        T mine = yr[0];
#pragma unroll
        for (int q = 1; q < KW; ++q)
            if (q == jq) mine = yr[q];
        T yj = __shfl(mine, jl, kWave);
        if (yj != T(0)) yj = yj / Hp[j * (j + 1) / 2 + j];
#pragma unroll
        for (int q = 0; q < KW; ++q) {
            const int i = lane + kWave * q;
            if (q == jq && lane == jl) yr[q] = yj;
            if (yj != T(0) && i < j) yr[q] = yr[q] - yj * Hp[j * (j + 1) / 2 + i];
        }
    }
#pragma unroll
    for (int q = 0; q < KW; ++q)
        if (lane + kWave * q < k) y[lane + kWave * q] = yr[q];
}

// The same upper solve by one wave64 (k <= 64): lane i holds y_i, the
// column sweep's scalar is broadcast with a shuffle, H(0:k,0:k) is in LDS
// (column j at Hs[j * 64]). No barrier inside the sweep.
template <class T>
__device__ __forceinline__ T trsv_upper_wave(int k, const T* Hs, T y, int lane) {
    for (int j = k - 1; j >= 0; --j) {
        T yj = __shfl(y, j, kWave);
        if (yj != T(0)) yj = yj / Hs[j * kWave + j];
        if (lane == j) y = yj;
        if (yj != T(0) && lane < j) y = y - yj * Hs[j * kWave + lane];
    }
    return y;
}
#pragma clang fp contract(on)

// x += X(T(V y)): mixed form gemv(1, V, y, 0, tmp); copy; axpy(1, tmp, x)
// (same-precision form gemv(1, V, y, 1, x) gives the same fl(t + x))
// SOLVE (k <= 64): y = H(0:k,0:k)^-1 s(0:k) is formed first by every
// workgroup (trsv_upper_wave) — one launch per restart instead of two. s is
// not overwritten (the next prologue resets it).
template <class T, class X, bool SOLVE, class A = double>
__global__ __launch_bounds__(kBlock) void k_update_x(int n, const T* __restrict__ V, int64_t ld, int k,
                                                     const T* __restrict__ y, const T* __restrict__ H, int ldh,
                                                     X* __restrict__ x) {
    __shared__ T ys[SOLVE ? kWave : 1024];
    if constexpr (SOLVE) {
        __shared__ T Hs[kWave * kWave];
        for (int e = threadIdx.x; e < k * kWave; e += kBlock) {
            const int j = e / kWave, i = e % kWave;
            Hs[e] = i <= j ? H[(int64_t)j * ldh + i] : T(0);
        }
        __syncthreads();
        if (threadIdx.x < kWave) {
            const int lane = threadIdx.x;
            T yv = lane < k ? y[lane] : T(0);
            yv = trsv_upper_wave(k, Hs, yv, lane);
            ys[lane] = yv;  // (s itself is left as is: every workgroup reads it)
        }
    } else {
        for (int j = threadIdx.x; j < k; j += kBlock) ys[j] = y[j];
    }
    __syncthreads();
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        A t = A(0);
        for (int j = 0; j < k; ++j) t += (A)V[(int64_t)j * ld + i] * (A)ys[j];
        x[i] = x[i] + (X)(T)t;
    }
}

// k_update_x<T, X, true> with the column count NC = k <= kNC a compile-time
// constant: each lane owns 4 rows and loads the basis in batches (the
// runtime-k form waited for every few columns in turn). Same arithmetic:
// t = sum_j V_ij y_j in fp64 in j order, x_i = x_i + X(T(t)).
// AT: the accumulation class, or WithBasis<A, B> for a compressed basis
// (basis.hpp), read as stored.
template <class T, class X, int NC, class AT = double>
__global__ __launch_bounds__(kCombineBlock) void k_update_x_nc(int n, const T* __restrict__ V_, int64_t ld,
                                                                const T* __restrict__ y, const T* __restrict__ H,
                                                                int ldh, X* __restrict__ x) {
    static_assert(NC >= 1 && NC <= kNC, "one panel");
    using A = typename AccOf<AT>::type;
    using Bs = BasisOf<T, AT>;
    const typename Bs::elem* __restrict__ V = basis_ptr<Bs>(V_);
    constexpr int BS = kCombineBlock, B = Bs::kBatch;
    __shared__ T Hs[NC * kWave];
    __shared__ A ys[NC];
    for (int e = threadIdx.x; e < NC * kWave; e += BS) {
        const int j = e / kWave, i = e % kWave;
        Hs[e] = i <= j && i < NC ? H[(int64_t)j * ldh + i] : T(0);
    }
    __syncthreads();
    if (threadIdx.x < kWave) {
        const int lane = threadIdx.x;
        T yv = lane < NC ? y[lane] : T(0);
        yv = trsv_upper_wave(NC, Hs, yv, lane);
        if (lane < NC) ys[lane] = (A)yv;
    }
    __syncthreads();
    const int n4 = n & ~3;
    for (int i = 4 * (blockIdx.x * BS + threadIdx.x); i < n4; i += 4 * gridDim.x * BS) {
        Raw4<X> xr;
        xr.load(x + i);
        A t[4] = {A(0), A(0), A(0), A(0)};
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += B) {
            typename Bs::Raw4 v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) v[u].load(V + (int64_t)(c0 + u) * ld + i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) {
                    const A yu = ys[c0 + u];
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] += v[u].template at<A>(r) * yu;
                }
        }
        X xo[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) xo[r] = (X)xr[r] + (X)(T)t[r];
        Row4<X>::store(x + i, xo);
    }
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        A t = A(0);
#pragma unroll
        for (int j = 0; j < NC; ++j) t += Bs::template get<A>(V + (int64_t)j * ld + i) * ys[j];
        x[i] = x[i] + (X)(T)t;
    }
}

// ---- the cycle's tail in one launch (k_update_tail_nc) ----
// Givens step m - 1 of a cycle whose update follows at once: the step's
// arguments, the ||w||^2 partials it sums (fold.nparts of them, at most
// kBlock: fold_parts_sum then has sum_partials<kBlock>'s order and bits), and
// where workgroup 0 leaves the rotated column H(0..m, m-1) -- m + 1 values of
// the workspace that no workgroup of the launch reads, copied into H by the
// residual prologue's finish launch.
template <class T>
struct UpdateTail {
    GivensFold<T> fold;
    T* stage;
};

// Givens step k = NC - 1 (givens_block's arithmetic) and y = H(0:NC,0:NC)^-1
// s(0:NC) (trsv_upper_wave's) by one wave with no LDS and no barrier: lane j
// holds entry j of the column, of cs / sn and of s, and row j of H; the
// chain's scalars go from lane to lane through readlane at compile-time
// indices. Every wave of the launch runs it on the same inputs, so every
// wave holds the same y. In three parts: the loads (branch-free, at clamped
// indices: they issue together, one latency) and their first use sit ahead
// of the launch's big requests, the serial chain behind them. Reads nothing the storing wave writes:
// cs / sn below k, s(0..k+1), H's columns, the correction and the partials.
template <class T, int NC, class A>
struct TailRegs {
    static constexpr int k = NC - 1, NG = kBlock / kWave;
    A part[NG];
    double nrm2sq;  // (tail_prepare)
    T col, corr, c, s, y, s_next;
    T h[NC];  // h[j]: H(lane, j), zero below the diagonal (h[k]: set by the Givens step)

    __device__ __forceinline__ void load(const UpdateTail<T>& tl, int lane) {
        const GivensArgs<T>& g = tl.fold.g;
        const int ldh = g.m + 1;
        fold_parts_load(tl.fold, lane, part);
        const int lk = lane <= k ? lane : k, lc = lane < k ? lane : 0;
        col = g.H[(int64_t)k * ldh + lk];
        corr = g.corr ? g.corr[lk] : T(0);
        y = g.s[lk];
        c = g.cs[lc];
        s = g.sn[lc];
        s_next = g.s[k + 1];
#pragma unroll
        for (int j = 0; j < k; ++j) h[j] = g.H[(int64_t)j * ldh + (lane <= j ? lane : 0)];
    }
};

#pragma clang fp contract(off)
// the loads' first use, ahead of the launch's big requests (the compiler
// waits for every request in flight at the first use of a load): entries
// outside the column / the triangle zeroed, the correction added, ||w||^2
template <class T, int NC, class A>
__device__ __forceinline__ void tail_prepare(const UpdateTail<T>& tl, TailRegs<T, NC, A>& q, int lane) {
    constexpr int k = NC - 1;
    q.col = lane <= k ? (tl.fold.g.corr ? q.col + T(1) * q.corr : q.col) : T(0);  // axpy(1.0, weights, h_col)
    q.y = lane <= k ? q.y : T(0);
#pragma unroll
    for (int j = 0; j < k; ++j)
        if (lane > j) q.h[j] = T(0);
    q.nrm2sq = fold_parts_sum(tl.fold, q.part);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): cs, sn and s(k+1) too, whose first use is in the chain
}
// returns y_j in lane j; `store`: this wave writes the step's results
template <class T, int NC, class A>
__device__ __forceinline__ T tail_givens_solve(const UpdateTail<T>& tl, TailRegs<T, NC, A>& q, int lane, bool store) {
    constexpr int k = NC - 1;
    const GivensArgs<T>& g = tl.fold.g;
    T colv = q.col, yv = q.y;
    const T hn = (T)sqrt(q.nrm2sq);
    const T iv = T(1) / hn;
    T a = wave_lane(colv, 0);
    static_for<0, k>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        T b = wave_lane(colv, j + 1);
        rot_pair(a, b, wave_lane(q.c, j), wave_lane(q.s, j));
        if (lane == j) colv = a;
        a = b;
    });
    T b = hn, ck, snk;
    rotg_ref(a, b, ck, snk);
    if (lane == k) colv = a;
    if (lane == k + 1) colv = b;
    T sk = wave_lane(yv, k), sk1 = q.s_next;
    rot_pair(sk, sk1, ck, snk);
    if (lane == k) yv = sk;
    q.h[k] = lane <= k ? colv : T(0);
    if (store) {
        if (lane <= k + 1) tl.stage[lane] = colv;
        if (lane == 0) {
            g.cs[k] = ck;
            g.sn[k] = snk;
            *g.inv = iv;
            g.report[4 + k] = (double)fabs(sk1);
        }
    }
    static_for<0, NC>([&](auto jj) {
        constexpr int j = NC - 1 - decltype(jj)::value;
        T yj = wave_lane(yv, j);
        if (yj != T(0)) yj = yj / wave_lane(q.h[j], j);
        if (lane == j) yv = yj;
        if (yj != T(0) && lane < j) yv = yv - yj * q.h[j];
    });
    return yv;
}
#pragma clang fp contract(on)

// givens_partials(NC - 1), update(NC) and the x snapshot in one launch, for a
// cycle of NC = m <= kNC steps on one GPU. Every lane first requests its row
// quad of x and of the first basis columns, right behind the Givens step's
// few inputs; the step and the upper solve then run in every wave
// (tail_givens_solve) while those are in flight, and the columns are added
// in ascending order, t = sum_j V_ij y_j in the class A, x_i = x_i + X(T(t)):
// k_update_x_nc's operands and order.
// STREAM (fp32 basis, fp32 class): the lane's first row quad takes its
// columns through the CGS update's ring of LDS slots (cgs_stream_*); further
// grid-stride passes and the n mod 4 rows take the batched loop. Otherwise
// nothing is requested early: k_update_x_nc's loop behind the chain.
// SNAP: the x read is also stored to x_snap (rows of [0, n): the cycle's
// undo; a template flag: as a branch in the loop it cost the batches their
// registers, 168 B of scratch per lane). Workgroup 0's first wave stores
// the step's results: cs, sn, 1/h, the report entry in place, the rotated
// column to tl.stage (the finish launch puts it into H; s is not updated:
// nothing reads it before the finish launch resets it).
template <class T, class X, int NC, class A, bool STREAM, bool SNAP>
__global__ __launch_bounds__(kCombineBlock) void k_update_tail_nc(int n, const T* __restrict__ V, int64_t ld,
                                                                   X* __restrict__ x, X* __restrict__ x_snap,
                                                                   UpdateTail<T> tl) {
    static_assert(NC >= 1 && NC <= kNC, "one panel");
    static_assert(!STREAM || (sizeof(T) == 4 && sizeof(A) == 4), "the ring holds an fp32 basis for fp32 sums");
    constexpr int BS = kCombineBlock, B = kColBatch<T>;
    constexpr int R = NC < kStreamSlots ? NC : kStreamSlots;  // the ring's depth
    __shared__ A ys[NC];
    const int lane = threadIdx.x & (kWave - 1);
    const int n4 = n & ~3;
    const int i_first = 4 * (blockIdx.x * BS + threadIdx.x);
    const int ip = i_first < n4 ? i_first : 0;  // clamped row of the early requests: every lane reads valid memory
    TailRegs<T, NC, A> q;
    q.load(tl, lane);
    tail_prepare(tl, q, lane);
    __builtin_amdgcn_sched_barrier(0);  // the step's few values have landed: nothing below waits for them
    Raw4<X> xr;
    if constexpr (STREAM) xr.load(x + ip);
    unsigned ring_lane = 0;  // LDS byte address of this lane's 16 bytes of slot 0
    if constexpr (STREAM) {
        // (the slot image and its ordering: k_cgs_update_nc's STREAM form)
        __shared__ float4 ring[R][BS];
        static_assert(sizeof(float4) == 16 && sizeof(ring[0]) == 16 * BS && BS % kWave == 0 &&
                          sizeof(ring) + sizeof(ys) + 64 <= 160 * 1024,
                      "lane-linear 16-B image, whole waves, inside the CU's LDS");
        const int wave0 = wave_id() * kWave;
        ring_lane = (unsigned)(size_t)(lds_ptr_t)&ring[0][threadIdx.x];
        const unsigned ring_wave0 = (unsigned)(size_t)(lds_ptr_t)&ring[0][wave0];
        __builtin_amdgcn_sched_barrier(0);  // x is older than every column
#pragma unroll
        for (int u = 0; u < R; ++u) cgs_stream_request(V + (int64_t)u * ld + ip, ring_wave0 + u * 16 * BS);
    }
    __builtin_amdgcn_sched_barrier(0);
    const T yv = tail_givens_solve<T, NC, A>(tl, q, lane, blockIdx.x == 0 && threadIdx.x < kWave);
    // every wave writes the same values and reads them back behind its own writes: no barrier
    if (lane < NC) ys[lane] = (A)yv;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_sched_barrier(0);  // no column load of the loops below moves up into the chain
    auto finish_rows = [&](int i, const A (&t)[4], const Raw4<X>& xq) {
        X xo[4], xk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xk[r] = (X)xq[r];
            xo[r] = (X)xq[r] + (X)(T)t[r];
        }
        if constexpr (SNAP) Row4<X>::store(x_snap + i, xk);
        Row4<X>::store(x + i, xo);
    };
    int i_loop = i_first;
    if constexpr (STREAM) {
        // every lane runs the ring to its end, so no request outlives the
        // workgroup's LDS; lanes past the last row quad store nothing
        A t[4] = {A(0), A(0), A(0), A(0)};
        const unsigned ys_lds = (unsigned)(size_t)(lds_ptr_t)&ys[0];
        const unsigned ring_wave = __builtin_amdgcn_readfirstlane(ring_lane);
        static_for<0, NC>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            constexpr unsigned slot = (unsigned)((c % R) * 16 * BS);
            // columns c + 1 .. c + R - 1 were requested after column c
            constexpr int behind = NC - 1 - c < R - 1 ? NC - 1 - c : R - 1;
            f32x4_t q;
            A yu;
            cgs_stream_take<behind>(ring_lane + slot, ys_lds + 4u * c, q, yu);
            if constexpr (c + R < NC) cgs_stream_request(V + (int64_t)(c + R) * ld + ip, ring_wave + slot);
            Raw4<T> v;
            v.v = make_float4(q.x, q.y, q.z, q.w);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] += v.template at<A>(r) * yu;
            cgs_stream_pin(t);
        });
        if (i_first < n4) finish_rows(i_first, t, xr);
        i_loop = i_first + 4 * gridDim.x * BS;
    }
    for (int i = i_loop; i < n4; i += 4 * gridDim.x * BS) {
        Raw4<X> xq;
        xq.load(x + i);
        A t[4] = {A(0), A(0), A(0), A(0)};
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += B) {
            Raw4<T> v[B];
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) v[u].load(V + (int64_t)(c0 + u) * ld + i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < B; ++u)
                if (c0 + u < NC) {
                    const A yu = ys[c0 + u];
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] += v[u].template at<A>(r) * yu;
                }
        }
        finish_rows(i, t, xq);
    }
    for (int i = n4 + blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS) {
        A t = A(0);
#pragma unroll
        for (int j = 0; j < NC; ++j) t += (A)V[(int64_t)j * ld + i] * ys[j];
        const X xi = x[i];
        if constexpr (SNAP) x_snap[i] = xi;
        x[i] = xi + (X)(T)t;
    }
}

}  // namespace
