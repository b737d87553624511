// The Givens step of the fused Arnoldi cycle (Givens on rounded products, as
// the reference orders them): the one-lane kernel, its folded forms inside
// the SpMV launches (GivensFold, fold_givens, fold_parts_*), and the wave
// broadcasts and wave stamps those forms use.
#pragma once

#include "arnoldi_reduce.hpp"

namespace {

// ---------------------------------------------------------------- step: Givens
#pragma clang fp contract(off)
template <class T>
__device__ void rot_pair(T& a, T& b, T c, T s) {
    const T a1 = a, a2 = b;
    a = c * a1 + s * a2;
    b = c * a2 - s * a1;
}
template <class T>
__device__ void rotg_ref(T& a, T& b, T& c, T& s) {
    const T av = a, bv = b;
    const T roe = fabs(av) > fabs(bv) ? av : bv;
    const T scale = fabs(av) + fabs(bv);
    T r;
    if (scale == T(0)) {
        c = T(1); s = T(0); r = T(0);
    } else {
        const T as = av / scale, bs = bv / scale;
        r = scale * sqrt(as * as + bs * bs);
        r = roe >= T(0) ? r : -r;
        c = av / r;
        s = bv / r;
    }
    a = r;
    b = T(0);
}

// h_{k+1,k} = ||w||; (CGSR: h(0:k,k) += correction); rotations; |s(k+1)|.
// norm2 = the squared norm: sums[0] (nparts == 0) or, on one GPU, the sum
// of `nparts` workgroup partials reduced here (saves a launch per step).
// Givens step k on one workgroup (gmres.cpp:217-226): col/c_s/s_s are LDS
// arrays of at least k + 2 entries; nrm2sq (= ||w||^2) is read in thread 0.
template <class T>
struct GivensArgs {
    int k, m;
    const T* corr;  // CGSR correction (h += corr) or nullptr
    T *H, *cs, *sn, *s, *inv;
    double* report;
};

template <class T>
__device__ void givens_block(const GivensArgs<T>& g, double nrm2sq, T* col, T* c_s, T* s_s) {
    // stage the column and the previous rotations in LDS with all lanes, so
    // the serial rotation chain runs on LDS instead of global latency
    const int k = g.k;
    T* gcol = g.H + (int64_t)k * (g.m + 1);
    for (int j = threadIdx.x; j <= k; j += blockDim.x) {
        col[j] = g.corr ? gcol[j] + T(1) * g.corr[j] : gcol[j];  // axpy(1.0, weights, h_col)
        c_s[j] = g.cs[j];
        s_s[j] = g.sn[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const T hn = (T)sqrt(nrm2sq);
        col[k + 1] = hn;
        *g.inv = T(1) / hn;  // scal(1/h_final, w, v_{k+1}) — no breakdown guard, as in the reference
        for (int j = 0; j < k; ++j) rot_pair(col[j], col[j + 1], c_s[j], s_s[j]);
        rotg_ref(col[k], col[k + 1], c_s[k], s_s[k]);
        T sk = g.s[k], sk1 = g.s[k + 1];
        rot_pair(sk, sk1, c_s[k], s_s[k]);
        g.s[k] = sk;
        g.s[k + 1] = sk1;
        g.cs[k] = c_s[k];
        g.sn[k] = s_s[k];
        g.report[4 + k] = (double)fabs(sk1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j <= k + 1; j += blockDim.x) gcol[j] = col[j];
}

// the scale 1/h_{k+1,k} exactly as givens_block forms it
template <class T>
__device__ __forceinline__ T inv_of_norm2(double nrm2sq) {
    return T(1) / (T)sqrt(nrm2sq);
}

// norm2 = the squared norm: sums[0] (nparts == 0) or, on one GPU, the sum
// of `nparts` workgroup partials reduced here (saves a launch per step).
template <class T, class A = double>
__global__ __launch_bounds__(kBlock) void k_givens(GivensArgs<T> g, const double* __restrict__ norm2, int nparts) {
    __shared__ T col[1026], c_s[1026], s_s[1026];
    __shared__ A scratch[kBlock / kWave];
    const double nrm2sq = nparts > 0 ? (double)sum_partials<kBlock, A>(norm2, nparts, scratch) : norm2[0];
    givens_block(g, nrm2sq, col, c_s, s_s);
}

// Givens step k-1 folded into the SpMV launch of step k (restart length
// <= kFoldMaxM): every workgroup sums the ||w||^2 partials in the same
// fixed order and forms 1/h_{k,k-1} itself; workgroup 0 also runs the
// rotation step. Returns the scale for v_k in every thread.
template <class T>
struct GivensFold {
    const double* norm2;  // nullptr: not folded (use *inv_p)
    int nparts;
    GivensArgs<T> g;
};

// measurement only (mpg_arnoldi_stamp_next): wave q's lane 0 stores the
// wall clock to stamp[2q + end] (end 0 at the wave's start, 1 at its end); a
// one-dimensional grid. Used by the one-panel dots and CGS update only: in
// the SpMVs, whose occupancy sits on VGPR thresholds, even this uniform
// branch cost up to 20 VGPRs (C4's stepped kernel 71 -> 91, -11 % in time),
// and a branch-free form with a sink word slowed the BAND SpMV; the SpMV is
// timed by duplicate launches instead (time_phase_dup, host/fused_timing.cpp).
// Round 5: a compile-time choice. The product instantiations
// (STAMP = false) hold no stamp code at all; the launch sites pick the STAMP
// = true instantiation only for a launch that mpg_arnoldi_stamp_next armed.
template <bool STAMP>
__device__ __forceinline__ void stamp_at(unsigned long long* stamp, int end) {
    if constexpr (STAMP) {
        if ((threadIdx.x & (kWave - 1)) == 0)
            stamp[2 * (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave) + end] = wall_clock64();
    }
}

template <bool FOLD, class T, class A = double>
__device__ __forceinline__ T fold_givens(const GivensFold<T>& f, const T* __restrict__ inv_p) {
    if constexpr (!FOLD) {
        return *inv_p;
    } else {
        __shared__ T col[kFoldMaxM + 2], c_s[kFoldMaxM + 2], s_s[kFoldMaxM + 2];
        __shared__ A scratch[kBlock / kWave];
        __shared__ T inv_s;
        const double nrm2sq = f.nparts > 0 ? (double)sum_partials<kBlock, A>(f.norm2, f.nparts, scratch) : f.norm2[0];
        if (threadIdx.x == 0) inv_s = inv_of_norm2<T>(nrm2sq);
        if (blockIdx.x == 0) givens_block(f.g, nrm2sq, col, c_s, s_s);
        __syncthreads();
        return inv_s;
    }
}
#pragma clang fp contract(on)

// lane 0's value in every lane (wave_sum's result), as a wave-uniform value
__device__ __forceinline__ float wave_first(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ double wave_first(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// The fold's ||w||^2 in every lane of a wave, in two parts so that the loads
// of the first can sit ahead of other work: lane l holds the partials of lane
// l of the waves 0..NG-1 of a kBlock workgroup (fold_parts_load), and the sum
// runs with the butterflies and in the order of k_step_sell2's waves 0..3
// (fold_parts_sum: the same value in every wave and lane).
template <class T, class A, int NG>
__device__ __forceinline__ void fold_parts_load(const GivensFold<T>& fold, int lane, A (&part)[NG]) {
#pragma unroll
    for (int q = 0; q < NG; ++q) {
        const int t = q * kWave + lane;
        part[q] = (A)fold.norm2[t < fold.nparts ? t : 0];
        if (t >= fold.nparts) part[q] = A(0);
    }
}
template <class T, class A, int NG>
__device__ __forceinline__ double fold_parts_sum(const GivensFold<T>& fold, const A (&part)[NG]) {
    if (fold.nparts > 0) {
        A r = A(0);
#pragma unroll
        for (int q = 0; q < NG; ++q) r += wave_first(wave_sum(part[q] + A(0)));
        return (double)r;
    }
    return fold.norm2[0];
}

// lane j's value in every lane, j a compile-time constant
__device__ __forceinline__ float wave_lane(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ double wave_lane(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j),
                            __builtin_amdgcn_readlane(__double2loint(v), j));
}

template <class T>
GivensArgs<T> givens_args(const mpg_arnoldi* a, int k) {
    return GivensArgs<T>{k,
                         a->d.m,
                         a->d.orth == kOrthCGSR ? static_cast<const T*>(a->corr()) : nullptr,
                         static_cast<T*>(a->H),
                         static_cast<T*>(a->cs()),
                         static_cast<T*>(a->sn()),
                         static_cast<T*>(a->s()),
                         static_cast<T*>(a->inv()),
                         a->report};
}

}  // namespace
