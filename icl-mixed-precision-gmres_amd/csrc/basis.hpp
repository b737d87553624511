// Storage types of the Krylov basis V of the fused Arnoldi cycle (gfx950).
//
// The Arnoldi kernels that touch V are templated on a storage tag B beside
// the Arnoldi precision T, through the one interface Basis<T, B>:
//
//   elem               what V holds
//   Raw4 / load(p)     4 consecutive rows of one column, kept as stored
//   Raw4::at<A>(r)     ... entry r as used, in the accumulation type A
//   get<A>(p)          one entry as used (the n mod 4 rows)
//   store(p, v)        one entry; v is a value round() returned
//   round(v)           the value every consumer of V sees for an Arnoldi
//                      vector entry v = T(w_prev * inv)
//   kBatch             columns per load batch of the panel kernels
//
// B = T (the default everywhere): V holds T, round is the identity, and the
// kernels compile to the device code they had before the tag existed.
//
// B = basis_f16 (fp32 Arnoldi): the compressed basis. An entry v is stored
// as h = fp16_rne(2^14 v) and used as v^ = 2^-14 float(h). Both scalings are
// exact; |v| <= 1 up to rounding, so 2^14 |v| stays far below 65504, and
// fp16's normal range reaches down to |v| = 2^-28 (3.7e-9) -- unscaled, the
// 3e-4 of a typical entry at 10M rows would sit next to fp16's smallest
// normal 6.1e-5. A non-finite v stays non-finite. The cast is _Float16's
// (v_cvt_f16_f32, round to nearest even); the packed cvt_pkrtz builtin rounds
// toward zero and is not used. The operator is applied to v^_k, not v_k
// (round() at every place the SpMV forms T(w_prev * inv)), which keeps
// A V^ = V^ H. Four rows are 8 bytes; a batch holds twice the columns of the
// fp32 basis, the same bytes in flight per lane.
//
// B = basis_f16emu: v^ stored as fp32. V keeps the fp32 layout and the panel
// kernels are the fp32 ones; only round() is active, in the SpMV. Every value
// and every product is the one basis_f16 forms, so whole solves agree bit for
// bit: the tests' reference for the compressed kernels.
#ifndef MPGMRES_BASIS_HPP
#define MPGMRES_BASIS_HPP

#include "panel.hpp"

namespace mpg {

struct basis_f16 {};
struct basis_f16emu {};

constexpr float kBasisScale = 16384.0f;             // 2^14
constexpr float kBasisUnscale = 1.0f / 16384.0f;    // 2^-14

// (the scale by ldexp, not a multiplication: the compiler folds v * 2^14 and the
// cast into one v_fma_mixlo_f16 with a +0 addend, which turns -0 into +0)
__device__ __forceinline__ _Float16 basis_pack(float v) { return (_Float16)__builtin_ldexpf(v, 14); }
__device__ __forceinline__ float basis_unpack(_Float16 h) { return (float)h * kBasisUnscale; }

template <class T, class B = T>
struct Basis;

template <class T>
struct Basis<T, T> {
    using elem = T;
    using Raw4 = mpg::Raw4<T>;
    static constexpr bool kRounds = false;
    static constexpr int kBatch = kColBatch<T>;
    static __device__ __forceinline__ T round(T v) { return v; }
    static __device__ __forceinline__ void store(elem* p, T v) { *p = v; }
    template <class A>
    static __device__ __forceinline__ A get(const elem* p) { return (A)*p; }
};

template <>
struct Basis<float, basis_f16emu> : Basis<float, float> {
    static constexpr bool kRounds = true;
    static __device__ __forceinline__ float round(float v) { return basis_unpack(basis_pack(v)); }
};

// 4 consecutive fp16 entries (i a multiple of 4: 8-B aligned, V's leading
// dimension is a multiple of 128 entries), kept packed until used
struct HalfRaw4 {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    h4 v;
    __device__ __forceinline__ void load(const _Float16* p) { v = *reinterpret_cast<const h4*>(p); }
    template <class A>
    __device__ __forceinline__ A at(int r) const {
        return (A)basis_unpack(r == 0 ? v.x : r == 1 ? v.y : r == 2 ? v.z : v.w);
    }
};

template <>
struct Basis<float, basis_f16> {
    using elem = _Float16;
    using Raw4 = HalfRaw4;
    static constexpr bool kRounds = true;
    static constexpr int kBatch = 2 * kColBatch<float>;
    static __device__ __forceinline__ float round(float v) { return basis_unpack(basis_pack(v)); }
    // (v = round(.): 2^14 v is a half exactly, the cast rounds nothing)
    static __device__ __forceinline__ void store(elem* p, float v) { *p = basis_pack(v); }
    template <class A>
    static __device__ __forceinline__ A get(const elem* p) { return (A)basis_unpack(*p); }
};

// How the tag reaches a kernel: on its accumulation-class parameter. A kernel
// template <..., class AT = double> is instantiated with AT = double / float
// (the fp32 basis: the same symbols and the same device code as before the
// tag existed) or with AT = WithBasis<A, B>; inside, AccOf<AT>::type is the
// accumulation class A and BasisOf<T, AT> the storage interface. The kernels'
// signatures keep `T* V`: a compressed V is passed as such and viewed through
// basis_ptr (the identity for B = T).
template <class A, class B>
struct WithBasis {};
template <class AT>
struct AccOf {
    using type = AT;
    template <class T> using basis = T;
};
template <class A, class B>
struct AccOf<WithBasis<A, B>> {
    using type = A;
    template <class T> using basis = B;
};
template <class T, class AT>
using BasisOf = Basis<T, typename AccOf<AT>::template basis<T>>;

template <class Bs, class T>
__device__ __forceinline__ typename Bs::elem* basis_ptr(T* V) {
    return reinterpret_cast<typename Bs::elem*>(V);
}
template <class Bs, class T>
__device__ __forceinline__ const typename Bs::elem* basis_ptr(const T* V) {
    return reinterpret_cast<const typename Bs::elem*>(V);
}

}  // namespace mpg

#endif  // MPGMRES_BASIS_HPP
