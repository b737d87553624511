// Derived from iamsonderr/icl-mixed-precision-gmres, Copyright (c) 2019-2021,
// University of Tennessee (BSD-3-Clause; the license text is in NOTICE).
// Operator surface of the GMRES hot path — the plugin boundary.
//
// Same operator set, names, argument order and <Type, Device> templating as
// the reference kernels.hpp:9-169 (dot / nrm2 with host or device result,
// axpy, naxpy, scal (x5), copy with cast, fill, rotg, rot (scalar and
// column), gemv, trsv, gdmv, spmv). A backend drops in by providing a Device
// tag (types.hpp) and explicit specialisations of these templates in its own
// translation unit — kernels_hip.cpp for `Hip`, the way kernels_mkl.cpp /
// kernels_cuda.cpp do for `MKL` / `Cuda` in the reference. The generic
// conveniences (scalar-type casting overloads, fill on any handle) are
// written once here on top of two backend primitives: fill_strided and
// jacobi_diag.
#ifndef MPGMRES_KERNELS_HPP
#define MPGMRES_KERNELS_HPP

#include <cassert>
#include <functional>
#include <utility>

#include "types.hpp"

// ---- copy with cast (kernels.hpp:11-30) ----
template <class Type1, class Type2, class Device>
void copy(Vect<Type1, Device> x, Vect<Type2, Device> y);
template <class Type1, class Type2, class Device>
void copy(Scalar<Type1, Device> x, Scalar<Type2, Device> y);

// ---- reductions ----
template <class Type, class Device>
Type dot(Vect<Type, Device> x, Vect<Type, Device> y);
template <class Type, class Device>
void dot(Vect<Type, Device> x, Vect<Type, Device> y, Scalar<Type, Device> result);
template <class Type, class Device>
Type nrm2(Vect<Type, Device> x);
template <class Type, class Device>
void nrm2(Vect<Type, Device> x, Scalar<Type, Device> result);

// ---- axpy family ----
template <class Type, class Device>
void axpy(Type alpha, Vect<Type, Device> x, Vect<Type, Device> y);
template <class Type, class Device>
void axpy(Scalar<Type, Device> alpha, Vect<Type, Device> x, Vect<Type, Device> y);
template <class ScalarType, class Type, class Device>
void axpy(ScalarType alpha, Vect<Type, Device> x, Vect<Type, Device> y) {
    axpy(Type(alpha), x, y);
}
// y <- y - alpha*x, alpha in device memory
template <class Type, class Device>
void naxpy(Scalar<Type, Device> alpha, Vect<Type, Device> x, Vect<Type, Device> y);

// ---- scal family ----
template <class Type, class Device>
void scal(Type alpha, Vect<Type, Device> x);
template <class Type, class Device>
void scal(Type alpha, Vect<Type, Device> x, Vect<Type, Device> y);
template <class ScalarType, class Type, class Device>
void scal(ScalarType alpha, Vect<Type, Device> x, Vect<Type, Device> y) {
    scal(Type(alpha), x, y);
}
template <class Type, class Device>
void scal(Scalar<Type, Device> alpha, Vect<Type, Device> x, Vect<Type, Device> y);
template <class Type, class Device>
void scal(Type alpha, Scalar<Type, Device> x, Scalar<Type, Device> y);
template <class ScalarType, class Type, class Device>
void scal(ScalarType alpha, Scalar<Type, Device> x, Scalar<Type, Device> y) {
    scal(Type(alpha), x, y);
}
template <class Type, class Device>
void scal(Scalar<Type, Device> alpha, Scalar<Type, Device> x, Scalar<Type, Device> y);
// y = (1/alpha) x with the reciprocal formed in Type where alpha lives: the
// reference's `inv = 1/h.access(); scal(inv, w, v)` (Orthogonalization.hpp:
// 51-60) without the host read (the same two roundings, so bit-identical).
// Addition to the reference surface; a backend without a device form can
// define it as exactly that host read.
template <class Type, class Device>
void scal_recip(Scalar<Type, Device> alpha, Vect<Type, Device> x, Vect<Type, Device> y);

// ---- fill (kernels.hpp:88-101) ----
// backend primitive: x[c*ld + r] = value for r < rows, c < cols
template <class Type, class Device>
void fill_strided(Type* x, size_t rows, size_t cols, size_t ld, Type value);

template <class Type, class Device, class ScalarType>
void fill(ScalarType alpha, Scalar<Type, Device> x) {
    fill_strided<Type, Device>(x.data(), 1, 1, 1, Type(alpha));
}
template <class Type, class Device, class ScalarType>
void fill(ScalarType alpha, Vect<Type, Device> x) {
    fill_strided<Type, Device>(x.data(), x.n(), 1, x.n(), Type(alpha));
}
template <class Type, class Device, class ScalarType>
void fill(ScalarType alpha, MultiVect<Type, Device> x) {
    fill_strided<Type, Device>(x.data(), x.nrows_base(), x.ncols_base(), x.stride(), Type(alpha));
}

// ---- Givens ----
template <class Type, class Device>
void rotg(Scalar<Type, Device> a, Scalar<Type, Device> b, Scalar<Type, Device> c, Scalar<Type, Device> s);
template <class Type, class Device>
void rot(Scalar<Type, Device> a, Scalar<Type, Device> b, Scalar<Type, Device> c, Scalar<Type, Device> s);
// apply rotations j = 0..c.n()-1 to the pairs (a[j], a[j+1])
template <class Type, class Device>
void rot(Vect<Type, Device> a, Vect<Type, Device> c, Vect<Type, Device> s);

// ---- BLAS-2 ----
template <class Type, class Device>
void gemv(Type alpha, MultiVect<Type, Device> matrix, Vect<Type, Device> x, Type beta, Vect<Type, Device> y);
template <class ScalarType, class Type, class Device>
void gemv(ScalarType alpha, MultiVect<Type, Device> matrix, Vect<Type, Device> x, ScalarType beta,
          Vect<Type, Device> y) {
    gemv(Type(alpha), matrix, x, Type(beta), y);
}
template <class Type, class Device>
void trsv(const char* upper, MultiVect<Type, Device> matrix, Vect<Type, Device> x);

// y = beta*y + alpha*diag∘x (kernels.hpp:131-151)
template <class Type, class Device>
void gdmv(Type alpha, Vect<Type, Device> diag, Vect<Type, Device> x, Type beta, Vect<Type, Device> y);
template <class ScalarType, class Type, class Device>
void gdmv(ScalarType alpha, Vect<Type, Device> diag, Vect<Type, Device> x, ScalarType beta, Vect<Type, Device> y) {
    gdmv(Type(alpha), diag, x, Type(beta), y);
}

// ---- sparse ----
template <class Type, class Device>
void spmv(Type alpha, SparseMatrix<Type, Device> matrix, Vect<Type, Device> x, Type beta, Vect<Type, Device> y);
template <class ScalarType, class Type, class Device>
void spmv(ScalarType alpha, SparseMatrix<Type, Device> matrix, Vect<Type, Device> x, ScalarType beta,
          Vect<Type, Device> y) {
    spmv(Type(alpha), matrix, x, Type(beta), y);
}

// backend primitive: Jacobi inverse diagonal with the eps_f32 * ||A||_inf
// boost of types.hpp:393-431
template <class Type, class Device>
void jacobi_diag(SparseMatrix<Type, Device> A, Vect<Type, Device> diag);

// ILU(0) of the fp64 matrix in precision Type (kernels.hpp:155-156), its
// triangular solves (kernels.hpp:168-169) and the Jacobi-sweep
// approximation of them (ilusv_jacobi, kernels.hpp:219-248).
template <class Type, class Device>
ILU<Type, Device> ilu0(SparseMatrix<double, Device> matrix);
template <class Type, class Device>
void ilusv(ILU<Type, Device> ilu, Vect<Type, Device> rhs);
template <class Type, class Device>
void ilusv_jacobi(ILU_Jacobi<Type, Device> ilu, Vect<Type, Device> x);

// Jacobi preconditioner M = D^-1 (types.hpp:381-448).
template <class Type, class Device>
class Jacobi : public LinearOperator<Type, Device> {
    Vect<Type, Device> diag_;

public:
    explicit Jacobi(SparseMatrix<Type, Device> A) : diag_(A.nrows()) { jacobi_diag(A, diag_); }
    int n() const { return (int)diag_.n(); }
    Type* diag_data() { return diag_.data(); }
    Vect<Type, Device> diag_vect() { return diag_; }
    void apply(Vect<Type, Device> rhs) override { gdmv(1.0, diag_, rhs, 0.0, rhs); }
};

// backend primitives: the inverses of A's bs x bs diagonal blocks (bs*bs
// values per block, row-major), and x <- blockdiag(dinv) x in place
template <class Type, class Device>
void bjacobi_setup(SparseMatrix<Type, Device> A, int bs, Vect<Type, Device> dinv);
template <class Type, class Device>
void bjacobi_apply(int bs, Vect<Type, Device> dinv, Vect<Type, Device> x);

// Block-Jacobi preconditioner M = blockdiag(D_r)^-1 for matrices ordered by
// node, bs = 2, 3 or 4 unknowns per node (an addition to the reference's
// set): built from A in the preconditioner precision, as Jacobi is.
template <class Type, class Device>
class BlockJacobi : public LinearOperator<Type, Device> {
    int bs_;
    Vect<Type, Device> dinv_;

public:
    BlockJacobi(SparseMatrix<Type, Device> A, int bs) : bs_(bs), dinv_((size_t)A.nrows() * (size_t)bs) {
        bjacobi_setup(A, bs_, dinv_);
    }
    int n() const { return (int)(dinv_.n() / (size_t)bs_); }
    int block() const { return bs_; }
    Vect<Type, Device> dinv_vect() { return dinv_; }
    void apply(Vect<Type, Device> rhs) override { bjacobi_apply(bs_, dinv_, rhs); }
};

// backend primitive: one Jacobi sweep z_out = z_in + dinv * (r - A z_in) on
// a square A, the three epilogue operations each rounded to Type; z_out may
// be r, never z_in
template <class Type, class Device>
void jacobi_sweep(SparseMatrix<Type, Device> A, Vect<Type, Device> dinv, Vect<Type, Device> r,
                  Vect<Type, Device> z_in, Vect<Type, Device> z_out);

// Jacobi-sweep polynomial preconditioner (an addition to the reference's
// set): `steps` Jacobi sweeps on A z = r from z = 0, the truncated Neumann
// series M^-1 = sum_{j<steps} (I - D A)^j D. D is Jacobi's inverse diagonal
// of A_diag (the matrix Jacobi is built from); the sweeps run on A, the
// matrix the Arnoldi cycle runs on. steps = 1 is Jacobi's apply.
template <class Type, class Device>
class Neumann : public LinearOperator<Type, Device> {
    SparseMatrix<Type, Device> A_;
    int steps_;
    Vect<Type, Device> diag_, work0_, work1_;

public:
    Neumann(SparseMatrix<Type, Device> A_diag, SparseMatrix<Type, Device> A, int steps)
        : A_(A), steps_(steps), diag_(A.nrows()) {
        jacobi_diag(A_diag, diag_);
        if (steps >= 2) work0_ = Vect<Type, Device>(A.nrows());
        if (steps >= 3) work1_ = Vect<Type, Device>(A.nrows());
    }
    int n() const { return (int)diag_.n(); }
    int steps() const { return steps_; }
    Vect<Type, Device> diag_vect() { return diag_; }
    // z_1 = D rhs (in place for one step), then the sweeps between the work
    // vectors with rhs as r; the last one stores into rhs
    void apply(Vect<Type, Device> rhs) override {
        gdmv(1.0, diag_, rhs, 0.0, steps_ == 1 ? rhs : work0_);
        for (int j = 1; j < steps_; ++j)
            jacobi_sweep(A_, diag_, rhs, (j - 1) & 1 ? work1_ : work0_, j == steps_ - 1 ? rhs : (j & 1 ? work1_ : work0_));
    }
};

// backend primitives of the Chebyshev preconditioner: one sweep
// z_out = z_in + alpha (z_in - z_prev) + beta dinv (r - A z_in), seven
// operations each rounded to Type (an empty z_prev: the first sweep, z_prev =
// 0); z_out may be r or z_prev, never z_in. And the Gershgorin bound
// max_i |dinv_i| sum_j |a_ij| of dinv A, a host value (set-up only).
template <class Type, class Device>
void cheb_sweep(SparseMatrix<Type, Device> A, Vect<Type, Device> dinv, Vect<Type, Device> r, Vect<Type, Device> z_in,
                Vect<Type, Device> z_prev, Vect<Type, Device> z_out, Type alpha, Type beta);
template <class Type, class Device>
double jacobi_bound(SparseMatrix<Type, Device> A, Vect<Type, Device> dinv);

// The interval [b / ratio, b] of the Chebyshev preconditioner, from the two
// settings read when it is set up: b = MPG_CHEB_LMAX (a real > 0) or, without
// it, gershgorin(); ratio = MPG_CHEB_RATIO (a real > 1), 30 without it. Throws
// (a status error naming the value) for a setting outside its range or a
// bound that is not finite and positive. Defined by the backend.
struct ChebInterval {
    double a, b;
    double theta() const { return 0.5 * (a + b); }
    double delta() const { return 0.5 * (b - a); }
};
ChebInterval cheb_interval(const std::function<double()>& gershgorin);
// mpg_cheb_coeffs (solve.h) for that interval; throws where it refuses
void cheb_coefficients(int steps, const ChebInterval& iv, double* alpha, double* beta);

// Chebyshev polynomial preconditioner (an addition to the reference's set):
// z_steps of the Chebyshev iteration on A z = r from z = 0 for a spectrum of
// D A near [a, b], D Jacobi's inverse diagonal of A_diag, the sweeps on A (as
// Neumann above). z_1 = (1 / theta) D r; steps = 1 is Jacobi scaled by
// 1 / theta. The coefficients are host constants rounded once to Type, so
// apply reads nothing on the host.
template <class Type, class Device>
class Chebyshev : public LinearOperator<Type, Device> {
    SparseMatrix<Type, Device> A_;
    int steps_;
    Vect<Type, Device> diag_, work0_, work1_;
    ChebInterval iv_{};
    double alpha_[64], beta_[64];

public:
    Chebyshev(SparseMatrix<Type, Device> A_diag, SparseMatrix<Type, Device> A, int steps)
        : A_(A), steps_(steps), diag_(A.nrows()) {
        jacobi_diag(A_diag, diag_);
        iv_ = cheb_interval([&] { return jacobi_bound(A_, diag_); });
        cheb_coefficients(steps_, iv_, alpha_, beta_);
        if (steps >= 2) work0_ = Vect<Type, Device>(A.nrows());
        if (steps >= 3) work1_ = Vect<Type, Device>(A.nrows());
    }
    int n() const { return (int)diag_.n(); }
    int steps() const { return steps_; }
    ChebInterval interval() const { return iv_; }
    Vect<Type, Device> diag_vect() { return diag_; }
    // z_1 into work0 (in place for one step); sweep j reads z_j from
    // buf[(j - 1) & 1] and z_{j-1} from buf[j & 1] and stores over the
    // latter, the last one into rhs
    void apply(Vect<Type, Device> rhs) override {
        gdmv(Type(alpha_[0]), diag_, rhs, Type(0), steps_ == 1 ? rhs : work0_);
        for (int j = 1; j < steps_; ++j) {
            Vect<Type, Device> keep = j & 1 ? work1_ : work0_;
            cheb_sweep(A_, diag_, rhs, (j - 1) & 1 ? work1_ : work0_, j == 1 ? Vect<Type, Device>() : keep,
                       j == steps_ - 1 ? rhs : keep, Type(alpha_[j]), Type(beta_[j]));
        }
    }
};

// backend primitives of the GMRES-polynomial preconditioner, whose residual
// polynomial is prod (1 - x / theta_i): with B = dinv A, the running product p
// and the result z (each operation rounded to Type)
//   poly_step: o = p - omega B g;  z += omega_next o;  out = o
//   poly_pair: t = 2a p - B p;     z += c t;           out = t
// g is p for a real root and the pair's t for a pair's second half (where
// out may be p). first: z is not read, it starts as omega p (step) or 0 p
// (pair). An empty out: the last form, z alone is stored. out is never g.
template <class Type, class Device>
void poly_step(SparseMatrix<Type, Device> A, Vect<Type, Device> dinv, Vect<Type, Device> g, Vect<Type, Device> p,
               Vect<Type, Device> z, Vect<Type, Device> out, bool first, Type omega, Type omega_next);
template <class Type, class Device>
void poly_pair(SparseMatrix<Type, Device> A, Vect<Type, Device> dinv, Vect<Type, Device> p, Vect<Type, Device> z,
               Vect<Type, Device> out, bool first, Type two_a, Type c);

// The roots of the GMRES polynomial in the order they are applied
// (mpg_gmres_poly_roots' Leja order, solve.h): `steps` Arnoldi steps on dinv A
// run once by the backend's set-up, fewer roots where those found an invariant
// subspace. A host value (set-up only); throws where there is no root.
struct PolyRoots {
    int count = 0;
    double re[64] = {}, im[64] = {};
};
template <class Type, class Device>
PolyRoots gmres_poly_roots(SparseMatrix<Type, Device> A, Vect<Type, Device> dinv, int steps);

// GMRES-polynomial preconditioner (an addition to the reference's set):
// p(D A) D rhs with 1 - x p(x) = prod (1 - x / theta_i), theta_i the harmonic
// Ritz values of `steps` Arnoldi steps on D A, D Jacobi's inverse diagonal of
// A_diag, the sweeps on A (as Neumann above). The constructor runs the
// set-up; the coefficients are host constants rounded once to Type, so apply
// reads nothing on the host.
template <class Type, class Device>
class GmresPoly : public LinearOperator<Type, Device> {
    SparseMatrix<Type, Device> A_;
    Vect<Type, Device> diag_, work0_, work1_;
    PolyRoots roots_;

    double omega_at(int k) const { return roots_.im[k] != 0.0 ? 0.0 : 1.0 / roots_.re[k]; }

public:
    GmresPoly(SparseMatrix<Type, Device> A_diag, SparseMatrix<Type, Device> A, int steps) : A_(A), diag_(A.nrows()) {
        jacobi_diag(A_diag, diag_);
        roots_ = gmres_poly_roots(A_, diag_, steps);
        if (roots_.count >= 2) work0_ = Vect<Type, Device>(A.nrows());
        if (roots_.count >= 3) work1_ = Vect<Type, Device>(A.nrows());
    }
    int n() const { return (int)diag_.n(); }
    int steps() const { return roots_.count; }
    const PolyRoots& roots() const { return roots_; }
    Vect<Type, Device> diag_vect() { return diag_; }
    // p_0 = D rhs into work0 (one root: (1 / theta) D rhs in place), z in rhs
    // from the first sweep on. A real root that is not the last: one step,
    // the new p into the other work vector. A pair: its first half stores t
    // there, its second half (unless the pair ends the list) gathers t and
    // stores the new p over the current one. A final real root's term came
    // with the sweep before it.
    void apply(Vect<Type, Device> rhs) override {
        const int count = roots_.count;
        const double *re = roots_.re, *im = roots_.im;
        if (count == 1) return gdmv(Type(1.0 / re[0]), diag_, rhs, Type(0), rhs);
        gdmv(Type(1), diag_, rhs, Type(0), work0_);
        Vect<Type, Device> cur = work0_, oth = work1_, none;
        bool first = true;
        for (int k = 0; k < count;) {
            const bool pair = im[k] != 0.0;
            const int kn = k + (pair ? 2 : 1);
            const bool next_ends = kn == count - 1 && im[kn] == 0.0;
            if (!pair) {
                if (kn >= count) break;
                poly_step(A_, diag_, cur, cur, rhs, next_ends ? none : oth, first, Type(1.0 / re[k]),
                          Type(omega_at(kn)));
                std::swap(cur, oth);
            } else {
                const double aa = re[k] * re[k], bb = im[k] * im[k];
                const double c = 1.0 / (aa + bb);
                const bool ends = kn >= count;
                poly_pair(A_, diag_, cur, rhs, ends ? none : oth, first, Type(2.0 * re[k]), Type(c));
                if (ends) break;
                poly_step(A_, diag_, oth, cur, rhs, next_ends ? none : cur, false, Type(c), Type(omega_at(kn)));
            }
            first = false;
            k = kn;
        }
    }
};

#endif  // MPGMRES_KERNELS_HPP
