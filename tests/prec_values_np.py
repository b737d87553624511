"""NumPy restatement of prec_values = "f16": the matrix A^ the polynomial
preconditioners' sweeps read, and the three preconditioners over it inside the
NumPy restart loop of tests/test_gmres_poly_cpu.py.

A^ = mpg_csr_half_values(A, scale = 1) (csrc/spmv.hip, k_half_rows): per row,
E = ilogb of the largest finite |a_ij|; the row is scaled by 2^e with
e = 14 - E when E < -2 or E > 14, else e = 0; every entry is then rounded
fp64 -> fp32 -> fp16. The sweeps' row sum is T(ldexp(sum_j half(a_ij) z_j, -e)),
which is the row sum of the fp32 matrix with entries float(half) 2^-e while none
of those is an fp32 subnormal: that matrix is what this module hands to the
restatements. Jacobi's diagonal, the Chebyshev interval and the GMRES-polynomial
roots stay those of float32(A), as in the engine.

Importing this module needs no GPU. The cases and their recorded cycle counts
(CASES, COUNTS) are read by tests/test_prec_values_gpu.py."""
import numpy as np

from tests.arnoldi_phase import gen_band_stiff
from tests.golden.make_golden import convdiff
from tests.test_chebyshev_cpu import np_cheb_apply, np_jacobi_bound
from tests.test_gmres_poly_cpu import np_arnoldi, np_poly_apply, np_roots, np_solve_apply, start_vector
from tests.test_neumann_cpu import np_neumann_apply

HALF_ROW_LO, HALF_ROW_HI, HALF_ROW_TOP = -2, 14, 14  # k_half_rows' constants


def half_values(A):
    """(fp16 values in CSR order, int8 row exponents) of mpg_csr_half_values(A.val, scale = 1)."""
    val = np.asarray(A.val, np.float64)
    rp = A.rowptr.astype(np.int64)
    rows = np.repeat(np.arange(A.nrows), np.diff(rp))
    mag = np.where(np.isfinite(val), np.abs(val), 0.0)
    m = np.zeros(A.nrows)
    np.maximum.at(m, rows, mag)
    e = np.zeros(A.nrows, np.int64)
    nz = m > 0
    E = np.zeros(A.nrows, np.int64)
    E[nz] = np.frexp(m[nz])[1] - 1  # ilogb
    out = nz & ((E < HALF_ROW_LO) | (E > HALF_ROW_HI))
    e[out] = HALF_ROW_TOP - E[out]
    assert np.all(np.abs(e) <= 127), "a row exponent outside int8"
    with np.errstate(over="ignore"):
        h = np.ldexp(val, e[rows]).astype(np.float32).astype(np.float16)
    return h, e.astype(np.int8)


def dequantised(h, e, rowptr):
    """float(half) 2^-e as fp32, the values prec_values = "f16emu" sweeps over."""
    rows = np.repeat(np.arange(len(e)), np.diff(rowptr.astype(np.int64)))
    return np.ldexp(h.astype(np.float32), -e.astype(np.int64)[rows]).astype(np.float32)


def hat_values(A):
    """A^'s entries as fp32, CSR order."""
    h, e = half_values(A)
    return dequantised(h, e, A.rowptr)


def hat_matrix(A):
    """A^ as a scipy CSR matrix of fp32."""
    import scipy.sparse as sp

    return sp.csr_matrix((hat_values(A), A.col.astype(np.int64), A.rowptr.astype(np.int64)),
                         shape=(A.nrows, A.ncols))


def differing_fraction(A):
    """The share of stored entries in which A^ is not float32(A)."""
    return float(np.mean(hat_values(A) != A.val.astype(np.float32)))


# ---------------------------------------------------------------- the preconditioners over A^
def make_apply(mpg, A, prec, steps, hat):
    """np_solve_apply's make_apply: the preconditioner `prec` with `steps`
    sweeps, its diagonal, interval and roots from the fp32 Arnoldi matrix Ain,
    its sweeps over A^ (hat) or over Ain itself."""
    Ahat = hat_matrix(A) if hat else None

    def make(Ain, d):
        T = d.dtype.type
        S = Ain if Ahat is None else Ahat.astype(T)
        if prec == "neumann":
            return lambda v: np_neumann_apply(S, d, v, steps)
        if prec == "chebyshev":
            b = np_jacobi_bound(A, T)
            return lambda v: np_cheb_apply(S, d, v, steps, (b / 30.0, b))
        assert prec == "gmres_poly", prec
        H, _ = np_arnoldi(Ain, d, start_vector(mpg, A.nrows, T), steps)
        roots = np_roots(H)
        S64 = S.astype(np.float64)
        return lambda v: np_poly_apply(Ain, d, v, roots, rowsum=lambda g: (S64 @ g.astype(np.float64)).astype(T))

    return make


def np_solve_prec_values(mpg, A, b, prec, steps, hat, orth="cgs", rlen=30, tol=1e-10, max_restarts=200):
    """Mixed GMRES(rlen) with the preconditioner's sweeps over A^ (hat) or float32(A)."""
    return np_solve_apply(A, b, "mixed", orth, rlen, tol, make_apply(mpg, A, prec, steps, hat), max_restarts)


# ---------------------------------------------------------------- the cases
def perturbed_lap(mpg, nx):
    A = mpg.gen_laplace3d(nx)
    return mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, mpg.perturb_values(A, 0.25, seed=5))


MATRICES = {
    "band4100": lambda m: m.gen_band(4100, 5, 4, seed=7),
    "band4099": lambda m: m.gen_band(4099, 5, 4, seed=7),
    "band8196": lambda m: m.gen_band(8196, 5, 4, seed=7),
    "convdiff32": lambda m: convdiff(m, 32),
    "lap12p": lambda m: perturbed_lap(m, 12),
    "lap16p": lambda m: perturbed_lap(m, 16),
    "band-stiff": lambda m: gen_band_stiff(m, 4099),
}

# (matrix, prec, sweeps): mixed CGS GMRES(30) to 1e-10, b = A rand_vect(n, 42)
CASES = [("lap16p", "chebyshev", 4), ("convdiff32", "gmres_poly", 4), ("band4100", "gmres_poly", 4)]

# Restart cycles of those cases in the restatement (Result.restarts: cycles
# run), with the sweeps over float32(A) and over A^: the same, which
# tests/test_prec_values_cpu.py asserts and tests/test_prec_values_gpu.py expects
# of the engine in both accumulation classes. (Recorded from the restatement.)
COUNTS = {("lap16p", "chebyshev", 4): 4, ("convdiff32", "gmres_poly", 4): 2, ("band4100", "gmres_poly", 4): 2}


def rhs(mpg, A):
    return mpg.host_spmv(A, mpg.rand_vect(A.nrows, 42))
