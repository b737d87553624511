"""NumPy restatement of the fused Arnoldi phase launches (include/mpgmres/arnoldi.h).

One function per phase: it takes the arrays the device would read and returns
what the launch must leave, in fp64 (longdouble for the long sums), with a
rounding to T exactly where the kernels' headers state one. Beside each
result come the magnitudes (abs_sum, scale, ...) the bounds below are built
from. The seeded input generators and the bounds are shared by the GPU tests
(tests/test_arnoldi_phases_gpu.py) and by the CPU test that shows each bound
can see the defects it is there for (tests/test_arnoldi_ref_cpu.py).

Layouts as in arnoldi.h: V column j starts at j * ld of the flat buffer, H is
(m + 1) x m column-major (column k at k * (m + 1)); here V is an (ld, ncols)
Fortran-ordered array whose rows >= n are padding, H an (m + 1, m) one."""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

LD = np.longdouble
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def unit(T):
    """Unit roundoff of T."""
    return UNIT[np.dtype(T)]


def csr64(A, T):
    """A's values rounded to T, as an fp64 SciPy matrix (what a kernel with values of type T multiplies)."""
    return sp.csr_matrix((A.val.astype(T).astype(np.float64), A.col, A.rowptr), shape=(A.nrows, A.ncols))


# ---------------------------------------------------------------- inputs
W_SEED = 24  # the w of the dots cases: a stream on which no two neighbouring dots lie within 4 bounds (cpu test)


def gen_vec(n, seed, j=0, dtype=np.float32):
    """Column j of the test data: magnitude uniform in [0.5, 1] (1 + j / 64),
    a random sign, its own seed stream per (seed, j). No entry is small, so a
    wrong row, column or stride cannot cancel."""
    rng = np.random.default_rng([seed, j])
    mag = rng.uniform(0.5, 1.0, n) * (1.0 + j / 64.0)
    return (mag * rng.choice([-1.0, 1.0], n)).astype(dtype)


def gen_basis(n, ld, ncols, seed, dtype=np.float32):
    """(ld, ncols) Fortran array: gen_vec columns in rows < n, and in the
    padding rows a value (3) that no correct launch reads."""
    V = np.full((ld, ncols), 3.0, dtype, order="F")
    for j in range(ncols):
        V[:n, j] = gen_vec(n, seed, j, dtype)
    return V


def partial_scale(n):
    """The power of two gen_basis_toward scales its columns by: sum_j |c_j| |v_ij| <= 0.15 at 128 columns."""
    return 2.0 ** -np.ceil(0.5 * np.log2(n * 112 / 0.15))


def gen_basis_toward(w, n, ld, ncols, seed, dtype=np.float32):
    """The basis of the cases whose coefficients are the dots themselves
    (cgs_partials, cgsr_wide_pass, the mgs_partials chain, the compressed
    basis). With gen_basis the dots are random sums of order sqrt(n): some lie
    near zero or near a neighbour, and w' = w - V c is a random vector of
    order n whose small rows no bound on ||w'||^2 can see. Here the magnitudes
    follow gen_vec's rule and the signs are still drawn per entry, but
    sign(v_ij w_i) = sign(b_j) with probability (1 + |b_j|) / 2, b_j =
    (-1)^j (0.3 + 0.15 (j mod 3)): <v_j, w> is about b_j sum_i |v_ij w_i|,
    neighbours differ in sign and size, and every column is scaled by
    partial_scale(n) (a power of two: the same mantissas), which keeps
    sum_j |c_j| |v_ij| below 0.15 and every |w'_i| above 0.35."""
    V = np.full((ld, ncols), 3.0, dtype, order="F")
    sw = np.sign(np.asarray(w[:n], np.float64))
    for j in range(ncols):
        rng = np.random.default_rng([seed, j, 1])
        b = (-1.0) ** j * (0.3 + 0.15 * (j % 3))
        sig = np.where(rng.random(n) < 0.5 * (1 + abs(b)), np.sign(b), -np.sign(b))
        V[:n, j] = (np.abs(gen_vec(n, seed, j, np.float64)) * sig * sw * partial_scale(n)).astype(dtype)
    return V


def gen_coefs(nc, seed=31):
    """fp64 coefficient sums for an update of gen_vec(., ., 5) by nc gen_basis
    columns: no T holds them exactly (the launch rounds them), and
    sum_j |c_j| max|v_ij| <= 0.15, so every |w'_i| >= 0.5 * (1 + 5 / 64) - 0.15:
    no row of w' is small beside the others, and the ||w'||^2 bound sees each."""
    rng = np.random.default_rng([seed, nc])
    mag = rng.uniform(0.5, 1.0, nc) * 0.15 / (nc * (1.0 + np.arange(nc) / 64.0))
    return mag * rng.choice([-1.0, 1.0], nc)


def gen_upper(m, k, seed, dtype=np.float32):
    """(m + 1, m) Fortran array: H(0:k, 0:k) upper triangular, diagonal in
    [2, 3], off-diagonals uniform(-1, 1) / k; 5 elsewhere (never read)."""
    rng = np.random.default_rng([seed, k])
    H = np.full((m + 1, m), 5.0, np.float64, order="F")
    H[:k, :k] = np.triu(rng.uniform(-1.0, 1.0, (k, k)) / k, 1) + np.diag(rng.uniform(2.0, 3.0, k))
    return np.asfortranarray(H.astype(dtype))


def gen_rotations(m, seed, dtype=np.float32):
    """cs, sn with cs^2 + sn^2 = 1 to rounding and both well away from 0, and s of both signs."""
    rng = np.random.default_rng([seed, 77])
    th = rng.uniform(0.3, 1.2, m + 1) * rng.choice([-1.0, 1.0], m + 1)
    return np.cos(th).astype(dtype), np.sin(th).astype(dtype), gen_vec(m + 1, seed + 1, 0, dtype)


# ---------------------------------------------------------------- phases
def ref_spmv_step(A64, w_prev, inv, diag=None, n_front=0):
    """v = T(w_prev * inv) (one multiply in T: exact bits), w = A v in fp64
    (d o (A v) with diag), and scale = |d| o (|A| |v|).
    With halo rows w_prev has n_front + n_ext entries (local ids [-n_front,
    n_ext)) and A64 is n x (n_front + n_ext), its columns shifted by n_front:
    v_ext = T(w_prev * inv) over all of them, the rows are summed in fp64 over
    v_ext, and the v returned -- what V(:,k) must hold, bit for bit -- is
    v_ext on the rows [0, n) only."""
    T = w_prev.dtype
    n = A64.shape[0]
    assert A64.shape[1] == len(w_prev) and n_front + n <= len(w_prev)
    v_ext = (w_prev * T.type(inv)).astype(T)
    v64 = v_ext.astype(np.float64)
    w = np.asarray(A64 @ v64)
    scale = np.asarray(abs(A64) @ np.abs(v64))
    if diag is not None:
        d = np.asarray(diag, np.float64)
        w, scale = d * w, np.abs(d) * scale
    return v_ext[n_front:n_front + n], w, scale


def half_values(A, scale=1, n_front=0):
    """mpg_csr_half_values' rule (capi.h) on A's fp64 values: e_i = 0 when the
    row's largest finite |a_ij| lies in [2^-2, 2^15) (or scale == 0, or the
    row holds no nonzero), else e_i = 14 - floor(log2 max |a_ij|); the stored
    entry is fp16_rne(fp32_rne(a_ij 2^e_i)) (the two roundings of the device's
    cast). Returns the fp16 bits (CSR order), e (int64 per row) and the fp64
    SciPy matrix of float(h_ij) 2^-e_i -- what a SpMV over the copy multiplies:
    it forms the row sum of the h_ij and unscales it by the power of two, which
    commutes with every rounding in the normal range, so the reference row sum
    is formed over this matrix and the bound of a T-valued matrix carries over.
    n_front: A's columns are local ids in [-n_front, A.ncols); the matrix
    returned is n x (n_front + A.ncols), the columns shifted by n_front."""
    n = A.nrows
    rows = np.repeat(np.arange(n), np.diff(A.rowptr))
    a = np.abs(A.val)
    fin = np.isfinite(a)
    m = np.zeros(n)
    np.maximum.at(m, rows[fin], a[fin])
    e = np.zeros(n, np.int64)
    if scale:
        E = np.frexp(np.where(m > 0, m, 1.0))[1] - 1  # floor(log2 m): m = f 2^x, f in [0.5, 1)
        out = (m > 0) & ((E < -2) | (E > 14))
        e[out] = 14 - E[out]
    with np.errstate(over="ignore"):
        h = np.ldexp(A.val, e[rows]).astype(np.float32).astype(np.float16)
    M = sp.csr_matrix((np.ldexp(h.astype(np.float64), -e[rows]), A.col.astype(np.int64) + n_front, A.rowptr),
                      shape=(n, n_front + A.ncols))
    return h.view(np.uint16), e, M


def ref_node_bj(A64, w_prev, inv, dinv):
    """k_step_node_bj (arnoldi_spmv.hpp): v = T(w_prev * inv); every row sum
    t_i = (A v)_i is rounded to T and taken to P; then, per 3 x 3 block, row i
    of w = Dinv t is formed in P as ((d_i0 t_0 + d_i1 t_1) + d_i2 t_2), each
    product rounded, summed left to right, no contraction, and stored as T.
    dinv: mpg_bjacobi_setup_*'s 3 values per row, row-major per block. Here t
    and w = Dinv t are exact fp64 sums; beside them the magnitudes
    tol_node_bj is built from: scale = |A| |v| and absDt = |Dinv| |t|."""
    v, t, scale = ref_spmv_step(A64, w_prev, inv)
    n = len(t)
    assert n % 3 == 0 and len(dinv) == 3 * n
    D = np.asarray(dinv, np.float64).reshape(n // 3, 3, 3)
    w = np.einsum("bij,bj->bi", D, t.reshape(-1, 3)).reshape(-1)
    absDt = np.einsum("bij,bj->bi", np.abs(D), np.abs(t).reshape(-1, 3)).reshape(-1)
    return dict(v=v, t=t, scale=scale, w=w, absDt=absDt, absD=np.abs(D))


def tol_node_bj(R, terms, T, P, acc32):
    """The bound of ref_node_bj's w, from k_step_node_bj's statement. The
    device's t^_j = P(T(sum_j)) differs from t_j by at most delta_j = u_T |t_j|
    + (terms + 1) (u_A + 2^-53) scale_j (the plain SpMV's bound: the row sum in
    the class A and the restatement's own fp64 sum, then the rounding to T; P
    holds T exactly or is wider). Through the exact product that is |Dinv|
    delta. The three products and two adds in P put at most three roundings on
    each term: 3 u_P |Dinv| (|t| + delta) (Higham, Accuracy and Stability,
    eq. 3.4 with gamma_3 <= 3 u (1 + 2^-20)). The store to T: u_T |w|. And the
    restatement's own 3-term fp64 sum: 3 2^-53 |Dinv| |t|."""
    ua = 2.0 ** -24 if acc32 else 2.0 ** -53
    delta = unit(T) * np.abs(R["t"]) + (terms + 1) * (ua + 2.0 ** -53) * R["scale"]
    Dd = np.einsum("bij,bj->bi", R["absD"], delta.reshape(-1, 3)).reshape(-1)
    return ((Dd + 3 * unit(P) * (R["absDt"] + Dd) + unit(T) * np.abs(R["w"])) * (1 + 2.0 ** -20)
            + 3 * 2.0 ** -53 * R["absDt"])


def ref_dots(V, w):
    """<v_j, w> per column of V (n x nc) and abs_sum_j = sum_i |v_ij w_i|, as fp64."""
    P = V.astype(LD) * w.astype(LD)[:, None]
    return P.sum(axis=0).astype(np.float64), np.abs(P).sum(axis=0).astype(np.float64)


def ref_cgs_update(V, c, w):
    """w - V c in fp64, t = V c, and the per-row scale |w_i| + sum_j |c_j| |v_ij|."""
    c = np.asarray(c)
    P = V.astype(LD) * c.astype(LD)[None, :]
    t = P.sum(axis=1)
    return ((w.astype(LD) - t).astype(np.float64), t.astype(np.float64),
            (np.abs(w.astype(LD)) + np.abs(P).sum(axis=1)).astype(np.float64))


def ref_mgs_update(vj, h, w):
    """w - h v_j by the same rule."""
    return ref_cgs_update(vj[:, None], np.array([h]), w)


def rotg_ref(a, b):
    """rotg_ref of csrc/arnoldi_givens.hpp on scalars of one NumPy type; returns r, c, s."""
    T = type(a)
    roe = a if abs(a) > abs(b) else b
    scale = abs(a) + abs(b)
    if scale == T(0):
        return T(0), T(1), T(0)
    as_, bs = a / scale, b / scale
    r = scale * np.sqrt(as_ * as_ + bs * bs)
    r = r if roe >= T(0) else -r
    return r, a / r, b / r


def ref_givens(k, Hcol, corr, cs, sn, s, nrm2sq, T):
    """givens_block: every operation one rounding in T, no contraction. Hcol,
    cs, sn, s: arrays of T with at least k + 2 entries (Hcol[k + 1] is
    overwritten). Returns col (k + 2 entries), cs_k, sn_k, s(k:k+2), inv, report."""
    T = np.dtype(T).type
    col = np.array(Hcol[:k + 2], T)
    if corr is not None:
        col[:k + 1] = col[:k + 1] + T(1) * np.asarray(corr[:k + 1], T)
    hn = T(np.sqrt(np.float64(nrm2sq)))
    col[k + 1] = hn
    with np.errstate(divide="ignore"):
        inv = T(1) / hn
    for j in range(k):
        a1, a2 = col[j], col[j + 1]
        col[j] = cs[j] * a1 + sn[j] * a2
        col[j + 1] = cs[j] * a2 - sn[j] * a1
    r, c, sv = rotg_ref(col[k], col[k + 1])
    col[k], col[k + 1] = r, T(0)
    a1, a2 = T(s[k]), T(s[k + 1])
    sk, sk1 = c * a1 + sv * a2, c * a2 - sv * a1
    return dict(col=col, cs=c, sn=sv, s=np.array([sk, sk1], T), inv=inv, hn=hn, report=float(abs(sk1)))


def ref_update(V, H, s, k, x):
    """y from an fp64 solve of the T-valued H(0:k,0:k) y = s(0:k); x + V y in
    fp64; t = V y; |V| |y|; and g = |H^-1| |H| |y|, the vector of the solve's bound."""
    Hk = np.asarray(H[:k, :k], np.float64)
    y = sl.solve_triangular(Hk, np.asarray(s[:k], np.float64), lower=False)
    Hinv = sl.solve_triangular(Hk, np.eye(k), lower=False)
    g = np.abs(Hinv) @ (np.abs(np.triu(Hk)) @ np.abs(y))
    V64 = V[:, :k].astype(LD)
    t = (V64 * y.astype(LD)[None, :]).sum(axis=1)
    return dict(y=y, x=(x.astype(LD) + t).astype(np.float64), t=t.astype(np.float64),
                absVy=(np.abs(V64) @ np.abs(y).astype(LD)).astype(np.float64), g=g,
                absVg=(np.abs(V64) @ g.astype(LD)).astype(np.float64))


def ref_prologue(A64, b, x, T, diag=None, n_front=0):
    """r = b - A x in fp64 with its cancellation scale |b| + |A| |x|; w0 =
    T(r), with Jacobi T(d o T(r)); r_norm = ||T(r)||, beta = ||w0|| rounded to
    T, x_norm; inv_beta = T(1) / beta.
    With halo rows x has n_front + n_ext entries and A64 is n x (n_front +
    n_ext) (ref_spmv_step's layout): the rows are summed over all of x, and
    x_norm is taken over the rows [0, n) only -- every k_prologue* adds x_i^2
    in the epilogue of row i, i < n, next to that row's own T(r)_i^2 and w_i^2
    (arnoldi_prologue.hpp), so a rank's three partials cover its own rows and
    the all-reduce over ranks counts each global row once."""
    T = np.dtype(T).type
    b64, x_all = np.asarray(b, np.float64), np.asarray(x, np.float64)
    assert A64.shape[1] == len(x_all)
    x_own = x_all[n_front:n_front + A64.shape[0]]
    r = b64 - np.asarray(A64 @ x_all)
    scale = np.abs(b64) + np.asarray(abs(A64) @ np.abs(x_all))
    tr = r.astype(T)
    w0 = tr if diag is None else (np.asarray(diag, T) * tr).astype(T)
    nrm = lambda v: float(np.sqrt((v.astype(LD) ** 2).sum()))
    beta = T(nrm(w0))
    return dict(r=r, scale=scale, w0=w0, r_norm=float(T(nrm(tr))), beta=float(beta), x_norm=nrm(x_own),
                inv_beta=float(T(1) / beta), nnz_row=int(np.diff(A64.indptr).max()))


# ---------------------------------------------------------------- bounds
DEPTH32 = 64  # the fp32 class' rounding-chain bound, below
REF = 2.0 ** -53  # the restatement's own error: its longdouble results are returned rounded to fp64


def tol_sum(ref, abs_sum, n, T, acc32):
    """A sum of n products read back as fp64 and compared with the exact one.
    fp64 class: the products of fp32 values are exact, any order of n fp64
    adds errs by at most n 2^-53 abs_sum (order-free), and a value stored in T
    adds one rounding u_T |ref|.
    fp32 class: the order-free n u is wider than one row's share, so the depth
    of the launch's own tree is used instead: a lane adds at most one quad of
    rows (4 fused multiply-adds), a wave tree has 6 levels, a workgroup at
    most 16 waves, at most 3 workgroup partials and 3 tail rows per column,
    and the row-grid forms about one row per lane under a 256-lane tree of
    partials: about 32 roundings on the longest path, doubled to DEPTH32 = 64,
    each at most u_32 abs_sum."""
    # (an fp64 Arnoldi's products are themselves rounded: one term more)
    ua = 2.0 ** -24 * DEPTH32 if acc32 else (n + (np.dtype(T) == np.float64)) * 2.0 ** -53
    return unit(T) * np.abs(ref) + ua * abs_sum + REF * np.abs(ref)


def tol_rows(ref, t, scale, terms, T, acc32):
    """A row update w_i - T(t_i), t_i a sum of `terms` products in the class A:
    order-free, (terms + 1) u_A scale_i for the sum; the kernels round t to T
    before the subtraction (arnoldi_orth.hpp: w = w - T(V coef)), u_T |t_i|;
    and the result is stored in T, u_T |ref_i|. (1 + 2^-20 covers the
    second-order terms.)"""
    ua = 2.0 ** -24 if acc32 else 2.0 ** -53
    return (unit(T) * (np.abs(ref) + np.abs(t)) + (terms + 1) * ua * scale) * (1 + 2.0 ** -20) + REF * np.abs(ref)


def tol_spmv(ref, scale, terms, T, acc32, jacobi=0):
    """w = M(A v) against ref_spmv_step's fp64 row sums (the expression of
    tests/test_arnoldi_phases_gpu.py::_check_spmv): tol_rows' sum term over
    the row's entries in the class A, the restatement's own fp64 row sum
    ((terms + 1) 2^-53 scale), and one rounding to T (three with Jacobi: the
    row sum, d * w and its store)."""
    ua = 2.0 ** -24 if acc32 else 2.0 ** -53
    return ((3 if jacobi else 1) * unit(T) * np.abs(ref) + (terms + 1) * (ua + 2.0 ** -53) * scale) * (1 + 2.0 ** -20)


def tol_prologue_w0(P, T, diag=None):
    """w0 = M(T(b - A x)) against ref_prologue (test_prologue's expression): r
    is an fp64 sum of nnz products and one subtraction, (nnz + 2) 2^-53 (|b| +
    |A| |x|) whatever the order, twice (the device's evaluation and the
    restatement's own); then T(r), and with Jacobi d * T(r) rounded to T."""
    u = unit(T)
    dr = 2 * (P["nnz_row"] + 2) * 2.0 ** -53 * P["scale"]
    d = np.abs(np.asarray(diag, np.float64)) if diag is not None else 1.0
    return d * (dr + u * np.abs(P["r"])) * (1 + 2 * u) + u * np.abs(P["w0"])


def tol_update(R, k, x_ref, T, X, acc32):
    """x + X(T(V y)): tol_rows' terms for the row sums over k columns (scale
    |V| |y|, rounded to T, then added in X), plus the triangular solve in T:
    substitution is backward stable, |dy| <= 2 k u_T |H^-1| |H| |y| (Higham,
    Accuracy and Stability, thm 8.5, gamma_k <= 2 k u for k u < 1/2),
    propagated through |V|."""
    ua = 2.0 ** -24 if acc32 else 2.0 ** -53
    return (unit(X) * np.abs(x_ref) + unit(T) * np.abs(R["t"]) + (k + 1) * ua * R["absVy"]
            + 2 * k * unit(T) * R["absVg"]) * (1 + 2.0 ** -20) + REF * np.abs(x_ref)
