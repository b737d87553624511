"""prec="gmres_poly" at the ABI level, its roots, and the NumPy restatement the
GPU tests compare against (CPU only: nothing here launches a kernel).

The preconditioner is M^-1 r = p(B) D r with B = D A, D the inverse diagonal
of prec="jacobi", A the matrix the Arnoldi cycle runs on, and

    1 - x p(x) = prod_{i <= s} (1 - x / theta_i),

theta_i the harmonic Ritz values of s Arnoldi steps on B from v_0 = D g,
g = rand_vect(n, 1) - 0.5: the eigenvalues of H_s + h^2 f e_s^T, h = h_{s+1,s},
H_s^T f = e_s (mpg_gmres_poly_roots, solve.h), in Leja order. It is applied in
product form (np_poly_apply below): with the running product p (p_0 = D r) and
the result z, a real root is  p <- p - (1/theta) B p,  z <- z + (1/theta_next) p;
a pair a +- bi is  t = 2a p - B p,  z <- z + c t,  p <- p - c B t,
c = 1 / (a^2 + b^2). The CPU oracle does not know it: the reference is
np_poly_apply inside the restart loop of tests/test_neumann_cpu.py::np_solve,
restated here with the apply as an argument."""
import ctypes as C

import numpy as np
import pytest

from oracle import gmres_np
from tests.golden.make_golden import convdiff
from tests.test_chebyshev_cpu import np_jacobi_bound, np_solve_cheb
from tests.test_neumann_cpu import np_solve

_DP = C.POINTER(C.c_double)

# ---------------------------------------------------------------- restatement


def np_poly_step(s_in, d, p, z, c0, c1, first=False):
    """MPG_POLY_STEP on a row sum already rounded to T: returns (z, out), each
    operation rounded to the arrays' type. first: z is not read (it may be None)."""
    T = p.dtype.type
    assert s_in.dtype == d.dtype == p.dtype
    c0, c1 = T(c0), T(c1)
    u = (d * s_in).astype(T)
    v = (c0 * u).astype(T)
    o = (p - v).astype(T)
    y = (c1 * o).astype(T)
    zin = (c0 * p).astype(T) if first else z
    return (zin + y).astype(T), o


def np_poly_pair(s_in, d, p, z, c0, c1, first=False):
    """MPG_POLY_PAIR (a pair's first half), c0 = 2a, c1 = 1 / (a^2 + b^2)."""
    T = p.dtype.type
    assert s_in.dtype == d.dtype == p.dtype
    c0, c1 = T(c0), T(c1)
    u = (d * s_in).astype(T)
    q = (c0 * p).astype(T)
    t = (q - u).astype(T)
    y = (c1 * t).astype(T)
    zin = (T(0) * p).astype(T) if first else z
    return (zin + y).astype(T), t


def np_poly_apply(Ain, d, r, roots, rowsum=None):
    """p(B) D r in r's type, the chain of mpg_arnoldi_poly_apply (arnoldi.h);
    Ain a scipy CSR matrix of that type (fp64 row sums, rounded once: the class
    of the stand-alone SpMVs), or rowsum(g) -> T(A g) in its place; roots
    complex, in the order applied."""
    T = r.dtype.type
    re, im = np.real(roots).astype(np.float64), np.imag(roots).astype(np.float64)
    count = len(re)
    if rowsum is None:
        A64 = Ain.astype(np.float64)
        rowsum = lambda g: (A64 @ g.astype(np.float64)).astype(T)
    if count == 1:
        return ((T(1.0 / re[0]) * d).astype(T) * r).astype(T)
    omega_at = lambda k: 0.0 if im[k] != 0.0 else 1.0 / re[k]
    p = ((T(1) * d).astype(T) * r).astype(T)
    z, first, k = None, True, 0
    while k < count:
        pair = im[k] != 0.0
        kn = k + (2 if pair else 1)
        if not pair:
            if kn >= count:
                break
            z, p = np_poly_step(rowsum(p), d, p, z, 1.0 / re[k], omega_at(kn), first)
        else:
            aa, bb = re[k] * re[k], im[k] * im[k]
            c = 1.0 / (aa + bb)
            z, t = np_poly_pair(rowsum(p), d, p, z, 2.0 * re[k], c, first)
            if kn >= count:
                break
            z, p = np_poly_step(rowsum(t), d, p, z, c, omega_at(kn))
        first, k = False, kn
    return z


def start_vector(mpg, n, T):
    """g of the set-up: T(u) - T(0.5), u = rand_vect(n, 1)."""
    return (mpg.rand_vect(n, 1).astype(T) - T(0.5)).astype(T)


def np_arnoldi(Ain, d, g, s):
    """s MGS steps on B = D A from v_0 = D g: vectors in the arrays' type,
    dots in fp64, H (s + 1) x s in fp64. Returns H and ||v_0||."""
    T = g.dtype.type
    A64 = Ain.astype(np.float64)
    v0 = (d * g).astype(T)
    beta = float(np.sqrt(np.dot(v0.astype(np.float64), v0.astype(np.float64))))
    V = [(T(1.0 / beta) * v0).astype(T)]
    H = np.zeros((s + 1, s))
    for k in range(s):
        w = (d * (A64 @ V[k].astype(np.float64)).astype(T)).astype(T)
        for j in range(k + 1):
            H[j, k] = float(np.dot(V[j].astype(np.float64), w.astype(np.float64)))
            w = (w + (T(-H[j, k]) * V[j]).astype(T)).astype(T)
        H[k + 1, k] = float(np.sqrt(np.dot(w.astype(np.float64), w.astype(np.float64))))
        V.append((T(1.0 / H[k + 1, k]) * w).astype(T))
    return H, beta


def harmonic_matrix(H):
    """H_s + h^2 f e_s^T with H_s^T f = e_s."""
    s = H.shape[1]
    Hs = H[:s, :s].copy()
    e = np.zeros(s)
    e[-1] = 1.0
    f = np.linalg.solve(Hs.T, e)
    Hs[:, -1] += H[s, s - 1] ** 2 * f
    return Hs


def leja_scores(placed, cand):
    if not placed:
        return np.abs(cand)
    with np.errstate(divide="ignore"):
        return np.sum(np.log(np.abs(np.asarray(cand)[:, None] - np.asarray(placed)[None, :])), axis=1)


def np_roots(H):
    """numpy's eigenvalues of the same matrix in the library's Leja order (a
    pair: the mean of the two real parts, +im first)."""
    ev = np.linalg.eigvals(harmonic_matrix(H))
    items = [complex(v.real, 0.0) for v in ev if v.imag == 0.0] + [v for v in ev if v.imag > 0.0]
    placed = []
    while items:
        sc = leja_scores(placed, np.array(items))
        v = items.pop(int(np.argmax(sc)))
        placed += [v] if v.imag == 0.0 else [v, v.conjugate()]
    return np.array(placed)


def lib_roots(mpg, H, lib=None):
    s = H.shape[1]
    Hc = np.ascontiguousarray(H, dtype=np.float64)
    re, im, cnt = np.full(s, np.nan), np.full(s, np.nan), C.c_int(-1)
    st = (lib or mpg.host_lib()).mpg_gmres_poly_roots(s, Hc.ctypes.data_as(_DP), s, re.ctypes.data_as(_DP),
                                                      im.ctypes.data_as(_DP), C.byref(cnt))
    assert st == 0 and cnt.value == s, (st, cnt.value)
    return re + 1j * im


def gmres_residual(H, beta=1.0):
    """min_y || beta e_1 - H y || / beta."""
    e = np.zeros(H.shape[0])
    e[0] = beta
    y = np.linalg.lstsq(H, e, rcond=None)[0]
    return float(np.linalg.norm(e - H @ y)) / beta


def np_solve_apply(A, b, mode, orth, rlen, tol, make_apply, max_restarts=1000):
    """tests/test_neumann_cpu.py::np_solve line for line, with the apply built
    by make_apply(Ain, d) -> f(v of T) -> T. Modes mixed and baseline (P = T)."""
    n, m = A.nrows, rlen
    T = np.float32 if mode == "mixed" else np.float64
    d = gmres_np.jacobi_diag(A.rowptr, A.col, A.val, T)
    A32 = gmres_np._Problem(A, np.float32).A
    A64 = gmres_np._Problem(A, np.float64).A
    if mode == "mixed":
        Ain, Aout, X = A32, A64, np.float64
        a_norm = float(np.linalg.norm(A.val.astype(np.float32)))
        bb = b.astype(np.float64)
    else:
        Ain = A32.astype(T)
        Aout, X = Ain, T
        a_norm = T(np.linalg.norm(Ain.data))
        bb = b.astype(T)
    fn = make_apply(Ain, d)

    def apply_m(v, into=T):
        return fn(v.astype(T)).astype(into)

    x = np.zeros(n, X)
    b_norm = X(np.linalg.norm(bb))
    minvb = float(np.linalg.norm(apply_m(bb)))
    cyc_r, cyc_norm, cyc_beta, hist, step_cycle = [], [], [], [], []
    restarts = 0
    for i in range(10**9):
        r = (bb - Aout @ x).astype(X)
        w = r.astype(T)
        r_norm = float(np.linalg.norm(w)) if mode == "mixed" else float(X(np.linalg.norm(r)))
        w = apply_m(w)
        beta = float(T(np.linalg.norm(w)))
        x_norm = float(np.linalg.norm(x))
        normal = float(X(b_norm + X(a_norm) * X(x_norm))) if mode != "mixed" else b_norm + a_norm * x_norm
        cyc_r.append(r_norm)
        cyc_norm.append(normal)
        cyc_beta.append(beta)
        restarts += 1
        if restarts > max_restarts:
            status = "aborted"
            break
        if r_norm / normal <= tol:
            status = "converged"
            break
        before = len(hist)
        y, V = gmres_np._cycle(lambda v: (Ain @ v).astype(T), apply_m, w, m, orth, T, minvb, hist)
        step_cycle += [i] * (len(hist) - before)
        inc = (V[:, :m] @ y).astype(T)
        x = (x + inc.astype(X)).astype(X)
    return dict(status=status, restarts=i, total_iters=len(hist), cyc_r_norm=np.array(cyc_r),
                cyc_normalization=np.array(cyc_norm), cyc_beta=np.array(cyc_beta), step_res=np.array(hist),
                step_cycle=np.array(step_cycle, dtype=np.int32), x=x.astype(np.float64), minvb_norm=minvb)


def np_solve_poly(mpg, A, b, mode, orth, rlen, tol, steps=None, roots=None, max_restarts=1000):
    """The loop with np_poly_apply; roots given (the engine's own), or from a
    NumPy set-up of `steps` Arnoldi steps in the mode's type."""

    def make(Ain, d):
        th = roots
        if th is None:
            H, _ = np_arnoldi(Ain, d, start_vector(mpg, A.nrows, d.dtype.type), steps)
            th = np_roots(H)
        return lambda v: np_poly_apply(Ain, d, v, th)

    return np_solve_apply(A, b, mode, orth, rlen, tol, make, max_restarts)


# ---------------------------------------------------------------- ABI
def test_make_args_fills_the_struct(mpg):
    from mpgmres_amd._abi import PRECS, SolveArgs

    A = mpg.gen_laplace3d(3)
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec="gmres_poly", jacobi_steps=4)
    assert a.prec == 7 and a.jacobi_steps == 4 and PRECS["gmres_poly"] == 7
    # no new field: the struct ends where it did
    assert [f for f, _ in SolveArgs._fields_][-2:] == ["accum", "prec_block"]


NEW_HIP = {"capi.h": ("mpg_csr_poly_sweep_f64", "mpg_csr_poly_sweep_f32", "mpg_sell_poly_sweep_f64",
                      "mpg_sell_poly_sweep_f32"),
           "arnoldi.h": ("mpg_arnoldi_poly_apply",)}
NEW_HOST = ("mpg_engine_prec_roots", "mpg_gmres_poly_roots")


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for header, fns in NEW_HIP.items():
        for name in fns:
            assert (header, name) in declared, name
            assert hasattr(mpg.hip_lib(), name)
    for name in NEW_HOST:
        assert ("solve.h", name) in declared, name
        assert hasattr(mpg.host_lib(), name)
    assert hasattr(mpg.hip_lib(), "mpg_gmres_poly_roots")  # (either library reaches it)
    text = (mpg.REPO_DIR / "include" / "mpgmres" / "solve.h").read_text()
    assert "MPG_PREC_GMRES_POLY = 7" in text


def test_null_context_calls_are_refused(mpg):
    """The argument checks come before any device work."""
    hip = mpg.hip_lib()
    for t, ct in (("f64", C.c_double), ("f32", C.c_float)):
        assert getattr(hip, f"mpg_csr_poly_sweep_{t}")(None, None, None, None, None, None, None, None, 0, 1, 1, ct(1),
                                                       ct(1)) == -2
        assert getattr(hip, f"mpg_sell_poly_sweep_{t}")(None, None, None, None, None, None, None, 0, 1, 1, ct(1),
                                                        ct(1)) == -2
    one = (C.c_double * 1)(1.0)
    zero = (C.c_double * 1)(0.0)
    assert hip.mpg_arnoldi_poly_apply(None, 1, one, zero, None, None, None) == -2
    host = mpg.host_lib()
    assert host.mpg_engine_prec_roots(None, None, None, 0) == -1
    cnt = C.c_int(0)
    two = (C.c_double * 2)(1.0, 1.0)
    assert host.mpg_gmres_poly_roots(0, two, 1, one, zero, C.byref(cnt)) == -2
    assert host.mpg_gmres_poly_roots(65, two, 65, one, zero, C.byref(cnt)) == -2
    assert host.mpg_gmres_poly_roots(1, None, 1, one, zero, C.byref(cnt)) == -2
    assert host.mpg_gmres_poly_roots(1, two, 0, one, zero, C.byref(cnt)) == -2
    assert host.mpg_gmres_poly_roots(1, two, 1, one, zero, None) == -2


def test_roots_breakdown_is_reported(mpg):
    """A zero root and a singular H_s (with h != 0) are MPG_ERR_BREAKDOWN (-6); h = 0
    gives the eigenvalues of H_s (the Ritz values of an invariant subspace)."""
    host = mpg.host_lib()
    re, im, cnt = (C.c_double * 2)(), (C.c_double * 2)(), C.c_int(0)
    H = np.array([[0.0], [0.0]])
    assert host.mpg_gmres_poly_roots(1, H.ctypes.data_as(_DP), 1, re, im, C.byref(cnt)) == -6 and cnt.value == 0
    H = np.array([[0.0], [1.0]])
    assert host.mpg_gmres_poly_roots(1, H.ctypes.data_as(_DP), 1, re, im, C.byref(cnt)) == -6
    H = np.array([[2.0, 1.0], [0.0, 3.0], [0.0, 0.0]])
    assert np.array_equal(lib_roots(mpg, H), [3.0, 2.0])
    H = np.array([[1.0, -2.0], [2.0, 1.0], [0.0, 0.0]])  # 1 +- 2i
    assert np.array_equal(lib_roots(mpg, H), [1.0 + 2.0j, 1.0 - 2.0j])


# ---------------------------------------------------------------- the roots
MATRICES = {"lap12": lambda mpg: mpg.gen_laplace3d(12), "convdiff32": lambda mpg: convdiff(mpg),
            "band4352": lambda mpg: mpg.gen_band(4352, 5, 4, seed=7)}
STEPS = (1, 2, 3, 5, 8, 12)
_H = {}


def arnoldi_case(mpg, name, s):
    """(H, ||v_0||, Ain, d, g) of the fp64 NumPy Arnoldi, computed once."""
    if (name, s) not in _H:
        A = MATRICES[name](mpg)
        d = gmres_np.jacobi_diag(A.rowptr, A.col, A.val, np.float64)
        Ain = gmres_np._Problem(A, np.float64).A
        g = start_vector(mpg, A.nrows, np.float64)
        _H[(name, s)] = np_arnoldi(Ain, d, g, s) + (Ain, d, g)
    return _H[(name, s)]


def multiset_distance(a, b):
    """Greedy matching distance of two equal-sized complex multisets."""
    b = list(b)
    worst = 0.0
    for v in a:
        j = int(np.argmin([abs(v - w) for w in b]))
        worst = max(worst, abs(v - b.pop(j)))
    return worst


def test_roots_against_numpy(mpg):
    """mpg_gmres_poly_roots against numpy.linalg.eigvals of the same modified
    matrix, as multisets, within 1e-8 max|theta| (a guard against a wrong
    algorithm: a missed deflation or a dropped pair is O(1) off; not a measured
    accuracy). The cases hold a complex pair and a list that ends in a pair.
    Measured worst difference / max|theta|: 5.7e-15 (convdiff32, s = 12)."""
    worst, any_pair, ends_in_pair = (0.0, ""), False, False
    for name in MATRICES:
        for s in STEPS:
            H = arnoldi_case(mpg, name, s)[0]
            got = lib_roots(mpg, H)
            want = np.linalg.eigvals(harmonic_matrix(H))
            scale = float(np.max(np.abs(want)))
            dist = multiset_distance(got, want) / scale
            worst = max(worst, (dist, f"{name} s = {s}"))
            any_pair |= bool(np.any(got.imag != 0.0))
            ends_in_pair |= got[-1].imag != 0.0
            assert dist <= 1e-8, (name, s, dist)
            assert np.array_equal(lib_roots(mpg, H, mpg.hip_lib()), got)  # the one function, through either library
    print(f"worst |theta - eigvals| / max|theta|: {worst[0]:.3e} ({worst[1]})")
    assert any_pair and ends_in_pair


def test_leja_order(mpg):
    """At each position the chosen root's score (|theta| first, then
    sum_j log|theta - theta_j| over the members placed) is within 1e-9 of the
    best among the roots left; pairs are adjacent, the +im member first, equal
    bits of re and opposite im."""
    for name in MATRICES:
        for s in STEPS:
            th = lib_roots(mpg, arnoldi_case(mpg, name, s)[0])
            k = 0
            while k < s:
                sc = leja_scores(list(th[:k]), th[k:])
                assert sc[0] >= np.max(sc) - 1e-9, (name, s, k, sc)
                if th[k].imag != 0.0:
                    assert th[k].imag > 0.0 and k + 1 < s, (name, s, k)
                    assert th[k + 1].real == th[k].real and th[k + 1].imag == -th[k].imag
                    k += 1
                k += 1


def test_product_form_is_the_gmres_polynomial(mpg):
    """With the library's roots and the apply restated in fp64: v_0 - B apply(g)
    is the residual polynomial at v_0, so its norm over ||v_0|| is the s-step
    GMRES residual from H, within 1e-10 absolute for s <= 12 (measured 1.1e-16
    with the library's roots; the cap guards against a wrong root)."""
    worst = 0.0
    for name in MATRICES:
        for s in STEPS:
            H, beta, Ain, d, g = arnoldi_case(mpg, name, s)
            u = np_poly_apply(Ain, d, g, lib_roots(mpg, H))
            v0 = d * g
            got = float(np.linalg.norm(v0 - d * (Ain @ u)) / np.linalg.norm(v0))
            want = gmres_residual(H)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-10, (name, s, got, want)
    print(f"worst |product-form residual - GMRES residual|: {worst:.3e}")


def test_first_forms_start_from_the_first_term():
    """first = True is the general form from z = c0 p (a step) or 0 p (a pair)."""
    rng = np.random.default_rng(2)
    for T in (np.float32, np.float64):
        s, d, p = (rng.standard_normal(129).astype(T) for _ in range(3))
        for fn, z0 in ((np_poly_step, (T(0.37) * p).astype(T)), (np_poly_pair, (T(0) * p).astype(T))):
            a, b = fn(s, d, p, None, 0.37, 0.81, first=True), fn(s, d, p, z0, 0.37, 0.81)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- it preconditions (NumPy)
def test_numpy_counts_lap16(mpg):
    """gen_laplace3d(16), rand_vect(n, 42), baseline, CGS, GMRES(10), tol
    1e-10. All runs converge; gmres_poly s = 6 takes no more iterations than
    neumann s = 6, and twice s = 3 no more than jacobi. (The counts are
    printed: jacobi 120, neumann 30 / 30 at s = 4 / 6, gmres_poly 40 / 30 / 20 at
    s = 3 / 4 / 6. "s = 4 fewer than neumann s = 4" held with a uniform stand-in
    for rand_vect but not with rand_vect itself, 30 against 30, so it is not
    asserted.)"""
    A = mpg.gen_laplace3d(16)
    b = mpg.host_spmv(A, mpg.rand_vect(A.nrows, 42))
    runs = {"jacobi": np_solve(A, b, "baseline", "cgs", 10, 1e-10, 1)}
    for s in (4, 6):
        runs[f"neumann{s}"] = np_solve(A, b, "baseline", "cgs", 10, 1e-10, s)
    for s in (3, 4, 6):
        runs[f"poly{s}"] = np_solve_poly(mpg, A, b, "baseline", "cgs", 10, 1e-10, steps=s)
    it = {k: r["total_iters"] for k, r in runs.items()}
    print("numpy total_iters (lap16):", it)
    assert all(r["status"] == "converged" for r in runs.values())
    assert it["poly6"] <= it["neumann6"]
    assert 2 * it["poly3"] <= it["jacobi"]


def test_numpy_counts_convdiff32(mpg):
    """convdiff(32) (nonsymmetric), the same settings: gmres_poly takes fewer
    iterations than neumann at s = 6 and at s = 8."""
    A = convdiff(mpg, 32)
    b = mpg.host_spmv(A, mpg.rand_vect(A.nrows, 42))
    runs = {}
    for s in (6, 8):
        runs[f"neumann{s}"] = np_solve(A, b, "baseline", "cgs", 10, 1e-10, s)
        runs[f"poly{s}"] = np_solve_poly(mpg, A, b, "baseline", "cgs", 10, 1e-10, steps=s)
    it = {k: r["total_iters"] for k, r in runs.items()}
    print("numpy total_iters (convdiff32):", it)
    assert all(r["status"] == "converged" for r in runs.values())
    assert it["poly6"] < it["neumann6"]
    assert it["poly8"] < it["neumann8"]


def test_numpy_counts_band(mpg):
    """gen_band(4352, 5, 4, seed=7) at s = 4: gmres_poly converges in no more
    iterations than jacobi (10 against 30). chebyshev on its default interval
    [b / 30, b], which a look-alike of this matrix left unconverged after 60
    restarts, converges on the generator's own matrix in this loop (30
    iterations), so that condition is printed and not asserted."""
    A = mpg.gen_band(4352, 5, 4, seed=7)
    b = mpg.host_spmv(A, mpg.rand_vect(A.nrows, 42))
    bound = np_jacobi_bound(A, np.float64)
    cheb = np_solve_cheb(A, b, "baseline", "cgs", 10, 1e-10, 4, (bound / 30.0, bound), max_restarts=60)
    jac = np_solve(A, b, "baseline", "cgs", 10, 1e-10, 1)
    poly = np_solve_poly(mpg, A, b, "baseline", "cgs", 10, 1e-10, steps=4)
    print("numpy (band4352): chebyshev", cheb["status"], cheb["total_iters"], "jacobi", jac["status"], jac["total_iters"],
          "gmres_poly", poly["status"], poly["total_iters"])
    assert jac["status"] == "converged" and poly["status"] == "converged"
    assert poly["total_iters"] <= jac["total_iters"]
