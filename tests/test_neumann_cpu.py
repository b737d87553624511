"""prec="neumann" at the ABI level, and the NumPy restatement the GPU tests
compare against (CPU only: nothing here launches a kernel).

The preconditioner is s Jacobi sweeps on A z = r from z = 0,

    z_1 = D r,    z_{j+1} = z_j + D (r - A z_j),   j = 1 .. s-1,

with D the inverse diagonal of prec="jacobi" (oracle.gmres_np.jacobi_diag) and
A the matrix the Arnoldi cycle runs on. The CPU oracle does not know it: the
reference is np_neumann_apply below inside a restart loop around
oracle.gmres_np._cycle, which is imported as it is (the pattern of
tests/test_bjacobi_gpu.py)."""
import ctypes as C

import numpy as np

from oracle import gmres_np
from tests.test_cycle_plan import describe, names, policy

# ---------------------------------------------------------------- restatement


def np_sweep(s_in, d, r, z):
    """The sweep's epilogue on a row sum already rounded to T: three
    operations, each rounded to the arrays' type."""
    T = z.dtype.type
    assert s_in.dtype == d.dtype == r.dtype == z.dtype
    t = (r - s_in).astype(T)
    u = (d * t).astype(T)
    return (z + u).astype(T)


def np_neumann_apply(Ain, d, r, steps):
    """z_s in r's type; Ain a scipy CSR matrix of that type (fp64 row sums,
    rounded once: the class of the stand-alone SpMVs)."""
    T = r.dtype.type
    A64 = Ain.astype(np.float64)
    z = (d * r).astype(T)
    for _ in range(steps - 1):
        s_in = (A64 @ z.astype(np.float64)).astype(T)
        z = np_sweep(s_in, d, r, z)
    return z


def np_solve(A, b, mode, orth, rlen, tol, steps, max_restarts=1000):
    """Restarted GMRES(m) with the Jacobi sweeps as M: the lines of
    oracle.gmres_np.solve around its call of _cycle. Modes mixed and baseline
    (P = T). steps = 0: no preconditioner."""
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

    def apply_m(v, into=T):
        return np_neumann_apply(Ain, d, v.astype(T), steps).astype(into)

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


# ---------------------------------------------------------------- ABI
def test_make_args_fills_the_struct(mpg):
    A = mpg.gen_laplace3d(3)
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec="neumann", jacobi_steps=4)
    assert a.prec == 5 and a.jacobi_steps == 4
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec="neumann")
    assert a.prec == 5 and a.jacobi_steps == 1  # the reference's default


NEW_HIP = {"capi.h": ("mpg_csr_jacobi_sweep_f64", "mpg_csr_jacobi_sweep_f32", "mpg_sell_jacobi_sweep_f64",
                      "mpg_sell_jacobi_sweep_f32"),
           "arnoldi.h": ("mpg_arnoldi_neumann_apply",)}


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for header, fns in NEW_HIP.items():
        for name in fns:
            assert (header, name) in declared, name
            assert hasattr(mpg.hip_lib(), name)
    assert ("solve.h", "mpg_engine_prec_sweeps") in declared
    assert hasattr(mpg.host_lib(), "mpg_engine_prec_sweeps")


def test_null_context_calls_are_refused(mpg):
    """The argument checks come before any device work."""
    hip = mpg.hip_lib()
    for t in ("f64", "f32"):
        assert getattr(hip, f"mpg_csr_jacobi_sweep_{t}")(None, None, None, None, None, None, None) == -2
        assert getattr(hip, f"mpg_sell_jacobi_sweep_{t}")(None, None, None, None, None, None) == -2
    assert hip.mpg_arnoldi_neumann_apply(None, 2, None, None, None) == -2


def test_arnoldi_desc_matches_the_header(mpg):
    """_abi.ArnoldiDesc lists mpg_arnoldi_desc's fields in the header's order."""
    import re

    from mpgmres_amd._abi import ArnoldiDesc

    text = (mpg.REPO_DIR / "include" / "mpgmres" / "arnoldi.h").read_text()
    body = text[text.index("typedef struct {"):text.index("} mpg_arnoldi_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f for f, _ in ArnoldiDesc._fields_]


def test_cycle_plan_applies_it_after_every_spmv(mpg):
    """With the sep_prec* flags the engine sets for this preconditioner the
    plan holds apply_prec(w0) after the prologue and one apply_prec(wK) per
    step, and no step takes the one-launch SpMV + dots forms."""
    m = 4
    p = policy(mpg, m=m, sep_prec=1, sep_prec_step=1, sep_prec_prologue=1, step_dots=-1, step_dots_ok=[1] * 32,
               spmv_dots_ok=[1] * 32, fuse_dots=1)
    got = names(describe(mpg, p))
    assert got.count("apply_prec(w0)") == 1 and got[got.index("prologue") + 1] == "apply_prec(w0)"
    for k in range(m):
        assert got.count(f"apply_prec(w{k + 1})") == 1
        i = got.index(f"apply_prec(w{k + 1})")
        assert got[i - 1] in (f"spmv({k})", f"givens+spmv({k})") and got[i + 1] == f"dots({k})"
    assert not any(t.startswith(("step_dots", "spmv_dots")) for t in got)
    assert describe(mpg, policy(mpg, m=m, sep_prec=1, sep_prec_step=1, sep_prec_prologue=1, step_dots=2,
                                step_dots_ok=[1] * 32)) == -5


# ---------------------------------------------------------------- it preconditions (NumPy)
def test_numpy_counts(mpg):
    """The condition of the GPU test test_it_preconditions, on the CPU:
    gen_laplace3d(12), rand_vect(n, 42), the NumPy loop at mode baseline, CGS,
    rlen 10, tol 1e-10 converges with s = 1, 2 and 4, in strictly fewer
    iterations each time, and s = 4 takes at most half of s = 1 (the counts
    are printed: 80 / 40 / 30 here; s = 3 takes 40, no fewer than s = 2)."""
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    runs = {s: np_solve(A, b, "baseline", "cgs", 10, 1e-10, s) for s in (1, 2, 4)}
    print("numpy total_iters:", {s: r["total_iters"] for s, r in runs.items()})
    assert all(r["status"] == "converged" for r in runs.values())
    assert runs[1]["total_iters"] > runs[2]["total_iters"] > runs[4]["total_iters"]
    assert 2 * runs[4]["total_iters"] <= runs[1]["total_iters"]


def test_one_sweep_is_jacobi(mpg):
    """s = 1 in the restatement is oracle.gmres_np's prec="jacobi"."""
    A = mpg.gen_laplace3d(5)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    for mode in ("baseline", "mixed"):
        ref = gmres_np.solve(A, b, mode=mode, orth="cgs", prec="jacobi", rlen=10, tol=1e-8)
        got = np_solve(A, b, mode, "cgs", 10, 1e-8, 1)
        assert np.array_equal(ref["step_res"], got["step_res"]) and np.array_equal(ref["x"], got["x"])
