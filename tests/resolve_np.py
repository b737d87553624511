"""tests/basis16_np.solve with an initial guess: the same outer loop (mode
mixed, fp64 residual and x, fp32 Arnoldi through basis16_np._cycle, the
update through basis16_np._gemv) started from x0 instead of zeros. The norms
of b and M^-1 b are the right-hand side's, as the drivers take them once
before the first restart; only x differs. With x0=None every operation is
basis16_np.solve's, in its order: the record is bit for bit the same.

Returns what tests/parity.py's compare() reads of a record."""
import numpy as np
import scipy.sparse as sp

from oracle import gmres_np
from tests.basis16_np import F32, _cycle, _gemv, round_f16


def solve(A, b, xt=None, x0=None, orth="cgs", prec="jacobi", rlen=30, tol=1e-10, basis="f32", sums="fp64",
          max_restarts=1000):
    assert basis in ("f32", "f16") and sums in ("fp64", "seq32") and orth in ("cgs", "cgsr")
    rnd = round_f16 if basis == "f16" else (lambda v: v)
    n, m = A.nrows, rlen
    d = gmres_np.jacobi_diag(A.rowptr, A.col, A.val, F32) if prec == "jacobi" else None
    A32 = sp.csr_matrix((A.val.astype(F32), A.col, A.rowptr), shape=(n, A.ncols))
    A64 = sp.csr_matrix((A.val.astype(np.float64), A.col, A.rowptr), shape=(n, A.ncols))
    A32w = A32.astype(np.float64)  # the fp32 values, for fp64 row sums

    def Aop(v):
        if sums == "fp64":
            return (A32w @ v.astype(np.float64)).astype(F32)
        return (A32 @ v).astype(F32)

    def apply_m(v):
        return v.astype(F32) if d is None else (d * v.astype(F32)).astype(F32)

    a_norm = float(np.linalg.norm(A.val.astype(F32)))
    bb = np.asarray(b, np.float64)
    x = np.zeros(n, np.float64) if x0 is None else np.array(x0, np.float64)
    assert x.shape == (n,)
    b_norm = float(np.linalg.norm(bb))
    minvb = float(np.linalg.norm(apply_m(bb)))
    cyc_r, cyc_norm, cyc_beta, hist, step_cycle = [], [], [], [], []
    restarts = 0
    for i in range(10**9):
        r = bb - A64 @ x
        w = r.astype(F32)
        r_norm = float(np.linalg.norm(w))
        w = apply_m(w)
        beta = float(F32(np.linalg.norm(w)))
        normal = b_norm + a_norm * float(np.linalg.norm(x))
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
        y, V = _cycle(Aop, apply_m, w, m, orth, rnd, sums, hist)
        step_cycle += [i] * (len(hist) - before)
        inc = _gemv(V[:, :m], y, sums)
        x = x + inc.astype(np.float64)
    out = dict(status=status, restarts=i, total_iters=len(hist), cyc_r_norm=np.array(cyc_r),
               cyc_normalization=np.array(cyc_norm), cyc_beta=np.array(cyc_beta), step_res=np.array(hist),
               step_cycle=np.array(step_cycle, dtype=np.int32), x=x, minvb_norm=minvb,
               x_head=x[:16].copy(), x_sum=float(np.sum(x)), res_norm=float(np.linalg.norm(bb - A64 @ x)))
    if xt is not None:
        out["err_norm"] = float(np.linalg.norm(x - np.asarray(xt, np.float64)))
    return out


def warm_guess(xt, seed=7, scale=1e-4):
    """x_true + scale * N(0, 1): the initial guess of the recorded warm cases."""
    return np.asarray(xt, np.float64) + scale * np.random.default_rng(seed).standard_normal(len(xt))
