"""NumPy restatement of the compressed Krylov basis (csrc/basis.hpp) and of a
mixed-precision CGS / CGSR GMRES(m) that stores its basis through it.

An Arnoldi vector entry v = fp32(w * inv) is stored as h = fp16_rne(2^14 v)
and used everywhere, by the operator too, as v^ = 2^-14 float(h). The loop is
oracle.gmres_np.solve's for mode mixed (fp64 residual and x, fp32 Arnoldi,
Jacobi or no preconditioner, the oracle's rotg and triangular solve), written
out so that the basis passes through `rnd` and every sum has a stated class:

  sums="fp64"   fp32 products added in fp64 and rounded once (the GPU's
                default accumulation class);
  sums="seq32"  products rounded to fp32 and added one after the other in
                fp32 (np.cumsum: the longest rounding chain an fp32 class has).

A GPU reduction is a tree of fp32 or fp64 adds, between the two; a count both
give cannot be moved by its order."""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

from oracle import gmres_np

F32 = np.float32
SCALE = F32(16384.0)      # 2^14
UNSCALE = F32(1.0 / 16384.0)


def pack_f16(v):
    """The stored bits: fp16_rne(2^14 v) of fp32 values, as uint16."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(v, F32) * SCALE).astype(np.float16).view(np.uint16)


def round_f16(v):
    """v^ = 2^-14 float(fp16_rne(2^14 v)), fp32 in and out."""
    h = np.asarray(pack_f16(v)).view(np.float16)
    return (h.astype(F32) * UNSCALE).astype(F32)


def _dots(Vk, w, sums):
    """V_k^T w rounded to fp32."""
    if sums == "fp64":
        return (Vk.astype(np.float64).T @ w.astype(np.float64)).astype(F32)
    prod = (Vk * w[:, None]).astype(F32)
    return np.cumsum(prod, axis=0, dtype=F32)[-1]


def _gemv(Vk, c, sums):
    """V_k c rounded to fp32 (row sums over the columns in order)."""
    if sums == "fp64":
        return (Vk.astype(np.float64) @ c.astype(np.float64)).astype(F32)
    prod = (Vk * c[None, :]).astype(F32)
    return np.cumsum(prod, axis=1, dtype=F32)[:, -1]


def _nrm2(w, sums):
    return F32(np.sqrt(_dots(w[:, None], w, sums)[0]))


def _cycle(Aop, apply_m, w, m, orth, rnd, sums, history):
    """oracle.gmres_np._cycle for T = fp32 with every basis column passed
    through rnd and the sums in the class `sums`; returns (y, V)."""
    n = len(w)
    V = np.zeros((n, m + 1), F32, order="F")
    H = np.zeros((m + 1, m), F32, order="F")
    cs, sn, s = np.zeros(m + 1, F32), np.zeros(m + 1, F32), np.zeros(m + 1, F32)
    beta = _nrm2(w, sums)
    V[:, 0] = rnd(((F32(1) / beta) * w).astype(F32)) if beta != 0 else 0
    s[0] = beta
    for k in range(m):
        w = apply_m(Aop(V[:, k])).astype(F32)
        Vk = V[:, :k + 1]
        H[:k + 1, k] = _dots(Vk, w, sums)
        w = (w - _gemv(Vk, H[:k + 1, k], sums)).astype(F32)
        if orth == "cgsr":
            c = _dots(Vk, w, sums)
            w = (w - _gemv(Vk, c, sums)).astype(F32)
            H[:k + 1, k] += c
        hn = _nrm2(w, sums)
        H[k + 1, k] = hn
        with np.errstate(divide="ignore", invalid="ignore"):
            V[:, k + 1] = rnd(((F32(1) / hn) * w).astype(F32))
        for j in range(k):
            a1, a2 = H[j, k], H[j + 1, k]
            H[j, k] = cs[j] * a1 + sn[j] * a2
            H[j + 1, k] = cs[j] * a2 - sn[j] * a1
        r, c_, sv = gmres_np.rotg(H[k, k], H[k + 1, k], F32)
        H[k, k], H[k + 1, k], cs[k], sn[k] = r, 0, c_, sv
        a1, a2 = s[k], s[k + 1]
        s[k] = c_ * a1 + sv * a2
        s[k + 1] = c_ * a2 - sv * a1
        history.append(abs(float(s[k + 1])))
    y = sl.solve_triangular(H[:m, :m], s[:m], lower=False).astype(F32)
    return y, V


def solve(A, b, xt=None, orth="cgs", prec="jacobi", rlen=30, tol=1e-10, basis="f32", sums="fp64",
          max_restarts=1000):
    """Mode mixed GMRES(rlen); basis "f32" or "f16" (f16emu is f16's values).
    Returns the fields of oracle.gmres_np.solve plus what tests/parity.py's
    compare() reads of a record (x_head, x_sum, res_norm, err_norm)."""
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
    x = np.zeros(n, np.float64)
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
