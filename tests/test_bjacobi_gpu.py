"""Block-Jacobi preconditioner (prec="bjacobi"): the set-up and apply kernels
against a NumPy restatement of their arithmetic, bit for bit; the refusals;
the storage forms; whole solves against a NumPy restart loop that applies
the same preconditioner; and that it preconditions better than point Jacobi
where the coupling inside a node dominates.

The CPU oracle does not know this preconditioner: the reference here is the
restatement below (fp64 Gauss-Jordan on [D | I] in the kernel's operation
order, the inverse rounded once to the preconditioner precision P; the apply
in P, products rounded, summed left to right) and, for whole solves, a
restart loop around oracle.gmres_np._cycle with that apply as M."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from oracle import gmres_np
from tests import parity

# ---------------------------------------------------------------- restatement


def np_blocks(A, bs, P):
    """The bs x bs diagonal blocks of A, values taken in P and widened to
    fp64: a missing entry is 0, the first occurrence of a column wins."""
    n = A.nrows
    assert n % bs == 0
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.rowptr))
    c = A.col.astype(np.int64) - rows // bs * bs
    keep = np.flatnonzero((c >= 0) & (c < bs))
    key = rows[keep] * bs + c[keep]
    key, first = np.unique(key, return_index=True)  # (index of the first occurrence of each key)
    D = np.zeros(n * bs, np.float64)
    D[key] = A.val.astype(P)[keep[first]].astype(np.float64)
    return D.reshape(n // bs, bs, bs)


def np_block_inverse(A, bs, P):
    """(dinv in P: bs*bs values per block, row-major; bad: blocks with a zero
    or non-finite pivot). Gauss-Jordan on [D | I] in fp64, every block in the
    same operation order: pivot = largest |entry| of the column at or below
    the diagonal (lowest row on a tie), rows swapped, the pivot row divided
    by the pivot, then row q -= M[q][c] * row c (product, then difference)."""
    D = np_blocks(A, bs, P)
    nb = D.shape[0]
    M = np.zeros((nb, bs, 2 * bs), np.float64)
    M[:, :, :bs] = D
    for i in range(bs):
        M[:, i, bs + i] = 1.0
    idx = np.arange(nb)
    bad = np.zeros(nb, bool)
    with np.errstate(all="ignore"):
        for c in range(bs):
            p = np.full(nb, c)
            best = np.abs(M[:, c, c])
            for q in range(c + 1, bs):
                a = np.abs(M[:, q, c])
                g = a > best
                best = np.where(g, a, best)
                p = np.where(g, q, p)
            bad |= ~(best > 0) | ~np.isfinite(best)
            rc, rp = M[idx, c, :].copy(), M[idx, p, :].copy()
            M[idx, p, :] = rc
            M[idx, c, :] = rp
            piv = M[:, c, c].copy()
            M[:, c, :] = M[:, c, :] / piv[:, None]
            for q in range(bs):
                if q == c:
                    continue
                f = M[:, q, c].copy()
                t = f[:, None] * M[:, c, :]
                M[:, q, :] = M[:, q, :] - t
        return M[:, :, bs:].astype(P).reshape(-1), bad


def np_block_apply(dinv, bs, x, P):
    """y_i = sum_j dinv[i][j] x_j per block in P (each product rounded, summed
    left to right); x cast to P before, the result back to x's type after."""
    xp = x.astype(P).reshape(-1, bs)
    d = dinv.reshape(-1, bs, bs)
    acc = d[:, :, 0] * xp[:, None, 0]
    for j in range(1, bs):
        acc = acc + d[:, :, j] * xp[:, None, j]
    assert acc.dtype == P
    return acc.reshape(-1).astype(x.dtype)


def np_solve(A, b, mode, orth, rlen, tol, max_restarts=1000, bs=3, prec="bjacobi"):
    """Restarted GMRES(m) with the block-Jacobi apply as M: the lines of
    oracle.gmres_np.solve around its call of _cycle, which is imported as it
    is. Modes mixed and baseline."""
    n, m = A.nrows, rlen
    T = np.float32 if mode == "mixed" else np.float64
    P = T
    dinv, bad = np_block_inverse(A, bs, P)
    assert not bad.any()

    def apply_m(v, into=T):
        return np_block_apply(dinv, bs, v.astype(P), P).astype(into)

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
    x = np.zeros(n, X)
    b_norm = X(np.linalg.norm(bb))
    minvb = float(np.linalg.norm(apply_m(bb)))
    cyc_r, cyc_norm, cyc_beta, steps, step_cycle = [], [], [], [], []
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
        before = len(steps)
        y, V = gmres_np._cycle(lambda v: (Ain @ v).astype(T), apply_m, w, m, orth, T, minvb, steps)
        step_cycle += [i] * (len(steps) - before)
        inc = (V[:, :m] @ y).astype(T)
        x = (x + inc.astype(X)).astype(X)
    return dict(status=status, restarts=i, total_iters=len(steps), cyc_r_norm=np.array(cyc_r),
                cyc_normalization=np.array(cyc_norm), cyc_beta=np.array(cyc_beta), step_res=np.array(steps),
                step_cycle=np.array(step_cycle, dtype=np.int32), x=x.astype(np.float64), minvb_norm=minvb)


def intra_scaled(mpg, A, scale, bs=3):
    """A with the off-diagonal entries inside each node's diagonal block
    multiplied by `scale` and the diagonal reset to 1 + sum |off-diagonals|
    (the generator's rule)."""
    rows = np.repeat(np.arange(A.nrows, dtype=np.int64), np.diff(A.rowptr))
    col = A.col.astype(np.int64)
    val = A.val.copy()
    diag = col == rows
    val[(col // bs == rows // bs) & ~diag] *= scale
    off = np.where(diag, 0.0, np.abs(val))
    val[diag] = 1.0 + np.add.reduceat(off, A.rowptr[:-1])[rows[diag]]
    return mpg.Csr(A.nrows, A.ncols, A.rowptr.copy(), A.col.copy(), val)


# the x16 intra-node variant of stencil27(5) (test 7); the NumPy loops' counts
# on it are in that test's docstring
INTRA_SCALE = 16.0


@pytest.fixture(scope="module")
def s5(mpg):
    A = mpg.gen_stencil27(5)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, xt, mpg.host_spmv(A, xt)


# ---------------------------------------------------------------- kernels
def _device_csr(mpg, hip, A):
    rp, col = hip.buf(A.rowptr, np.int32), hip.buf(A.col, np.int32)
    h = C.c_void_p()
    hip.call("mpg_csr_create", A.nrows, A.ncols, A.nnz, A.rowptr.ctypes.data, rp.p, col.p, C.byref(h))
    return h, (rp, col)


def _setup(mpg, hip, A, bs, P):
    """(status, dinv, first_bad_block) of mpg_bjacobi_setup_* on A's values in P."""
    h, keep = _device_csr(mpg, hip, A)
    try:
        vals = hip.buf(A.val.astype(P))
        out = hip.buf(np.zeros(A.nrows * bs, P))
        bad = C.c_int32(-7)
        name = "mpg_bjacobi_setup_f64" if P == np.float64 else "mpg_bjacobi_setup_f32"
        st = getattr(hip.lib, name)(hip.ctx, h, vals.p, bs, out.p, C.byref(bad))
        err = hip.lib.mpg_ctx_last_error(hip.ctx).decode()
        return st, out.get(), bad.value, err
    finally:
        hip.lib.mpg_csr_destroy(h)


SETUP_CASES = {
    "stencil27_2": (lambda m: m.gen_stencil27(2), 3),          # 8 nodes, every block at a boundary
    "stencil27_5_dof2": (lambda m: m.gen_stencil27(5, dof=2), 2),
    "stencil27_4_dof4": (lambda m: m.gen_stencil27(4, dof=4), 4),
    "laplace3d_6": (lambda m: m.gen_laplace3d(6), 3),          # entry (i, i+2) absent: reads as 0
    "band_13316": (lambda m: m.gen_band(13_316), 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("P", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(SETUP_CASES))
def test_setup_bits(mpg, hip, case, P):
    """mpg_bjacobi_setup_* gives the bits of the NumPy Gauss-Jordan."""
    gen, bs = SETUP_CASES[case]
    A = gen(mpg)
    ref, bad = np_block_inverse(A, bs, P)
    assert not bad.any()
    st, got, first_bad, _ = _setup(mpg, hip, A, bs, P)
    assert st == 0 and first_bad == -1
    assert got.dtype == ref.dtype and np.array_equal(got, ref)
    if case == "laplace3d_6":
        assert np.all(np_blocks(A, bs, P)[:, 0, 2] == 0)  # the absent entry


def _apply_sizes(bs):
    tile = 256 // bs * bs  # rows of one workgroup
    return [24, {2: 1030, 3: 1029, 4: 1028}[bs], 2 * tile, bs * (256 * 3) + bs]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f64", "f32", "f64_p32"])
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_apply_bits(mpg, hip, bs, kind):
    """mpg_bjacobi_apply_* gives the bits of the NumPy apply: 24 rows, a
    partial last workgroup and wave (343 nodes at bs = 3), two whole
    workgroups, and 3 * 256 nodes + 1."""
    T = np.float32 if kind == "f32" else np.float64
    P = np.float64 if kind == "f64" else np.float32
    rng = np.random.default_rng(17 + bs)
    for n in _apply_sizes(bs):
        assert n % bs == 0
        dinv = rng.standard_normal(n * bs).astype(P)
        x = rng.standard_normal(n).astype(T)
        ref = np_block_apply(dinv, bs, x, P)
        d, v = hip.buf(dinv), hip.buf(x)
        hip.call(f"mpg_bjacobi_apply_{kind}", n, bs, d.p, v.p)
        got = v.get()
        d.free(), v.free()
        assert np.array_equal(got, ref), (n, int(np.sum(got != ref)))


# ---------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals(mpg, hip, s5):
    """n % bs != 0, bs = 5, a singular block (named) and a row-partitioned
    solve are clean errors."""
    B = mpg.gen_laplace3d(5)  # 125 rows
    xb = mpg.rand_vect(B.nrows, 42)
    bb = mpg.host_spmv(B, xb)
    assert _setup(mpg, hip, B, 3, np.float64)[0] == -2
    A, xt, b = s5
    assert _setup(mpg, hip, A, 5, np.float32)[0] == -2
    v = hip.buf(np.ones(25))
    assert hip.lib.mpg_bjacobi_apply_f64(hip.ctx, 25, 5, v.p, v.p) == -2
    assert hip.lib.mpg_bjacobi_apply_f64(hip.ctx, 25, 3, v.p, v.p) == -2
    v.free()
    opts = dict(mode="mixed", orth="cgs", prec="bjacobi", rlen=30, tol=1e-8, max_restarts=20)
    for engine in ("fused", "surface"):
        with pytest.raises(RuntimeError, match="not a multiple of the block size 3"):
            mpg.solve(B, bb, xb, engine=engine, **opts)
        with pytest.raises(RuntimeError, match="prec_block must be 2, 3 or 4"):
            mpg.solve(A, b, xt, engine=engine, prec_block=5, **opts)
    # node 7's diagonal block zeroed in a copy of the arrays
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    val = A.val.copy()
    val[(rows // 3 == 7) & (A.col // 3 == 7)] = 0.0
    S = mpg.Csr(A.nrows, A.ncols, A.rowptr.copy(), A.col.copy(), val)
    assert np.flatnonzero(np_block_inverse(S, 3, np.float64)[1]).tolist() == [7]
    for P in (np.float64, np.float32):
        st, _, first_bad, err = _setup(mpg, hip, S, 3, P)
        assert st == -6 and first_bad == 7 and "block 7 " in err, (st, first_bad, err)
    for engine in ("fused", "surface"):
        for mode in ("mixed", "baseline"):
            with pytest.raises(RuntimeError, match="diagonal block 7 "):
                mpg.solve(S, b, xt, engine=engine, **{**opts, "mode": mode})
    with pytest.raises(RuntimeError, match="row-partitioned"):
        mpg.solve_loopback(A, b, xt, nranks=2, **opts)
    # the one-launch SpMV + dots step cannot hold a launch between the two
    got = mpg.solve(A, b, xt, engine="fused", **opts)  # (the context still works)
    assert got.status == "converged"


@pytest.mark.gpu
def test_step_dots_refuses_a_separate_apply(mpg, s5, monkeypatch):
    """MPG_STEP_DOTS=2 (required) with the apply in a launch of its own
    between the SpMV and the dots: MPG_ERR_UNSUPPORTED, -5."""
    A, xt, b = s5
    monkeypatch.setenv("MPG_STEP_DOTS", "2")
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed", orth="cgs", prec="bjacobi", rlen=30, tol=0.0,
                  max_restarts=1, accum="f32", spmv_format="sell")


# ---------------------------------------------------------------- fused form
_FUSE_CASES = [(mode, orth, accum) for mode in ("mixed", "single", "baseline") for orth in ("cgs", "mgs", "cgsr")
               for accum in (("f64", "f32") if mode != "baseline" else ("f64",))]
_STENCILS = {}


def _stencil(mpg, nx):
    if nx not in _STENCILS:
        A = mpg.gen_stencil27(nx)
        xt = mpg.rand_vect(A.nrows, 42)
        _STENCILS[nx] = (A, xt, mpg.host_spmv(A, xt))
    return _STENCILS[nx]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,orth,accum", _FUSE_CASES)
@pytest.mark.parametrize("nx", [5, 7])
def test_fused_form_equals_separate_launch(mpg, monkeypatch, nx, mode, orth, accum):
    """On node blocks at bs = 3 the apply can run inside the Arnoldi SpMV and
    the residual prologue (MPG_BJACOBI_FUSE=1) with the bits of the launch of
    its own (=0): x, the step residuals and the restart residuals of two
    cycles at tol = 0, and the layout says which form ran. Unset takes the
    separate launch: the fused form measured slower."""
    A, xt, b = _stencil(mpg, nx)
    opts = dict(mode=mode, orth=orth, accum=accum, prec="bjacobi", rlen=30, tol=0.0, max_restarts=2,
                spmv_format="node")
    got = {}
    for env in ("1", "0"):
        monkeypatch.setenv("MPG_BJACOBI_FUSE", env)
        eng = mpg.Engine(A, b, xt, **opts)
        lay = eng.spmv_layout()
        eng.close()
        assert lay["format"] == "node" and lay["prec_fused"] == int(env), lay
        got[env] = mpg.solve(A, b, xt, engine="fused", **opts)
        assert got[env].total_iters == 60
    f, s = got["1"], got["0"]
    assert np.array_equal(f.step_res, s.step_res)
    assert np.array_equal(f.cyc_r_norm, s.cyc_r_norm)
    assert np.array_equal(f.x, s.x)
    monkeypatch.delenv("MPG_BJACOBI_FUSE")
    eng = mpg.Engine(A, b, xt, **opts)
    assert eng.spmv_layout()["prec_fused"] == 0  # unset: the separate launch
    sep_bytes = eng.phase_bytes("spmv")
    eng.close()
    monkeypatch.setenv("MPG_BJACOBI_FUSE", "1")
    eng = mpg.Engine(A, b, xt, **opts)
    # the launch of its own reads and writes w once more: 2 sizeof(T) per row
    sT = 8 if mode == "baseline" else 4
    assert sep_bytes - eng.phase_bytes("spmv") == 2 * sT * A.nrows
    eng.close()


def _few_blocks_per_node(mpg, nn=700):
    """3-dof nodes with one or two 3 x 3 blocks per node row (its own, and for
    every other node its successor's): a node tile then holds 256 node rows,
    768 matrix rows -- three turns of the kernel's rows loop, nodes that
    straddle a turn (rows 255..257) and waves."""
    rng = np.random.default_rng(23)
    rowptr, col, val = [0], [], []
    for q in range(nn):
        nbr = [q] + ([(q + 1) % nn] if q % 2 == 0 else [])
        for i in range(3):
            for t in sorted(nbr):
                for j in range(3):
                    c = 3 * t + j
                    col.append(c)
                    val.append(8.0 + rng.random() if c == 3 * q + i else rng.standard_normal())
            rowptr.append(len(col))
    A = mpg.Csr(3 * nn, 3 * nn, np.array(rowptr, np.int32), np.array(col, np.int32), np.array(val))
    xt = mpg.rand_vect(A.nrows, 42)
    return A, xt, mpg.host_spmv(A, xt)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mixed", "baseline", "single-prec"])
def test_fused_form_on_full_tiles(mpg, monkeypatch, mode):
    """The fused form where a tile holds more rows than the workgroup has
    lanes: the bits of the separate launch, and of the CSR row blocks."""
    A, xt, b = _few_blocks_per_node(mpg)
    opts = dict(mode=mode, orth="cgs", prec="bjacobi", rlen=20, tol=0.0, max_restarts=2)
    got = {}
    for env in ("1", "0"):
        monkeypatch.setenv("MPG_BJACOBI_FUSE", env)
        eng = mpg.Engine(A, b, xt, spmv_format="node", **opts)
        lay = eng.spmv_layout()
        eng.close()
        assert lay["format"] == "node" and lay["prec_fused"] == int(env), lay
        got[env] = mpg.solve(A, b, xt, engine="fused", spmv_format="node", **opts)
    csr = mpg.solve(A, b, xt, engine="fused", spmv_format="csr", **opts)
    for r in (got["0"], csr):
        assert np.array_equal(got["1"].step_res, r.step_res)
        assert np.array_equal(got["1"].cyc_r_norm, r.cyc_r_norm)
        assert np.array_equal(got["1"].x, r.x)
    assert np.all(np.isfinite(got["1"].step_res)) and got["1"].total_iters == 40


# ---------------------------------------------------------------- storage forms
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mixed", "baseline", "single-prec"])
def test_storage_forms_same_first_cycle(mpg, s5, mode):
    """The project's rule for storage forms, with the block apply after the
    SpMV: an fp32 Arnoldi (mode mixed) has the same first cycle on CSR row
    blocks, SELL-64 and node blocks; node blocks give the CSR tiles' bits in
    every value type, so under an fp64 Arnoldi those two are compared (its
    SELL sums differ from the CSR tiles' in the last bits with any
    preconditioner, and are held to rounding level here)."""
    A, xt, b = s5
    res = {}
    for fmt in ("csr", "sell", "node"):
        eng = mpg.Engine(A, b, xt, mode=mode, orth="cgs", prec="bjacobi", rlen=30, tol=0.0, max_restarts=2,
                         spmv_format=fmt)
        lay = eng.spmv_layout()
        eng.close()
        assert lay["format"] == fmt and lay["prec_fused"] == 0, lay
        res[fmt] = mpg.solve(A, b, xt, engine="fused", mode=mode, orth="cgs", prec="bjacobi", rlen=30, tol=0.0,
                             max_restarts=2, spmv_format=fmt)
        assert res[fmt].total_iters == 60
    assert np.array_equal(res["node"].step_res[:30], res["csr"].step_res[:30])
    if mode == "mixed":
        assert np.array_equal(res["sell"].step_res[:30], res["csr"].step_res[:30])
    else:
        np.testing.assert_allclose(res["sell"].step_res[:12], res["csr"].step_res[:12], rtol=1e-9)


@pytest.mark.gpu
def test_block_size_2_converges_unfused(mpg):
    A = mpg.gen_stencil27(5, dof=2)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(mode="mixed", orth="cgs", prec="bjacobi", prec_block=2, rlen=30, tol=1e-8, max_restarts=20)
    eng = mpg.Engine(A, b, xt, **opts)
    lay = eng.spmv_layout()
    eng.close()
    assert lay["prec_fused"] == 0, lay
    for engine in ("fused", "surface"):
        got = mpg.solve(A, b, xt, engine=engine, **opts)
        assert got.status == "converged" and got.cyc_r_norm[-1] / got.cyc_normalization[-1] <= 1e-8


# ---------------------------------------------------------------- parity
@pytest.fixture(scope="module")
def np_runs(mpg, s5):
    """The NumPy loop on stencil27(5), rlen 30, tol 1e-8 (computed once)."""
    A, xt, b = s5
    runs = {}
    for mode in ("baseline", "mixed"):
        r = np_solve(A, b, mode, "cgs", 30, 1e-8)
        r["err_norm"] = float(np.linalg.norm(r["x"] - xt))
        r["res_norm"] = float(np.linalg.norm(b - gmres_np._Problem(A, np.float64).A @ r["x"]))
        r["x_head"], r["x_sum"] = r["x"][:16].copy(), float(np.sum(r["x"]))
        # at most 3 cycles: no cycle sits at the fp32 attainable-accuracy floor
        assert r["status"] == "converged" and len(r["cyc_r_norm"]) <= 3, (mode, r["restarts"])
        runs[mode] = r
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_parity_baseline(mpg, s5, np_runs, engine):
    """fp64 Arnoldi: parity.compare's baseline rule (equal counts)."""
    A, xt, b = s5
    got = mpg.solve(A, b, xt, engine=engine, mode="baseline", orth="cgs", prec="bjacobi", rlen=30, tol=1e-8,
                    max_restarts=1000)
    parity.compare(np_runs["baseline"], got, "baseline", 1e-8, 30, f"bjacobi/baseline/{engine}")


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_parity_mixed(mpg, s5, np_runs, engine):
    """fp32 Arnoldi: status, restarts within 1, compare's cycle-0 history
    rule, and every cycle's backward error at most 3x the NumPy loop's."""
    from types import SimpleNamespace

    A, xt, b = s5
    ref = np_runs["mixed"]
    got = mpg.solve(A, b, xt, engine=engine, mode="mixed", orth="cgs", prec="bjacobi", rlen=30, tol=1e-8,
                    max_restarts=1000)
    assert got.status == ref["status"]
    assert abs(got.restarts - ref["restarts"]) <= 1
    parity.compare(ref, got, "mixed", 1e-8, 30, f"bjacobi/mixed/{engine}")
    parity.not_worse_than(SimpleNamespace(**ref), got, "mixed", f"bjacobi/mixed/{engine}", factor=3)


# ---------------------------------------------------------------- it preconditions
@pytest.fixture(scope="module")
def intra(mpg, s5):
    A, xt, _ = s5
    S = intra_scaled(mpg, A, INTRA_SCALE)
    return S, xt, mpg.host_spmv(S, xt)


def test_intra_variant_numpy_counts(mpg, intra):
    """The condition of the test below, on the CPU: on stencil27(5) with the
    intra-node off-diagonals x16 (diagonal reset to 1 + sum |off|) the NumPy
    loops at mode baseline, CGS, rlen 30, tol 1e-10 take fewer iterations
    with block Jacobi than with point Jacobi: 30 against 60 on the
    generator's values (the base strategy checks at restarts only: backward
    error 6.1e-16 after bjacobi's first cycle, 3.4e-10 after jacobi's; at
    scales 1 and 4 both take 30)."""
    S, xt, b = intra
    bj = np_solve(S, b, "baseline", "cgs", 30, 1e-10)
    pj = gmres_np.solve(S, b, mode="baseline", orth="cgs", prec="jacobi", rlen=30, tol=1e-10)
    print("numpy total_iters: bjacobi", bj["total_iters"], "jacobi", pj["total_iters"])
    assert bj["status"] == pj["status"] == "converged"
    assert bj["total_iters"] < pj["total_iters"]


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_it_preconditions(mpg, intra, engine):
    """Fewer iterations than point Jacobi where the coupling inside a node
    dominates (see test_intra_variant_numpy_counts for the NumPy counts)."""
    S, xt, b = intra
    opts = dict(engine=engine, mode="baseline", orth="cgs", rlen=30, tol=1e-10, max_restarts=1000)
    bj = mpg.solve(S, b, xt, prec="bjacobi", **opts)
    pj = mpg.solve(S, b, xt, prec="jacobi", **opts)
    print("total_iters: bjacobi", bj.total_iters, "jacobi", pj.total_iters)
    assert bj.status == pj.status == "converged"
    assert bj.total_iters < pj.total_iters


# ---------------------------------------------------------------- CLI
# automated.py:33-38, as tests/test_cli_gpu.py restates it
SUMMARY = re.compile(
    r"Found solution with rel prec res norm = (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*) when k = (\d+) and i = (\d+)\n"
    r"  total iterations = (\d+)\n"
    r"  ilu took (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*)s; gmres took (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*)s\n"
    r"  resNorm = (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*); errNorm = (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*)\n")


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_cli(mpg, engine):
    out = subprocess.run([str(mpg.CLI), "--matrix", "stencil27:5", "--rlen", "30", "--mode", "mixed", "--orth", "cgs",
                          "--prec", "bjacobi", "--tol", "1e-9", "--engine", engine, "--gpu"],
                         capture_output=True, text=True, timeout=120, check=True).stdout
    m = SUMMARY.search(out)
    assert m, out
    assert float(m.group(1)) <= 1e-9 and int(m.group(4)) > 0
    assert out.startswith("||x|| = ") and "Doing Mixed Precision test" in out
    r = subprocess.run([str(mpg.CLI), "--matrix", "stencil27:5:2", "--rlen", "30", "--prec", "bjacobi",
                        "--prec-block", "2", "--orth", "cgs", "--tol", "1e-9", "--engine", engine],
                       capture_output=True, text=True, timeout=120, check=True)
    assert SUMMARY.search(r.stdout), r.stdout
