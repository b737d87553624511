"""Jacobi-sweep polynomial preconditioner (prec="neumann"): the sweep kernels
against the existing SpMV launch plus three NumPy operations, bit for bit;
the engine's apply; s = 1 against prec="jacobi"; the storage forms; whole
solves against the NumPy restart loop of tests/test_neumann_cpu.py; that it
preconditions; mode single; the operator surface's cycle recording; the
refusals; the CLI.

Every kernel comparison is array_equal: the sweep's row sum is the SpMV's of
the same storage, value type and accumulation class, and its epilogue is
t = r - s, u = d * t, z + u, each rounded to the vectors' type."""
import ctypes as C
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import parity
from tests.arnoldi_phase import PhaseWorkspace
from tests.test_neumann_cpu import np_solve, np_sweep
from tests.test_step_dots_waves_gpu import _edge_matrix

pytestmark = pytest.mark.gpu

TYPES = {"f64": (np.float64, C.c_double, 0), "f32": (np.float32, C.c_float, 1)}  # dtype, ctype, mpg_dtype_t


# ---------------------------------------------------------------- helpers
def _device_csr(hip, A):
    rp, col = hip.buf(A.rowptr, np.int32), hip.buf(A.col, np.int32)
    h = C.c_void_p()
    hip.call("mpg_csr_create", A.nrows, A.ncols, A.nnz, A.rowptr.ctypes.data, rp.p, col.p, C.byref(h))
    return h, [rp, col]


def _vectors(n, T, seed):
    """d like an inverse diagonal, r and z_in of both signs."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.04, 0.25, n).astype(T), rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T))


class Storage:
    """A's values of one type on the device as CSR row blocks and, on
    request, a SELL-64 copy (mpg_sell_create format 2: always)."""

    def __init__(self, hip, A, t, sell=False):
        self.hip, self.t, self.n = hip, t, A.nrows
        self.T, self.ct, self.vt = TYPES[t]
        self.csr, self.keep = _device_csr(hip, A)
        self.vals = hip.buf(A.val.astype(self.T))
        self.sell = C.c_void_p()
        if sell:
            hip.call("mpg_sell_create", self.csr, self.vt, self.vals.p, 2, C.byref(self.sell))
            assert self.sell.value

    def layout(self):
        form, exc, imp = C.c_int32(), C.c_int64(), C.c_int64()
        self.hip.check(self.hip.lib.mpg_sell_columns(self.sell, C.byref(form), C.byref(exc), C.byref(imp)))
        w, cb, stored, win = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        self.hip.check(self.hip.lib.mpg_sell_layout(self.sell, C.byref(w), C.byref(cb), C.byref(stored), C.byref(win)))
        return dict(form=form.value, csr_slices=exc.value, implicit=imp.value, W=w.value, window=win.value)

    def spmv(self, x, on_sell):
        """T(A x) by the existing launch (alpha 1, beta 0)."""
        dx, dy = self.hip.buf(x), self.hip.buf(self.n, self.T)
        if on_sell:
            self.hip.call(f"mpg_sell_spmv_{self.t}", self.sell, self.ct(1), dx.p, self.ct(0), dy.p)
        else:
            self.hip.call(f"mpg_csr_spmv_{self.t}", self.csr, self.ct(1), self.vals.p, dx.p, self.ct(0), dy.p)
        y = dy.get()
        dx.free(), dy.free()
        return y

    def sweep_status(self, on_sell, d, r, zi, zo):
        lib = self.hip.lib
        if on_sell:
            return getattr(lib, f"mpg_sell_jacobi_sweep_{self.t}")(self.hip.ctx, self.sell, d, r, zi, zo)
        return getattr(lib, f"mpg_csr_jacobi_sweep_{self.t}")(self.hip.ctx, self.csr, self.vals.p, d, r, zi, zo)

    def sweep(self, on_sell, d, r, z, alias=False):
        """z_out of one sweep; alias: stored into r's buffer."""
        dd, dr, dz = self.hip.buf(d), self.hip.buf(r), self.hip.buf(z)
        out = dr if alias else self.hip.buf(np.full(self.n, 7, self.T))
        self.hip.check(self.sweep_status(on_sell, dd.p, dr.p, dz.p, out.p), "jacobi sweep")
        got = out.get()
        for b in {dd, dr, dz, out}:
            b.free()
        return got

    def close(self):
        if self.sell.value:
            self.hip.lib.mpg_sell_destroy(self.sell)
        self.hip.lib.mpg_csr_destroy(self.csr)
        for b in self.keep + [self.vals]:
            b.free()


def _check_sweep(hip, A, t, on_sell, seed=3):
    S = Storage(hip, A, t, sell=on_sell)
    try:
        d, r, z = _vectors(A.nrows, S.T, seed)
        ref = np_sweep(S.spmv(z, on_sell), d, r, z)
        got = S.sweep(on_sell, d, r, z)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), int(np.sum(got != ref))
        # z_out may be r itself: the same bits
        assert np.array_equal(S.sweep(on_sell, d, r, z, alias=True), ref)
        # z_out == z_in is refused
        dd, dr, dz = hip.buf(d), hip.buf(r), hip.buf(z)
        assert S.sweep_status(on_sell, dd.p, dr.p, dz.p, dz.p) == -2
        for b in (dd, dr, dz):
            b.free()
        return S.layout() if on_sell else None
    finally:
        S.close()


def _long_row_matrix(mpg, n=4100, row=17, width=2100):
    """Tridiagonal rows, and one row of `width` entries (above kNnzCap = 2040:
    the CSR tile's long-row mode), with a dominant diagonal."""
    rng = np.random.default_rng(5)
    rowptr, col, val = [0], [], []
    for i in range(n):
        cs = list(range(width)) if i == row else [c for c in (i - 1, i, i + 1) if 0 <= c < n]
        for c in cs:
            col.append(c)
            val.append(float(len(cs)) + rng.random() if c == i else rng.uniform(-1.0, 1.0))
        rowptr.append(len(col))
    return mpg.Csr(n, n, np.array(rowptr, np.int32), np.array(col, np.int32), np.array(val))


# ---------------------------------------------------------------- 1. sweep bits
CSR_CASES = {
    "band_1": lambda m: m.gen_band(1, 5, 4, seed=7),          # one row
    "band_63": lambda m: m.gen_band(63, 5, 4, seed=7),        # a partial wave
    "band_257": lambda m: m.gen_band(257, 5, 4, seed=7),      # a partial workgroup
    "band_13316": lambda m: m.gen_band(13316, 5, 4, seed=7),  # several row blocks
    "stencil27_2": lambda m: m.gen_stencil27(2),              # 24 rows, every row at a boundary
    "long_row": _long_row_matrix,                             # row 17 in long-row mode
}


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(CSR_CASES))
def test_csr_sweep_bits(mpg, hip, case, t):
    """mpg_csr_jacobi_sweep_* = mpg_csr_spmv_* (alpha 1, beta 0) on the same
    handle, then the three NumPy operations."""
    A = CSR_CASES[case](mpg)
    if case == "long_row":
        assert np.diff(A.rowptr)[17] == 2100
    _check_sweep(hip, A, t, on_sell=False)


SELL_CASES = {
    "band_64": lambda m: m.gen_band(64, 5, 4, seed=7),      # one slice
    "band_65": lambda m: m.gen_band(65, 5, 4, seed=7),      # a slice of one row
    "band_129": lambda m: m.gen_band(129, 5, 4, seed=7),    # a partial wave of slices
    "band_4352": lambda m: m.gen_band(4352, 5, 4, seed=7),  # 17 workgroups; implicit columns
    "edges_4352": lambda m: _edge_matrix(m, 4352),          # the window form, entries at its edges
    "stencil27p_4": lambda m: m.gen_stencil27p(4),          # stored columns
}


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(SELL_CASES))
def test_sell_sweep_bits(mpg, hip, case, t):
    """mpg_sell_jacobi_sweep_* = mpg_sell_spmv_* (alpha 1, beta 0) on the same
    copy, then the three NumPy operations."""
    A = SELL_CASES[case](mpg)
    lay = _check_sweep(hip, A, t, on_sell=True)
    print(case, t, lay)
    if case == "band_4352":
        assert lay["implicit"] > 0, lay
    if case == "edges_4352":
        assert lay["window"] == 1, lay
    if case == "stencil27p_4":
        assert lay["implicit"] == 0, lay


# ---------------------------------------------------------------- 2. engine apply
MPG_F64, MPG_F32 = 0, 1


class Workspace(PhaseWorkspace):
    """mpg_arnoldi_create on A with no preconditioner inside the launches and
    Jacobi's inverse diagonal in the descriptor (what prec="neumann" sets up):
    tests/arnoldi_phase.py's workspace at its defaults, on this file's Storage.
    (Inherited with it: a HIP runtime error in a copy or launch made through
    the helper's own methods ends the pytest session, PhaseWorkspace._check.)"""

    def __init__(self, mpg, hip, A, t, fmt, accum):
        super().__init__(mpg, hip, A, t, fmt, accum, storage=Storage(hip, A, t, sell=fmt == 2))

    def spmv(self, x):
        """T(A x) in the workspace's accumulation class: its own Arnoldi SpMV."""
        hip, lib = self.hip, self.hip.lib
        x = np.ascontiguousarray(x, self.T)
        hip.check(lib.mpg_memcpy_h2d(hip.ctx, lib.mpg_arnoldi_wprev_dev(self.arn, 0), x.ctypes.data, x.nbytes))
        hip.check(lib.mpg_arnoldi_spmv(self.arn, 0), "mpg_arnoldi_spmv")
        y = np.empty(self.n, self.T)
        hip.check(lib.mpg_memcpy_d2h(hip.ctx, y.ctypes.data, lib.mpg_arnoldi_wprev_dev(self.arn, 1), y.nbytes))
        return y

    def apply(self, steps, r):
        w, w0, w1 = self.hip.buf(r), self.hip.buf(np.zeros(self.n, self.T)), self.hip.buf(np.zeros(self.n, self.T))
        self.hip.check(self.hip.lib.mpg_arnoldi_neumann_apply(self.arn, steps, w.p, w0.p if steps >= 2 else None,
                                                              w1.p if steps >= 3 else None), "neumann_apply")
        got = w.get()
        for b in (w, w0, w1):
            b.free()
        return got

    def close(self):
        super().close()
        self.S.close()


APPLY_CASES = [("band_4352", 2), ("stencil27_5", 1), ("stencil27_5", 3)]  # (matrix, mpg_arnoldi_desc.spmv_format)


@pytest.mark.parametrize("t,accum", [("f32", 0), ("f32", 1), ("f64", 0)], ids=["f32-acc64", "f32-acc32", "f64"])
@pytest.mark.parametrize("case,fmt", APPLY_CASES, ids=["band-sell", "stencil-csr", "stencil-node"])
def test_engine_apply_bits(mpg, hip, case, fmt, t, accum):
    """mpg_arnoldi_neumann_apply at s = 1, 2, 3, 5 = gdmv, then s - 1 sweeps
    whose row sums are the workspace's own Arnoldi SpMV's (its storage and
    accumulation class); in the fp64 class that is also the stand-alone sweep
    launches of test 1 on the same storage."""
    A = mpg.gen_band(4352, 5, 4, seed=7) if case == "band_4352" else mpg.gen_stencil27(5)
    W = Workspace(mpg, hip, A, t, fmt, accum)
    try:
        assert W.format == fmt, W.format
        d = W.diag.get()
        r = np.random.default_rng(9).standard_normal(A.nrows).astype(W.T)
        zs = [(d * r).astype(W.T)]  # gdmv(1, d, r, 0, .)
        for _ in range(4):
            zs.append(np_sweep(W.spmv(zs[-1]), d, r, zs[-1]))
        for s in (1, 2, 3, 5):
            got = W.apply(s, r)
            assert got.dtype == zs[s - 1].dtype and np.array_equal(got, zs[s - 1]), (s, int(np.sum(got != zs[s - 1])))
        if accum == 0:
            z = zs[0]
            for j in range(1, 5):
                z = W.S.sweep(fmt == 2, d, r, z)
                assert np.array_equal(z, zs[j]), j
        # refused before any launch
        w = hip.buf(r)
        lib = hip.lib
        assert lib.mpg_arnoldi_neumann_apply(W.arn, 0, w.p, w.p, w.p) == -2
        assert lib.mpg_arnoldi_neumann_apply(W.arn, 65, w.p, None, None) == -2
        assert lib.mpg_arnoldi_neumann_apply(W.arn, 2, w.p, None, None) == -2
        assert lib.mpg_arnoldi_neumann_apply(W.arn, 2, w.p, w.p, None) == -2
        w.free()
    finally:
        W.close()


# ---------------------------------------------------------------- solves
@pytest.fixture(scope="module")
def s5(mpg):
    A = mpg.gen_stencil27(5)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, xt, mpg.host_spmv(A, xt)


def _same(a, b, label):
    assert np.array_equal(a.step_res, b.step_res), label
    assert np.array_equal(a.cyc_r_norm, b.cyc_r_norm), label
    assert np.array_equal(a.x, b.x), label


# 3. s = 1 is point Jacobi
ONE_SWEEP = [("fused", "mixed", "f64"), ("fused", "mixed", "f32"), ("fused", "baseline", "f64"),
             ("surface", "mixed", "f64"), ("surface", "baseline", "f64")]


@pytest.mark.parametrize("orth", ["cgs", "mgs"])
@pytest.mark.parametrize("engine,mode,accum", ONE_SWEEP)
def test_one_sweep_is_point_jacobi(mpg, s5, engine, mode, accum, orth):
    """prec="neumann", jacobi_steps=1 has the bits of prec="jacobi": two
    cycles at tol 0. (The fused engine runs one sweep as point Jacobi, inside
    its launches: a launch of its own would re-sum the prologue's ||w||^2 in
    another order, which an fp64 Arnoldi sees in the last bits.)"""
    A, xt, b = s5
    opts = dict(engine=engine, mode=mode, orth=orth, accum=accum, rlen=30, tol=0.0, max_restarts=2)
    nm = mpg.solve(A, b, xt, prec="neumann", jacobi_steps=1, **opts)
    pj = mpg.solve(A, b, xt, prec="jacobi", **opts)
    assert nm.total_iters == pj.total_iters == 60
    _same(nm, pj, (engine, mode, accum, orth))
    if engine == "fused":
        eng = mpg.Engine(A, b, xt, prec="neumann", jacobi_steps=1, **{k: v for k, v in opts.items() if k != "engine"})
        assert eng.spmv_layout()["prec_sweeps"] == 1
        eng.close()


# 4. storage forms
def test_storage_forms_same_first_cycle(mpg, s5):
    """With s = 3 the first cycle (30 steps) has the same bits on CSR row
    blocks, SELL-64 and node blocks under an fp32 Arnoldi (mode mixed); under
    an fp64 Arnoldi node blocks and CSR agree bit for bit, and SELL is held
    as tests/test_bjacobi_gpu.py::test_storage_forms_same_first_cycle holds
    it (its fp64 sums differ from the tiles' in the last bits)."""
    A, xt, b = s5
    for mode in ("mixed", "baseline"):
        res = {}
        for fmt in ("csr", "sell", "node"):
            opts = dict(mode=mode, orth="cgs", prec="neumann", jacobi_steps=3, rlen=30, tol=0.0, max_restarts=2,
                        spmv_format=fmt)
            eng = mpg.Engine(A, b, xt, **opts)
            lay = eng.spmv_layout()
            eng.close()
            assert lay["format"] == fmt and lay["prec_sweeps"] == 3 and "prec_fused" not in lay, lay
            res[fmt] = mpg.solve(A, b, xt, engine="fused", **opts)
            assert res[fmt].total_iters == 60
        assert np.array_equal(res["node"].step_res[:30], res["csr"].step_res[:30])
        if mode == "mixed":
            assert np.array_equal(res["sell"].step_res[:30], res["csr"].step_res[:30])
        else:
            np.testing.assert_allclose(res["sell"].step_res[:12], res["csr"].step_res[:12], rtol=1e-9)
    eng = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=0.0, max_restarts=1)
    assert "prec_sweeps" not in eng.spmv_layout()
    eng.close()


# 5. parity with the NumPy loop
PARITY_STEPS = 2


@pytest.fixture(scope="module")
def np_runs(mpg, s5):
    """The NumPy loop on stencil27(5), rlen 30, tol 1e-8, s = 2 (computed once)."""
    from oracle import gmres_np

    A, xt, b = s5
    runs = {}
    for mode in ("baseline", "mixed"):
        r = np_solve(A, b, mode, "cgs", 30, 1e-8, PARITY_STEPS)
        r["err_norm"] = float(np.linalg.norm(r["x"] - xt))
        r["res_norm"] = float(np.linalg.norm(b - gmres_np._Problem(A, np.float64).A @ r["x"]))
        r["x_head"], r["x_sum"] = r["x"][:16].copy(), float(np.sum(r["x"]))
        # at most 3 cycles: no cycle sits at the fp32 attainable-accuracy floor
        assert r["status"] == "converged" and len(r["cyc_r_norm"]) <= 3, (mode, r["restarts"])
        runs[mode] = r
    return runs


@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_parity_baseline(mpg, s5, np_runs, engine):
    """fp64 Arnoldi: parity.compare's baseline rule (equal counts)."""
    A, xt, b = s5
    got = mpg.solve(A, b, xt, engine=engine, mode="baseline", orth="cgs", prec="neumann", jacobi_steps=PARITY_STEPS,
                    rlen=30, tol=1e-8, max_restarts=1000)
    parity.compare(np_runs["baseline"], got, "baseline", 1e-8, 30, f"neumann/baseline/{engine}")


@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_parity_mixed(mpg, s5, np_runs, engine):
    """fp32 Arnoldi: status, restarts within 1, compare's cycle-0 history
    rule, and every cycle's backward error at most 3x the NumPy loop's."""
    A, xt, b = s5
    ref = np_runs["mixed"]
    got = mpg.solve(A, b, xt, engine=engine, mode="mixed", orth="cgs", prec="neumann", jacobi_steps=PARITY_STEPS,
                    rlen=30, tol=1e-8, max_restarts=1000)
    assert got.status == ref["status"]
    assert abs(got.restarts - ref["restarts"]) <= 1
    parity.compare(ref, got, "mixed", 1e-8, 30, f"neumann/mixed/{engine}")
    parity.not_worse_than(SimpleNamespace(**ref), got, "mixed", f"neumann/mixed/{engine}", factor=3)


# 6. it preconditions
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_it_preconditions(mpg, engine):
    """gen_laplace3d(12), baseline, CGS, GMRES(10), tol 1e-10: s = 4 takes
    fewer iterations than s = 2, which takes fewer than prec="jacobi"; all
    converge (the NumPy loop's counts: tests/test_neumann_cpu.py::test_numpy_counts)."""
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(engine=engine, mode="baseline", orth="cgs", rlen=10, tol=1e-10, max_restarts=1000)
    pj = mpg.solve(A, b, xt, prec="jacobi", **opts)
    n2 = mpg.solve(A, b, xt, prec="neumann", jacobi_steps=2, **opts)
    n4 = mpg.solve(A, b, xt, prec="neumann", jacobi_steps=4, **opts)
    print("total_iters: jacobi", pj.total_iters, "s=2", n2.total_iters, "s=4", n4.total_iters)
    assert pj.status == n2.status == n4.status == "converged"
    assert n4.total_iters < n2.total_iters < pj.total_iters


@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_mode_single(mpg, engine):
    """Mode single (T = X = P = float) takes it too: it converges to what an
    fp32 residual can show, in no more iterations than prec="jacobi"."""
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(engine=engine, mode="single", orth="cgs", rlen=10, tol=1e-5, max_restarts=200)
    pj = mpg.solve(A, b, xt, prec="jacobi", **opts)
    n2 = mpg.solve(A, b, xt, prec="neumann", jacobi_steps=2, **opts)
    print("single total_iters: jacobi", pj.total_iters, "s=2", n2.total_iters)
    assert pj.status == n2.status == "converged"
    assert n2.total_iters <= pj.total_iters


@pytest.mark.parametrize("mode", ["mixed", "baseline", "single"])
def test_surface_still_records_the_cycle(mpg, mode, monkeypatch):
    """Nothing in Neumann<Type, Hip>::apply reads on the host, so the
    operator-surface driver records the cycle's calls as with Jacobi
    (CycleProgram<Hip>: first cycle eager, second recorded, later replayed),
    and the replays have the bits of issuing every call on its own."""
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(engine="surface", mode=mode, orth="cgs", prec="neumann", jacobi_steps=3, rlen=10, tol=1e-10,
                max_restarts=5)
    got = {}
    for g in ("1", "0"):
        monkeypatch.setenv("MPG_SURFACE_GRAPH", g)
        monkeypatch.setenv("MPG_SURFACE_BATCH", g)
        monkeypatch.setenv("MPG_SURFACE_FUSE", g)
        before = mpg.cycle_program_counts()
        got[g] = mpg.solve(A, b, xt, **opts)
        after = mpg.cycle_program_counts()
        delta = {k: after[k] - before[k] for k in after}
        cycles = got[g].total_iters // 10
        assert cycles >= 3, cycles
        if g == "0":
            assert delta == {"recorded": 0, "replayed": 0, "voided": 0}, delta
        else:
            assert delta == {"recorded": 1, "replayed": cycles - 2, "voided": 0}, delta
    _same(got["1"], got["0"], mode)


# 7. refusals
def test_refusals(mpg, s5, monkeypatch):
    """Each refusal is a RuntimeError that names its reason, and the next
    solve runs normally."""
    A, xt, b = s5
    opts = dict(orth="cgs", prec="neumann", rlen=30, tol=1e-8, max_restarts=20)
    for engine in ("fused", "surface"):
        with pytest.raises(RuntimeError, match=r"jacobi_steps = 0 is outside \[1, 64\]"):
            mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=0, **opts)
        with pytest.raises(RuntimeError, match=r"jacobi_steps = 65 is outside \[1, 64\]"):
            mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=65, **opts)
        with pytest.raises(RuntimeError, match="not available in mode single-prec"):
            mpg.solve(A, b, xt, engine=engine, mode="single-prec", jacobi_steps=2, **opts)
    with pytest.raises(RuntimeError, match="not available in mode mixed-half"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed-half", jacobi_steps=2, **opts)
    with pytest.raises(RuntimeError, match="row-partitioned.*halo exchange"):
        mpg.solve_loopback(A, b, xt, nranks=2, mode="mixed", jacobi_steps=2, **opts)
    monkeypatch.setenv("MPG_STEP_DOTS", "2")
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed", jacobi_steps=2, accum="f32", spmv_format="sell", **opts)
    monkeypatch.delenv("MPG_STEP_DOTS")
    for engine in ("fused", "surface"):
        got = mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=2, **opts)
        assert got.status == "converged"


# 8. CLI
# automated.py:33-38, as tests/test_cli_gpu.py restates it
SUMMARY = re.compile(
    r"Found solution with rel prec res norm = (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*) when k = (\d+) and i = (\d+)\n"
    r"  total iterations = (\d+)\n"
    r"  ilu took (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*)s; gmres took (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*)s\n"
    r"  resNorm = (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*); errNorm = (\d\.?\d*e(?:\+|-)\d+|\d+\.?\d*)\n")


def test_cli(mpg):
    """--prec neumann --jacobi-steps 2 keeps the reference's stdout contract
    and reports the iterations of mpg.solve with the same options."""
    out = subprocess.run([str(mpg.CLI), "--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs",
                          "--prec", "neumann", "--jacobi-steps", "2", "--tol", "1e-9", "--gpu"],
                         capture_output=True, text=True, timeout=120, check=True).stdout
    m = SUMMARY.search(out)
    assert m, out
    assert float(m.group(1)) <= 1e-9
    assert out.startswith("||x|| = ") and "Doing Mixed Precision test" in out
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    got = mpg.solve(A, mpg.host_spmv(A, xt), xt, engine="fused", mode="mixed", orth="cgs", prec="neumann",
                    jacobi_steps=2, rlen=30, tol=1e-9, max_restarts=1_000_000)
    assert int(m.group(4)) == got.total_iters > 0
