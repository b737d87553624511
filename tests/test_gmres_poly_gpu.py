"""GMRES-polynomial preconditioner (prec="gmres_poly"): the sweep kernels
against the existing SpMV launch plus the NumPy operations, bit for bit; the
engine's apply against the restated chain; the set-up; whole solves against
the NumPy restart loop of tests/test_gmres_poly_cpu.py with the engine's own
roots; that it preconditions; the storage forms; the operator surface's cycle
recording; the refusals; the CLI.

Every sweep comparison is array_equal: the row sum is the SpMV's of the same
storage, value type and accumulation class, and the epilogue is
np_poly_step / np_poly_pair of the CPU file, each operation rounded to the
vectors' type."""
import ctypes as C
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import gmres_np
from tests import parity
from tests.golden.make_golden import convdiff
from tests.test_gmres_poly_cpu import (gmres_residual, np_arnoldi, np_poly_apply, np_poly_pair, np_poly_step,
                                       np_solve_poly, start_vector)
from tests.test_neumann_gpu import (APPLY_CASES, CSR_CASES, SELL_CASES, SUMMARY, Storage, Workspace, _same, _vectors)

pytestmark = pytest.mark.gpu

C0, C1 = 0.37, 0.81  # rounded to T by the launch's argument type and by the restatement
STEP, PAIR = 0, 1
_DP = C.POINTER(C.c_double)


# ---------------------------------------------------------------- helpers
class PolyStorage(Storage):
    """Storage with the GMRES-polynomial sweep launches."""

    def poly_status(self, on_sell, d, g, p, z, out, form, first, last, c0=C0, c1=C1):
        lib = self.hip.lib
        if on_sell:
            return getattr(lib, f"mpg_sell_poly_sweep_{self.t}")(self.hip.ctx, self.sell, d, g, p, z, out, form, first,
                                                                 last, self.ct(c0), self.ct(c1))
        return getattr(lib, f"mpg_csr_poly_sweep_{self.t}")(self.hip.ctx, self.csr, self.vals.p, d, g, p, z, out, form,
                                                            first, last, self.ct(c0), self.ct(c1))

    def poly(self, on_sell, d, g, p, z, form, first, last, over_p=False):
        """(z, out) of one sweep; g None: the gathered vector is p's own
        buffer; last: no second output; over_p: out is p's buffer."""
        dd, dp, dz = self.hip.buf(d), self.hip.buf(p), self.hip.buf(z)
        dg = self.hip.buf(g) if g is not None else dp
        out = None if last else dp if over_p else self.hip.buf(np.full(self.n, 7, self.T))
        self.hip.check(self.poly_status(on_sell, dd.p, dg.p, dp.p, dz.p, out.p if out else None, form, first, last),
                       "poly sweep")
        got = dz.get(), (out.get() if out else None)
        for b in {dd, dp, dz, dg} | ({out} if out else set()):
            b.free()
        return got


class PolyWorkspace(Workspace):
    def apply_status(self, roots, w, w0, w1):
        re = np.ascontiguousarray(np.real(roots), np.float64)
        im = np.ascontiguousarray(np.imag(roots), np.float64)
        return self.hip.lib.mpg_arnoldi_poly_apply(self.arn, len(re), re.ctypes.data_as(_DP), im.ctypes.data_as(_DP), w,
                                                   w0, w1)

    def apply(self, roots, r):
        n = len(roots)
        w, w0, w1 = self.hip.buf(r), self.hip.buf(np.zeros(self.n, self.T)), self.hip.buf(np.zeros(self.n, self.T))
        self.hip.check(self.apply_status(roots, w.p, w0.p if n >= 2 else None, w1.p if n >= 3 else None), "poly_apply")
        got = w.get()
        for b in (w, w0, w1):
            b.free()
        return got


def _check_sweep(hip, A, t, on_sell, seed=3):
    S = PolyStorage(hip, A, t, sell=on_sell)
    try:
        d, p, z = _vectors(A.nrows, S.T, seed)
        g = np.random.default_rng(seed + 1).standard_normal(A.nrows).astype(S.T)
        s_p, s_g = S.spmv(p, on_sell), S.spmv(g, on_sell)
        for form, fn in ((STEP, np_poly_step), (PAIR, np_poly_pair)):
            for first in (0, 1):
                ref_z, ref_o = fn(s_p, d, p, z, C0, C1, first=bool(first))
                for last in (0, 1):
                    got_z, got_o = S.poly(on_sell, d, None, p, z, form, first, last)
                    assert got_z.dtype == ref_z.dtype and np.array_equal(got_z, ref_z), (form, first, last)
                    assert (got_o is None) if last else np.array_equal(got_o, ref_o), (form, first, last)
        # a pair's second half: a step that gathers another vector, with and without storing over p
        for first in (0, 1):
            ref_z, ref_o = np_poly_step(s_g, d, p, z, C0, C1, first=bool(first))
            for last, over_p in ((0, False), (0, True), (1, False)):
                got_z, got_o = S.poly(on_sell, d, g, p, z, STEP, first, last, over_p=over_p)
                assert np.array_equal(got_z, ref_z), (first, last, over_p)
                assert (got_o is None) if last else np.array_equal(got_o, ref_o), (first, last, over_p)
        assert not np.array_equal(np_poly_step(s_p, d, p, z, C0, C1)[0], np_poly_pair(s_p, d, p, z, C0, C1)[0])
        assert not np.array_equal(np_poly_step(s_p, d, p, z, C0, C1)[0], np_poly_step(s_p, d, p, z, C0, C1, True)[0])
        # refused before any launch: out == g, z among the other vectors, the flag against out, another form
        dd, dg, dp, dz, do = (hip.buf(v) for v in (d, g, p, z, z))
        for form in (STEP, PAIR):
            assert S.poly_status(on_sell, dd.p, dp.p, dp.p, dz.p, dp.p, form, 0, 0) == -2
            assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dz.p, dg.p, form, 0, 0) == -2
            assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dg.p, do.p, form, 0, 0) == -2
            assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dp.p, do.p, form, 0, 0) == -2
            assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dz.p, dz.p, form, 0, 0) == -2
            assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dz.p, None, form, 0, 0) == -2
            assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dz.p, do.p, form, 0, 1) == -2
        assert S.poly_status(on_sell, dd.p, dg.p, dp.p, dz.p, do.p, 2, 0, 0) == -2
        assert np.array_equal(dz.get(), z) and np.array_equal(dp.get(), p) and np.array_equal(do.get(), z)
        for b in (dd, dg, dp, dz, do):
            b.free()
        return S.layout() if on_sell else None
    finally:
        S.close()


# ---------------------------------------------------------------- 1. sweep bits
@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(CSR_CASES))
def test_csr_sweep_bits(mpg, hip, case, t):
    """mpg_csr_poly_sweep_* = mpg_csr_spmv_* (alpha 1, beta 0) on the same
    handle, then the NumPy operations: step and pair, with and without first,
    with and without last, the gathered vector p or another one, out over p."""
    A = CSR_CASES[case](mpg)
    if case == "long_row":
        assert np.diff(A.rowptr)[17] == 2100
    _check_sweep(hip, A, t, on_sell=False)


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(SELL_CASES))
def test_sell_sweep_bits(mpg, hip, case, t):
    """mpg_sell_poly_sweep_* = mpg_sell_spmv_* (alpha 1, beta 0) on the same
    copy, then the NumPy operations (the forms of test_csr_sweep_bits)."""
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
PAIR_A, PAIR_B = 1.1 + 0.6j, 0.7 + 0.9j
ROOT_LISTS = {
    "real1": [1.7], "real2": [1.7, 0.6], "real3": [1.7, 0.3, 0.9], "real5": [1.9, 0.2, 1.1, 0.6, 1.5],
    "lead2": [PAIR_A, PAIR_A.conjugate()], "lead3": [PAIR_A, PAIR_A.conjugate(), 0.4],
    "lead5": [PAIR_A, PAIR_A.conjugate(), 1.8, 0.3, 1.2],
    "middle5": [1.8, 0.3, PAIR_A, PAIR_A.conjugate(), 1.1],
    "final3": [1.8, PAIR_A, PAIR_A.conjugate()], "final5": [1.8, 0.3, 1.2, PAIR_A, PAIR_A.conjugate()],
    "pairs5": [PAIR_A, PAIR_A.conjugate(), PAIR_B, PAIR_B.conjugate(), 0.5],
    "pairs5_final": [0.5, PAIR_A, PAIR_A.conjugate(), PAIR_B, PAIR_B.conjugate()],
}
BAD_ROOT_LISTS = [[0.0], [float("nan")], [1.0 + 1.0j], [1.0 + 1.0j, 2.0], [1.0 - 1.0j, 1.0 + 1.0j], [1.7, 1.0 + 1.0j],
                  [1.0 + 1.0j, 1.5 - 1.0j], [float("inf"), 1.0]]


@pytest.mark.parametrize("t,accum", [("f32", 0), ("f32", 1), ("f64", 0)], ids=["f32-acc64", "f32-acc32", "f64"])
@pytest.mark.parametrize("case,fmt", APPLY_CASES, ids=["band-sell", "stencil-csr", "stencil-node"])
def test_engine_apply_bits(mpg, hip, case, fmt, t, accum):
    """mpg_arnoldi_poly_apply with hand-chosen roots at s = 1, 2, 3, 5 (all
    real, a leading, a middle and a final pair, two pairs) = the chain of
    np_poly_apply whose row sums are the workspace's own Arnoldi SpMV's (its
    storage and accumulation class); the argument refusals leave w untouched."""
    A = mpg.gen_band(4352, 5, 4, seed=7) if case == "band_4352" else mpg.gen_stencil27(5)
    W = PolyWorkspace(mpg, hip, A, t, fmt, accum)
    try:
        assert W.format == fmt, W.format
        T = W.T
        d = W.diag.get()
        r = np.random.default_rng(9).standard_normal(A.nrows).astype(T)
        for name, roots in ROOT_LISTS.items():
            ref = np_poly_apply(None, d, r, np.array(roots, complex), rowsum=W.spmv)
            got = W.apply(np.array(roots, complex), r)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (name, int(np.sum(got != ref)))
        # refused before any launch
        w, w0 = hip.buf(r), hip.buf(np.zeros(A.nrows, T))
        two, three = np.array([1.7, 0.6], complex), np.array([1.7, 0.6, 0.9], complex)
        assert W.apply_status(np.zeros(0, complex), w.p, w0.p, None) == -2
        assert W.apply_status(np.full(65, 1.5, complex), w.p, w0.p, w0.p) == -2
        assert W.apply_status(two, w.p, None, None) == -2
        assert W.apply_status(two, w.p, w.p, None) == -2
        assert W.apply_status(three, w.p, w0.p, None) == -2
        assert W.apply_status(three, w.p, w0.p, w0.p) == -2
        assert W.apply_status(three, w.p, w0.p, w.p) == -2
        assert W.apply_status(two, None, w0.p, None) == -2
        for bad in BAD_ROOT_LISTS:
            assert W.apply_status(np.array(bad, complex), w.p, w0.p, w0.p) == -2, bad
        assert np.array_equal(w.get(), r)
        w.free(), w0.free()
    finally:
        W.close()


# ---------------------------------------------------------------- 3. the set-up
def _layout(mpg, A, b, xt, **opts):
    eng = mpg.Engine(A, b, xt, **opts)
    lay = eng.spmv_layout()
    eng.close()
    return lay


SETUP_MATRICES = {"lap12": lambda mpg: mpg.gen_laplace3d(12), "convdiff32": lambda mpg: convdiff(mpg, 32),
                  "band4352": lambda mpg: mpg.gen_band(4352, 5, 4, seed=7)}


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(SETUP_MATRICES))
def test_setup_residual(mpg, hip, case, t):
    """The engine's roots at s = 3, 6, 12 come out the same twice, and one
    application u of them to g (the set-up's start vector) on the device gives
    ||D g - D A u|| / ||D g||, formed in fp64 NumPy from the device's output,
    within 16 eps_T absolute of the fp64 GMRES residual of (D A, D g) on the
    T-rounded operator (a CPU restatement measured <= 1.1 eps_T; the factor of
    16 allows for the device's summation orders)."""
    A0 = SETUP_MATRICES[case](mpg)
    # (the engines' Arnoldi matrix holds the values rounded to fp32 in every mode: hand them over already rounded,
    # so that the workspace below holds the matrix the engine's set-up ran on)
    A = mpg.Csr(A0.nrows, A0.ncols, A0.rowptr, A0.col, A0.val.astype(np.float32).astype(np.float64))
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    W = PolyWorkspace(mpg, hip, A, t, 1, 0)
    try:
        T = W.T
        eps = float(np.finfo(T).eps)
        d64 = W.diag.get().astype(np.float64)
        A64 = gmres_np._Problem(A, np.float64).A  # the Arnoldi matrix's values, widened
        g = start_vector(mpg, A.nrows, T)
        v0 = d64 * g.astype(np.float64)
        H12, _ = np_arnoldi(A64, d64, g.astype(np.float64), 12)
        for s in (3, 6, 12):
            opts = dict(mode="baseline" if t == "f64" else "mixed", orth="cgs", prec="gmres_poly", jacobi_steps=s,
                        rlen=10, tol=0.0, max_restarts=1)
            lay = _layout(mpg, A, b, xt, **opts)
            roots = np.array(lay["prec_roots"])
            assert lay["prec_sweeps"] == s == len(roots), lay
            assert np.array_equal(np.array(_layout(mpg, A, b, xt, **opts)["prec_roots"]), roots)
            u = W.apply(roots, g).astype(np.float64)
            got = float(np.linalg.norm(v0 - d64 * (A64 @ u)) / np.linalg.norm(v0))
            want = gmres_residual(H12[: s + 1, :s])
            print(f"{case} {t} s = {s}: residual {got:.9e}, GMRES {want:.9e}, difference {abs(got - want) / eps:.3f} eps")
            assert abs(got - want) <= 16 * eps, (case, t, s, got, want)
    finally:
        W.close()


# ---------------------------------------------------------------- solves
@pytest.fixture(scope="module")
def s5(mpg):
    A = mpg.gen_stencil27(5)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, xt, mpg.host_spmv(A, xt)


@pytest.fixture(scope="module")
def cd32(mpg):
    A = convdiff(mpg, 32)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, xt, mpg.host_spmv(A, xt)


# 4. storage forms
def test_storage_forms_same_first_cycle(mpg, s5):
    """With s = 3 the first cycle (30 steps) has the same bits on CSR row
    blocks, SELL-64 and node blocks under an fp32 Arnoldi (mode mixed); under
    an fp64 Arnoldi node blocks and CSR agree bit for bit, and SELL is held
    as tests/test_neumann_gpu.py::test_storage_forms_same_first_cycle holds
    it, with an absolute term for the steps that are already converged.
    The roots do not depend on the storage (the set-up runs on the CSR arrays)."""
    A, xt, b = s5
    for mode in ("mixed", "baseline"):
        res, roots = {}, {}
        for fmt in ("csr", "sell", "node"):
            opts = dict(mode=mode, orth="cgs", prec="gmres_poly", jacobi_steps=3, rlen=30, tol=0.0, max_restarts=2,
                        spmv_format=fmt)
            lay = _layout(mpg, A, b, xt, **opts)
            assert lay["format"] == fmt and lay["prec_sweeps"] == 3 and "prec_fused" not in lay, lay
            assert "prec_interval" not in lay and len(lay["prec_roots"]) == 3, lay
            roots[fmt] = lay["prec_roots"]
            res[fmt] = mpg.solve(A, b, xt, engine="fused", **opts)
            assert res[fmt].total_iters == 60
        assert roots["csr"] == roots["sell"] == roots["node"]
        assert np.array_equal(res["node"].step_res[:30], res["csr"].step_res[:30])
        if mode == "mixed":
            assert np.array_equal(res["sell"].step_res[:30], res["csr"].step_res[:30])
        else:
            # SELL's fp64 row sums differ from the tiles' in the last bits. The Neumann test's rtol of 1e-9 on
            # 12 steps holds while the residual is O(r_0); this polynomial brings step 12 to 6e-12 r_0, where a
            # last-bit difference of the vectors (c eps of r_0; c = 100 covers 27 entries a row in 3 sweeps and
            # the step's sums) is no longer small beside the estimate itself: it stays an absolute term.
            a, c = res["sell"].step_res[:12], res["csr"].step_res[:12]
            np.testing.assert_allclose(a, c, rtol=1e-9, atol=100 * np.finfo(np.float64).eps * c[0])
    for prec in ("jacobi", "neumann", "chebyshev"):
        lay = _layout(mpg, A, b, xt, mode="mixed", orth="cgs", prec=prec, jacobi_steps=2, rlen=30, tol=0.0,
                      max_restarts=1)
        assert "prec_roots" not in lay


# 5. parity with the NumPy loop
PARITY = {"s5": 3, "cd32": 6}  # (convdiff32 at s = 6: the roots hold a pair)


@pytest.fixture(scope="module")
def np_runs(mpg, s5, cd32):
    """The NumPy loop, rlen 30, tol 1e-8, with the roots the engine reports
    for the mode (computed once)."""
    runs = {}
    for name, (A, xt, b) in (("s5", s5), ("cd32", cd32)):
        for mode in ("baseline", "mixed"):
            lay = _layout(mpg, A, b, xt, mode=mode, orth="cgs", prec="gmres_poly", jacobi_steps=PARITY[name], rlen=30,
                          tol=1e-8, max_restarts=10)
            roots = np.array(lay["prec_roots"])
            print(name, mode, "roots", roots)
            assert len(roots) == PARITY[name]
            if name == "cd32":
                assert np.any(roots.imag != 0.0), roots
            r = np_solve_poly(mpg, A, b, mode, "cgs", 30, 1e-8, roots=roots)
            r["err_norm"] = float(np.linalg.norm(r["x"] - xt))
            r["res_norm"] = float(np.linalg.norm(b - gmres_np._Problem(A, np.float64).A @ r["x"]))
            r["x_head"], r["x_sum"] = r["x"][:16].copy(), float(np.sum(r["x"]))
            assert r["status"] == "converged", (name, mode, r["restarts"])
            runs[name, mode] = r
    return runs


@pytest.mark.parametrize("engine", ["fused", "surface"])
@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_baseline(mpg, s5, cd32, np_runs, name, engine):
    """fp64 Arnoldi: parity.compare's baseline rule (equal counts)."""
    A, xt, b = {"s5": s5, "cd32": cd32}[name]
    got = mpg.solve(A, b, xt, engine=engine, mode="baseline", orth="cgs", prec="gmres_poly", jacobi_steps=PARITY[name],
                    rlen=30, tol=1e-8, max_restarts=1000)
    parity.compare(np_runs[name, "baseline"], got, "baseline", 1e-8, 30, f"gmres_poly/{name}/baseline/{engine}")


@pytest.mark.parametrize("engine", ["fused", "surface"])
@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_mixed(mpg, s5, cd32, np_runs, name, engine):
    """fp32 Arnoldi: status, restarts within 1, compare's mixed rule, and every
    cycle's backward error at most 3x the NumPy loop's."""
    A, xt, b = {"s5": s5, "cd32": cd32}[name]
    ref = np_runs[name, "mixed"]
    got = mpg.solve(A, b, xt, engine=engine, mode="mixed", orth="cgs", prec="gmres_poly", jacobi_steps=PARITY[name],
                    rlen=30, tol=1e-8, max_restarts=1000)
    assert got.status == ref["status"]
    assert abs(got.restarts - ref["restarts"]) <= 1
    parity.compare(ref, got, "mixed", 1e-8, 30, f"gmres_poly/{name}/mixed/{engine}")
    parity.not_worse_than(SimpleNamespace(**ref), got, "mixed", f"gmres_poly/{name}/mixed/{engine}", factor=3)


# 6. it preconditions
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_it_preconditions(mpg, engine):
    """Baseline, CGS, GMRES(10), tol 1e-10, the conditions the NumPy loop
    meets (tests/test_gmres_poly_cpu.py::test_numpy_counts_*): all converge; on
    gen_laplace3d(16) gmres_poly s = 6 takes no more iterations than neumann
    s = 6 and twice s = 3 no more than jacobi; on convdiff(32) fewer than
    neumann at s = 6 and s = 8; on gen_band(4352, 5, 4, seed=7) s = 4 no more
    than jacobi."""
    opts = dict(engine=engine, mode="baseline", orth="cgs", rlen=10, tol=1e-10, max_restarts=1000)

    def run(A, **kw):
        xt = mpg.rand_vect(A.nrows, 42)
        r = mpg.solve(A, mpg.host_spmv(A, xt), xt, **kw, **opts)
        assert r.status == "converged", kw
        return r.total_iters

    A = mpg.gen_laplace3d(16)
    it = {"jacobi": run(A, prec="jacobi"), "neumann6": run(A, prec="neumann", jacobi_steps=6),
          "poly3": run(A, prec="gmres_poly", jacobi_steps=3), "poly4": run(A, prec="gmres_poly", jacobi_steps=4),
          "poly6": run(A, prec="gmres_poly", jacobi_steps=6)}
    print("lap16 total_iters:", it)
    assert it["poly6"] <= it["neumann6"]
    assert 2 * it["poly3"] <= it["jacobi"]
    A = convdiff(mpg, 32)
    it = {f"{p}{s}": run(A, prec={"neumann": "neumann", "poly": "gmres_poly"}[p], jacobi_steps=s)
          for p in ("neumann", "poly") for s in (6, 8)}
    print("convdiff32 total_iters:", it)
    assert it["poly6"] < it["neumann6"]
    assert it["poly8"] < it["neumann8"]
    A = mpg.gen_band(4352, 5, 4, seed=7)
    it = {"jacobi": run(A, prec="jacobi"), "poly4": run(A, prec="gmres_poly", jacobi_steps=4)}
    print("band4352 total_iters:", it)
    assert it["poly4"] <= it["jacobi"]


# 7. the operator surface still records the cycle
@pytest.mark.parametrize("mode", ["mixed", "baseline", "single"])
def test_surface_still_records_the_cycle(mpg, mode, monkeypatch):
    """Nothing in GmresPoly<Type, Hip>::apply reads on the host (the set-up
    ran in the constructor and the coefficients are launch arguments), so the
    operator-surface driver records the cycle's calls as with Jacobi (first
    cycle eager, second recorded, later replayed), and the replays have the
    bits of issuing every call on its own."""
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(engine="surface", mode=mode, orth="cgs", prec="gmres_poly", jacobi_steps=3, rlen=10, tol=1e-10,
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


# 8. refusals
def test_refusals(mpg, s5, monkeypatch):
    """Each refusal is a RuntimeError that names its reason and the
    preconditioner, and the next solve runs normally."""
    A, xt, b = s5
    opts = dict(orth="cgs", prec="gmres_poly", rlen=30, tol=1e-8, max_restarts=20)
    for engine in ("fused", "surface"):
        with pytest.raises(RuntimeError, match=r"prec gmres_poly: jacobi_steps = 0 is outside \[1, 64\]"):
            mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=0, **opts)
        with pytest.raises(RuntimeError, match=r"prec gmres_poly: jacobi_steps = 65 is outside \[1, 64\]"):
            mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=65, **opts)
        with pytest.raises(RuntimeError, match="prec gmres_poly is not available in mode single-prec"):
            mpg.solve(A, b, xt, engine=engine, mode="single-prec", jacobi_steps=2, **opts)
    with pytest.raises(RuntimeError, match="prec gmres_poly is not available in mode mixed-half"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed-half", jacobi_steps=2, **opts)
    with pytest.raises(RuntimeError, match="prec gmres_poly.*row-partitioned.*halo exchange"):
        mpg.solve_loopback(A, b, xt, nranks=2, mode="mixed", jacobi_steps=2, **opts)
    monkeypatch.setenv("MPG_STEP_DOTS", "2")
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed", jacobi_steps=2, accum="f32", spmv_format="sell", **opts)
    monkeypatch.delenv("MPG_STEP_DOTS")
    for engine in ("fused", "surface"):
        for s in (1, 2):  # (one root is Jacobi scaled by 1 / theta: a launch of its own, not prec jacobi's path)
            got = mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=s, **opts)
            assert got.status == "converged"


# 9. CLI
def test_cli(mpg):
    """--prec gmres_poly --jacobi-steps 4 keeps the reference's stdout
    contract and reports the iterations of mpg.solve with the same options."""
    cmd = [str(mpg.CLI), "--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec",
           "gmres_poly", "--jacobi-steps", "4", "--tol", "1e-9", "--gpu"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, check=True).stdout
    m = SUMMARY.search(out)
    assert m, out
    assert float(m.group(1)) <= 1e-9
    assert out.startswith("||x|| = ") and "Doing Mixed Precision test" in out
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    got = mpg.solve(A, mpg.host_spmv(A, xt), xt, engine="fused", mode="mixed", orth="cgs", prec="gmres_poly",
                    jacobi_steps=4, rlen=30, tol=1e-9, max_restarts=1_000_000)
    assert int(m.group(4)) == got.total_iters > 0
