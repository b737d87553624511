"""Chebyshev polynomial preconditioner (prec="chebyshev"): the sweep kernels
against the existing SpMV launch plus seven NumPy operations, bit for bit; the
Gershgorin bound; the engine's apply; the storage forms; whole solves against
the NumPy restart loop of tests/test_chebyshev_cpu.py; that it preconditions
better than the Neumann series; the two settings; the operator surface's
cycle recording; the refusals; the CLI.

Every sweep comparison is array_equal: the row sum is the SpMV's of the same
storage, value type and accumulation class, and the epilogue is t = r - s,
u = d * t, v = beta * u, p = z - z_prev, q = alpha * p, y = z + q, y + v, each
rounded to the vectors' type."""
import ctypes as C
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import parity
from tests.test_chebyshev_cpu import (COUNTS_INTERVAL, lib_cheb_coeffs, np_cheb_sweep, np_jacobi_bound, np_solve_cheb,
                                      theta_delta)
from tests.test_neumann_gpu import (APPLY_CASES, CSR_CASES, SELL_CASES, SUMMARY, Storage, Workspace, _long_row_matrix,
                                    _same, _vectors)

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.37, 0.81  # rounded to T by the launch's argument type and by np_cheb_sweep


# ---------------------------------------------------------------- helpers
class ChebStorage(Storage):
    """Storage with the Chebyshev sweep and the bound launches."""

    def cheb_status(self, on_sell, d, r, zi, zp, zo, alpha=ALPHA, beta=BETA):
        lib = self.hip.lib
        if on_sell:
            return getattr(lib, f"mpg_sell_cheb_sweep_{self.t}")(self.hip.ctx, self.sell, d, r, zi, zp, zo, alpha, beta)
        return getattr(lib, f"mpg_csr_cheb_sweep_{self.t}")(self.hip.ctx, self.csr, self.vals.p, d, r, zi, zp, zo, alpha,
                                                            beta)

    def cheb(self, on_sell, d, r, z, zp, alias=None):
        """z_out of one sweep; zp None: the first-sweep form; alias "r" /
        "prev": stored into that operand's buffer."""
        dd, dr, dz = self.hip.buf(d), self.hip.buf(r), self.hip.buf(z)
        dp = self.hip.buf(zp) if zp is not None else None
        out = {None: None, "r": dr, "prev": dp}[alias] or self.hip.buf(np.full(self.n, 7, self.T))
        self.hip.check(self.cheb_status(on_sell, dd.p, dr.p, dz.p, dp.p if dp else None, out.p), "cheb sweep")
        got = out.get()
        for b in {dd, dr, dz, out} | ({dp} if dp else set()):
            b.free()
        return got

    def jacobi_diag(self):
        diag = self.hip.buf(self.n, self.T)
        self.hip.call(f"mpg_jacobi_setup_{self.t}", self.csr, self.vals.p, diag.p)
        return diag

    def bound(self, diag):
        b = C.c_double(-1.0)
        self.hip.call(f"mpg_csr_jacobi_bound_{self.t}", self.csr, self.vals.p, diag.p, C.byref(b))
        return b.value


class ChebWorkspace(Workspace):
    def apply(self, steps, r, theta, delta):
        w, w0, w1 = self.hip.buf(r), self.hip.buf(np.zeros(self.n, self.T)), self.hip.buf(np.zeros(self.n, self.T))
        self.hip.check(self.hip.lib.mpg_arnoldi_cheb_apply(self.arn, steps, theta, delta, w.p,
                                                           w0.p if steps >= 2 else None,
                                                           w1.p if steps >= 3 else None), "cheb_apply")
        got = w.get()
        for b in (w, w0, w1):
            b.free()
        return got


def _check_sweep(hip, A, t, on_sell, seed=3):
    S = ChebStorage(hip, A, t, sell=on_sell)
    try:
        d, r, z = _vectors(A.nrows, S.T, seed)
        zp = np.random.default_rng(seed + 1).standard_normal(A.nrows).astype(S.T)
        s_in = S.spmv(z, on_sell)
        for prev in (zp, None):
            ref = np_cheb_sweep(s_in, d, r, z, prev, ALPHA, BETA)
            got = S.cheb(on_sell, d, r, z, prev)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (prev is None, int(np.sum(got != ref)))
            # z_out may be r itself, or z_prev: the same bits
            assert np.array_equal(S.cheb(on_sell, d, r, z, prev, alias="r"), ref)
            if prev is not None:
                assert np.array_equal(S.cheb(on_sell, d, r, z, prev, alias="prev"), ref)
        assert not np.array_equal(np_cheb_sweep(s_in, d, r, z, zp, ALPHA, BETA),
                                  np_cheb_sweep(s_in, d, r, z, None, ALPHA, BETA))
        # z_out == z_in is refused
        dd, dr, dz = hip.buf(d), hip.buf(r), hip.buf(z)
        assert S.cheb_status(on_sell, dd.p, dr.p, dz.p, dr.p, dz.p) == -2
        assert S.cheb_status(on_sell, dd.p, dr.p, dz.p, None, dz.p) == -2
        for b in (dd, dr, dz):
            b.free()
        return S.layout() if on_sell else None
    finally:
        S.close()


# ---------------------------------------------------------------- 1. sweep bits
@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(CSR_CASES))
def test_csr_sweep_bits(mpg, hip, case, t):
    """mpg_csr_cheb_sweep_* = mpg_csr_spmv_* (alpha 1, beta 0) on the same
    handle, then the seven NumPy operations; with and without z_prev."""
    A = CSR_CASES[case](mpg)
    if case == "long_row":
        assert np.diff(A.rowptr)[17] == 2100
    _check_sweep(hip, A, t, on_sell=False)


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(SELL_CASES))
def test_sell_sweep_bits(mpg, hip, case, t):
    """mpg_sell_cheb_sweep_* = mpg_sell_spmv_* (alpha 1, beta 0) on the same
    copy, then the seven NumPy operations; with and without z_prev."""
    A = SELL_CASES[case](mpg)
    lay = _check_sweep(hip, A, t, on_sell=True)
    print(case, t, lay)
    if case == "band_4352":
        assert lay["implicit"] > 0, lay
    if case == "edges_4352":
        assert lay["window"] == 1, lay
    if case == "stencil27p_4":
        assert lay["implicit"] == 0, lay


# ---------------------------------------------------------------- 2. the bound
BOUND_CASES = {"band_13316": CSR_CASES["band_13316"], "stencil27_2": CSR_CASES["stencil27_2"],
               "long_row": _long_row_matrix}


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BOUND_CASES))
def test_bound(mpg, hip, case, t):
    """mpg_csr_jacobi_bound_* = max |d| sum |a| of the device's own values and
    diagonal, widened, within 1e-12 relative (NumPy sums each row in another
    order); two calls give the same bits."""
    A = BOUND_CASES[case](mpg)
    S = ChebStorage(hip, A, t)
    try:
        diag = S.jacobi_diag()
        got = S.bound(diag)
        d = diag.get().astype(np.float64)
        absval = np.abs(A.val.astype(S.T).astype(np.float64))
        ref = float(np.max(np.abs(d) * np.add.reduceat(absval, A.rowptr[:-1].astype(np.int64))))
        print(case, t, repr(got), repr(ref))
        assert abs(got - ref) <= 1e-12 * ref
        assert S.bound(diag) == got
        diag.free()
    finally:
        S.close()


def test_bound_of_the_laplacian_is_two(mpg, hip):
    """gen_laplace3d(5) with Jacobi's diagonal: 12 / 6, exactly."""
    S = ChebStorage(hip, mpg.gen_laplace3d(5), "f64")
    try:
        diag = S.jacobi_diag()
        assert S.bound(diag) == 2.0
        diag.free()
    finally:
        S.close()


# ---------------------------------------------------------------- 3. engine apply
@pytest.mark.parametrize("t,accum", [("f32", 0), ("f32", 1), ("f64", 0)], ids=["f32-acc64", "f32-acc32", "f64"])
@pytest.mark.parametrize("case,fmt", APPLY_CASES, ids=["band-sell", "stencil-csr", "stencil-node"])
def test_engine_apply_bits(mpg, hip, case, fmt, t, accum):
    """mpg_arnoldi_cheb_apply at s = 1, 2, 3, 5 on [2/30, 2] = gdmv with
    alpha_0, then s - 1 restated sweeps whose row sums are the workspace's own
    Arnoldi SpMV's (its storage and accumulation class) and whose coefficients
    are mpg_cheb_coeffs' rounded to T."""
    A = mpg.gen_band(4352, 5, 4, seed=7) if case == "band_4352" else mpg.gen_stencil27(5)
    W = ChebWorkspace(mpg, hip, A, t, fmt, accum)
    try:
        assert W.format == fmt, W.format
        T = W.T
        theta, delta = theta_delta(2.0 / 30.0, 2.0)
        alpha, beta = lib_cheb_coeffs(mpg, 5, theta, delta)
        d = W.diag.get()
        r = np.random.default_rng(9).standard_normal(A.nrows).astype(T)
        zs = [((T(alpha[0]) * d).astype(T) * r).astype(T)]  # gdmv(alpha_0, d, r, 0, .)
        for j in range(1, 5):
            zs.append(np_cheb_sweep(W.spmv(zs[-1]), d, r, zs[-1], zs[-2] if j >= 2 else None, alpha[j], beta[j]))
        for s in (1, 2, 3, 5):
            a_s, b_s = lib_cheb_coeffs(mpg, s, theta, delta)
            assert np.array_equal(a_s, alpha[:s]) and np.array_equal(b_s, beta[:s])
            got = W.apply(s, r, theta, delta)
            assert got.dtype == zs[s - 1].dtype and np.array_equal(got, zs[s - 1]), (s, int(np.sum(got != zs[s - 1])))
        # refused before any launch
        w = hip.buf(r)
        lib = hip.lib
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 0, theta, delta, w.p, w.p, w.p) == -2
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 65, theta, delta, w.p, None, None) == -2
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 2, theta, delta, w.p, None, None) == -2
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 2, theta, delta, w.p, w.p, None) == -2
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 1, theta, theta, w.p, None, None) == -2   # a = 0
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 1, theta, 0.0, w.p, None, None) == -2     # a = b
        assert lib.mpg_arnoldi_cheb_apply(W.arn, 1, float("nan"), delta, w.p, None, None) == -2
        assert np.array_equal(w.get(), r)
        w.free()
    finally:
        W.close()


# ---------------------------------------------------------------- solves
@pytest.fixture(scope="module")
def s5(mpg):
    A = mpg.gen_stencil27(5)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, xt, mpg.host_spmv(A, xt)


def _interval(mpg, A, b, xt, **opts):
    eng = mpg.Engine(A, b, xt, **opts)
    lay = eng.spmv_layout()
    eng.close()
    return lay


# 4. storage forms
def test_storage_forms_same_first_cycle(mpg, s5):
    """With s = 3 the first cycle (30 steps) has the same bits on CSR row
    blocks, SELL-64 and node blocks under an fp32 Arnoldi (mode mixed); under
    an fp64 Arnoldi node blocks and CSR agree bit for bit, and SELL is held
    as tests/test_neumann_gpu.py::test_storage_forms_same_first_cycle holds it."""
    A, xt, b = s5
    for mode in ("mixed", "baseline"):
        res = {}
        for fmt in ("csr", "sell", "node"):
            opts = dict(mode=mode, orth="cgs", prec="chebyshev", jacobi_steps=3, rlen=30, tol=0.0, max_restarts=2,
                        spmv_format=fmt)
            lay = _interval(mpg, A, b, xt, **opts)
            assert lay["format"] == fmt and lay["prec_sweeps"] == 3 and "prec_fused" not in lay, lay
            assert lay["prec_interval"][0] * 30 == pytest.approx(lay["prec_interval"][1], rel=1e-15), lay
            res[fmt] = mpg.solve(A, b, xt, engine="fused", **opts)
            assert res[fmt].total_iters == 60
        assert np.array_equal(res["node"].step_res[:30], res["csr"].step_res[:30])
        if mode == "mixed":
            assert np.array_equal(res["sell"].step_res[:30], res["csr"].step_res[:30])
        else:
            np.testing.assert_allclose(res["sell"].step_res[:12], res["csr"].step_res[:12], rtol=1e-9)
    for prec in ("jacobi", "neumann"):
        lay = _interval(mpg, A, b, xt, mode="mixed", orth="cgs", prec=prec, jacobi_steps=2, rlen=30, tol=0.0,
                        max_restarts=1)
        assert "prec_interval" not in lay


# 5. parity with the NumPy loop
PARITY_STEPS = 3


@pytest.fixture(scope="module")
def np_runs(mpg, s5):
    """The NumPy loop on stencil27(5), rlen 30, tol 1e-8, s = 3 on the
    interval the engine reports for the mode (computed once); that interval
    is NumPy's bound and a 30th of it."""
    from oracle import gmres_np

    A, xt, b = s5
    runs = {}
    for mode, T in (("baseline", np.float64), ("mixed", np.float32)):
        lay = _interval(mpg, A, b, xt, mode=mode, orth="cgs", prec="chebyshev", jacobi_steps=PARITY_STEPS, rlen=30,
                        tol=1e-8, max_restarts=10)
        lo, hi = lay["prec_interval"]
        ref_hi = np_jacobi_bound(A, T)
        print(mode, "interval", (lo, hi), "numpy bound", ref_hi)
        assert abs(hi - ref_hi) <= 1e-12 * ref_hi and abs(lo - ref_hi / 30) <= 1e-12 * ref_hi / 30
        r = np_solve_cheb(A, b, mode, "cgs", 30, 1e-8, PARITY_STEPS, (lo, hi))
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
    got = mpg.solve(A, b, xt, engine=engine, mode="baseline", orth="cgs", prec="chebyshev", jacobi_steps=PARITY_STEPS,
                    rlen=30, tol=1e-8, max_restarts=1000)
    parity.compare(np_runs["baseline"], got, "baseline", 1e-8, 30, f"chebyshev/baseline/{engine}")


@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_parity_mixed(mpg, s5, np_runs, engine):
    """fp32 Arnoldi: status, restarts within 1, compare's cycle-0 history
    rule, and every cycle's backward error at most 3x the NumPy loop's."""
    A, xt, b = s5
    ref = np_runs["mixed"]
    got = mpg.solve(A, b, xt, engine=engine, mode="mixed", orth="cgs", prec="chebyshev", jacobi_steps=PARITY_STEPS,
                    rlen=30, tol=1e-8, max_restarts=1000)
    assert got.status == ref["status"]
    assert abs(got.restarts - ref["restarts"]) <= 1
    parity.compare(ref, got, "mixed", 1e-8, 30, f"chebyshev/mixed/{engine}")
    parity.not_worse_than(SimpleNamespace(**ref), got, "mixed", f"chebyshev/mixed/{engine}", factor=3)


# 6. it preconditions
@pytest.mark.parametrize("engine", ["fused", "surface"])
def test_it_preconditions(mpg, engine):
    """gen_laplace3d(16), baseline, CGS, GMRES(10), tol 1e-10, the interval
    [2/30, 2] (this matrix's own bound and the default ratio): all converge;
    chebyshev s = 3 takes fewer iterations than neumann s = 3, s = 4 no more
    than neumann s = 4, s = 3 at most half of jacobi's (the NumPy loop's
    counts: tests/test_chebyshev_cpu.py::test_numpy_counts)."""
    A = mpg.gen_laplace3d(16)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(engine=engine, mode="baseline", orth="cgs", rlen=10, tol=1e-10, max_restarts=1000)
    if engine == "fused":
        lay = _interval(mpg, A, b, xt, prec="chebyshev", jacobi_steps=3, **{k: v for k, v in opts.items() if k != "engine"})
        assert lay["prec_interval"] == COUNTS_INTERVAL, lay
    runs = {"jacobi": mpg.solve(A, b, xt, prec="jacobi", **opts)}
    for s in (3, 4):
        runs[f"neumann{s}"] = mpg.solve(A, b, xt, prec="neumann", jacobi_steps=s, **opts)
        runs[f"cheb{s}"] = mpg.solve(A, b, xt, prec="chebyshev", jacobi_steps=s, **opts)
    it = {k: r.total_iters for k, r in runs.items()}
    print("total_iters:", it)
    assert all(r.status == "converged" for r in runs.values())
    assert it["cheb3"] < it["neumann3"]
    assert it["cheb4"] <= it["neumann4"]
    assert 2 * it["cheb3"] <= it["jacobi"]


# 7. the settings
def test_settings(mpg, s5, monkeypatch):
    """MPG_CHEB_RATIO and MPG_CHEB_LMAX are read when the preconditioner is
    set up: they show in prec_interval and change the arithmetic; a value
    outside its range is a RuntimeError naming it, and the next solve runs."""
    A, xt, b = s5
    opts = dict(mode="mixed", orth="cgs", prec="chebyshev", jacobi_steps=3, rlen=30, tol=0.0, max_restarts=1)
    default = _interval(mpg, A, b, xt, **opts)["prec_interval"]
    base = mpg.solve(A, b, xt, engine="fused", **opts)
    monkeypatch.setenv("MPG_CHEB_RATIO", "4")
    lo, hi = _interval(mpg, A, b, xt, **opts)["prec_interval"]
    assert hi == default[1] and lo == hi / 4.0
    ratio4 = mpg.solve(A, b, xt, engine="fused", **opts)
    assert not np.array_equal(ratio4.step_res, base.step_res)
    monkeypatch.setenv("MPG_CHEB_LMAX", "1.5")
    assert _interval(mpg, A, b, xt, **opts)["prec_interval"] == (1.5 / 4.0, 1.5)
    assert not np.array_equal(mpg.solve(A, b, xt, engine="fused", **opts).step_res, ratio4.step_res)
    surface_set = mpg.solve(A, b, xt, engine="surface", **opts)
    monkeypatch.delenv("MPG_CHEB_LMAX")
    monkeypatch.delenv("MPG_CHEB_RATIO")
    assert not np.array_equal(mpg.solve(A, b, xt, engine="surface", **opts).step_res, surface_set.step_res)
    for engine in ("fused", "surface"):
        monkeypatch.setenv("MPG_CHEB_RATIO", "1")
        with pytest.raises(RuntimeError, match=r"MPG_CHEB_RATIO = 1 is not a real > 1"):
            mpg.solve(A, b, xt, engine=engine, **opts)
        monkeypatch.delenv("MPG_CHEB_RATIO")
        monkeypatch.setenv("MPG_CHEB_LMAX", "-1")
        with pytest.raises(RuntimeError, match=r"MPG_CHEB_LMAX = -1 is not a real > 0"):
            mpg.solve(A, b, xt, engine=engine, **opts)
        monkeypatch.delenv("MPG_CHEB_LMAX")
        again = mpg.solve(A, b, xt, engine=engine, **opts)
        assert again.total_iters == 30
        if engine == "fused":
            assert np.array_equal(again.step_res, base.step_res)


# 8. the operator surface still records the cycle
@pytest.mark.parametrize("mode", ["mixed", "baseline", "single"])
def test_surface_still_records_the_cycle(mpg, mode, monkeypatch):
    """Nothing in Chebyshev<Type, Hip>::apply reads on the host (the
    coefficients are launch arguments), so the operator-surface driver
    records the cycle's calls as with Jacobi (first cycle eager, second
    recorded, later replayed), and the replays have the bits of issuing
    every call on its own."""
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(engine="surface", mode=mode, orth="cgs", prec="chebyshev", jacobi_steps=3, rlen=10, tol=1e-10,
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


# 9. refusals
def test_refusals(mpg, s5, monkeypatch):
    """Each refusal is a RuntimeError that names its reason and the
    preconditioner, and the next solve runs normally."""
    A, xt, b = s5
    opts = dict(orth="cgs", prec="chebyshev", rlen=30, tol=1e-8, max_restarts=20)
    for engine in ("fused", "surface"):
        with pytest.raises(RuntimeError, match=r"prec chebyshev: jacobi_steps = 0 is outside \[1, 64\]"):
            mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=0, **opts)
        with pytest.raises(RuntimeError, match=r"prec chebyshev: jacobi_steps = 65 is outside \[1, 64\]"):
            mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=65, **opts)
        with pytest.raises(RuntimeError, match="prec chebyshev is not available in mode single-prec"):
            mpg.solve(A, b, xt, engine=engine, mode="single-prec", jacobi_steps=2, **opts)
    with pytest.raises(RuntimeError, match="prec chebyshev is not available in mode mixed-half"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed-half", jacobi_steps=2, **opts)
    with pytest.raises(RuntimeError, match="prec chebyshev.*row-partitioned.*halo exchange"):
        mpg.solve_loopback(A, b, xt, nranks=2, mode="mixed", jacobi_steps=2, **opts)
    monkeypatch.setenv("MPG_STEP_DOTS", "2")
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        mpg.solve(A, b, xt, engine="fused", mode="mixed", jacobi_steps=2, accum="f32", spmv_format="sell", **opts)
    monkeypatch.delenv("MPG_STEP_DOTS")
    for engine in ("fused", "surface"):
        for s in (1, 2):  # (one step is Jacobi scaled by 1 / theta: a launch of its own, not prec jacobi's path)
            got = mpg.solve(A, b, xt, engine=engine, mode="mixed", jacobi_steps=s, **opts)
            assert got.status == "converged"


# 10. CLI
def test_cli(mpg):
    """--prec chebyshev --jacobi-steps 3 --cheb-ratio 30 keeps the
    reference's stdout contract and reports the iterations of mpg.solve with
    the same options; a ratio outside its range ends the run with an error
    that names it."""
    base = [str(mpg.CLI), "--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec",
            "chebyshev", "--jacobi-steps", "3", "--tol", "1e-9", "--gpu"]
    out = subprocess.run(base + ["--cheb-ratio", "30"], capture_output=True, text=True, timeout=120, check=True).stdout
    m = SUMMARY.search(out)
    assert m, out
    assert float(m.group(1)) <= 1e-9
    assert out.startswith("||x|| = ") and "Doing Mixed Precision test" in out
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    got = mpg.solve(A, mpg.host_spmv(A, xt), xt, engine="fused", mode="mixed", orth="cgs", prec="chebyshev",
                    jacobi_steps=3, rlen=30, tol=1e-9, max_restarts=1_000_000)
    assert int(m.group(4)) == got.total_iters > 0
    bad = subprocess.run(base + ["--cheb-ratio", "1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "MPG_CHEB_RATIO = 1" in bad.stdout + bad.stderr
