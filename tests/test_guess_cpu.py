"""The initial-guess store without a GPU: the NumPy restatement (tests/guess_np.py)
of project and keep against a stand-in solver, on the bounds the GPU tests
(tests/test_guess_gpu.py) use; the new symbols, the NULL-engine argument checks
and the CLI's argument errors.

The stand-in solver returns the exact solution plus an error that leaves a
relative residual of 0.5 tol -- or the guess itself where the guess already
meets that, as a solver that converges in 0 iterations does."""
import dataclasses
import subprocess

import numpy as np
import pytest

from tests import guess_np as GS
from tests.golden.make_golden import convdiff

TOL = 1e-9
U = GS.U


@pytest.fixture(scope="module", params=["lap12", "convdiff32"])
def prob(request, mpg):
    A = mpg.gen_laplace3d(12) if request.param == "lap12" else convdiff(mpg, 32)
    xts = [mpg.rand_vect(A.nrows, 42 + j) for j in range(4)]
    return A, [(mpg.host_spmv(A, xt), xt) for xt in xts]


def _solver(mpg, A, seed=0):
    rng = np.random.default_rng(100 + seed)

    def solve(b, xt, x0=None):
        if x0 is not None and np.linalg.norm(b - mpg.host_spmv(A, x0)) <= 0.5 * TOL * np.linalg.norm(b):
            return x0.copy()
        e = rng.standard_normal(A.nrows)
        e *= 0.5 * TOL * np.linalg.norm(b) / np.linalg.norm(mpg.host_spmv(A, e))
        return xt + e

    return solve


def _rho(mpg, A, b, x):
    return float(np.linalg.norm(b - mpg.host_spmv(A, x)))


def _normalization(A, b, x):
    return float(np.linalg.norm(b) + np.linalg.norm(A.val) * np.linalg.norm(x))


def _check_invariants(mpg, A, st):
    n, p = A.nrows, st.held
    Z, Q = st.Z[:, :p], st.Q[:, :p]
    assert GS.orth_defect(Q) <= p * n * U
    for err, znorm in GS.image_defects(lambda v: mpg.host_spmv(A, v), Z, Q):
        assert err <= n * U * np.linalg.norm(A.val) * znorm


def test_store_invariants_after_four_kept_solves(mpg, prob):
    A, rhs = prob
    solve = _solver(mpg, A)
    st = GS.Store(lambda v: mpg.host_spmv(A, v), A.nrows, 8, TOL)
    for b, xt in rhs:
        assert st.keep(solve(b, xt))
    assert st.held == 4
    _check_invariants(mpg, A, st)


def test_recall(mpg, prob):
    A, rhs = prob
    b1, xt1 = rhs[0]
    solve = _solver(mpg, A)
    st = GS.Store(lambda v: mpg.host_spmv(A, v), A.nrows, 8, TOL)
    x1 = solve(b1, xt1)
    st.keep(x1)
    x0 = st.project(b1)
    n = A.nrows
    assert _rho(mpg, A, b1, x0) <= (1 + 1e-6) * _rho(mpg, A, b1, x1) + n * U * _normalization(A, b1, x0)
    assert st.rho1 <= st.rho0
    assert not st.keep(solve(b1, xt1, x0)) and st.held == 1


def test_span(mpg, prob):
    A, rhs = prob
    (b1, xt1), (b2, xt2) = rhs[:2]
    solve = _solver(mpg, A)
    st = GS.Store(lambda v: mpg.host_spmv(A, v), A.nrows, 8, TOL)
    x1, x2 = solve(b1, xt1), solve(b2, xt2)
    st.keep(x1), st.keep(x2)
    b3 = 2 * b1 - 3 * b2
    x0 = st.project(b3)
    n = A.nrows
    cap = (1 + 1e-6) * (2 * _rho(mpg, A, b1, x1) + 3 * _rho(mpg, A, b2, x2)) + n * U * _normalization(A, b3, x0)
    assert _rho(mpg, A, b3, x0) <= cap
    assert _rho(mpg, A, b3, x0) < 1e-3 * _rho(mpg, A, b3, x2)  # the previous solution alone is no guess for b3


def test_depth_and_restart(mpg, prob):
    A, rhs = prob
    solve = _solver(mpg, A)
    st = GS.Store(lambda v: mpg.host_spmv(A, v), A.nrows, 2, TOL)
    xs = [solve(b, xt) for b, xt in rhs[:3]]
    for x, held in zip(xs, (1, 2, 1)):
        st.keep(x)
        assert st.held == held
    b3 = rhs[2][0]
    x0 = st.project(b3)
    assert _rho(mpg, A, b3, x0) <= (1 + 1e-6) * _rho(mpg, A, b3, xs[2]) + A.nrows * U * _normalization(A, b3, x0)


def test_reimaging_after_new_values(mpg, prob):
    A, rhs = prob
    solve = _solver(mpg, A)
    st = GS.Store(lambda v: mpg.host_spmv(A, v), A.nrows, 8, TOL)
    for b, xt in rhs[:3]:
        st.keep(solve(b, xt))
    A2 = dataclasses.replace(A, val=mpg.perturb_values(A, 1e-3, 1))
    st.reimage(lambda v: mpg.host_spmv(A2, v))
    assert st.held == 3
    _check_invariants(mpg, A2, st)
    b = mpg.host_spmv(A2, rhs[3][1])
    x0 = st.project(b)
    assert st.rho1 <= st.rho0
    assert abs(_rho(mpg, A2, b, x0) - st.rho1) <= 1e-9 * st.rho0  # the prediction is the residual


def test_base_guess_is_honoured(mpg, prob):
    A, rhs = prob
    solve = _solver(mpg, A)
    st = GS.Store(lambda v: mpg.host_spmv(A, v), A.nrows, 8, TOL)
    for b, xt in rhs[:2]:
        st.keep(solve(b, xt))
    b, xt = rhs[2]
    xbar = xt + 1e-4 * mpg.rand_vect(A.nrows, 7)
    x0 = st.project(b, xbar)
    assert st.rho0 == pytest.approx(_rho(mpg, A, b, xbar), rel=1e-12)
    assert _rho(mpg, A, b, x0) <= st.rho0 * (1 + 1e-12)
    assert np.linalg.norm(x0 - xbar) > 0


NEW_SYMBOLS = (("solve.h", "mpg_engine_guess_depth", "host"), ("solve.h", "mpg_engine_guess_keep", "host"),
               ("solve.h", "mpg_engine_guess_info", "host"), ("solve.h", "mpg_engine_guess_store", "host"),
               ("capi.h", "mpg_guess_groups", "hip"), ("capi.h", "mpg_guess_dots_f64", "hip"),
               ("capi.h", "mpg_guess_update_f64", "hip"), ("capi.h", "mpg_guess_scale_f64", "hip"))


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for header, name, lib in NEW_SYMBOLS:
        assert (header, name) in declared, name
        assert hasattr(mpg.host_lib() if lib == "host" else mpg.hip_lib(), name), name


def test_null_arguments_are_refused_without_a_device(mpg):
    import inspect

    lib, hip = mpg.host_lib(), mpg.hip_lib()
    assert lib.mpg_engine_guess_depth(None, 4) == -2
    assert lib.mpg_engine_guess_keep(None) == -2
    assert lib.mpg_engine_guess_info(None, None, None, None, None, None) == -2
    assert lib.mpg_engine_guess_store(None, None, None) == -2
    assert hip.mpg_guess_groups(0) == -2
    assert hip.mpg_guess_groups(1) == 1 and hip.mpg_guess_groups(1025) == 2 and hip.mpg_guess_groups(1 << 30) == 512
    assert hip.mpg_guess_dots_f64(None, 4, 1, 4, None, None, None) == -2
    assert hip.mpg_guess_update_f64(None, 4, 1, 4, None, 1.0, None, None, None, None, None, None, None) == -2
    assert hip.mpg_guess_scale_f64(None, 4, None, None, 0.0, None, None, None, None, None) == -2
    for name in ("guess_info", "guess_store", "guess_keep", "set_guess_depth"):
        assert hasattr(mpg.Engine, name)
    assert "guess" in inspect.signature(mpg.Engine.solve).parameters
    assert "guess" in inspect.signature(mpg.Engine.rearm).parameters
    assert "guess_depth" in inspect.signature(mpg.Engine.__init__).parameters


CLI_BASE = ["--matrix", "laplace:4", "--rlen", "10", "--orth", "cgs", "--prec", "jacobi"]


@pytest.mark.parametrize("extra,words", [
    (["--guess", "project"], ("--guess", "--solves")),
    (["--guess", "project", "--solves", "1"], ("--guess", "--solves")),
    (["--solves", "2", "--guess", "previous"], ("Unknown guess",)),
    (["--solves", "2", "--guess"], ("Missing value for --guess",)),
    (["--solves", "2", "--rhs-path", "2", "--bpath", "b.mtx"], ("--rhs-path", "--bpath")),
    (["--rhs-path", "-1"], ("--rhs-path",)),
], ids=["no --solves", "--solves 1", "unknown guess", "missing value", "rhs-path with bpath", "negative rhs-path"])
def test_cli_argument_errors(mpg, extra, words):
    r = subprocess.run([str(mpg.CLI)] + CLI_BASE + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and all(w in r.stdout for w in words), (r.stdout, r.stderr)
    assert "Doing" not in r.stdout
