"""A sequence of solves on one engine, from an initial guess, on the CPU: the
NumPy restatement with an x0 argument (tests/resolve_np.py), the cycle counts
the GPU tests expect of it, and the new entry points at the ABI level.
Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

from tests import basis16_np as B16
from tests import resolve_np as RS

# (matrix, rlen): gen_laplace3d(nx), x_true = rand_vect(n, 42), b = A x_true, Jacobi, tol 1e-10, mode mixed.
# cold: restart cycles from x0 = 0; warm: from resolve_np.warm_guess(x_true) = x_true + 1e-4 N(0, 1) (seed 7);
# be_warm: the first backward error r / (||b|| + ||A||_F ||x0||) of the warm start (from zeros it is 1).
# The counts are the same for cgs and cgsr and for both summation classes of the restatement ("fp64", "seq32").
# Recorded here (printed by the test, asserted below): tests/test_resolve_gpu.py expects them of the GPU.
CASES = {
    "lap10": dict(nx=10, rlen=10, cold=6, warm=3, be_warm=4.98e-6),
    "lap12": dict(nx=12, rlen=30, cold=2, warm=1, be_warm=4.08e-6),
    "lap16": dict(nx=16, rlen=10, cold=12, warm=3, be_warm=2.66e-6),
}
# the GPU test's cap on a warm start's first backward error: at least 10x above every be_warm
WARM_BE_CAP = 1e-4
TOL = 1e-10


@pytest.fixture(scope="module")
def problems(mpg):
    out = {}
    for name, c in CASES.items():
        A = mpg.gen_laplace3d(c["nx"])
        xt = mpg.rand_vect(A.nrows, 42)
        out[name] = (A, mpg.host_spmv(A, xt), xt)
    return out


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_no_guess_restates_basis16_np(problems, name, orth):
    A, b, xt = problems[name]
    rlen = CASES[name]["rlen"]
    ref = B16.solve(A, b, xt, orth=orth, prec="jacobi", rlen=rlen, tol=TOL)
    got = RS.solve(A, b, xt, x0=None, orth=orth, prec="jacobi", rlen=rlen, tol=TOL)
    assert set(got) == set(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k


@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_counts(problems, name, orth):
    """cold, warm and again (from the converged x): the warm start saves
    cycles, the converged x needs none."""
    A, b, xt = problems[name]
    c = CASES[name]
    kw = dict(orth=orth, prec="jacobi", rlen=c["rlen"], tol=TOL)
    cold = RS.solve(A, b, xt, **kw)
    warm = RS.solve(A, b, xt, x0=RS.warm_guess(xt), **kw)
    again = RS.solve(A, b, xt, x0=cold["x"], **kw)
    be = lambda r: float(r["cyc_r_norm"][0] / r["cyc_normalization"][0])  # noqa: E731
    print(name, orth, "cycles cold", cold["restarts"], "warm", warm["restarts"], "again", again["restarts"],
          "first backward error cold", be(cold), "warm", be(warm))
    assert cold["status"] == warm["status"] == again["status"] == "converged"
    assert (cold["restarts"], warm["restarts"]) == (c["cold"], c["warm"])
    assert again["restarts"] == 0 and again["total_iters"] == 0
    assert np.array_equal(again["x"], cold["x"])
    assert warm["restarts"] < cold["restarts"]
    assert be(cold) > 0.1
    assert abs(be(warm) - c["be_warm"]) <= 0.02 * c["be_warm"]
    assert 10 * be(warm) <= WARM_BE_CAP


def test_guess_does_not_move_the_norms_of_b(problems):
    A, b, xt = problems["lap10"]
    cold = RS.solve(A, b, xt, rlen=10, tol=TOL)
    warm = RS.solve(A, b, xt, x0=RS.warm_guess(xt), rlen=10, tol=TOL)
    assert warm["minvb_norm"] == cold["minvb_norm"]


# ---------------------------------------------------------------- the ABI
NEW_SYMBOLS = ("mpg_engine_rearm", "mpg_engine_x", "mpg_engine_solves", "mpg_engine_graph_captures", "mpg_solve_from")


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for name in NEW_SYMBOLS:
        assert ("solve.h", name) in declared, name
        assert hasattr(mpg.host_lib(), name), name


def test_null_arguments_are_refused_without_a_device(mpg):
    lib = mpg.host_lib()
    v = np.zeros(4)
    p = v.ctypes.data
    assert lib.mpg_engine_rearm(None, p, p, p, 0) == -2
    assert lib.mpg_engine_rearm(None, None, None, None, 3) == -2
    assert lib.mpg_engine_x(None, p, 0) == -2
    from mpgmres_amd._abi import SolveResult

    r = SolveResult()
    assert lib.mpg_solve_from(None, p, C.byref(r)) == -2
    assert lib.mpg_solve_from(None, None, C.byref(r)) == -2
    assert lib.mpg_engine_solves(None) == -2 and lib.mpg_engine_graph_captures(None) == -2
    assert not v.any()


def test_make_args_keeps_its_fields(mpg):
    """x0 travels beside mpg_solve_args, not in it (tests/test_bjacobi_cpu.py
    pins the layout): the struct's fields and make_args' keywords are as they
    were."""
    import inspect

    from mpgmres_amd._abi import SolveArgs

    assert [f for f, _ in SolveArgs._fields_][-3:] == ["stop_on_breakdown", "accum", "prec_block"]
    assert len(SolveArgs._fields_) == 26
    assert "x0" not in inspect.signature(mpg.make_args).parameters
    assert "x0" in inspect.signature(mpg.solve).parameters
    A = mpg.gen_laplace3d(3)
    a, keep = mpg.make_args(A, np.ones(A.nrows), np.ones(A.nrows), mode="mixed", orth="cgs", prec="jacobi", rlen=7)
    assert (a.n, a.nnz, a.mode, a.orth, a.prec, a.engine, a.rlen) == (27, A.nnz, 0, 0, 2, 1, 7)
    assert a.b and a.x_true
    with pytest.raises(TypeError):
        mpg.make_args(A, np.ones(A.nrows), x0=np.ones(A.nrows))


def test_vectors_are_checked_before_any_call(mpg):
    from mpgmres_amd import _arm_vector

    for bad in (np.zeros(5), np.zeros((2, 3)), "abc", [1.0, "x"]):
        with pytest.raises(ValueError):
            _arm_vector(bad, 6, 0, "b")
    ptr, on_dev, keep = _arm_vector(np.arange(6, dtype=np.float32), 6, 0, "b")
    assert not on_dev and keep.dtype == np.float64 and ptr == keep.ctypes.data
    with pytest.raises(ValueError):
        _arm_vector(np.zeros(6, dtype=np.float32), 6, 0, "out", writable=True)


def test_host_tensors_are_refused(mpg):
    from mpgmres_amd import _arm_vector

    torch = pytest.importorskip("torch")
    for bad in (torch.zeros(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float32)):  # (CPU tensors)
        with pytest.raises(ValueError):
            _arm_vector(bad, 6, 0, "b")
