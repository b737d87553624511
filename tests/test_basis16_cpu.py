"""The compressed Krylov basis (basis="f16") on the CPU: the rounding function
of tests/basis16_np.py (what csrc/basis.hpp states), the keyword at the ABI
level, and the two cycle counts the feature rests on, from the NumPy
restatement with matrices of the project's generators. Nothing here launches
a kernel."""
import os

import numpy as np
import pytest

from tests import basis16_np as B16

F32 = np.float32

# the special values the GPU test stores too (tests/test_basis16_gpu.py)
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -14, 2.0 ** -27, 2.0 ** -28, 2.0 ** -29, 2.0 ** -38,
                     2.0 ** -39, 2.0 ** -40, 3 * 2.0 ** -38, 2049.0 / 16384, 2051.0 / 16384, -2049.0 / 16384,
                     2050.0 / 16384, 1.0 - 2.0 ** -12, 1.0 + 2.0 ** -11, 3.0e-4, -3.0e-4, 6.1e-5, np.inf, -np.inf,
                     np.nan], dtype=F32)


# ---------------------------------------------------------------- the rounding function
def _samples():
    rng = np.random.default_rng(11)
    mags = np.exp2(rng.uniform(-28.0, 0.0, 20000))
    return (mags * rng.choice([-1.0, 1.0], mags.size)).astype(F32)


def test_round_is_idempotent():
    v = np.concatenate([_samples(), SPECIALS])
    r = B16.round_f16(v)
    assert r.dtype == F32
    assert np.array_equal(B16.round_f16(r), r, equal_nan=True)
    # ... and a rounded value packs to the bits it came from
    assert np.array_equal(B16.pack_f16(r), B16.pack_f16(v))


def test_round_is_exact_on_powers_of_two():
    p = np.exp2(np.arange(-28, 1)).astype(F32)
    assert np.array_equal(B16.round_f16(p), p) and np.array_equal(B16.round_f16(-p), -p)


def test_round_relative_error():
    """fp16 keeps 11 significant bits over its normal range, which the scale
    2^14 puts at 2^-28 <= |v| <= 1: half an ulp is 2^-11 relative."""
    v = _samples()
    v = v[(np.abs(v) >= F32(2.0 ** -28)) & (np.abs(v) <= 1)]
    rel = np.abs(B16.round_f16(v).astype(np.float64) - v.astype(np.float64)) / np.abs(v.astype(np.float64))
    print("max relative error", rel.max(), "of 2^-11 =", 2.0 ** -11)
    assert rel.max() <= 2.0 ** -11
    assert rel.max() > 2.0 ** -13  # (it is a rounding to 11 bits, not to more)


def test_round_ties_to_even():
    r = B16.round_f16(np.array([2049, 2051, -2049, 2050, 4098, 4102], F32) / F32(16384))
    assert np.array_equal(r * F32(16384), np.array([2048, 2052, -2048, 2050, 4096, 4104], F32))
    # not toward zero (what the packed cvt_pkrtz conversion would give: 2050)
    assert B16.round_f16(F32(2051.0 / 16384)) * F32(16384) == 2052


def test_round_subnormal_halves():
    """Below 2^-28 the stored half is subnormal: multiples of 2^-38, ties to even, zero below 2^-39."""
    q = F32(2.0 ** -38)
    v = np.array([2.0 ** -29, 2.0 ** -38, 3 * 2.0 ** -38, 2.0 ** -39, 3 * 2.0 ** -39, 2.0 ** -40, 1.6 * 2.0 ** -38], F32)
    want = np.array([2.0 ** -29, 2.0 ** -38, 3 * 2.0 ** -38, 0.0, 2 * 2.0 ** -38, 0.0, 2 * 2.0 ** -38], F32)
    got = B16.round_f16(v)
    assert np.array_equal(got, want)
    assert np.all(np.mod(got / q, 1) == 0)
    bits = B16.pack_f16(v)
    assert np.all((bits & 0x7C00) == 0)  # exponent field 0: subnormal or zero


def test_round_keeps_zero_inf_nan():
    r = B16.round_f16(np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F32))
    assert r[0] == 0 and not np.signbit(r[0]) and r[1] == 0 and np.signbit(r[1])
    assert r[2] == np.inf and r[3] == -np.inf and np.isnan(r[4])
    assert list(B16.pack_f16(np.array([0.0, -0.0, np.inf, -np.inf], F32))) == [0x0000, 0x8000, 0x7C00, 0xFC00]


def test_scale_keeps_unit_vectors_in_range():
    """|v| <= 1 up to rounding: 2^14 |v| stays far below fp16's 65504."""
    assert np.isfinite(B16.round_f16(F32(1.0 + 2.0 ** -11))) and np.isfinite(B16.round_f16(F32(3.99)))
    assert 16384 * (1 + 2.0 ** -11) < 65504 / 3


# ---------------------------------------------------------------- the keyword and the ABI
def test_make_args_carries_the_keyword(mpg):
    """mpg_solve_args does not change (tests/test_bjacobi_cpu.py pins its last
    field): the keyword rides on the structure and becomes MPG_BASIS around
    the creating call only."""
    A = mpg.gen_laplace3d(3)
    a, keep = mpg.make_args(A, np.ones(A.nrows), basis="f16")
    assert a._basis == "f16"
    a0, keep0 = mpg.make_args(A, np.ones(A.nrows))
    assert a0._basis is None
    from mpgmres_amd import _basis_setting

    before = os.environ.get("MPG_BASIS")
    with _basis_setting(a):
        assert os.environ["MPG_BASIS"] == "f16"
    assert os.environ.get("MPG_BASIS") == before
    with _basis_setting(a0):
        assert os.environ.get("MPG_BASIS") == before


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for name in ("mpg_arnoldi_set_basis", "mpg_arnoldi_basis"):
        assert ("arnoldi.h", name) in declared, name
        assert hasattr(mpg.hip_lib(), name)
    assert ("solve.h", "mpg_engine_basis") in declared
    assert hasattr(mpg.host_lib(), "mpg_engine_basis")


def test_null_workspace_is_refused(mpg):
    hip = mpg.hip_lib()
    assert hip.mpg_arnoldi_set_basis(None, 1) == -2 and hip.mpg_arnoldi_basis(None) == -2


# ---------------------------------------------------------------- the counts
@pytest.fixture(scope="module")
def problems(mpg):
    out = {}
    for name, nx in (("lap16", 16), ("lap10", 10)):
        A = mpg.gen_laplace3d(nx)
        xt = mpg.rand_vect(A.nrows, 42)
        out[name] = (A, mpg.host_spmv(A, xt), xt)
    return out


def _counts(problem, rlen, orth):
    A, b, xt = problem
    got = {}
    for sums in ("fp64", "seq32"):
        for basis in ("f32", "f16"):
            r = B16.solve(A, b, xt, orth=orth, prec="jacobi", rlen=rlen, tol=1e-10, basis=basis, sums=sums)
            assert r["status"] == "converged"
            got[sums, basis] = r["restarts"]
    print("cycles", got)
    # the summation order does not move the count: the GPU's trees cannot either
    for basis in ("f32", "f16"):
        assert got["fp64", basis] == got["seq32", basis]
    return got["fp64", "f32"], got["fp64", "f16"]


# recorded here (printed by the test, asserted below): tests/test_basis16_gpu.py expects them of the GPU
SLOW_CASE = dict(matrix="lap16", rlen=10, cycles_f32=12, cycles_f16=12)
FAST_CASE = dict(matrix="lap10", rlen=30, cycles_f32=2, cycles_f16=3)


@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
def test_slow_case_costs_no_cycle(problems, orth):
    """gen_laplace3d(16), GMRES(10), Jacobi, tol 1e-10: a cycle gains a factor
    4-6, far less than the 2.5e-4 an fp16 basis allows: the same count."""
    f32, f16 = _counts(problems[SLOW_CASE["matrix"]], SLOW_CASE["rlen"], orth)
    assert (f32, f16) == (SLOW_CASE["cycles_f32"], SLOW_CASE["cycles_f16"])
    assert f16 == f32


@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
def test_fast_case_costs_at_most_two_cycles(problems, orth):
    """gen_laplace3d(10), GMRES(30): the fp32 basis gains 2.5e-8 in its first
    cycle, the fp16 one 4.7e-6: one cycle more."""
    f32, f16 = _counts(problems[FAST_CASE["matrix"]], FAST_CASE["rlen"], orth)
    assert (f32, f16) == (FAST_CASE["cycles_f32"], FAST_CASE["cycles_f16"])
    assert f32 < f16 <= f32 + 2


def test_first_cycle_floor(problems):
    """One cycle with an fp16 basis does not reduce the backward error below
    the 2^-11-level loss of orthonormality, where the fp32 basis goes on."""
    A, b, xt = problems["lap10"]
    be = {}
    for basis in ("f32", "f16"):
        r = B16.solve(A, b, xt, orth="cgs", prec="jacobi", rlen=30, tol=1e-10, basis=basis)
        be[basis] = (r["cyc_r_norm"] / r["cyc_normalization"])[1]
    print("backward error after cycle 1", be)
    assert be["f32"] < 1e-6 < be["f16"] < 2.5e-4


def test_f32_basis_restates_the_oracle(problems):
    """With the identity hook and fp64 sums the loop is oracle.gmres_np.solve's:
    the same counts and histories to fp32 rounding."""
    from oracle import gmres_np

    A, b, xt = problems["lap10"]
    ref = gmres_np.solve(A, b, mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-10)
    got = B16.solve(A, b, xt, orth="cgs", prec="jacobi", rlen=30, tol=1e-10, basis="f32")
    assert got["restarts"] == ref["restarts"] and got["total_iters"] == ref["total_iters"]
    k = 30
    assert np.allclose(got["step_res"][:k], ref["step_res"][:k], rtol=1e-3, atol=1e-5 * ref["minvb_norm"])
