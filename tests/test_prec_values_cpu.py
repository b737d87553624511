"""prec_values = "f16" on the CPU: the quantisation's restatement, the keyword
and the ABI, and the premise -- mixed GMRES(30) with the polynomial
preconditioners' sweeps over the fp16 copy A^ takes the restart cycles it takes
with the sweeps over float32(A) (tests/prec_values_np.py)."""
import os

import numpy as np
import pytest

from tests import prec_values_np as pv


# ---------------------------------------------------------------- the quantisation
def test_quantisation_rule(mpg):
    """k_half_rows' rule on hand-made rows: in range [2^-2, 2^15) no scaling;
    below and above it the row's largest entry lands in [2^14, 2^15); the
    values round fp64 -> fp32 -> fp16 after the scaling."""
    rp = np.array([0, 2, 4, 6, 7, 7], np.int32)
    col = np.array([0, 1, 0, 1, 1, 2, 3], np.int32)
    val = np.array([0.3, -1.0 / 3.0,          # E = -2: left alone
                    0.2, 0.01,                # E = -3: scaled up
                    40000.0, 1.0 / 3.0,       # E = 15: scaled down
                    2.0 ** 14 * 1.999,        # E = 14: left alone
                    ])
    A = mpg.Csr(5, 5, rp, col, val)
    h, e = pv.half_values(A)
    assert e.dtype == np.int8 and list(e) == [0, 17, -1, 0, 0]
    want = np.array([0.3, -1.0 / 3.0, 0.2 * 2.0 ** 17, 0.01 * 2.0 ** 17, 20000.0, 1.0 / 6.0, 2.0 ** 14 * 1.999])
    assert np.array_equal(h, want.astype(np.float32).astype(np.float16))
    assert 2.0 ** 14 <= float(h[2]) < 2.0 ** 15 and 2.0 ** 14 <= float(h[4]) < 2.0 ** 15
    hat = pv.dequantised(h, e, rp)
    assert hat.dtype == np.float32
    assert np.array_equal(hat.astype(np.float64), np.ldexp(h.astype(np.float64), -e.astype(np.int64)[[0, 0, 1, 1, 2, 2, 3]]))
    # the relative entry error is fp16's unit roundoff at most
    assert np.max(np.abs(hat - val) / np.abs(val)) <= 2.0 ** -11


@pytest.mark.parametrize("name", sorted(pv.MATRICES))
def test_matrices_are_not_fp16_exact(mpg, name):
    """A^ != float32(A) in at least half of the entries: a test that silently
    ran the fp32 sweeps on these matrices cannot pass. The entries stay within
    2^-11 relative of A's."""
    A = pv.MATRICES[name](mpg)
    frac = pv.differing_fraction(A)
    print(name, "entries rounded:", frac)
    assert frac >= 0.5, frac
    hat = pv.hat_values(A).astype(np.float64)
    _, e = pv.half_values(A)
    # (half an ulp: 2^-11 relative, or half of fp16's subnormal spacing 2^-24 before the unscale)
    ulp2 = np.maximum(2.0 ** -11 * np.abs(A.val), np.ldexp(2.0 ** -25, -e.astype(np.int64))[np.repeat(np.arange(A.nrows), np.diff(A.rowptr))])
    assert np.all(np.abs(hat - A.val) <= ulp2 * (1 + 2.0 ** -20))  # (the fp32 rounding on the way)
    if name == "band-stiff":
        for s in range(0, 4032, 64):  # every 64-row slice holds rows scaled up, scaled down and left alone
            seg = e[s:s + 64]
            assert np.any(seg > 0) and np.any(seg < 0) and np.any(seg == 0), s


# ---------------------------------------------------------------- the premise
@pytest.mark.parametrize("name,prec,steps", pv.CASES, ids=[f"{c[0]}-{c[1]}{c[2]}" for c in pv.CASES])
def test_cycle_counts_are_those_of_fp32_values(mpg, name, prec, steps):
    A = pv.MATRICES[name](mpg)
    b = pv.rhs(mpg, A)
    runs = {hat: pv.np_solve_prec_values(mpg, A, b, prec, steps, hat) for hat in (False, True)}
    print(name, prec, steps, {("f16" if k else "f32"): (r["status"], r["restarts"], r["total_iters"]) for k, r in runs.items()})
    assert all(r["status"] == "converged" for r in runs.values())
    assert runs[True]["restarts"] == runs[False]["restarts"]
    assert pv.COUNTS[(name, prec, steps)] == runs[False]["restarts"]
    # ... and the rounding was there: the two runs are not the same run
    assert not np.array_equal(runs[True]["step_res"], runs[False]["step_res"])


# ---------------------------------------------------------------- the keyword and the ABI
def test_make_args_carries_the_keyword(mpg):
    """mpg_solve_args does not change: the keyword rides on the structure and
    becomes MPG_PREC_VALUES around the creating call only, beside MPG_BASIS."""
    from mpgmres_amd import _basis_setting

    A = mpg.gen_laplace3d(3)
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec_values="f16", basis="f16")
    assert a._prec_values == "f16"
    a0, keep0 = mpg.make_args(A, np.ones(A.nrows))
    assert a0._prec_values is None
    before = os.environ.get("MPG_PREC_VALUES"), os.environ.get("MPG_BASIS")
    with _basis_setting(a):
        assert os.environ["MPG_PREC_VALUES"] == "f16" and os.environ["MPG_BASIS"] == "f16"
    assert (os.environ.get("MPG_PREC_VALUES"), os.environ.get("MPG_BASIS")) == before
    with _basis_setting(a0):
        assert (os.environ.get("MPG_PREC_VALUES"), os.environ.get("MPG_BASIS")) == before


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for name in ("mpg_arnoldi_set_prec_copy", "mpg_arnoldi_prec_values"):
        assert ("arnoldi.h", name) in declared, name
        assert hasattr(mpg.hip_lib(), name)
    for st in ("csr", "sell"):
        for kind in ("jacobi", "cheb", "poly"):
            name = f"mpg_{st}_{kind}_sweep_f16f32"
            assert ("capi.h", name) in declared, name
            assert hasattr(mpg.hip_lib(), name)
    assert ("capi.h", "mpg_csr_half_dequant_f32") in declared
    assert ("solve.h", "mpg_engine_prec_values") in declared
    assert hasattr(mpg.host_lib(), "mpg_engine_prec_values")


def test_null_arguments_are_refused(mpg):
    hip = mpg.hip_lib()
    assert hip.mpg_arnoldi_set_prec_copy(None, 1, None, None, None) == -2
    assert hip.mpg_arnoldi_prec_values(None) == -2
    assert mpg.host_lib().mpg_engine_prec_values(None) == -2
    assert hip.mpg_csr_jacobi_sweep_f16f32(None, None, None, None, None, None, None, None) == -2
    assert hip.mpg_sell_jacobi_sweep_f16f32(None, None, None, None, None, None, None) == -2
    assert hip.mpg_csr_half_dequant_f32(None, None, None, None, None, None) == -2


def test_cli_flags_list_names_the_flag():
    """The CLI's list of flags (the head of its source, where every flag is described) names --prec-values."""
    src = os.path.join(os.path.dirname(os.path.dirname(__file__)), "icl-mixed-precision-gmres_amd", "host",
                       "gmres_perf_test.cpp")
    head = open(src).read().split("#include", 1)[0]
    assert "--prec-values {f32,f16,f16emu}" in head
