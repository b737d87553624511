"""prec="bjacobi" at the ABI level (CPU only: nothing here launches a kernel)."""
import ctypes as C

import numpy as np

# mpg_solve_args before prec_block was appended (include/mpgmres/solve.h): the
# layout the oracle is compiled against
FIELDS_BEFORE = [
    ("n", C.c_int32), ("nnz", C.c_int64), ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p),
    ("b", C.c_void_p), ("x_true", C.c_void_p), ("mode", C.c_int32), ("orth", C.c_int32), ("prec", C.c_int32),
    ("engine", C.c_int32), ("rlen", C.c_int32), ("tol", C.c_double), ("max_restarts", C.c_int64),
    ("rtol", C.c_double), ("repeat_iter", C.c_int32), ("orthloss", C.c_int32), ("jacobi_steps", C.c_int32),
    ("verbose", C.c_int32), ("device", C.c_int32), ("threads", C.c_int32), ("spmv_format", C.c_int32),
    ("half_unscaled", C.c_int32), ("stop_on_breakdown", C.c_int32), ("accum", C.c_int32),
]


class ArgsBefore(C.Structure):
    _fields_ = FIELDS_BEFORE


def test_make_args_fills_the_struct(mpg):
    A = mpg.gen_stencil27(2, dof=4)
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec="bjacobi", prec_block=4)
    assert a.prec == 4 and a.prec_block == 4
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec="bjacobi")
    assert a.prec == 4 and a.prec_block == 3
    a, keep = mpg.make_args(A, np.ones(A.nrows), prec="jacobi")
    assert a.prec == 2


def test_struct_grew_by_the_appended_field_only(mpg):
    from mpgmres_amd._abi import SolveArgs

    names = [f for f, _ in SolveArgs._fields_]
    assert names == [f for f, _ in FIELDS_BEFORE] + ["prec_block"]
    for f, _ in FIELDS_BEFORE:
        assert getattr(SolveArgs, f).offset == getattr(ArgsBefore, f).offset, f
        assert getattr(SolveArgs, f).size == getattr(ArgsBefore, f).size, f
    # accum ended the struct on a 4-byte boundary inside its 8-byte alignment:
    # the new int32 takes that tail or one more aligned word, nothing else
    assert SolveArgs.prec_block.offset == ArgsBefore.accum.offset + 4
    assert SolveArgs.prec_block.offset >= C.sizeof(ArgsBefore) - 4
    assert C.sizeof(SolveArgs) in (C.sizeof(ArgsBefore), C.sizeof(ArgsBefore) + 8)
    assert C.sizeof(SolveArgs) == (SolveArgs.prec_block.offset + 4 + 7) // 8 * 8


def test_new_symbols_are_declared_in_capi_h(mpg):
    declared = set(mpg.exported_capi_symbols())
    for name in ("mpg_bjacobi_setup_f64", "mpg_bjacobi_setup_f32", "mpg_bjacobi_apply_f64", "mpg_bjacobi_apply_f32",
                 "mpg_bjacobi_apply_f64_p32"):
        assert ("capi.h", name) in declared, name
        assert hasattr(mpg.hip_lib(), name)
    assert ("solve.h", "mpg_engine_prec_fused") in declared


def test_refused_without_a_gpu_where_possible(mpg):
    """The kernel-level argument checks come before any device work."""
    hip = mpg.hip_lib()
    assert hip.mpg_bjacobi_apply_f32(None, 24, 3, None, None) == -2
    assert hip.mpg_bjacobi_setup_f64(None, None, None, 3, None, None) == -2
