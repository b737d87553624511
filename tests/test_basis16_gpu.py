"""The compressed Krylov basis (basis="f16": V holds fp16_rne(2^14 v), all
arithmetic in the Arnoldi precision; csrc/basis.hpp) on the GPU.

The emulated form basis="f16emu" stores the same rounded values as fp32 and
runs the fp32 panel kernels on them, so every comparison of the compressed
kernels is array_equal: the stored bits against NumPy's fp16 cast, the SpMV
against the fp32 workspace's on the rounded vector, whole solves against the
emulation. That the rounding happens and is the stated one is checked against
the NumPy restatement (tests/basis16_np.py, tests/test_basis16_cpu.py)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import basis16_np as B16
from tests import parity
from tests.golden.make_golden import convdiff
from tests.test_basis16_cpu import FAST_CASE, SLOW_CASE, SPECIALS
from tests.test_cli_gpu import SUMMARY
from tests.test_cycle_plan import describe, names
from tests.test_neumann_gpu import Workspace

pytestmark = pytest.mark.gpu

F32 = np.float32
BASIS_F32, BASIS_F16, BASIS_F16EMU = 0, 1, 2
UNSUPPORTED = -5
CSR, SELL = 1, 2


# ---------------------------------------------------------------- helpers
def _band(mpg, n):
    return mpg.gen_band(n, 5, 4, seed=7)


def _vector(n, seed=3):
    """Entries of an Arnoldi vector's size with the CPU test's special values among them."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n) * np.exp2(rng.uniform(-30.0, 0.0, n))).astype(F32)
    at = rng.choice(n, SPECIALS.size, replace=False)
    w[at] = SPECIALS
    w[n - 1], w[n - 2] = F32(2051.0 / 16384), F32(-2.0 ** -38)  # the last rows (n mod 4, n mod 64)
    return w


def _workspace(mpg, hip, A, fmt, accum, basis):
    W = Workspace(mpg, hip, A, "f32", fmt, accum)
    assert W.format == fmt, W.format
    if basis:
        hip.check(hip.lib.mpg_arnoldi_set_basis(W.arn, basis), "set_basis")
    assert hip.lib.mpg_arnoldi_basis(W.arn) == basis
    return W


def _column(hip, W, k, dtype):
    """Column k of the workspace's basis, n entries read as dtype."""
    ld = C.c_int64()
    V = hip.lib.mpg_arnoldi_basis_dev(W.arn, C.byref(ld))
    out = np.empty(W.n, dtype)
    hip.check(hip.lib.mpg_memcpy_d2h(hip.ctx, out.ctypes.data, C.c_void_p(V + k * ld.value * out.itemsize), out.nbytes))
    return out, ld.value


def _spmv_folded(hip, W, x):
    """Step 1 with the Givens step folded in (mpg_arnoldi_givens_spmv): ||w||^2 = 1
    in sums[0], so inv = 1 and V(:,1) receives round(x); returns w = A round(x)."""
    lib = hip.lib
    x = np.ascontiguousarray(x, F32)
    one = np.ones(1, np.float64)
    hip.check(lib.mpg_memcpy_h2d(hip.ctx, lib.mpg_arnoldi_sums_dev(W.arn), one.ctypes.data, 8))
    hip.check(lib.mpg_memcpy_h2d(hip.ctx, lib.mpg_arnoldi_wprev_dev(W.arn, 1), x.ctypes.data, x.nbytes))
    hip.check(lib.mpg_arnoldi_givens_spmv(W.arn, 1), "givens_spmv")
    y = np.empty(W.n, F32)
    hip.check(lib.mpg_memcpy_d2h(hip.ctx, y.ctypes.data, lib.mpg_arnoldi_wprev_dev(W.arn, 0), y.nbytes))
    return y


STORAGES = {"csr": (CSR, None), "sell-pair": (SELL, None), "sell-one": (SELL, "0")}


def _storage(monkeypatch, storage):
    fmt, pair = STORAGES[storage]
    if pair is not None:
        monkeypatch.setenv("MPG_SELL_PAIR", pair)
    return fmt


# ---------------------------------------------------------------- 1. stored bits, 2. the SpMV consumes v^
@pytest.mark.parametrize("accum", [0, 1], ids=["acc64", "acc32"])
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("n", [4100, 4099, 4103])
@pytest.mark.parametrize("storage", list(STORAGES))
def test_stored_bits_and_spmv(mpg, hip, monkeypatch, storage, n, fold, accum):
    fmt = _storage(monkeypatch, storage)
    A = _band(mpg, n)
    w = _vector(n)
    want = B16.pack_f16(w)
    assert np.array_equal(want, np.float16(np.float32(w) * np.float32(16384)).view(np.uint16))
    W16 = _workspace(mpg, hip, A, fmt, accum, BASIS_F16)
    W32 = _workspace(mpg, hip, A, fmt, accum, BASIS_F32)
    try:
        if fmt == SELL:  # the kernel under test: two slices per wave or one
            spw = hip.lib.mpg_arnoldi_slices_per_wave(W16.arn)
            print(storage, n, "slices per wave", spw)
            # (n = 4099 ends in a slice of 3 short rows: not the uniform copy the pair kernel takes, it runs
            # one slice per wave either way; 4103 is the pair kernel's n mod 4 = 3)
            assert spw == (2 if storage == "sell-pair" and n != 4099 else 1)
        k = 1 if fold else 0
        run = (lambda W, x: _spmv_folded(hip, W, x)) if fold else (lambda W, x: W.spmv(x))
        y16 = run(W16, w)
        bits, ld = _column(hip, W16, k, np.uint16)
        assert ld % 128 == 0 and ld >= n
        bad = np.flatnonzero(bits != want)
        print("stored bits differing:", [(int(i), float(w[i]), hex(bits[i]), hex(want[i])) for i in bad[:8]])
        # the whole column, the NaN included (v_cvt_f16_f32 stores NumPy's quiet NaN, 0x7e00)
        assert np.isnan(w).sum() == 1
        assert np.array_equal(bits, want), int(np.sum(bits != want))
        # 2. w = A v^: the fp32 workspace's SpMV of the rounded vector (finite entries: the
        # products of a non-finite one are NaN in both, compared as such)
        y32 = run(W32, B16.round_f16(w))
        col32, ld32 = _column(hip, W32, k, F32)
        assert ld32 % 64 == 0
        assert np.array_equal(col32, B16.round_f16(w), equal_nan=True)
        assert np.array_equal(y16, y32, equal_nan=True), int(np.sum(y16 != y32))
        fin = np.isfinite(y16)
        assert fin.sum() > n - 64 and np.any(y16[fin] != 0)
        # the raw vector gives other bits: the rounding is in the operator, not only in the store
        assert not np.array_equal(y16, run(W32, w), equal_nan=True)
    finally:
        W16.close()
        W32.close()


def test_emulated_spmv_is_the_compressed_one(mpg, hip):
    """f16emu (CSR): the same w, and V holds the rounded values as fp32."""
    A = _band(mpg, 4099)
    w = _vector(4099, seed=5)
    for accum in (0, 1):
        We = _workspace(mpg, hip, A, CSR, accum, BASIS_F16EMU)
        Wh = _workspace(mpg, hip, A, CSR, accum, BASIS_F16)
        try:
            assert np.array_equal(We.spmv(w), Wh.spmv(w), equal_nan=True)
            col, _ = _column(hip, We, 0, F32)
            assert np.array_equal(col, B16.round_f16(w), equal_nan=True)
            assert np.array_equal(_spmv_folded(hip, We, w), _spmv_folded(hip, Wh, w), equal_nan=True)
        finally:
            We.close()
            Wh.close()


def test_workspace_refusals(mpg, hip):
    """Phase entry points without a compressed form answer MPG_ERR_UNSUPPORTED; so does
    set_basis on a workspace it is not built for."""
    lib = hip.lib
    A = _band(mpg, 4100)
    W = _workspace(mpg, hip, A, SELL, 1, BASIS_F16)
    try:
        for name, args in (("mpg_arnoldi_mgs", (0, 0)), ("mpg_arnoldi_mgs_partials", (0, 0)),
                           ("mpg_arnoldi_spmv_dots", (0, 0)), ("mpg_arnoldi_spmv_dots_supported", (0,)),
                           ("mpg_arnoldi_step_dots", (0, 0)),
                           ("mpg_arnoldi_step_dots_supported", (0,)), ("mpg_arnoldi_update_tail", (4, 0)),
                           ("mpg_arnoldi_update_tail_supported", ()), ("mpg_arnoldi_cgs_stream_at", (0,)),
                           ("mpg_arnoldi_dots_sums", (0,)), ("mpg_arnoldi_cgs_givens", (0, 0)),
                           ("mpg_arnoldi_cgsr_wide_pass", (0, 0))):
            fn = getattr(lib, name)
            fn.argtypes = [C.c_void_p] + [C.c_int] * len(args)
            fn.restype = C.c_int
            assert fn(W.arn, *args) == UNSUPPORTED, name
        assert lib.mpg_arnoldi_set_basis(W.arn, 7) == -2
        # set once: the same value again is accepted, a change is not
        assert lib.mpg_arnoldi_set_basis(W.arn, BASIS_F16) == 0 and lib.mpg_arnoldi_set_basis(W.arn, BASIS_F32) == -2
        assert lib.mpg_arnoldi_basis(W.arn) == BASIS_F16
    finally:
        W.close()
    W = Workspace(mpg, hip, A, "f32", SELL, 0)
    try:  # the emulation is built for the CSR kernel
        assert lib.mpg_arnoldi_set_basis(W.arn, BASIS_F16EMU) == UNSUPPORTED
        assert lib.mpg_arnoldi_basis(W.arn) == BASIS_F32
    finally:
        W.close()
    W = Workspace(mpg, hip, mpg.gen_stencil27(5), "f32", 3, 0)  # node blocks
    try:
        assert W.format == 3 and lib.mpg_arnoldi_set_basis(W.arn, BASIS_F16) == UNSUPPORTED
    finally:
        W.close()
    W = Workspace(mpg, hip, A, "f64", CSR, 0)  # an fp64 Arnoldi
    try:
        assert lib.mpg_arnoldi_set_basis(W.arn, BASIS_F16) == UNSUPPORTED
    finally:
        W.close()


# ---------------------------------------------------------------- 3. f16 against f16emu, whole solves on CSR
MATRICES = {
    "band4100": lambda m: _band(m, 4100),
    "band4099": lambda m: _band(m, 4099),
    "band8196": lambda m: _band(m, 8196),
    "lap12": lambda m: m.gen_laplace3d(12),
    "convdiff32": lambda m: convdiff(m, 32),
}
_PROBLEMS = {}


def _problem(mpg, name):
    if name not in _PROBLEMS:
        A = MATRICES[name](mpg)
        xt = mpg.rand_vect(A.nrows, 42)
        _PROBLEMS[name] = (A, mpg.host_spmv(A, xt), xt)
    return _PROBLEMS[name]


def _same(a, b, label):
    assert a.status == b.status and a.restarts == b.restarts and a.total_iters == b.total_iters, label
    assert np.array_equal(a.step_res, b.step_res, equal_nan=True), label
    assert np.array_equal(a.cyc_r_norm, b.cyc_r_norm, equal_nan=True), label
    assert np.array_equal(a.x, b.x, equal_nan=True), label


PRECS = {"identity": dict(prec="identity"), "jacobi": dict(prec="jacobi"),
         "chebyshev": dict(prec="chebyshev", jacobi_steps=3)}


@pytest.mark.parametrize("rlen", [1, 4, 30, 32])
@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
@pytest.mark.parametrize("accum", ["f32", "f64"])
@pytest.mark.parametrize("matrix", list(MATRICES))
def test_f16_equals_emulation(mpg, matrix, accum, orth, prec, rlen):
    A, b, xt = _problem(mpg, matrix)
    opts = dict(mode="mixed", orth=orth, rlen=rlen, tol=1e-10, max_restarts=12, accum=accum, spmv_format="csr",
                engine="fused", **PRECS[prec])
    got = mpg.solve(A, b, xt, basis="f16", **opts)
    emu = mpg.solve(A, b, xt, basis="f16emu", **opts)
    _same(got, emu, (matrix, accum, orth, prec, rlen))
    assert got.total_iters > 0 and np.all(np.isfinite(got.x))


def test_f16_equals_emulation_past_one_pass(mpg):
    """n > 4096 * 256 rows: the dots, the update and the solution update take a second
    grid-stride pass, where an index in 8-byte units could go wrong."""
    n = 1_048_576 + 4_100
    A = _band(mpg, n)
    xt = mpg.rand_vect(n, 42)
    b = mpg.host_spmv(A, xt)
    for orth in ("cgs", "cgsr"):
        opts = dict(mode="mixed", orth=orth, prec="jacobi", rlen=3, tol=0.0, max_restarts=2, accum="f32",
                    spmv_format="csr", engine="fused")
        _same(mpg.solve(A, b, xt, basis="f16", **opts), mpg.solve(A, b, xt, basis="f16emu", **opts), orth)


# ---------------------------------------------------------------- 4. SELL against CSR under f16
@pytest.mark.parametrize("matrix", ["band8196", "lap12"])
def test_f16_storage_forms(mpg, matrix):
    """As tests/test_accum32_gpu.py compares the forms for the fp32 basis: in the fp32
    class the SELL and CSR SpMVs give one another's bits, so cycle 0's step history is
    the same (from the first restart on the fp64 prologues differ)."""
    A, b, xt = _problem(mpg, matrix)
    opts = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=0.0, max_restarts=3, accum="f32", basis="f16",
                engine="fused")
    got = {f: mpg.solve(A, b, xt, spmv_format=f, **opts) for f in ("csr", "sell")}
    np.testing.assert_array_equal(got["sell"].step_res[:30], got["csr"].step_res[:30])
    auto = mpg.solve(A, b, xt, **opts)  # auto picks one of the two
    assert any(np.array_equal(auto.x, got[f].x) for f in got)


# ---------------------------------------------------------------- 5. the rounding happens and is the stated one
def test_emulation_differs_from_f32(mpg):
    A, b, xt = _problem(mpg, "lap12")
    opts = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-10, accum="f64", spmv_format="csr",
                engine="fused")
    emu, f32 = mpg.solve(A, b, xt, basis="f16emu", **opts), mpg.solve(A, b, xt, basis="f32", **opts)
    assert not np.array_equal(emu.x, f32.x) and not np.array_equal(emu.step_res[:30], f32.step_res[:30])
    # the keyword's default is the f32 basis
    _same(f32, mpg.solve(A, b, xt, **opts), "default")


@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
@pytest.mark.parametrize("case", [SLOW_CASE, FAST_CASE], ids=["slow", "fast"])
def test_numpy_counts_and_parity(mpg, case, orth):
    """The CPU test's recorded cases: the GPU gives the restatement's cycle counts under
    both storages, and passes parity.compare() against a record made from the restatement
    with the project's own fp32-Arnoldi tolerances."""
    nx = {"lap16": 16, "lap10": 10}[case["matrix"]]
    A = mpg.gen_laplace3d(nx)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    opts = dict(mode="mixed", orth=orth, prec="jacobi", rlen=case["rlen"], tol=1e-10)
    for basis, cycles in (("f32", case["cycles_f32"]), ("f16", case["cycles_f16"])):
        ref = B16.solve(A, b, xt, orth=orth, prec="jacobi", rlen=case["rlen"], tol=1e-10, basis=basis)
        assert ref["restarts"] == cycles
        for accum in ("f64", "f32"):
            got = mpg.solve(A, b, xt, engine="fused", accum=accum, basis=basis, **opts)
            print(case["matrix"], orth, basis, accum, "cycles", got.restarts, "numpy", ref["restarts"])
            assert got.status == "converged" and got.restarts == cycles, (basis, accum, got.restarts)
            parity.compare(ref, got, "mixed", 1e-10, case["rlen"], f"{case['matrix']}/{orth}/{basis}/{accum}")


# ---------------------------------------------------------------- 6. reports and plan
FUSED = ("step_dots", "spmv_dots", "givens+update", "dots_sums", "cgs_givens")


def test_reports_and_plan(mpg):
    A, b, xt = _problem(mpg, "band8196")
    n, m = A.nrows, 30
    opts = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=m, tol=0.0, max_restarts=2, accum="f32")
    lay, plan, nbytes = {}, {}, {}
    for basis in (None, "f32", "f16", "f16emu"):
        e = mpg.Engine(A, b, xt, basis=basis, **opts)
        try:
            lay[basis] = e.spmv_layout()
            plan[basis] = names(describe(mpg, e.cycle_policy()))
            nbytes[basis] = {p: e.phase_bytes(p) for p in ("dots", "cgs_update", "spmv_storage", "spmv")}
            assert e.run(2)[0] == 2
        finally:
            e.close()
    assert lay[None]["basis"] == lay["f32"]["basis"] == "f32"
    assert lay["f16"]["basis"] == "f16" and lay["f16emu"]["basis"] == "f16emu"
    assert lay["f16"]["format"] == "sell" and lay["f16emu"]["format"] == "csr"  # auto: CSR or SELL; the emulation CSR
    for key in ("dots_fused", "cgs_stream", "tail_fold", "givens_rider"):
        assert key not in lay["f16"] and key not in lay["f16emu"], key
    # the default engine keeps the plan and the layout it has today (the fp32 class: fused forms)
    assert plan[None] == plan["f32"] and lay[None] == lay["f32"]
    assert "tail_fold" in lay[None] and "cgs_stream" in lay[None] and "givens+update(30,1)" in plan[None]
    for basis in ("f16", "f16emu"):
        assert not any(t.startswith(FUSED) for t in plan[basis]), plan[basis]
        assert plan[basis].count("update(30)") == 1 and sum(t.startswith("dots(") for t in plan[basis]) == m
    # V at 2 bytes: dots (mean k + 1 columns at 2 B, w at 4 B), update (mean columns at 2 B, w read + written)
    cols = (m + 1) / 2.0
    assert nbytes["f16"]["dots"] == cols * n * 2 + n * 4
    assert nbytes["f16"]["cgs_update"] == ((m - 1) / 2.0 + 1) * n * 2 + 2 * n * 4
    assert nbytes["f16emu"]["dots"] == cols * n * 4 + n * 4
    assert nbytes["f16emu"]["cgs_update"] == ((m - 1) / 2.0 + 1) * n * 4 + 2 * n * 4
    assert nbytes["f16"]["spmv"] == nbytes["f32"]["spmv"]


def test_plain_plan_is_the_f32_plain_plan(mpg, monkeypatch):
    A, b, xt = _problem(mpg, "band8196")
    opts = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=0.0, max_restarts=2, accum="f32")
    e = mpg.Engine(A, b, xt, basis="f16", **opts)
    try:
        got = names(describe(mpg, e.cycle_policy()))
    finally:
        e.close()
    for k, v in (("MPG_STEP_DOTS", "0"), ("MPG_CGS_PREFETCH", "0"), ("MPG_TAIL_FOLD", "0")):
        monkeypatch.setenv(k, v)
    e = mpg.Engine(A, b, xt, **opts)
    try:
        assert names(describe(mpg, e.cycle_policy())) == got
    finally:
        e.close()
    # ... whatever the variables say, short of asking for a fused form
    e = mpg.Engine(A, b, xt, basis="f16", **opts)
    try:
        assert names(describe(mpg, e.cycle_policy())) == got
    finally:
        e.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(mpg, monkeypatch):
    A, b, xt = _problem(mpg, "lap12")
    base = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-10, engine="fused", basis="f16")

    def refused(words, call=mpg.solve, **kw):
        with pytest.raises(RuntimeError, match=r"\(-5\)") as ei:
            call(A, b, xt, **{**base, **kw})
        for w in words:
            assert w in str(ei.value), (w, str(ei.value))

    for mode in ("baseline", "single-prec", "single", "mixed-half"):
        refused(["basis f16", "mode mixed"], mode=mode)
    refused(["basis f16", "mgs", "MGS"], orth="mgs")
    refused(["basis f16", "rlen <= 32", "33"], rlen=33)
    refused(["basis f16", "orthloss"], orthloss=True, rtol=1e-3)
    refused(["basis f16", "node"], spmv_format="node")
    refused(["basis f16", "operator-surface"], engine="surface")
    refused(["basis f16emu", "CSR"], basis="f16emu", spmv_format="sell")
    refused(["basis f16", "row-partitioned"], call=lambda *a, **k: mpg.solve_loopback(*a, nranks=2, **k))
    refused(["basis f16", "row-partitioned"], call=lambda *a, **k: mpg.solve_multi_gpu(*a, ngpus=1, **k))
    # a value that is none of the three: MPG_ERR_ARG naming it
    with pytest.raises(RuntimeError, match=r"\(-2\).*MPG_BASIS = f8"):
        mpg.solve(A, b, xt, **{**base, "basis": "f8"})
    # asking for a fused form explicitly
    for var, val in (("MPG_STEP_DOTS", "2"), ("MPG_CGS_PREFETCH", "1"), ("MPG_TAIL_FOLD", "1"), ("MPG_FUSE_DOTS", "1"),
                     ("MPG_FUSE_DOTS", "2")):
        monkeypatch.setenv(var, val)
        refused(["basis f16", f"{var}={val}"], accum="f32")
        monkeypatch.delenv(var)
    # the context still solves afterwards, with and without the option
    ok = mpg.solve(A, b, xt, **base)
    assert ok.status == "converged"
    assert mpg.solve(A, b, xt, **{**base, "basis": "f32"}).status == "converged"


def test_rtol_strategy_equals_emulation(mpg):
    """The stepwise (rtol) strategy runs unchanged: the same launches one step at a time."""
    A, b, xt = _problem(mpg, "lap12")
    opts = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-10, rtol=1e-2, engine="fused",
                spmv_format="csr")
    _same(mpg.solve(A, b, xt, basis="f16", **opts), mpg.solve(A, b, xt, basis="f16emu", **opts), "rtol")


# ---------------------------------------------------------------- 8. CLI
def test_cli_basis_flag(mpg):
    args = [str(mpg.CLI), "--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec",
            "jacobi", "--tol", "1e-9", "--gpu"]
    out = subprocess.run(args + ["--basis", "f16"], capture_output=True, text=True, timeout=120, check=True).stdout
    m = SUMMARY.search(out)
    assert m and "Doing Mixed Precision test" in out and out.startswith("||x|| = "), out
    assert float(m.group(1)) <= 1e-9 and int(m.group(4)) % 30 == 0
    A = mpg.gen_spec("laplace:12")
    xt = mpg.rand_vect(A.nrows, 42)
    got = mpg.solve(A, mpg.host_spmv(A, xt), xt, engine="fused", mode="mixed", orth="cgs", prec="jacobi", rlen=30,
                    tol=1e-9, basis="f16")
    assert int(m.group(4)) == got.total_iters
    ref = SUMMARY.search(subprocess.run(args + ["--basis", "f32"], capture_output=True, text=True, timeout=120,
                                        check=True).stdout)
    assert ref and SUMMARY.search(subprocess.run(args, capture_output=True, text=True, timeout=120,
                                                 check=True).stdout).group(4) == ref.group(4)
    r = subprocess.run(args + ["--basis", "f8"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and re.search(r"MPG_BASIS = f8", r.stdout + r.stderr)
