"""The Arnoldi SpMV inside the panel dots' launch (k_step_dots,
mpg_arnoldi_step_dots; MPG_STEP_DOTS).

The one launch runs on the dots' grid: a 1024-lane workgroup forms its own
4096 rows of w and v_k with k_step_sell2's row sums, leaves them in LDS and
runs dots_panel's arithmetic on them, so the step's bits are those of the two
launches it replaces. Every case here is BAND (gen_band(n, 5, 4, seed=7)),
tol = 0, two restart cycles, and compares MPG_STEP_DOTS=2 (required: an
unsupported step is an error, so the launch provably ran) or =1 (wherever
supported) against =0 with array_equal.

The fp64 accumulation class is not built (mpg_arnoldi_step_dots returns
MPG_ERR_UNSUPPORTED under it), and neither is a second pass over the row
blocks (n > 1,048,576 is refused): both are checked as refusals.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5  # MPG_ERR_UNSUPPORTED (include/mpgmres/capi.h)
_PROBLEMS = {}


def _problem(mpg, n):
    if n not in _PROBLEMS:
        A = mpg.gen_band(n, 5, 4, seed=7)
        xt = mpg.rand_vect(A.nrows, 42)
        _PROBLEMS[n] = (A, xt, mpg.host_spmv(A, xt))
    return _PROBLEMS[n]


def _run(mpg, monkeypatch, n, step_dots, cycles=2, want_fused=None, **opts):
    """`cycles` restart cycles of the fused engine under MPG_STEP_DOTS=step_dots:
    (report, spmv_layout)."""
    A, xt, b = _problem(mpg, n)
    monkeypatch.setenv("MPG_STEP_DOTS", str(step_dots))
    kw = dict(mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=cycles, accum="f32")
    kw.update(opts)
    eng = mpg.Engine(A, b, xt, **kw)
    try:
        lay = eng.spmv_layout()
        if want_fused is not None:
            assert lay.get("dots_fused", 0) == want_fused, lay
        eng.run(cycles)
        eng.sync()
        return eng.report(), lay
    finally:
        eng.close()


def _same(a, b, what):
    for f in ("x", "step_res", "cyc_r_norm"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    assert a.res_norm == b.res_norm, (what, a.res_norm, b.res_norm)
    assert np.all(np.isfinite(a.x)) and np.isfinite(a.res_norm), what


# 12: one partial slice; 132: a pair plus a 4-row slice, dead waves; 4096: one
# full block; 4100: the second workgroup owns 4 rows; 13,316 = 3 * 4096 + 1028:
# an odd slice count, a last slice of 4 rows, a partial last block
@pytest.mark.parametrize("fold", ["0", "1"])
@pytest.mark.parametrize("prec", ["identity", "jacobi"])
@pytest.mark.parametrize("mode", ["mixed", "single"])
@pytest.mark.parametrize("rlen", [30, 32])
@pytest.mark.parametrize("n", [12, 132, 4096, 4100, 13_316])
def test_same_bits_as_split(mpg, monkeypatch, n, rlen, mode, prec, fold):
    """x, the per-step residuals, the cycles' true residuals and the final
    residual of the one-launch steps are those of the split launches, and
    every step of the cycle took the one launch (rlen 32: NC = 31 and 32, the
    panel's last columns)."""
    monkeypatch.setenv("MPG_FOLD_GIVENS", fold)
    opts = dict(mode=mode, prec=prec, rlen=rlen, spmv_format="sell")  # (auto leaves the smallest to CSR)
    ref, lay0 = _run(mpg, monkeypatch, n, 0, want_fused=0, **opts)
    got, lay = _run(mpg, monkeypatch, n, 2, want_fused=rlen, **opts)
    assert lay["dots_fused"] and "dots_fused" not in lay0
    assert lay["accum"] == "f32" and lay["givens_folded"] == (fold == "1")
    assert ref.total_iters == 2 * rlen and got.total_iters == 2 * rlen
    _same(got, ref, (n, rlen, mode, prec, fold))


CASES = {
    "tail-rows": (13_318, {}, 0),            # n % 4 == 2: dots_panel's tail rows
    "csr": (13_316, {"spmv_format": "csr"}, 0),
    "mgs": (13_316, {"orth": "mgs"}, 0),
    "past-32-columns": (13_316, {"rlen": 40}, 32),  # steps with k + 1 > 32 stay split
    "accum-f64": (13_316, {"accum": "f64"}, 0),     # the class is not built
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fallback_and_refusal(mpg, monkeypatch, case):
    """Where the one launch does not apply, =1 runs the split launches (the
    bits of =0) and =2 is an error."""
    n, opts, fused = CASES[case]
    ref, _ = _run(mpg, monkeypatch, n, 0, want_fused=0, **opts)
    got, _ = _run(mpg, monkeypatch, n, 1, want_fused=fused, **opts)
    assert got.total_iters == ref.total_iters == 2 * opts.get("rlen", 30)
    _same(got, ref, case)
    with pytest.raises(RuntimeError):
        _run(mpg, monkeypatch, n, 2, **opts)


def test_more_than_one_pass_is_refused(mpg, monkeypatch):
    """n > 4096 * 256 rows would need a second pass over the row blocks,
    which is not built: the launch's support check says so (no solve)."""
    monkeypatch.setenv("MPG_STEP_DOTS", "1")
    n = 1_048_576 + 4096
    A, xt, b = _problem(mpg, n)
    del _PROBLEMS[n]
    eng = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=1,
                     accum="f32")
    try:
        assert eng.step_dots_status(0) == UNSUPPORTED and eng.step_dots_status(29) == UNSUPPORTED
        assert "dots_fused" not in eng.spmv_layout()
    finally:
        eng.close()


def test_measurement_hooks(mpg, monkeypatch):
    """With every step on the one launch, the duplicate-launch timing of the
    SpMV phase doubles that launch (rlen added launches, a positive time), the
    update's works around it, and the cycle has no dots launch to time."""
    A, xt, b = _problem(mpg, 13_316)
    monkeypatch.setenv("MPG_STEP_DOTS", "1")
    eng = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=50,
                     accum="f32")
    try:
        assert eng.spmv_layout()["dots_fused"] == 30
        eng.run(1)
        ms, launches = eng.time_phase_dup("spmv", 5)
        assert ms > 0 and launches == 30
        with pytest.raises(RuntimeError, match="no launch of that phase"):
            eng.time_phase_dup("dots", 5)
        ms_u, launches_u = eng.time_phase_dup("cgs_update", 5)
        assert np.isfinite(ms_u) and launches_u == 30
        # bytes of the cycle as run: the basis columns the dots read moved into the SpMV phase's launch
        n, m = A.nrows, 30
        cols = sum(range(m)) / m * n * 4
        monkeypatch.setenv("MPG_STEP_DOTS", "0")
        split = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=50,
                           accum="f32")
        try:
            assert eng.phase_bytes("dots") == 0.0
            assert eng.phase_bytes("spmv_storage") == pytest.approx(split.phase_bytes("spmv_storage") + cols, rel=1e-12)
            assert split.phase_bytes("dots") == pytest.approx(cols + 2 * n * 4, rel=1e-12)
        finally:
            split.close()
    finally:
        eng.close()


def test_cycle_policy_of_live_engines(mpg, monkeypatch):
    """The resolved policy of a default engine (mpg_engine_cycle_policy): the
    fp32 class may take the one launch at every step of BAND's cycle and folds
    the Givens step, the fp64 class may take it at none; and the plan that
    policy describes holds as many SpMV + dots launches as the layout reports."""
    import ctypes as C
    for var in ("MPG_STEP_DOTS", "MPG_STEP_DOTS_LO", "MPG_STEP_DOTS_HI", "MPG_FOLD_GIVENS"):
        monkeypatch.delenv(var, raising=False)
    A, xt, b = _problem(mpg, 13_316)
    for accum in ("f32", "f64"):
        eng = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=1,
                         accum=accum)
        try:
            p = eng.cycle_policy()
            assert (p.m, p.ranks, p.orth, p.step_dots) == (30, 0, 0, -1)
            if accum == "f32":
                assert all(p.step_dots_ok[k] == 1 for k in range(30)) and p.fold == 1
            else:
                assert not any(p.step_dots_ok)
            buf = C.create_string_buffer(1 << 14)
            assert 0 < mpg.host_lib().mpg_cycle_plan_describe(C.byref(p), buf, len(buf)) < len(buf)
            plan = buf.value.decode().split(" ")
            fused = sum(t.startswith("step_dots(") for t in plan)
            assert fused == eng.spmv_layout().get("dots_fused", 0) == (30 if accum == "f32" else 0)
        finally:
            eng.close()
