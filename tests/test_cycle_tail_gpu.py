"""The cycle's tail in one launch (k_update_tail_nc, mpg_arnoldi_update_tail;
MPG_TAIL_FOLD): Givens step m-1, update(m) and the x snapshot.

MPG_TAIL_FOLD=0 -- givens_partials(m-1), update(m) and the snapshot copy as
launches of their own -- is the reference. Every comparison is array_equal on
x, the per-step residuals and the cycles' histories: a column added out of
order, a neighbour's slot or a rotation applied to the wrong entry would
still give finite numbers, so nothing weaker would see it. Unset, the form is
taken in the fp32 accumulation class; the fp64 class takes it under =1.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def _problem(mpg, key):
    if key not in _PROBLEMS:
        A = mpg.gen_laplace3d(12) if key == "lap12" else mpg.gen_band(key, 5, 4, seed=7)
        xt = mpg.rand_vect(A.nrows, 42)
        _PROBLEMS[key] = (A, xt, mpg.host_spmv(A, xt))
    return _PROBLEMS[key]


def _plan_text(mpg, eng):
    p = eng.cycle_policy()
    lib = mpg.host_lib()
    need = lib.mpg_cycle_plan_describe(C.byref(p), None, 0)
    buf = C.create_string_buffer(need + 1)
    assert lib.mpg_cycle_plan_describe(C.byref(p), buf, need + 1) == need
    return buf.value.decode().split(" ")


def _env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _run(mpg, monkeypatch, key, tail, cycles=2, keep=True, env=None, **opts):
    """`cycles` restart cycles under MPG_TAIL_FOLD=tail (None: unset): (report, layout, plan)."""
    A, xt, b = _problem(mpg, key)
    if not keep:
        del _PROBLEMS[key]
    _env(monkeypatch, "MPG_TAIL_FOLD", tail)
    for name, value in (env or {}).items():
        _env(monkeypatch, name, value)
    kw = dict(mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=cycles, accum="f32")
    kw.update(opts)
    eng = mpg.Engine(A, b, xt, **kw)
    try:
        lay, plan = eng.spmv_layout(), _plan_text(mpg, eng)
        eng.run(cycles)
        eng.sync()
        return eng.report(), lay, plan
    finally:
        eng.close()


def _same(a, b, what):
    for f in ("x", "step_res", "step_cycle", "cyc_r_norm", "cyc_normalization", "cyc_beta"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    assert a.res_norm == b.res_norm and a.total_iters == b.total_iters, (what, a.res_norm, b.res_norm)
    assert np.all(np.isfinite(a.x)) and np.isfinite(a.res_norm), what


def _check(mpg, monkeypatch, key, on=None, cycles=2, keep=True, **opts):
    """MPG_TAIL_FOLD=0 against `on` (None: unset, the default)."""
    rlen = opts.get("rlen", 30)
    ref, lay0, plan0 = _run(mpg, monkeypatch, key, "0", cycles, **opts)
    got, lay, plan = _run(mpg, monkeypatch, key, on, cycles, keep=keep, **opts)
    assert "tail_fold" not in lay0 and f"update({rlen})" in plan0 and f"givens_partials({rlen - 1})" in plan0, plan0
    assert lay["tail_fold"] is True and "x_snapshot" not in plan and f"givens+update({rlen},1)" in plan, (lay, plan)
    assert ref.total_iters == got.total_iters == cycles * rlen
    _same(got, ref, (key, on, opts))


# 64: one live wave, 960 lanes whose clamped requests contribute nothing;
# 4096: one full workgroup; 4100: a second workgroup with one live lane;
# 8196: two full workgroups plus one row group
@pytest.mark.parametrize("n", [64, 4096, 4100, 8196])
def test_same_bits(mpg, monkeypatch, n):
    _check(mpg, monkeypatch, n)


@pytest.mark.parametrize("n", [4099, 4101])
def test_tail_rows(mpg, monkeypatch, n):
    """n % 4 != 0: the rows past the last quad take the scalar loop."""
    _check(mpg, monkeypatch, n)


@pytest.mark.parametrize("n", [255 * 4096, 256 * 4096 + 4100])
def test_second_grid_stride_pass(mpg, monkeypatch, n):
    """255 workgroups' worth of rows: the last workgroup's lanes have no row;
    256 * 4096 + 4100: the first two workgroups own a second row quad, which
    the ring does not cover (the batched loop behind it)."""
    _check(mpg, monkeypatch, n, cycles=1, keep=False)


# 1 / 2: no rotation to apply / one; 8: below the ring's depth; 9 / 10: NC =
# the ring's depth (no refill) and one past it; 17 / 18: the second lap of the
# ring ends / begins; 30: the bench's; 32: NC = kNC
@pytest.mark.parametrize("rlen", [1, 2, 8, 9, 10, 17, 18, 30, 32])
def test_restart_lengths(mpg, monkeypatch, rlen):
    _check(mpg, monkeypatch, 8196, rlen=rlen)


def test_past_one_panel(mpg, monkeypatch):
    """rlen 33: the form is not taken, the layout says so, the results are the same."""
    ref, lay0, plan0 = _run(mpg, monkeypatch, 8196, "0", rlen=33)
    got, lay, plan = _run(mpg, monkeypatch, 8196, None, rlen=33)
    assert "tail_fold" not in lay0 and "tail_fold" not in lay and plan == plan0 and plan[0] == "x_snapshot"
    _same(got, ref, "rlen 33")


@pytest.mark.parametrize("prec", ["identity", "jacobi"])
@pytest.mark.parametrize("orth", ["cgs", "mgs", "cgsr"])
def test_orthogonalisations(mpg, monkeypatch, orth, prec):
    """CGSR: the correction goes through the same rotation chain."""
    _check(mpg, monkeypatch, 8196, orth=orth, prec=prec)


@pytest.mark.parametrize("mode,accum,on", [("mixed", "f64", "1"), ("single", "f32", None), ("single", "f64", "1"),
                                           ("baseline", "f64", "1")])
@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
def test_modes_and_classes(mpg, monkeypatch, mode, accum, on, orth):
    """The fp64 accumulation class and the fp64 Arnoldi run the chain in the
    same registers and add the columns with the batched loop; they take the
    form under MPG_TAIL_FOLD=1 only."""
    _check(mpg, monkeypatch, 4100, on=on, mode=mode, accum=accum, orth=orth)
    if on == "1":
        _, lay, plan = _run(mpg, monkeypatch, 4100, None, cycles=1, mode=mode, accum=accum, orth=orth)
        assert "tail_fold" not in lay and plan[0] == "x_snapshot"


@pytest.mark.parametrize("rlen", [2, 30])
def test_unfolded_steps(mpg, monkeypatch, rlen):
    """MPG_FOLD_GIVENS=0: every step's Givens launch of its own but the last."""
    _check(mpg, monkeypatch, 8196, rlen=rlen, env={"MPG_FOLD_GIVENS": "0"})
    _, _, plan = _run(mpg, monkeypatch, 8196, None, cycles=1, rlen=rlen, env={"MPG_FOLD_GIVENS": "0"})
    assert sum(t.startswith("givens_partials") for t in plan) == rlen - 1, plan


@pytest.mark.parametrize("prec", ["identity", "jacobi"])
def test_another_storage(mpg, monkeypatch, prec):
    _check(mpg, monkeypatch, "lap12", prec=prec)


def test_undo(mpg, monkeypatch):
    """A solve that converges after several cycles: the pipelined engine has
    then launched one cycle too many and puts back the x that cycle's
    givens+update launch kept. Same x, iterations and histories under the
    default, under MPG_TAIL_FOLD=0 and without the pipeline."""
    A, xt, b = _problem(mpg, 4100)
    res = {}
    for name, tail, pipe in (("default", None, None), ("split", "0", None), ("serial", None, "0")):
        _env(monkeypatch, "MPG_TAIL_FOLD", tail)
        _env(monkeypatch, "MPG_PIPELINE", pipe)
        eng = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="identity", rlen=4, tol=1e-10, max_restarts=500,
                         accum="f32")
        try:
            lay, plan = eng.spmv_layout(), _plan_text(mpg, eng)
            ran, done = eng.run(500)
            eng.sync()
            res[name] = eng.report()
        finally:
            eng.close()
        assert done and res[name].status == "converged", (name, res[name].status)
        assert ("tail_fold" in lay) == (tail is None), (name, lay)
        if name == "default":
            assert "x_snapshot" not in plan and "givens+update(4,1)" in plan, plan
        if name == "serial":
            assert "x_snapshot" not in plan and "givens+update(4,0)" in plan, plan
        if name == "split":
            assert plan[0] == "x_snapshot", plan
    assert res["default"].restarts >= 3, res["default"].restarts
    for name in ("split", "serial"):
        _same(res[name], res["default"], name)
        assert res[name].restarts == res["default"].restarts


@pytest.mark.parametrize("accum", [1, 0])
def test_workspace_state(mpg, hip, accum):
    """One cycle of GMRES(4) through the C ABI on two workspaces: after the
    finish launch H(:, m-1), s, cs, sn, the report and x are those the
    separate givens / update launches leave, and the snapshot is the x the
    update read."""
    from tests.test_neumann_gpu import Workspace

    lib, m = hip.lib, 4
    A = mpg.gen_band(4100, 5, 4, seed=7)
    x0 = np.random.default_rng(5).standard_normal(A.nrows)
    state = {}
    for form in ("split", "tail"):
        W = Workspace(mpg, hip, A, "f32", 2, accum)
        snap = hip.buf(np.zeros(A.nrows))
        try:
            arn = W.arn
            hip.check(lib.mpg_memcpy_h2d(hip.ctx, W.x.p, x0.ctypes.data, x0.nbytes), "h2d")
            assert lib.mpg_arnoldi_update_tail_supported(arn) == 0
            hip.check(lib.mpg_arnoldi_set_x_snapshot(arn, snap.p), "snapshot")
            hip.check(lib.mpg_arnoldi_prologue(arn), "prologue")
            hip.check(lib.mpg_arnoldi_prologue_finish_partials(arn), "finish")
            for k in range(m):
                hip.check(lib.mpg_arnoldi_spmv(arn, k), "spmv")
                hip.check(lib.mpg_arnoldi_dots(arn, k), "dots")
                hip.check(lib.mpg_arnoldi_cgs_partials(arn, k), "cgs")
                if k < m - 1:
                    hip.check(lib.mpg_arnoldi_givens_partials(arn, k), "givens")
            if form == "split":
                hip.check(lib.mpg_arnoldi_givens_partials(arn, m - 1), "givens")
                hip.check(lib.mpg_arnoldi_update(arn, m), "update")
            else:
                assert lib.mpg_arnoldi_update_tail(arn, m - 1, 1) == -2  # not the whole restart length
                assert lib.mpg_arnoldi_update_tail(arn, m, 2) == -2      # an unknown flag
                hip.check(lib.mpg_arnoldi_update_tail(arn, m, 1), "update_tail")
            hip.check(lib.mpg_arnoldi_prologue(arn), "prologue")
            hip.check(lib.mpg_arnoldi_prologue_finish_partials(arn), "finish")
            hip.sync()

            def read(ptr, count, dtype):
                out = np.empty(count, dtype)
                hip.check(lib.mpg_memcpy_d2h(hip.ctx, out.ctypes.data, ptr, out.nbytes), "d2h")
                return out

            state[form] = dict(
                H=read(lib.mpg_arnoldi_hessenberg_dev(arn), (m + 1) * m, np.float32),
                cs=read(lib.mpg_arnoldi_rotations_dev(arn, 0), m + 1, np.float32),
                sn=read(lib.mpg_arnoldi_rotations_dev(arn, 1), m + 1, np.float32),
                s=read(lib.mpg_arnoldi_rotations_dev(arn, 2), m + 1, np.float32),
                inv=read(lib.mpg_arnoldi_inv_dev(arn), 1, np.float32),
                report=read(lib.mpg_arnoldi_report_dev(arn), lib.mpg_arnoldi_report_len(arn), np.float64),
                x=W.x.get(), snap=snap.get())
        finally:
            W.close()
            snap.free()
    for f in ("H", "cs", "sn", "s", "inv", "report", "x"):
        assert np.array_equal(state["tail"][f], state["split"][f]), f
    assert np.all(state["tail"]["H"].reshape(m, m + 1)[m - 1, :m] != 0) and np.all(state["tail"]["report"][4:4 + m] > 0)
    assert not np.array_equal(state["tail"]["x"], x0)
    assert np.array_equal(state["tail"]["snap"], x0) and not state["split"]["snap"].any()
