"""New matrix values on an unchanged sparsity pattern (mpg_sell_refresh_values,
mpg_arnoldi_refresh_values, mpg_engine_refresh_values; Engine.refresh /
solve(values=), --vary-values): a refilled SELL copy has the bits of a copy
created from the new values in every layout, a refreshed engine is a new
engine on the new matrix, the captured graph is kept where its launch
arguments did not change, device values are read in place, and what is out of
scope is refused with the old matrix intact.

Not tested here: the row-partitioned refusal through the loopback path (it
hands out no engine handle; the RCCL P = 1 engine below is the reachable one),
and a refresh "on the operator surface" -- that engine has no live handle, so
there is nothing to call; the CLI refuses --solves there."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import resolve_np as RS
from tests.test_cli_gpu import SUMMARY
from tests.test_irregular_gpu import _problem as _irregular
from tests.test_resolve_gpu import MODE_ORTH, PRECS, _opts, _problem, _same
from tests.test_sell_stepped_gpu import _far, _wide

pytestmark = pytest.mark.gpu

EPS = 0.1  # the engine tests' perturbation: every small matrix stays diagonally dominant


# ---------------------------------------------------------------- 1. the kernel, bit for bit
_mats = {}


def _matrix(mpg, key):
    if key not in _mats:
        if key in ("wide", "wide-int32"):
            _mats[key] = _matrix(mpg, "wide") if key != "wide" else _wide(mpg)
        elif key == "far":
            _mats[key] = _far(mpg)
        elif key in ("fem27", "fem27-sorted"):
            _mats[key] = _irregular(mpg, "fem27")[0]
        else:
            _mats[key] = _problem(mpg, key)[0]
    return _mats[key]


def _describe(hip, sell):
    lib = hip.lib
    w, cb, st, win = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    hip.check(lib.mpg_sell_layout(sell, C.byref(w), C.byref(cb), C.byref(st), C.byref(win)))
    form, exc, imp = C.c_int32(), C.c_int64(), C.c_int64()
    hip.check(lib.mpg_sell_columns(sell, C.byref(form), C.byref(exc), C.byref(imp)))
    return dict(W=w.value, col_bytes=cb.value, stored=st.value, window=win.value, form=form.value, csr=exc.value,
                implicit=imp.value, shared=int(lib.mpg_sell_shared_slices(sell)), bytes=int(lib.mpg_sell_bytes(sell)))


# what the layout under test must show at the builder's own vector width
EXPECT = {
    "band4099": lambda d: d["form"] == 1 and d["implicit"] > 0,   # int16 slice-relative, implicit slices; n % 64 != 0
    "band8196": lambda d: d["form"] == 1 and d["implicit"] > 0,   # ... a 4-row tail slice (8196 = 128 * 64 + 4)
    "lap12": lambda d: d["form"] == 1 and d["shared"] > 0,        # shared int16 column blocks; n = 1728 = 27 * 64
    "wide": lambda d: d["form"] == 2 and d["csr"] == 0,           # stepped int16
    "far": lambda d: d["form"] == 2 and d["csr"] == 1,            # stepped int16 with a CSR-summed slice
    "wide-int32": lambda d: d["form"] == 0,                       # int32 columns (MPG_SELL_STEPPED=0)
    "fem27": lambda d: d["form"] == 1 and d["implicit"] == 0,     # rows of varying length, every slice stored
    "fem27-sorted": lambda d: d["form"] == 0,                     # ... rows sorted by length (SELL-C-sigma)
}


@pytest.mark.parametrize("W", [None, 1, 2, 4])
@pytest.mark.parametrize("key", list(EXPECT))
def test_refilled_copy_has_a_new_copys_bits(hip, mpg, key, W, monkeypatch):
    for name in ("MPG_SELL_W", "MPG_SELL_SIGMA", "MPG_SELL_STEPPED"):
        monkeypatch.delenv(name, raising=False)
    if key == "wide-int32":
        monkeypatch.setenv("MPG_SELL_STEPPED", "0")
    if W is not None:
        monkeypatch.setenv("MPG_SELL_W", str(W))
    A = _matrix(mpg, key)
    n = A.nrows
    lib = hip.lib
    unsorted_stored = None
    drp, dci = hip.buf(A.rowptr), hip.buf(A.col)
    csr = C.c_void_p()
    hip.check(lib.mpg_csr_create(hip.ctx, n, n, A.nnz, A.rowptr.ctypes.data, drp.p, dci.p, C.byref(csr)))
    if key == "fem27-sorted":
        s0 = C.c_void_p()
        d0 = hip.buf(A.val)
        hip.check(lib.mpg_sell_create(hip.ctx, csr, 0, d0.p, 2, C.byref(s0)))
        unsorted_stored = _describe(hip, s0)["stored"]
        lib.mpg_sell_destroy(s0)
        monkeypatch.setenv("MPG_SELL_SIGMA", "-1")
    v1 = A.val
    v2 = mpg.perturb_values(v1, 0.3, 1)
    x = np.random.default_rng(5).uniform(-1, 1, n)
    made = []
    try:
        for name, vt, cast, xdt in (("f64", 0, lambda v: v, np.float64), ("f32", 1, lambda v: v.astype(np.float32), np.float32),
                                    ("f16f32", 2, lambda v: v.astype(np.float16).view(np.uint16), np.float32)):
            d1, d2 = hip.buf(cast(v1)), hip.buf(cast(v2))
            live, ref = C.c_void_p(), C.c_void_p()
            hip.check(lib.mpg_sell_create(hip.ctx, csr, vt, d1.p, 2, C.byref(live)))
            hip.check(lib.mpg_sell_create(hip.ctx, csr, vt, d2.p, 2, C.byref(ref)))
            assert live.value and ref.value
            made += [live, ref]
            lay = _describe(hip, live)
            print(key, W, name, lay)
            if W is None:
                assert EXPECT[key](lay), lay
                if unsorted_stored is not None:
                    assert lay["stored"] < unsorted_stored  # the sorted slicing took place
            else:
                assert lay["W"] == W
            assert _describe(hip, ref) == lay  # the layout reads no value
            dx = hip.buf(x.astype(xdt))

            def spmv(s):
                dy = hip.buf(np.full(n, 7.0, dtype=xdt))
                hip.call(f"mpg_sell_spmv_{name}", s, xdt(1), dx.p, xdt(0), dy.p)
                out = dy.get()
                dy.free()
                return out

            y1, y2 = spmv(live), spmv(ref)
            assert not np.array_equal(y1, y2)
            # a wrong value type is refused and nothing changes
            assert lib.mpg_sell_refresh_values(hip.ctx, live, csr, (vt + 1) % 3, d2.p) == -2
            assert np.array_equal(spmv(live), y1)
            hip.check(lib.mpg_sell_refresh_values(hip.ctx, live, csr, vt, d2.p))
            assert np.array_equal(spmv(live), y2), f"{key} W={W} {name}: refreshed to v2"
            assert _describe(hip, live) == lay
            hip.check(lib.mpg_sell_refresh_values(hip.ctx, live, csr, vt, d1.p))
            assert np.array_equal(spmv(live), y1), f"{key} W={W} {name}: back to v1 (stale pads or xval)"
            assert _describe(hip, live) == lay
            for d in (d1, d2, dx):
                d.free()
    finally:
        for s in made:
            lib.mpg_sell_destroy(s)
        lib.mpg_csr_destroy(csr)
        drp.free()
        dci.free()


# ---------------------------------------------------------------- 2. a refreshed engine is a new engine
def _second(mpg, key, eps=EPS):
    """(A2, b2, x_true): the matrix perturb_values(A, eps, 1) and b2 = A2 x_true"""
    A, ((b1, xt1), _) = _problem(mpg, key)
    A2 = mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, mpg.perturb_values(A, eps, 1))
    return A2, mpg.host_spmv(A2, xt1), xt1


def _structure(layout):
    return {k: v for k, v in layout.items() if not k.startswith("prec_")}


def _sequence(mpg, key, opts):
    """solve (A1, b1), refresh to A2 and solve b2, refresh back and solve b1; A2 on a new engine"""
    A, ((b1, xt1), _) = _problem(mpg, key)
    A2, b2, _ = _second(mpg, key)
    e = mpg.Engine(A, b1, xt1, **opts)
    try:
        lay1 = e.spmv_layout()
        r1 = e.solve()
        e.refresh(A2.val)
        r2 = e.solve(b2, x_true=xt1)
        lay2 = e.spmv_layout()
        r1b = e.solve(b1, x_true=xt1, values=A.val)
        assert e.spmv_layout() == lay1 and e.solves == 3 and e.refresh_seconds > 0
        caps = e.graph_captures
    finally:
        e.close()
    f = mpg.Engine(A2, b2, xt1, **opts)
    lay_new = f.spmv_layout()
    f.close()
    fresh = mpg.solve(A2, b2, xt1, engine="fused", **opts)
    _same(r2, fresh, f"{key} {opts}: refreshed vs new engine")
    _same(r1b, r1, f"{key} {opts}: the first matrix again")
    assert lay2 == lay_new and _structure(lay2) == _structure(lay1)
    assert r1.total_iters > 0 and not np.array_equal(r1.x, r2.x)
    return caps


@pytest.mark.parametrize("mode,orth,key", MODE_ORTH)
def test_refresh_modes_and_orthogonalisations(mpg, mode, orth, key):
    _sequence(mpg, key, _opts(mode=mode, orth=orth))


# ---------------------------------------------------------------- 3. the graph rule (with every preconditioner)
KEPT = {"identity", "jacobi", "bjacobi", "neumann"}


@pytest.mark.parametrize("prec,key,extra", PRECS, ids=[p[0] for p in PRECS])
def test_refresh_preconditioners_and_the_graph_rule(mpg, monkeypatch, prec, key, extra):
    for name in ("MPG_PIPELINE", "MPG_NO_GRAPH"):
        monkeypatch.delenv(name, raising=False)
    A, ((b1, xt1), _) = _problem(mpg, key)
    A2, b2, _ = _second(mpg, key)
    e = mpg.Engine(A, b1, xt1, **_opts(prec=prec, **extra))
    e.solve()
    assert e.graph_captures == 1
    e.solve(b2, x_true=xt1, values=A2.val)
    assert e.graph_captures == (1 if prec in KEPT else 2), prec
    e.close()
    _sequence(mpg, key, _opts(prec=prec, **extra))


@pytest.mark.parametrize("fmt,key", [("csr", "band8196"), ("sell", "band8196"), ("node", "stencil5")])
def test_refresh_storages(mpg, fmt, key):
    A, rhs = _problem(mpg, key)
    e = mpg.Engine(A, *rhs[0], **_opts(spmv_format=fmt))
    assert e.spmv_layout()["format"] == fmt
    e.close()
    _sequence(mpg, key, _opts(spmv_format=fmt))


@pytest.mark.parametrize("accum", ["f32", "f64"])
def test_refresh_accumulation_classes(mpg, accum):
    _sequence(mpg, "band8196", _opts(accum=accum))


def test_refresh_compressed_basis(mpg):
    _sequence(mpg, "lap12", _opts(basis="f16"))


@pytest.mark.parametrize("rlen", [1, 30])
def test_refresh_restart_lengths(mpg, rlen):
    _sequence(mpg, "band4099", _opts(rlen=rlen))


@pytest.mark.parametrize("strategy", [{}, dict(rtol=1e-2)], ids=["base", "rtol"])
def test_refresh_strategies(mpg, strategy):
    _sequence(mpg, "convdiff32", _opts(prec="identity", rlen=40, max_restarts=400, **strategy))


@pytest.mark.parametrize("env", [{"MPG_PIPELINE": "0"}, {"MPG_NO_GRAPH": "1"}], ids=["unpipelined", "eager"])
def test_refresh_unpipelined_and_eager(mpg, monkeypatch, env):
    for name in ("MPG_PIPELINE", "MPG_NO_GRAPH"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    caps = _sequence(mpg, "band8196", _opts())
    assert caps == (0 if "MPG_NO_GRAPH" in env else 1)


# ---------------------------------------------------------------- 4. device values
def test_device_values(mpg):
    torch = pytest.importorskip("torch")
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    A2, b2, _ = _second(mpg, "band8196")
    dev = torch.device("cuda", 0)
    e = mpg.Engine(A, b1, xt1, **_opts())
    host = e.solve(b2, x_true=xt1, values=A2.val)
    e.solve(b1, x_true=xt1, values=A.val)
    vd = torch.from_numpy(A2.val).to(dev)
    keep = vd.clone()
    got = e.solve(b2, x_true=xt1, values=vd)
    _same(got, host, "device values")
    assert torch.equal(vd, keep)
    for bad in (vd.to(torch.float32), vd[:-1], torch.from_numpy(A2.val), np.zeros(A.nnz + 1)):
        with pytest.raises(ValueError):
            e.refresh(bad)
    _same(e.solve(b2, x_true=xt1), host, "after the refused values")
    e.close()


# ---------------------------------------------------------------- 5. the contract
def test_run_before_the_rearm_is_an_error(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    A2, b2, _ = _second(mpg, "band8196")
    e = mpg.Engine(A, b1, xt1, **_opts())
    e.solve()
    e.refresh(A2.val)
    with pytest.raises(RuntimeError, match=r"\(-2\).*mpg_engine_rearm"):
        e.run(1)
    e.rearm(b2, x_true=xt1)
    got = e.solve()
    e.close()
    # (res_norm among the fields: ||b2 - A2 x|| with the new fp64 values, as the new engine forms it)
    _same(got, mpg.solve(A2, b2, xt1, engine="fused", **_opts()), "re-armed after the refused run")


def test_a_wrong_nnz_touches_nothing(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    e = mpg.Engine(A, b1, xt1, **_opts())
    r1 = e.solve()
    lib = mpg.host_lib()
    v = mpg.perturb_values(A, EPS, 1)
    assert lib.mpg_engine_refresh_values(e._h, v.ctypes.data, A.nnz - 1, 0) == -2
    assert b"sparsity pattern" in lib.mpg_engine_last_error(e._h)
    _same(e.solve(b1, x_true=xt1), r1, "after a refused refresh")
    e.close()


def test_refresh_is_refused_after_measurement_launches(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    e = mpg.Engine(A, b1, xt1, **_opts())
    e.time_phase("spmv", 2)
    with pytest.raises(RuntimeError, match=r"\(-5\).*measurement launches"):
        e.refresh(A.val)
    e.close()


def test_refresh_is_refused_on_a_row_partitioned_engine(mpg):
    A = mpg.gen_band(20_000, 5, 4, seed=7)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    plan = mpg.HaloPlan(0, 1, [0, A.nrows], A)
    e = mpg.Engine.distributed(A, b, xt, plan, mpg.rccl_unique_id(), 1, 0, **_opts())
    try:
        with pytest.raises(RuntimeError, match=r"\(-5\).*row-partitioned"):
            e.refresh(A.val)
        ran, done = e.run(40)
        assert done and e.report().status == "converged"
    finally:
        e.close()


def _scaled_row(A, row=5, factor=2.0 ** 20):
    v = A.val.copy()
    v[A.rowptr[row]:A.rowptr[row + 1]] *= factor
    return v


def test_mixed_half_scaled_engine_takes_in_range_values(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    opts = _opts(mode="mixed-half", tol=1e-6)
    A1 = mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, _scaled_row(A))
    e = mpg.Engine(A1, mpg.host_spmv(A1, xt1), xt1, **opts)
    assert e.half_stats()["rows_scaled"] > 0
    e.solve()
    got = e.solve(b1, x_true=xt1, values=A.val)
    assert e.half_stats()["rows_scaled"] == 0
    e.close()
    _same(got, mpg.solve(A, b1, xt1, engine="fused", **opts), "scaled engine, in-range values")


def test_mixed_half_unscaled_engine_refuses_values_that_need_scaling(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    opts = _opts(mode="mixed-half", tol=1e-6)
    e = mpg.Engine(A, b1, xt1, **opts)
    assert e.half_stats()["rows_scaled"] == 0
    r1 = e.solve()
    with pytest.raises(RuntimeError, match=r"\(-5\).*row scaling"):
        e.refresh(_scaled_row(A))
    _same(e.solve(b1, x_true=xt1), r1, "the old matrix after the refusal")
    e.close()


# ---------------------------------------------------------------- 6. the CLI
def test_cli_vary_values(mpg):
    args = ["--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec", "jacobi", "--tol",
            "1e-9", "--gpu", "--solves", "3", "--vary-values", "0.1"]
    out = subprocess.run([str(mpg.CLI)] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    found = SUMMARY.findall(out.stdout)
    assert len(found) == 3, out.stdout
    A = mpg.gen_spec("laplace:12")
    e = None
    for j in range(3):
        Aj = A if j == 0 else mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, mpg.perturb_values(A, 0.1, j))
        xt = mpg.rand_vect(A.nrows, 42 + j)
        b = mpg.host_spmv(Aj, xt)
        if e is None:
            e = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-9)
            r = e.solve()
        else:
            r = e.solve(b, x_true=xt, values=Aj.val)
        line = found[j]
        assert (int(line[1]), int(line[2]), int(line[3])) == (r.inner_k, r.restarts, r.total_iters), (j, line)
        # resNorm and errNorm as the CLI prints them (6 significant digits)
        assert float(line[6]) == float(f"{r.res_norm:.6g}") and float(line[7]) == float(f"{r.err_norm:.6g}"), (j, line)
    e.close()


# ---------------------------------------------------------------- 7. a warm start across a values change
def test_warm_start_across_a_values_change(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "lap12")
    A2, b2, _ = _second(mpg, "lap12", eps=1e-3)
    opts = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=10, tol=1e-10)
    e = mpg.Engine(A, b1, xt1, **opts)
    prev = e.solve()
    cold = e.solve(b2, x_true=xt1, values=A2.val)
    warm = e.solve(b2, x0=prev.x, x_true=xt1)
    e.close()
    ref = RS.solve(A2, b2, xt1, x0=prev.x, orth="cgs", prec="jacobi", rlen=10, tol=1e-10)
    print("cycles from zeros", cold.restarts, "from the previous x", warm.restarts, "restatement", ref["restarts"])
    assert warm.restarts < cold.restarts
    assert warm.restarts == ref["restarts"]
