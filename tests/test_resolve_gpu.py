"""A sequence of systems on one live engine, from an initial guess
(mpg_engine_rearm, mpg_engine_x, mpg_solve_from; Engine.rearm / solve / x and
solve(x0=)): a re-armed engine gives a new engine's bits whatever ran on it
before, nothing of the set-up is redone, the guess is where the solve starts,
device vectors are read in place, and what is out of scope is refused."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import resolve_np as RS
from tests.golden.make_golden import convdiff
from tests.parity import compare
from tests.test_cli_gpu import SUMMARY
from tests.test_resolve_cpu import CASES, TOL, WARM_BE_CAP

pytestmark = pytest.mark.gpu

_cache = {}


def _problem(mpg, key):
    """(A, [(b, x_true) for the rand_vect seeds 42, 43])"""
    if key not in _cache:
        if key.startswith("lap"):
            A = mpg.gen_laplace3d(int(key[3:]))
        elif key.startswith("band"):
            A = mpg.gen_band(int(key[4:]), 5, 4, seed=7)
        elif key == "convdiff32":
            A = convdiff(mpg, 32)
        else:
            assert key == "stencil5"
            A = mpg.gen_stencil27(5)
        rhs = []
        for seed in (42, 43):
            xt = mpg.rand_vect(A.nrows, seed)
            rhs.append((mpg.host_spmv(A, xt), xt))
        _cache[key] = (A, rhs)
    return _cache[key]


def _same(a, b, label=""):
    for f in ("status", "restarts", "total_iters", "inner_k", "res_norm", "err_norm", "minvb_norm"):
        assert getattr(a, f) == getattr(b, f), f"{label}: {f} {getattr(a, f)} vs {getattr(b, f)}"
    for f in ("step_res", "step_cycle", "cyc_r_norm", "cyc_normalization", "cyc_beta", "x"):
        u, v = getattr(a, f), getattr(b, f)
        assert u.shape == v.shape and np.array_equal(u, v, equal_nan=True), f"{label}: {f}"


BASE = dict(mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-9, max_restarts=30)


def _opts(**kw):
    o = dict(BASE)
    o.update(kw)
    if o["mode"] == "single" and "tol" not in kw:
        o["tol"] = 1e-5
    return o


def _sequence(mpg, key, opts):
    """solve b1, b2, b1 again on one engine; b2 on a new one"""
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, key)
    assert not np.array_equal(b1, b2)
    e = mpg.Engine(A, b1, xt1, **opts)
    try:
        r1 = e.solve()
        r2 = e.solve(b2, x_true=xt2)
        r1b = e.solve(b1, x_true=xt1)
        assert e.solves == 3
    finally:
        e.close()
    fresh = mpg.solve(A, b2, xt2, engine="fused", **opts)
    _same(r2, fresh, f"{key} {opts}: re-armed vs new engine")
    _same(r1b, r1, f"{key} {opts}: first system again")
    assert r1.total_iters > 0 and not np.array_equal(r1.x, r2.x)
    return r1, r2


# ---------------------------------------------------------------- 1. a re-armed engine is a fresh engine
MODES = ["mixed", "baseline", "single-prec", "single", "mixed-half"]
KEYS = ["lap12", "band4099", "band8196", "convdiff32"]
MODE_ORTH = [(m, o, KEYS[(3 * i + j) % 4]) for i, m in enumerate(MODES) for j, o in enumerate(["cgs", "mgs", "cgsr"])]


@pytest.mark.parametrize("mode,orth,key", MODE_ORTH)
def test_rearm_modes_and_orthogonalisations(mpg, mode, orth, key):
    _sequence(mpg, key, _opts(mode=mode, orth=orth))


PRECS = [("identity", "lap12", {}), ("jacobi", "band8196", {}), ("ilu", "convdiff32", {}),
         ("ilu_jacobi", "lap12", dict(jacobi_steps=3)), ("bjacobi", "stencil5", {}),
         ("neumann", "lap12", dict(jacobi_steps=2)), ("chebyshev", "lap12", dict(jacobi_steps=3)),
         ("gmres_poly", "convdiff32", dict(jacobi_steps=4))]


@pytest.mark.parametrize("prec,key,extra", PRECS, ids=[p[0] for p in PRECS])
def test_rearm_preconditioners(mpg, prec, key, extra):
    _sequence(mpg, key, _opts(prec=prec, **extra))


@pytest.mark.parametrize("fmt,key", [("csr", "band8196"), ("sell", "band8196"), ("node", "stencil5")])
def test_rearm_storages(mpg, fmt, key):
    A, rhs = _problem(mpg, key)
    e = mpg.Engine(A, *rhs[0], **_opts(spmv_format=fmt))
    assert e.spmv_layout()["format"] == fmt
    e.close()
    _sequence(mpg, key, _opts(spmv_format=fmt))


@pytest.mark.parametrize("accum", ["f32", "f64"])
def test_rearm_accumulation_classes(mpg, accum):
    _sequence(mpg, "band8196", _opts(accum=accum))


def test_rearm_compressed_basis(mpg):
    _sequence(mpg, "lap12", _opts(basis="f16"))


@pytest.mark.parametrize("rlen", [1, 4, 30, 100])
def test_rearm_restart_lengths(mpg, rlen):
    _sequence(mpg, "band4099", _opts(rlen=rlen))


STRATEGIES = {"base": {}, "rtol": dict(rtol=1e-2), "repeat": dict(rtol=1e-2, repeat_iter=True),
              "orthloss": dict(rtol=1e-2, orthloss=True)}


@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_rearm_strategies(mpg, strategy):
    _sequence(mpg, "convdiff32", _opts(prec="identity", rlen=40, max_restarts=400, **STRATEGIES[strategy]))


@pytest.mark.parametrize("env,graph,pipeline", [({}, 1, 1), ({"MPG_PIPELINE": "0"}, 1, 0), ({"MPG_NO_GRAPH": "1"}, 0, None)])
def test_rearm_graph_pipelined_and_eager(mpg, monkeypatch, env, graph, pipeline):
    for name in ("MPG_PIPELINE", "MPG_NO_GRAPH"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    A, rhs = _problem(mpg, "band8196")
    e = mpg.Engine(A, *rhs[0], **_opts())
    p = e.cycle_policy()
    e.close()
    assert p.graph == graph and (pipeline is None or p.pipeline == pipeline)
    _sequence(mpg, "band8196", _opts())


# ---------------------------------------------------------------- 2. any prior state
def test_rearm_after_an_unfinished_solve(mpg):
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "band8196")
    e = mpg.Engine(A, b1, xt1, **_opts())
    ran, done = e.run(1)
    assert ran == 1 and not done
    got = e.solve(b2, x_true=xt2)
    e.close()
    _same(got, mpg.solve(A, b2, xt2, engine="fused", **_opts()), "after run(1)")


def test_rearm_after_an_aborted_solve(mpg):
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "lap12")
    opts = _opts(rlen=4, max_restarts=2)
    e = mpg.Engine(A, b1, xt1, **opts)
    assert e.solve().status == "aborted"
    got = e.solve(b2, x_true=xt2)
    e.close()
    assert got.status == "aborted"
    _same(got, mpg.solve(A, b2, xt2, engine="fused", **opts), "after an abort")


@pytest.mark.parametrize("strategy", [dict(rtol=0.1), dict(rtol=1e-2, orthloss=True)], ids=["rtol", "orthloss"])
def test_rearm_after_a_stepwise_solve(mpg, strategy):
    """A solve run step by step that restarted early and converged. (It ends
    with inner_k = 0: no strategy's check() answers "converged" -- in
    IterUtil.hpp only check_initial does, as in the reference -- so the
    engine's inner_k > 0 exit cannot be reached through the library; the
    partial update(k) it would leave is what every early restart runs.)"""
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "convdiff32")
    opts = _opts(prec="identity", rlen=40, max_restarts=400, **strategy)
    e = mpg.Engine(A, b1, xt1, **opts)
    r1 = e.solve()
    assert r1.status == "converged" and r1.inner_k == 0
    assert np.bincount(r1.step_cycle).min() < 40  # it did restart inside a cycle
    assert e.graph_captures == 0  # a stepwise engine captures nothing
    got = e.solve(b2, x_true=xt2)
    e.close()
    _same(got, mpg.solve(A, b2, xt2, engine="fused", **opts), "after a stepwise solve")


# ---------------------------------------------------------------- 3. nothing is rebuilt
def test_nothing_is_rebuilt(mpg):
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "band8196")
    e = mpg.Engine(A, b1, xt1, **_opts())
    lib = mpg.host_lib()
    assert lib.mpg_engine_solves(e._h) == 1 and lib.mpg_engine_graph_captures(e._h) == 0
    lay, pol = e.spmv_layout(), bytes(e.cycle_policy())
    assert e.cycle_policy().graph == 1
    e.solve()
    assert lib.mpg_engine_graph_captures(e._h) == 1
    e.solve(b2, x_true=xt2)
    e.solve(b1, x0=xt1 + 1e-3)
    assert lib.mpg_engine_graph_captures(e._h) == 1 and lib.mpg_engine_solves(e._h) == 3
    assert e.spmv_layout() == lay and bytes(e.cycle_policy()) == pol
    e.close()


# ---------------------------------------------------------------- 4. the initial guess
def test_zero_guess_is_the_default(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band4099")
    e = mpg.Engine(A, b1, xt1, **_opts())
    r0 = e.solve()
    rz = e.solve(x0=np.zeros(A.nrows), x_true=xt1)
    e.close()
    _same(rz, r0, "x0 = zeros")


@pytest.mark.parametrize("mode", ["mixed", "single"])
def test_x_after_rearm_is_the_guess(mpg, mode):
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "band4099")
    e = mpg.Engine(A, b1, xt1, **_opts(mode=mode))
    assert np.array_equal(e.x(), np.zeros(A.nrows))
    e.solve()
    g = xt2 + 1e-3 * np.cos(np.arange(A.nrows))
    e.rearm(b2, x0=g)
    want = g.astype(np.float32).astype(np.float64) if mode == "single" else g
    assert np.array_equal(e.x(), want)
    out = np.empty(A.nrows)
    assert e.x(out) is out and np.array_equal(out, want)
    e.close()


@pytest.mark.parametrize("mode", ["mixed", "baseline"])
def test_converged_x_as_guess_needs_no_iteration(mpg, mode):
    A, ((b1, xt1), _) = _problem(mpg, "lap12")
    e = mpg.Engine(A, b1, xt1, **_opts(mode=mode))
    r = e.solve()
    assert r.status == "converged" and r.total_iters > 0
    again = e.solve(x0=r.x, x_true=xt1)
    e.close()
    assert (again.status, again.restarts, again.total_iters) == ("converged", 0, 0)
    assert np.array_equal(again.x, r.x)


_helper = {}


def _helper_record(mpg, name, orth):
    if (name, orth) not in _helper:
        c = CASES[name]
        A = mpg.gen_laplace3d(c["nx"])
        xt = mpg.rand_vect(A.nrows, 42)
        b = mpg.host_spmv(A, xt)
        g = RS.warm_guess(xt)
        ref = RS.solve(A, b, xt, x0=g, orth=orth, prec="jacobi", rlen=c["rlen"], tol=TOL)
        _helper[name, orth] = (A, b, xt, g, ref)
    return _helper[name, orth]


@pytest.mark.parametrize("accum", ["f64", "f32"])
@pytest.mark.parametrize("orth", ["cgs", "cgsr"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_warm_start_matches_the_restatement(mpg, name, orth, accum):
    A, b, xt, g, ref = _helper_record(mpg, name, orth)
    c = CASES[name]
    assert ref["restarts"] == c["warm"]
    e = mpg.Engine(A, b, xt, mode="mixed", orth=orth, prec="jacobi", rlen=c["rlen"], tol=TOL, accum=accum)
    cold = e.solve()
    got = e.solve(x0=g, x_true=xt)
    e.close()
    print(name, orth, accum, "cycles cold", cold.restarts, "warm", got.restarts, "restatement", ref["restarts"],
          "first backward error", got.backward_error[0])
    assert cold.restarts == c["cold"]
    assert got.restarts == ref["restarts"]
    compare(ref, got, "mixed", TOL, c["rlen"], f"warm {name} {orth} {accum}")


@pytest.mark.parametrize("mode", ["baseline", "single-prec", "single", "mixed-half"])
def test_warm_start_is_used_in_every_mode(mpg, mode):
    A, b, xt, g, ref = _helper_record(mpg, "lap10", "cgs")
    e = mpg.Engine(A, b, xt, **_opts(mode=mode, rlen=10))
    cold = e.solve()
    warm = e.solve(x0=g, x_true=xt)
    e.close()
    be = warm.backward_error[0]
    print(mode, "first backward error cold", cold.backward_error[0], "warm", be, "restatement",
          CASES["lap10"]["be_warm"])
    assert cold.backward_error[0] > 0.1
    assert be <= WARM_BE_CAP


def test_solve_from_is_the_engine_from_a_guess(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "band8196")
    g = xt1 + 1e-3 * np.sin(np.arange(A.nrows))
    one = mpg.solve(A, b1, xt1, x0=g, engine="fused", **_opts())
    e = mpg.Engine(A, b1, xt1, **_opts())
    two = e.solve(x0=g, x_true=xt1)
    e.close()
    _same(one, two, "solve(x0=) vs Engine.solve(x0=)")
    cold = mpg.solve(A, b1, xt1, engine="fused", **_opts())
    assert one.backward_error[0] < 1e-2 * cold.backward_error[0]


# ---------------------------------------------------------------- 5. device vectors
def test_device_vectors(mpg):
    torch = pytest.importorskip("torch")
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "band8196")
    n = A.nrows
    g = xt2 + 1e-3 * np.sin(np.arange(n))
    dev = torch.device("cuda", 0)
    e = mpg.Engine(A, b1, xt1, **_opts())
    host = e.solve(b2, x0=g, x_true=xt2)
    bd, gd = torch.from_numpy(b2).to(dev), torch.from_numpy(g).to(dev)
    got = e.solve(bd, x0=gd, x_true=xt2)
    _same(got, host, "device b and x0")
    xd = torch.empty(n, dtype=torch.float64, device=dev)
    assert e.x(out=xd) is xd
    assert np.array_equal(xd.cpu().numpy(), got.x)
    # only the right-hand side on the device, the guess on the host
    _same(e.solve(bd, x0=g, x_true=xt2), host, "device b, host x0")
    for bad in (bd.to(torch.float32), torch.zeros(2 * n, dtype=torch.float64, device=dev)[::2],
                torch.zeros(n + 1, dtype=torch.float64, device=dev), torch.from_numpy(b2)):
        with pytest.raises(ValueError):
            e.rearm(bad)
        with pytest.raises(ValueError):
            e.rearm(b2, x0=bad)
    with pytest.raises(ValueError):
        e.x(out=torch.empty(n, dtype=torch.float32, device=dev))
    _same(e.solve(b2, x0=g, x_true=xt2), host, "after the refused vectors")
    e.close()


# ---------------------------------------------------------------- 6. refusals
def test_rearm_is_refused_on_a_row_partitioned_engine(mpg):
    A = mpg.gen_band(20_000, 5, 4, seed=7)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    plan = mpg.HaloPlan(0, 1, [0, A.nrows], A)
    e = mpg.Engine.distributed(A, b, xt, plan, mpg.rccl_unique_id(), 1, 0, **_opts())
    try:
        with pytest.raises(RuntimeError, match=r"\(-5\).*row-partitioned"):
            e.rearm(b)
        with pytest.raises(RuntimeError, match=r"\(-5\).*row-partitioned"):
            e.solve(x0=xt)
        ran, done = e.run(40)
        assert done
        r = e.report()
        assert r.status == "converged" and r.total_iters > 0
    finally:
        e.close()


def test_rearm_is_refused_after_measurement_launches(mpg):
    A, ((b1, xt1), (b2, xt2)) = _problem(mpg, "band8196")
    e = mpg.Engine(A, b1, xt1, **_opts())
    e.time_phase("spmv", 2)
    with pytest.raises(RuntimeError, match=r"\(-5\)") as run_err:
        e.run(1)
    with pytest.raises(RuntimeError, match=r"\(-5\)") as arm_err:
        e.rearm(b2)
    e.close()
    text = lambda ex: str(ex.value).split("): ", 1)[1]  # noqa: E731
    assert text(arm_err) == text(run_err) and "measurement launches" in text(arm_err)


def test_a_guess_is_refused_on_the_operator_surface(mpg):
    A, ((b1, xt1), _) = _problem(mpg, "lap12")
    with pytest.raises(RuntimeError, match=r"\(-5\).*fused engine"):
        mpg.solve(A, b1, xt1, x0=xt1, engine="surface", **_opts())
    assert mpg.solve(A, b1, xt1, x0=None, engine="surface", **_opts()).status == "converged"


# ---------------------------------------------------------------- 7. the CLI
CLI_ARGS = ["--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec", "jacobi", "--tol",
            "1e-9", "--gpu"]


def test_cli_solves(mpg):
    run = lambda extra: subprocess.run([str(mpg.CLI)] + CLI_ARGS + extra, capture_output=True, text=True,  # noqa: E731
                                       timeout=120)
    one = run([])
    assert one.returncode == 0, one.stderr
    assert run(["--solves", "1"]).stdout.split("ilu took")[0] == one.stdout.split("ilu took")[0]
    three = run(["--solves", "3"])
    assert three.returncode == 0, three.stderr
    found = SUMMARY.findall(three.stdout)
    assert len(found) == 3, three.stdout
    assert three.stdout.count("||x|| = ") == 3 and three.stdout.count("Doing Mixed Precision test") == 3
    assert found[0][3] == SUMMARY.search(one.stdout).group(4)
    A = mpg.gen_spec("laplace:12")
    e = None
    for j in range(3):
        xt = mpg.rand_vect(A.nrows, 42 + j)
        b = mpg.host_spmv(A, xt)
        if e is None:
            e = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="jacobi", rlen=30, tol=1e-9)
            r = e.solve()
        else:
            r = e.solve(b, x_true=xt)
        assert int(found[j][3]) == r.total_iters and int(found[j][2]) == r.restarts
    e.close()
    assert len({re.sub(r"took \S+", "", "|".join(f)) for f in found}) == 3  # three different systems


def test_cli_solves_needs_the_fused_engine(mpg):
    r = subprocess.run([str(mpg.CLI)] + CLI_ARGS + ["--solves", "2", "--engine", "surface"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "fused engine" in r.stderr, (r.stdout, r.stderr)
    assert not SUMMARY.search(r.stdout)
