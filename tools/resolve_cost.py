"""What a sequence of solves with one matrix pays per solve on one MI355X: the
engine's set-up against a re-arm (Engine.rearm, mpg_engine_rearm) and against
the solve itself. A GPU tool, not a test.

Cases (mode mixed, CGS, GMRES(30), to 1e-10):
  lap1m    laplace:100 (LAP-1M), chebyshev with 4 sweeps
  band10m  band:1000000 (BAND-10M), jacobi, accum f32

  --what create   mpg_engine_create: setup_seconds as the engine reports it, the
                  wall time of the creating call, and the solve that follows
                  (run to done, timed around run + sync); a new engine per round.
                  Runs on any tree that has Engine: --tree names the checkout
                  whose package is measured (built; default this repository),
                  e.g. one of the parent commit.
  --what rearm    one engine, then per round a re-arm with another right-hand
                  side (x_true from rand_vect seeds 43, 44, ...): the re-arm's
                  setup_seconds, its wall time, and the solve that follows.

usage: python tools/resolve_cost.py --what create [--tree DIR] [--rounds 5] [--case lap1m --case band10m]
One JSON line per (case, what) on stdout: medians with ranges."""
import argparse
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

CASES = {
    "lap1m": ("laplace:100", dict(mode="mixed", orth="cgs", prec="chebyshev", jacobi_steps=4, rlen=30, tol=1e-10)),
    "band10m": ("band:1000000", dict(mode="mixed", orth="cgs", prec="jacobi", accum="f32", rlen=30, tol=1e-10)),
}


def load(tree: Path):
    pkg = tree / "icl-mixed-precision-gmres_amd"
    spec = importlib.util.spec_from_file_location("mpgmres_amd", pkg / "__init__.py",
                                                  submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mpgmres_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return dict(median=statistics.median(v), lo=min(v), hi=max(v), runs=len(v))


def run_to_done(e):
    e.sync()
    t = time.perf_counter()
    done = False
    while not done:
        _, done = e.run(1 << 20)
    e.sync()
    return time.perf_counter() - t


def create(mpg, name, rounds):
    spec, opts = CASES[name]
    A = mpg.gen_spec(spec)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    setup, wall, solve, iters = [], [], [], None
    for r in range(rounds + 1):  # (round 0: the process's first engine, not counted)
        t = time.perf_counter()
        e = mpg.Engine(A, b, xt, **opts)
        e.sync()
        w = time.perf_counter() - t
        try:
            s = run_to_done(e)
            res = e.report()
        finally:
            e.close()
        if r:
            setup.append(res.setup_seconds), wall.append(w), solve.append(s)
        iters = res.total_iters
        assert res.status == "converged", res.status
    return dict(what="create", case=name, spec=spec, opts=opts, setup_seconds=med(setup), create_wall_seconds=med(wall),
                solve_seconds=med(solve), iters=iters)


def rearm(mpg, name, rounds):
    spec, opts = CASES[name]
    A = mpg.gen_spec(spec)
    xt = mpg.rand_vect(A.nrows, 42)
    e = mpg.Engine(A, mpg.host_spmv(A, xt), xt, **opts)
    arm, wall, solve, iters = [], [], [], []
    try:
        run_to_done(e)
        for r in range(rounds + 1):  # (round 0 not counted)
            xt = mpg.rand_vect(A.nrows, 43 + r)
            b = mpg.host_spmv(A, xt)
            e.sync()
            t = time.perf_counter()
            e.rearm(b, x_true=xt)
            e.sync()
            w = time.perf_counter() - t
            s = run_to_done(e)
            res = e.report()
            assert res.status == "converged", res.status
            if r:
                arm.append(res.setup_seconds), wall.append(w), solve.append(s), iters.append(res.total_iters)
        captures = e.graph_captures
    finally:
        e.close()
    return dict(what="rearm", case=name, spec=spec, opts=opts, rearm_setup_seconds=med(arm), rearm_wall_seconds=med(wall),
                solve_seconds=med(solve), iters=iters, graph_captures=captures)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["create", "rearm"], required=True)
    ap.add_argument("--tree", default=str(REPO))
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    mpg = load(Path(args.tree).resolve())
    for name in args.case or list(CASES):
        out = {"create": create, "rearm": rearm}[args.what](mpg, name, args.rounds)
        out["tree"] = "this" if Path(args.tree).resolve() == REPO else Path(args.tree).name
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
