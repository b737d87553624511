"""GMRES-polynomial sweep measurements (profiles/r16_gmres_poly/): what one
sweep launch of prec gmres_poly costs inside the cycle, beside the Chebyshev
sweep's cost measured in the same process, by the method of
tools/cheb_bench.py.

Engines with prec chebyshev and prec gmres_poly at s = 3 and s = 4 run the
same fixed work (mixed CGS GMRES(30), tol 0, fp32 accumulation class)
interleaved; a cycle applies the preconditioner m + 1 times, so one sweep
launch costs (t_cycle(s = 4) - t_cycle(s = 3)) / (m + 1): two graph replays
that differ by exactly that launch per application. For chebyshev that launch
is the general sweep (with z_prev); for gmres_poly it is a step that is
neither first nor last (z read and written, the second output stored), as long
as the four roots are real, which the record states. One JSON file, progress
lines on stdout.

usage: python tools/poly_bench.py [out.json] [--matrices BAND-10M,LAP-1M]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from tests.conftest import load_package  # noqa: E402

MATS = {"BAND-10M": lambda m: m.gen_band(1_000_000, 5, 4, seed=7), "LAP-1M": lambda m: m.gen_laplace3d(100)}
PRECS = ("chebyshev", "gmres_poly")


def say(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="profiles/r16_gmres_poly/poly_bench.json")
    ap.add_argument("--matrices", default="BAND-10M,LAP-1M")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cycles", type=int, default=10)
    args = ap.parse_args()
    mpg = load_package()
    m = 30
    out = {}
    for name in args.matrices.split(","):
        A = MATS[name](mpg)
        xt = mpg.rand_vect(A.nrows, 42)
        b = mpg.host_spmv(A, xt)
        eng, lay, setup = {}, {}, {}
        for prec in PRECS:
            for s in (3, 4):
                t = time.perf_counter()
                e = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec=prec, jacobi_steps=s, rlen=m, tol=0.0,
                               max_restarts=10_000_000, accum="f32")
                e.sync()
                setup[prec, s] = time.perf_counter() - t
                eng[prec, s], lay[prec, s] = e, e.spmv_layout()
                e.run(3)
                e.sync()
        roots = {s: lay["gmres_poly", s]["prec_roots"] for s in (3, 4)}
        say(name, {k: v for k, v in lay["gmres_poly", 4].items() if k != "prec_roots"}, roots)
        runs = {k: [] for k in eng}
        for rep in range(args.reps):  # interleaved
            for k, e in eng.items():
                t = time.perf_counter()
                e.run(args.cycles)
                e.sync()
                runs[k].append((time.perf_counter() - t) / args.cycles * 1e6)
            say("rep", rep, {f"{p}:{s}": round(v[-1], 1) for (p, s), v in runs.items()})
        # per repetition, so that drift between repetitions cancels
        sweep = {p: [(runs[p, 4][i] - runs[p, 3][i]) / (m + 1) for i in range(args.reps)] for p in PRECS}
        med = {p: statistics.median(v) for p, v in sweep.items()}
        out[name] = {
            "n": A.nrows, "nnz": int(A.nnz),
            "layout": {k: v for k, v in lay["gmres_poly", 4].items() if k != "prec_roots"},
            "roots": {str(s): [[r.real, r.imag] for r in roots[s]] for s in (3, 4)},
            "all_roots_real": all(r.imag == 0.0 for s in (3, 4) for r in roots[s]),
            "setup_seconds": {f"{p}:{s}": round(v, 3) for (p, s), v in setup.items()},
            "cycle_us_median": {f"{p}:{s}": round(statistics.median(v), 1) for (p, s), v in runs.items()},
            "cycle_us_min_max": {f"{p}:{s}": [round(min(v), 1), round(max(v), 1)] for (p, s), v in runs.items()},
            "sweep_us_in_cycle_median": {p: round(v, 2) for p, v in med.items()},
            "sweep_us_in_cycle_min_max": {p: [round(min(v), 2), round(max(v), 2)] for p, v in sweep.items()},
            "gmres_poly_over_chebyshev": round(med["gmres_poly"] / med["chebyshev"], 3),
            "phase_bytes_spmv": {f"{p}:{s}": eng[p, s].phase_bytes("spmv") for p in PRECS for s in (3, 4)},
            "method": f"{args.reps} interleaved repetitions of {args.cycles} graph-replayed cycles per engine",
        }
        say(name, out[name])
        for e in eng.values():
            e.close()
        del A, b, xt
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    say("done")


if __name__ == "__main__":
    main()
