"""Chebyshev-sweep measurements (profiles/r14_chebyshev/): what one Chebyshev
sweep launch costs inside the cycle, beside the Neumann sweep's cost measured
in the same process, by the method of tools/neumann_bench.py.

Engines with prec neumann and prec chebyshev at s = 2 and s = 3 run the same
fixed work (mixed CGS GMRES(30), tol 0, fp32 accumulation class) interleaved;
a cycle applies the preconditioner m + 1 times, so one sweep launch costs
(t_cycle(s = 3) - t_cycle(s = 2)) / (m + 1): two graph replays that differ by
exactly that launch per application. For chebyshev that launch is the general
sweep (the one that also reads z_prev; the sweep s = 2 already has is the
first-step form). The bytes predict one more n-vector read than the Neumann
sweep. One JSON file, progress lines on stdout.

usage: python tools/cheb_bench.py [out.json] [--matrices BAND-10M,LAP-1M]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from tests.conftest import load_package  # noqa: E402

MATS = {"BAND-10M": lambda m: m.gen_band(1_000_000, 5, 4, seed=7), "LAP-1M": lambda m: m.gen_laplace3d(100)}


def say(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="profiles/r14_chebyshev/cheb_bench.json")
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
        eng, lay = {}, {}
        for prec in ("neumann", "chebyshev"):
            for s in (2, 3):
                e = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec=prec, jacobi_steps=s, rlen=m, tol=0.0,
                               max_restarts=10_000_000, accum="f32")
                eng[prec, s], lay[prec, s] = e, e.spmv_layout()
                e.run(3)
                e.sync()
        say(name, lay["chebyshev", 3])
        runs = {k: [] for k in eng}
        for rep in range(args.reps):  # interleaved
            for k, e in eng.items():
                t = time.perf_counter()
                e.run(args.cycles)
                e.sync()
                runs[k].append((time.perf_counter() - t) / args.cycles * 1e6)
            say("rep", rep, {f"{p}:{s}": round(v[-1], 1) for (p, s), v in runs.items()})
        spmv = []
        for _ in range(5):
            ms, added = eng["chebyshev", 2].time_phase_dup("spmv", 5)
            spmv.append(ms * 1e3)
        # per repetition, so that drift between repetitions cancels
        sweep = {p: [(runs[p, 3][i] - runs[p, 2][i]) / (m + 1) for i in range(args.reps)]
                 for p in ("neumann", "chebyshev")}
        med = {p: statistics.median(v) for p, v in sweep.items()}
        n = float(A.nrows)
        storage = eng["chebyshev", 2].phase_bytes("spmv_storage")
        out[name] = {
            "n": A.nrows, "nnz": int(A.nnz), "layout": lay["chebyshev", 3],
            "columns": eng["chebyshev", 3].sell_columns(),
            "cycle_us_median": {f"{p}:{s}": round(statistics.median(v), 1) for (p, s), v in runs.items()},
            "cycle_us_min_max": {f"{p}:{s}": [round(min(v), 1), round(max(v), 1)] for (p, s), v in runs.items()},
            "sweep_us_in_cycle_median": {p: round(v, 2) for p, v in med.items()},
            "sweep_us_in_cycle_min_max": {p: [round(min(v), 2), round(max(v), 2)] for p, v in sweep.items()},
            "chebyshev_over_neumann": round(med["chebyshev"] / med["neumann"], 3),
            "spmv_us_in_cycle_median": round(statistics.median(spmv), 2),
            "spmv_storage_bytes": storage,
            "neumann_sweep_bytes": storage + 3 * 4 * n,
            "chebyshev_sweep_bytes": storage + 4 * 4 * n,
            "method": f"{args.reps} interleaved repetitions of {args.cycles} graph-replayed cycles per engine; "
                      "time_phase_dup(spmv, 5) x 5",
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
