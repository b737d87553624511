"""Jacobi-sweep preconditioner measurements (profiles/r10_neumann/): what one
sweep launch costs inside the cycle, against the Arnoldi SpMV's in-cycle cost
measured in the same process (mpg_engine_time_phase_dup, phase 0).

The sweep's cost is a difference of whole cycles: engines with s = 1, 2, 3
sweeps run the same fixed work (mixed CGS GMRES(30), tol 0, fp32 accumulation
class) interleaved; a cycle applies the preconditioner m + 1 times (after the
prologue and after every SpMV), so one sweep launch costs
(t_cycle(s = 3) - t_cycle(s = 2)) / (m + 1): two graph replays that differ by
exactly that launch per application, the way time_phase_dup measures the SpMV.
(s = 2) - (s = 1) is what the first extra sweep costs per application: s = 1
runs as point Jacobi inside the SpMV, so it adds the gdmv launch, one sweep
and, once per cycle, the prologue's second norm. One JSON file, progress
lines on stdout.

usage: python tools/neumann_bench.py [out.json] [--matrices BAND-10M,LAP-1M]"""
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
    ap.add_argument("out", nargs="?", default="profiles/r10_neumann/neumann_bench.json")
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
        for s in (1, 2, 3):
            eng[s] = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="neumann", jacobi_steps=s, rlen=m, tol=0.0,
                                max_restarts=10_000_000, accum="f32")
            lay[s] = eng[s].spmv_layout()
            eng[s].run(3)
            eng[s].sync()
        say(name, lay[2])
        runs = {s: [] for s in eng}
        for rep in range(args.reps):  # interleaved
            for s, e in eng.items():
                t = time.perf_counter()
                e.run(args.cycles)
                e.sync()
                runs[s].append((time.perf_counter() - t) / args.cycles * 1e6)
            say("rep", rep, {s: round(v[-1], 1) for s, v in runs.items()})
        # the Arnoldi SpMV inside the s = 2 engine's cycle, same process
        spmv = []
        for _ in range(5):
            ms, added = eng[2].time_phase_dup("spmv", 5)
            spmv.append(ms * 1e3)  # (per added launch already)
        med = {s: statistics.median(v) for s, v in runs.items()}
        # per repetition, so that drift between repetitions cancels
        sweep = [(runs[3][i] - runs[2][i]) / (m + 1) for i in range(args.reps)]
        first = [(runs[2][i] - runs[1][i]) / (m + 1) for i in range(args.reps)]
        sv = statistics.median(spmv)
        n = float(A.nrows)
        out[name] = {
            "n": A.nrows, "nnz": int(A.nnz), "layout": lay[2],
            "cycle_us_median": {str(s): round(v, 1) for s, v in med.items()},
            "cycle_us_min_max": {str(s): [round(min(v), 1), round(max(v), 1)] for s, v in runs.items()},
            "sweep_us_in_cycle_median": round(statistics.median(sweep), 2),
            "sweep_us_in_cycle_min_max": [round(min(sweep), 2), round(max(sweep), 2)],
            "second_application_step_us_median": round(statistics.median(first), 2),
            "spmv_us_in_cycle_median": round(sv, 2),
            "spmv_us_in_cycle_min_max": [round(min(spmv), 2), round(max(spmv), 2)],
            "sweep_over_spmv": round(statistics.median(sweep) / sv, 3),
            "spmv_storage_bytes": eng[2].phase_bytes("spmv_storage"),
            "sweep_extra_vector_bytes": 3 * 4 * n,
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
