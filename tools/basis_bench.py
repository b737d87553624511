"""Measurements of the compressed Krylov basis (basis="f16") on
one MI355X, interleaved: every variant in rotation, medians with ranges.

Variants:
  f16        basis="f16" (plain launch forms by construction)
  f32plain   basis="f32" under MPG_STEP_DOTS=0 MPG_CGS_PREFETCH=0 MPG_TAIL_FOLD=0
  f32        basis="f32", the default plan with its fused launches

  --what panels   time_phase_dup of the dots and the CGS update (us per launch),
                  phase_bytes and the fraction of 8 TB/s: f16 against f32plain
  --what cycle    fixed-work it/s (tol 0): all three variants
  --what solve    gmres_seconds and cycles to 1e-10: f16 against f32

usage: python tools/basis_bench.py --what panels --case band:10000000 --case laplace:100 [--rounds 5]
One JSON line per (case, variant, quantity) on stdout."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests.conftest import load_package  # noqa: E402

PLAIN = {"MPG_STEP_DOTS": "0", "MPG_CGS_PREFETCH": "0", "MPG_TAIL_FOLD": "0"}
VARIANTS = {"f16": ("f16", {}), "f32plain": ("f32", PLAIN), "f32": ("f32", {})}
HBM = 8.0e12  # bytes / s


class env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def problem(mpg, spec):
    A = mpg.gen_spec(spec)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, mpg.host_spmv(A, xt), xt


def med(v):
    return dict(median=statistics.median(v), lo=min(v), hi=max(v), runs=len(v))


def panels(mpg, spec, P, args):
    out = {}
    for r in range(args.rounds):
        for name in ("f16", "f32plain"):
            basis, kv = VARIANTS[name]
            with env(kv):
                e = mpg.Engine(*P, mode="mixed", orth=args.orth, prec=args.prec, rlen=args.rlen, tol=0.0,
                               max_restarts=10 ** 6, accum=args.accum, basis=basis)
            try:
                e.run(2)
                for phase in ("dots", "cgs_update"):
                    ms, launches = e.time_phase_dup(phase, 5)
                    out.setdefault((name, phase), dict(us=[], bytes=e.phase_bytes(phase), launches=launches))["us"].append(
                        ms * 1e3)
            finally:
                e.close()
    for (name, phase), v in out.items():
        m = med(v["us"])
        print(json.dumps(dict(what="panel", case=spec, variant=name, phase=phase, rlen=args.rlen, us=m, bytes=v["bytes"],
                              hbm_fraction=v["bytes"] / (m["median"] * 1e-6) / HBM, launches=v["launches"])), flush=True)


def cycle(mpg, spec, P, args):
    out = {}
    for r in range(args.rounds):
        for name, (basis, kv) in VARIANTS.items():
            with env(kv):
                e = mpg.Engine(*P, mode="mixed", orth=args.orth, prec=args.prec, rlen=args.rlen, tol=0.0,
                               max_restarts=10 ** 6, accum=args.accum, basis=basis)
            try:
                e.run(args.warmup)
                e.sync()
                t = time.perf_counter()
                e.run(args.cycles)
                e.sync()
                dt = time.perf_counter() - t
                out.setdefault(name, []).append(args.cycles * args.rlen / dt)
            finally:
                e.close()
    for name, v in out.items():
        print(json.dumps(dict(what="cycle", case=spec, variant=name, rlen=args.rlen, its_per_s=med(v))), flush=True)


def solve(mpg, spec, P, args):
    out = {}
    for r in range(args.rounds):
        for name in ("f16", "f32"):
            basis, kv = VARIANTS[name]
            res = mpg.solve(*P, mode="mixed", orth=args.orth, prec=args.prec, jacobi_steps=args.jacobi_steps,
                            rlen=args.rlen, tol=1e-10, accum=args.accum, basis=basis, engine="fused")
            o = out.setdefault(name, dict(s=[], cycles=res.restarts, iters=res.total_iters, status=res.status))
            o["s"].append(res.gmres_seconds)
    for name, v in out.items():
        print(json.dumps(dict(what="solve", case=spec, variant=name, prec=args.prec, steps=args.jacobi_steps,
                              rlen=args.rlen, gmres_seconds=med(v["s"]), cycles=v["cycles"], iters=v["iters"],
                              status=v["status"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["panels", "cycle", "solve"], required=True)
    ap.add_argument("--case", action="append", required=True)
    ap.add_argument("--rlen", type=int, default=30)
    ap.add_argument("--orth", default="cgs")
    ap.add_argument("--prec", default="jacobi")
    ap.add_argument("--jacobi-steps", type=int, default=1)
    ap.add_argument("--accum", default="f32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    mpg = load_package()
    for spec in args.case:
        P = problem(mpg, spec)
        {"panels": panels, "cycle": cycle, "solve": solve}[args.what](mpg, spec, P, args)


if __name__ == "__main__":
    main()
