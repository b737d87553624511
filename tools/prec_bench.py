"""GMRES it/s with each preconditioner on one MI355X (fused engine, mixed
CGS GMRES(m), tol = 0, fixed work): identity, Jacobi, the Jacobi-sweep
polynomial (neumann, 2 and 4 sweeps; chebyshev:2/3/4/6/8, gmres_poly:4/6/8 and neumann:6/8 on request), ILU(0) (sync-free triangular solves) and
ILU-Jacobi (5 sweeps), on LAP-1M (the 100^3 7-point Laplacian,
triangular-solve depth ~ 300) and a BAND matrix (depth = n).

--tol T adds a solve to that tolerance next to the fixed-work rate:
iterations, restarts and the wall time of the solve (gmres_seconds). A
preconditioner that changes the iteration count cannot be judged by it/s alone.

usage: python tools/prec_bench.py [--cycles 3] [--rlen 30] [--tol 1e-10] [--precs jacobi,neumann:2]"""
import argparse
import json
import sys
import time

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from __graft_entry__ import _load

# name -> (prec, jacobi_steps)
PRECS = {"identity": ("identity", 1), "jacobi": ("jacobi", 1), "neumann:2": ("neumann", 2), "neumann:4": ("neumann", 4),
         "ilu": ("ilu", 1), "ilu_jacobi": ("ilu_jacobi", 5),
         # on request (--precs): the Chebyshev polynomial, its interval from MPG_CHEB_RATIO / MPG_CHEB_LMAX
         "chebyshev:2": ("chebyshev", 2), "chebyshev:3": ("chebyshev", 3), "chebyshev:4": ("chebyshev", 4),
         "chebyshev:6": ("chebyshev", 6), "chebyshev:8": ("chebyshev", 8),
         # ... and the GMRES polynomial (no setting), with neumann at the same counts
         "gmres_poly:4": ("gmres_poly", 4), "gmres_poly:6": ("gmres_poly", 6), "gmres_poly:8": ("gmres_poly", 8),
         "neumann:6": ("neumann", 6), "neumann:8": ("neumann", 8)}
DEFAULT_PRECS = "identity,jacobi,neumann:2,neumann:4,ilu,ilu_jacobi"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--rlen", type=int, default=30)
    ap.add_argument("--tol", type=float, default=0.0, help="also solve to this tolerance (0: fixed work only)")
    ap.add_argument("--max-restarts", type=int, default=2000)
    ap.add_argument("--accum", default="f64", choices=["f64", "f32"])
    ap.add_argument("--precs", default=DEFAULT_PRECS)
    ap.add_argument("--matrices", default="LAP-1M,BAND-100k")
    args = ap.parse_args()
    mpg = _load()
    mats = {"LAP-1M": lambda: mpg.gen_laplace3d(100), "BAND-100k": lambda: mpg.gen_band(100_000, 5, 4, seed=7),
            "BAND-10M": lambda: mpg.gen_band(1_000_000, 5, 4, seed=7)}
    for name in args.matrices.split(","):
        A = mats[name]()
        xt = mpg.rand_vect(A.nrows, 42)
        b = mpg.host_spmv(A, xt)
        for pname in args.precs.split(","):
            prec, steps = PRECS[pname]
            opts = dict(mode="mixed", orth="cgs", prec=prec, jacobi_steps=steps, rlen=args.rlen, accum=args.accum)
            t0 = time.time()
            eng = mpg.Engine(A, b, xt, max_restarts=args.cycles + 3, tol=0.0, **opts)
            setup = time.time() - t0
            eng.run(1)
            eng.sync()
            it0 = eng.total_iters
            t = time.perf_counter()
            eng.run(args.cycles)
            eng.sync()
            dt = time.perf_counter() - t
            its = eng.total_iters - it0
            interval = eng.spmv_layout().get("prec_interval")
            eng.close()
            rec = {"matrix": name, "prec": pname, "rlen": args.rlen, "it_s": round(its / dt, 1),
                   "setup_s": round(setup, 3)}
            if interval:
                rec["prec_interval"] = [round(v, 6) for v in interval]
            if args.tol > 0:
                r = mpg.solve(A, b, xt, engine="fused", tol=args.tol, max_restarts=args.max_restarts, **opts)
                rec.update({"tol": args.tol, "status": r.status, "total_iters": int(r.total_iters),
                            "restarts": int(r.restarts), "gmres_seconds": round(r.gmres_seconds, 5),
                            "backward_error": float(r.cyc_r_norm[-1] / r.cyc_normalization[-1])})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
