"""What the initial-guess store (Engine(guess_depth=), solve(guess="project"))
costs and saves on one MI355X. A GPU tool, not a test.

Cases (mode mixed, CGS, GMRES(30), to 1e-10), as tools/resolve_cost.py:
  lap1m    laplace:100 (LAP-1M), chebyshev with 4 sweeps
  band10m  band:1000000 (BAND-10M), jacobi, accum f32

  --what kernels   mpg_guess_dots_f64 / mpg_guess_update_f64 / mpg_guess_scale_f64 on
                   raw buffers of n rows and p columns, each launch between two HIP
                   events on the context's stream, the median of --reps after 3
                   warm-up launches; bytes = what the algorithm needs ((p + 1) 8n
                   for the dots, (p + 2) 8n for the update, 2 (p + 2) 8n for the
                   pair form, 4 * 8n for the scale) over 8 TB/s; and the launch
                   sequences of project (dots, update) and of keep without its
                   SpMV (dots, two pair updates, scale) between one pair of events.
  --what engine    per case: project as the engine runs it (the growth of
                   guess_info()["seconds"] over a re-arm with guess="project" on a
                   full store of depth 8: host clock around launches that end in a
                   synchronise, the SpMV-free xbar = 0 form) beside the whole
                   re-arm; keep by the number of columns held (SpMV, launches, the
                   read-back of the decision); and a sequence of 12 systems on the
                   curve of the CLI's --rhs-path 4, with and without
                   guess="project": restart cycles per system and the wall time
                   of re-arm + run.

usage: python tools/guess_bench.py --what kernels [--n 1000000] [--p 8] [--reps 25]
       python tools/guess_bench.py --what engine [--case lap1m --case band10m] [--reps 25]
One JSON line per measurement on stdout."""
import argparse
import ctypes as C
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
PEAK = 8e12  # bytes / s

CASES = {
    "lap1m": ("laplace:100", dict(mode="mixed", orth="cgs", prec="chebyshev", jacobi_steps=4, rlen=30, tol=1e-10)),
    "band10m": ("band:1000000", dict(mode="mixed", orth="cgs", prec="jacobi", accum="f32", rlen=30, tol=1e-10)),
}


def load():
    pkg = REPO / "icl-mixed-precision-gmres_amd"
    spec = importlib.util.spec_from_file_location("mpgmres_amd", pkg / "__init__.py",
                                                  submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mpgmres_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def med(v):
    return dict(median=statistics.median(v), lo=min(v), hi=max(v), runs=len(v))


class Events:
    """pairs of HIP events on one stream, read back in ms"""

    def __init__(self, mpg, stream):
        path = mpg.hip_runtime()
        self.rt = C.CDLL(path if path != "system" else "libamdhip64.so.7")
        self.stream = C.c_void_p(stream)
        for f in ("hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime", "hipEventDestroy"):
            getattr(self.rt, f).restype = C.c_int
        self.rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.rt.hipEventSynchronize.argtypes = [C.c_void_p]
        self.rt.hipEventDestroy.argtypes = [C.c_void_p]

    def _ck(self, st, what):
        if st != 0:
            raise RuntimeError(f"{what} failed ({st})")

    def time(self, fn, reps, warm=3):
        for _ in range(warm):
            fn()
        pairs = []
        for _ in range(reps):
            a, b = C.c_void_p(), C.c_void_p()
            self._ck(self.rt.hipEventCreate(C.byref(a)), "hipEventCreate")
            self._ck(self.rt.hipEventCreate(C.byref(b)), "hipEventCreate")
            self._ck(self.rt.hipEventRecord(a, self.stream), "hipEventRecord")
            fn()
            self._ck(self.rt.hipEventRecord(b, self.stream), "hipEventRecord")
            pairs.append((a, b))
        out = []
        for a, b in pairs:
            self._ck(self.rt.hipEventSynchronize(b), "hipEventSynchronize")
            ms = C.c_float()
            self._ck(self.rt.hipEventElapsedTime(C.byref(ms), a, b), "hipEventElapsedTime")
            out.append(ms.value * 1e-3)
            self.rt.hipEventDestroy(a), self.rt.hipEventDestroy(b)
        return out


def kernels(mpg, n, p, reps):
    lib = mpg.hip_lib()
    ctx = C.c_void_p()
    assert lib.mpg_ctx_create(0, C.byref(ctx)) == 0
    ev = Events(mpg, lib.mpg_ctx_stream(ctx))
    ld = (n + 31) // 32 * 32
    G = lib.mpg_guess_groups(n)
    rng = np.random.default_rng(5)

    def dev(arr_or_bytes):
        ptr = C.c_void_p()
        host = arr_or_bytes if isinstance(arr_or_bytes, np.ndarray) else None
        nbytes = host.nbytes if host is not None else int(arr_or_bytes)
        assert lib.mpg_malloc(ctx, nbytes, C.byref(ptr)) == 0
        if host is not None:
            assert lib.mpg_memcpy_h2d(ctx, ptr, host.ctypes.data, nbytes) == 0
        return ptr

    # (an orthonormal Q is not needed to time a pass; the coefficients stay O(1))
    Q = dev(rng.standard_normal(p * ld) / np.sqrt(n))
    Z = dev(rng.standard_normal(p * ld) / np.sqrt(n))
    r, y, w = (dev(rng.standard_normal(ld)) for _ in range(3))
    pa, pb, pc = (dev((p + 1) * G * 8) for _ in range(3))
    info = dev(64)
    qcol, zcol = dev(ld * 8), dev(ld * 8)
    at = lambda ptr, k: C.c_void_p(ptr.value + 8 * k)  # noqa: E731

    def ck(st):
        assert st == 0, lib.mpg_ctx_last_error(ctx)

    dots = lambda: ck(lib.mpg_guess_dots_f64(ctx, n, p, ld, Q, r, pa))  # noqa: E731
    upd = lambda: ck(lib.mpg_guess_update_f64(ctx, n, p, ld, pa, 1e-3, Z, y, y, None, None, None, None))  # noqa: E731
    pair1 = lambda: ck(lib.mpg_guess_update_f64(ctx, n, p, ld, pa, -1e-3, Z, y, y, Q, w, pb, None))  # noqa: E731
    pair2 = lambda: ck(lib.mpg_guess_update_f64(ctx, n, p, ld, pb, -1e-3, Z, y, y, Q, w, pc, None))  # noqa: E731
    scale = lambda: ck(lib.mpg_guess_scale_f64(ctx, n, at(pc, p * G), at(pa, p * G), 0.0, w, y, qcol, zcol, info))  # noqa: E731

    def project():
        dots(), upd()

    def keep():
        dots(), pair1(), pair2(), scale()

    n8 = 8.0 * n
    for name, fn, nbytes in (("k_guess_dots", dots, (p + 1) * n8), ("k_guess_update", upd, (p + 2) * n8),
                             ("k_guess_update pair", pair1, 2 * (p + 2) * n8), ("k_guess_scale", scale, 4 * n8),
                             ("project launches", project, (2 * p + 3) * n8),
                             ("keep launches (no SpMV)", keep, ((p + 1) + 4 * (p + 2) + 4) * n8)):
        t = ev.time(fn, reps)
        m = statistics.median(t)
        print(json.dumps(dict(what="kernels", name=name, n=n, p=p, groups=G, seconds=med(t), bytes=nbytes,
                              fraction_of_8TBs=nbytes / m / PEAK)), flush=True)
    assert lib.mpg_ctx_sync(ctx) == 0
    lib.mpg_ctx_destroy(ctx)


def path_x(mpg, n, j, K=4, seed=42):
    """x_true of system j on the CLI's --rhs-path K curve"""
    return sum(np.cos(0.37 * (k + 1) * j + k) * mpg.rand_vect(n, seed + k) for k in range(K))


def engine(mpg, name, reps):
    spec, opts = CASES[name]
    A = mpg.gen_spec(spec)
    n = A.nrows
    systems = []
    for j in range(8):
        xt = mpg.rand_vect(n, 42 + j)
        systems.append((mpg.host_spmv(A, xt), xt))
    e = mpg.Engine(A, *systems[0], guess_depth=8, **opts)
    try:
        xs, solve_s = [], []
        for j, (b, xt) in enumerate(systems):
            res = e.solve(b, x_true=xt) if j else e.solve()
            assert res.status == "converged"
            xs.append(e.x())
            solve_s.append(res.gmres_seconds)
        assert e.guess_info()["held"] == 8
        # project on the full store, beside the whole re-arm
        proj, arm, plain = [], [], []
        for i in range(reps + 3):
            b = systems[i % 8][0]
            s0 = e.guess_info()["seconds"]
            e.sync()
            t = time.perf_counter()
            e.rearm(b, guess="project")
            e.sync()
            wall = time.perf_counter() - t
            t = time.perf_counter()
            e.rearm(b)
            e.sync()
            wall0 = time.perf_counter() - t
            if i >= 3:
                proj.append(e.guess_info()["seconds"] - s0), arm.append(wall), plain.append(wall0)
        print(json.dumps(dict(what="project", case=name, n=n, held=8, project_seconds=med(proj),
                              rearm_with_project_seconds=med(arm), rearm_seconds=med(plain),
                              solve_seconds=med(solve_s[1:]))), flush=True)
        # keep by the number of columns held: the engine is handed x_j by a re-arm, no solve
        by_p = {p: [] for p in range(8)}
        for _ in range(5):
            e.set_guess_depth(0)
            e.set_guess_depth(8)
            for p in range(8):
                e.rearm(systems[p][0], x0=xs[p])
                s0 = e.guess_info()["seconds"]
                e.guess_keep()
                by_p[p].append(e.guess_info()["seconds"] - s0)
                assert e.guess_info()["held"] == p + 1
        print(json.dumps(dict(what="keep", case=name, n=n,
                              keep_seconds_by_held={p: med(v) for p, v in by_p.items()})), flush=True)
    finally:
        e.close()
    # 12 systems on the --rhs-path 4 curve, with and without the projected guess
    seq = []
    for j in range(12):
        xt = path_x(mpg, n, j)
        seq.append((mpg.host_spmv(A, xt), xt))
    for guess in (None, "project"):
        e = mpg.Engine(A, *seq[0], guess_depth=8 if guess else 0, **opts)
        try:
            cycles, iters, wall = [], [], []
            for j, (b, xt) in enumerate(seq):
                e.sync()
                t = time.perf_counter()
                res = e.solve(b, x_true=xt, guess=guess) if j else e.solve()
                wall.append(time.perf_counter() - t)
                assert res.status == "converged"
                cycles.append(int(res.restarts)), iters.append(int(res.total_iters))
            print(json.dumps(dict(what="sequence", case=name, guess=guess, cycles=cycles, iterations=iters,
                                  wall_seconds_per_system=[round(w, 6) for w in wall], wall_seconds=sum(wall),
                                  guess_info=e.guess_info())), flush=True)
        finally:
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernels", "engine"], required=True)
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--reps", type=int, default=25)
    args = ap.parse_args()
    mpg = load()
    if args.what == "kernels":
        kernels(mpg, args.n, args.p, args.reps)
    else:
        for name in args.case or list(CASES):
            engine(mpg, name, args.reps)


if __name__ == "__main__":
    main()
