"""prec_values measurements (profiles/r23_prec_values/): the polynomial
preconditioners' sweeps on the fp32 values against the fp16 copy of A.

--part sweeps: one SELL sweep launch (Neumann and Chebyshev epilogue) on the
fp32 copy and on the fp16 copy with its row exponents, each launch between two
HIP events on the context's stream, f32 and f16 alternating in one process,
medians of --reps launches after a warm-up. Bytes by the model of
FusedEngine::phase_bytes: the copy's own bytes (mpg_sell_bytes, plus n exponent
bytes for fp16), the gathered vector, the lane's own operands (r, d, z; z_prev
for Chebyshev) and the store.
--part solves: mixed CGS GMRES(30) to 1e-10 in the fp32 accumulation class
(bench.py's), prec_values f32 against f16 in alternating pairs, median of
--pairs; time is the solve's own (gmres_seconds).

One process per (part, matrix), so that the caller gives each its own time
limit; every result is one JSON line appended to the output file.

usage: python tools/prec_values_bench.py --part sweeps --matrix LAP-1M [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from tests.conftest import load_package  # noqa: E402

MATS = {"LAP-1M": lambda m: m.gen_laplace3d(100), "LAP-200": lambda m: m.gen_laplace3d(200),
        "BAND-10M": lambda m: m.gen_band(1_000_000, 5, 4, seed=7)}
SOLVES = {"LAP-1M": [("chebyshev", 4), ("gmres_poly", 4)], "LAP-200": [("chebyshev", 4), ("gmres_poly", 4)],
          "BAND-10M": [("gmres_poly", 4)]}
PEAK = 8.0e12  # bytes per second


def say(*a):
    print(*a, flush=True)


class Events:
    """Two HIP events on a stream; us(fn): the device time between them around fn()."""

    def __init__(self, stream):
        self.rt = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.rt.hipEventCreate(C.byref(e)) == 0

    def us(self, fn):
        assert self.rt.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.rt.hipEventRecord(self.b, self.stream) == 0
        assert self.rt.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.rt.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3


def sweeps(mpg, name, reps, warm):
    from tests.devbuf import Hip

    hip = Hip(mpg.hip_lib())
    lib = hip.lib
    lib.mpg_ctx_stream.restype = C.c_void_p
    lib.mpg_ctx_stream.argtypes = [C.c_void_p]
    lib.mpg_sell_bytes.restype = C.c_int64
    ev = Events(lib.mpg_ctx_stream(hip.ctx))
    A = MATS[name](mpg)
    n, nnz = A.nrows, int(A.nnz)
    rp, col = hip.buf(A.rowptr, np.int32), hip.buf(A.col, np.int32)
    csr = C.c_void_p()
    hip.call("mpg_csr_create", n, n, nnz, A.rowptr.ctypes.data, rp.p, col.p, C.byref(csr))
    v64, v32 = hip.buf(A.val), hip.buf(A.val.astype(np.float32))
    half, rexp = hip.buf(nnz, np.uint16), hip.buf(n + 64, np.int8)
    stats = (C.c_int64 * 4)()
    hip.call("mpg_csr_half_values", csr, v64.p, 1, half.p, rexp.p, stats)
    s32, s16 = C.c_void_p(), C.c_void_p()
    hip.call("mpg_sell_create", csr, 1, v32.p, 2, C.byref(s32))
    hip.call("mpg_sell_create", csr, 2, half.p, 2, C.byref(s16))
    rng = np.random.default_rng(1)
    d, r, z, zp = (hip.buf(rng.uniform(0.01, 0.1, n).astype(np.float32)) for _ in range(4))
    o = hip.buf(n, np.float32)
    cf = C.c_float
    launch = {
        ("neumann", "f32"): lambda: lib.mpg_sell_jacobi_sweep_f32(hip.ctx, s32, d.p, r.p, z.p, o.p),
        ("neumann", "f16"): lambda: lib.mpg_sell_jacobi_sweep_f16f32(hip.ctx, s16, rexp.p, d.p, r.p, z.p, o.p),
        ("chebyshev", "f32"): lambda: lib.mpg_sell_cheb_sweep_f32(hip.ctx, s32, d.p, r.p, z.p, zp.p, o.p, cf(0.3), cf(1.1)),
        ("chebyshev", "f16"): lambda: lib.mpg_sell_cheb_sweep_f16f32(hip.ctx, s16, rexp.p, d.p, r.p, z.p, zp.p, o.p,
                                                                    cf(0.3), cf(1.1)),
    }
    times = {k: [] for k in launch}
    for it in range(warm + reps):  # alternating
        for k, fn in launch.items():
            st = []
            t = ev.us(lambda: st.append(fn()))
            assert st == [0], (k, st)
            if it >= warm:
                times[k].append(t)
    mat = {"f32": int(lib.mpg_sell_bytes(s32)), "f16": int(lib.mpg_sell_bytes(s16)) + n}
    res = {"part": "sweeps", "matrix": name, "n": n, "nnz": nnz, "scaled_rows": int(stats[0]), "reps": reps}
    for ep, nvec in (("neumann", 5), ("chebyshev", 6)):
        for v in ("f32", "f16"):
            us = statistics.median(times[ep, v])
            by = mat[v] + nvec * 4 * n
            res[f"{ep}_{v}"] = {"us_median": round(us, 2), "us_min": round(min(times[ep, v]), 2),
                                "us_max": round(max(times[ep, v]), 2), "bytes": by,
                                "fraction_of_8TBs": round(by / (us * 1e-6) / PEAK, 3)}
        res[f"{ep}_f16_over_f32"] = round(res[f"{ep}_f16"]["us_median"] / res[f"{ep}_f32"]["us_median"], 3)
        res[f"{ep}_bytes_f16_over_f32"] = round(res[f"{ep}_f16"]["bytes"] / res[f"{ep}_f32"]["bytes"], 3)
    for s in (s32, s16):
        lib.mpg_sell_destroy(s)
    lib.mpg_csr_destroy(csr)
    hip.close()
    return [res]


def solves(mpg, name, pairs):
    A = MATS[name](mpg)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    out = []
    for prec, s in SOLVES[name]:
        opts = dict(engine="fused", mode="mixed", orth="cgs", prec=prec, jacobi_steps=s, rlen=30, tol=1e-10,
                    max_restarts=500, accum="f32")
        runs = {"f32": [], "f16": []}
        for p in range(pairs + 1):  # (the first pair warms up)
            for v in runs:
                r = mpg.solve(A, b, xt, prec_values=v, **opts)
                if p:
                    runs[v].append(r)
                say(name, prec, s, v, r.status, r.total_iters, round(r.gmres_seconds * 1e3, 3), "ms")
        res = {"part": "solves", "matrix": name, "n": A.nrows, "prec": prec, "sweeps": s, "pairs": pairs}
        for v, rs in runs.items():
            res[v] = {"ms_median": round(statistics.median(r.gmres_seconds for r in rs) * 1e3, 3),
                      "ms_min": round(min(r.gmres_seconds for r in rs) * 1e3, 3),
                      "ms_max": round(max(r.gmres_seconds for r in rs) * 1e3, 3),
                      "iterations": rs[-1].total_iters, "status": rs[-1].status, "res_norm": rs[-1].res_norm}
        res["f16_over_f32"] = round(res["f16"]["ms_median"] / res["f32"]["ms_median"], 3)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sweeps", "solves"], required=True)
    ap.add_argument("--matrix", choices=sorted(MATS), required=True)
    ap.add_argument("--out", default="profiles/r23_prec_values/prec_values_bench.jsonl")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    args = ap.parse_args()
    mpg = load_package()
    res = sweeps(mpg, args.matrix, args.reps, args.warmup) if args.part == "sweeps" else solves(mpg, args.matrix, args.pairs)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        for r in res:
            say(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
