"""Block-Jacobi measurements (profiles/r08_bjacobi/): the stand-alone apply at
C4's size, the C4 stand-in's step time under jacobi and under bjacobi in its
fused and separate forms (interleaved runs, medians), and solves to 1e-8 with
both preconditioners on C4 and on an intra-node x16 variant. One JSON file,
progress lines on stdout.

usage: python tools/bjacobi_bench.py [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from tests.conftest import load_package  # noqa: E402
from tests.devbuf import Hip  # noqa: E402

mpg = load_package()
out = {}


def say(*a):
    print(*a, flush=True)


# ---- 1. stand-alone apply, fp32, 3 * 111^3 rows
hip = Hip(mpg.hip_lib())
n = 3 * 111 ** 3
rng = np.random.default_rng(1)
d = hip.buf(rng.standard_normal(n * 3).astype(np.float32) * 0.3)
v = hip.buf(rng.standard_normal(n).astype(np.float32))
for _ in range(20):
    hip.call("mpg_bjacobi_apply_f32", n, 3, d.p, v.p)
hip.sync()
batches = []
for _ in range(9):
    t = time.perf_counter()
    for _ in range(200):
        hip.lib.mpg_bjacobi_apply_f32(hip.ctx, n, 3, d.p, v.p)
    hip.sync()
    batches.append((time.perf_counter() - t) / 200 * 1e6)
us = statistics.median(batches)
byts = n * (2 * 4 + 3 * 4)
out["apply_f32"] = {"rows": n, "bytes": byts, "us_per_launch_median": round(us, 2),
                    "us_batches": [round(b, 2) for b in batches], "gbs": round(byts / us / 1e3, 1),
                    "frac_8tbs": round(byts / (us * 1e-6) / 8e12, 3),
                    "method": "200 back-to-back launches on one stream between host syncs, 9 batches"}
say("apply", out["apply_f32"])
d.free(), v.free()
hip.close()

# ---- 2. C4 stand-in, mixed CGS GMRES(30), fixed work (tol 0): step time by preconditioner
t0 = time.time()
A = mpg.gen_stencil27(111, 3)
xt = mpg.rand_vect(A.nrows, 42)
b = mpg.host_spmv(A, xt)
say("C4 built", A.nrows, A.nnz, round(time.time() - t0, 1), "s")
forms = {"jacobi": dict(prec="jacobi"), "bjacobi_fused": dict(prec="bjacobi"),
         "bjacobi_separate": dict(prec="bjacobi")}
eng, lay = {}, {}
for name, o in forms.items():
    os.environ["MPG_BJACOBI_FUSE"] = "0" if name.endswith("separate") else "1"
    eng[name] = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", rlen=30, tol=0.0, max_restarts=10_000, accum="f32",
                           **o)
    lay[name] = eng[name].spmv_layout()
    eng[name].run(2)
    eng[name].sync()
    say(name, lay[name])
runs = {k: [] for k in forms}
for rep in range(7):  # interleaved
    for name in forms:
        e = eng[name]
        it0 = e.total_iters
        t = time.perf_counter()
        e.run(5)
        e.sync()
        dt = time.perf_counter() - t
        runs[name].append((e.total_iters - it0) / dt)
    say("rep", rep, {k: round(v[-1], 1) for k, v in runs.items()})
out["c4_step"] = {k: {"it_s_median": round(statistics.median(v), 1), "it_s_min": round(min(v), 1),
                      "it_s_max": round(max(v), 1), "us_per_step_median": round(1e6 / statistics.median(v), 2),
                      "layout": lay[k], "spmv_phase_bytes": eng[k].phase_bytes("spmv_storage")}
                  for k, v in runs.items()}
for e in eng.values():
    e.close()
say(out["c4_step"])

os.environ.pop("MPG_BJACOBI_FUSE", None)
# ---- 3. solves to 1e-8 on C4 (the default form)
out["c4_solve"] = {}
for prec in ("jacobi", "bjacobi"):
    r = mpg.solve(A, b, xt, engine="fused", mode="mixed", orth="cgs", prec=prec, rlen=30, tol=1e-8, max_restarts=200,
                  accum="f32")
    out["c4_solve"][prec] = {"status": r.status, "total_iters": int(r.total_iters), "restarts": int(r.restarts),
                             "gmres_seconds": round(r.gmres_seconds, 4), "setup_seconds": round(r.setup_seconds, 3),
                             "backward_error": float(r.cyc_r_norm[-1] / r.cyc_normalization[-1])}
    say(prec, out["c4_solve"][prec])
del A, b, xt

# ---- 4. the x16 intra-node variant (stencil27:64: the NumPy rescale of C4's 3.3e8 entries is left out)
from tests.test_bjacobi_gpu import intra_scaled  # noqa: E402

A = intra_scaled(mpg, mpg.gen_stencil27(64, 3), 16.0)
xt = mpg.rand_vect(A.nrows, 42)
b = mpg.host_spmv(A, xt)
out["intra16_solve"] = {"spec": "stencil27:64, intra-node off-diagonals x16", "n": A.nrows, "nnz": int(A.nnz)}
for prec in ("jacobi", "bjacobi"):
    r = mpg.solve(A, b, xt, engine="fused", mode="mixed", orth="cgs", prec=prec, rlen=30, tol=1e-8, max_restarts=200,
                  accum="f32")
    out["intra16_solve"][prec] = {"status": r.status, "total_iters": int(r.total_iters),
                                  "gmres_seconds": round(r.gmres_seconds, 4),
                                  "backward_error": float(r.cyc_r_norm[-1] / r.cyc_normalization[-1])}
    say(prec, out["intra16_solve"][prec])

OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/r08_bjacobi/bjacobi_bench.json"
os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
say("done")
