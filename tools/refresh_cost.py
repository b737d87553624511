"""What a sequence of systems whose matrix values change pays per system on one
MI355X (tools/resolve_cost.py's sibling): mpg_engine_create's set-up against a
values refresh (Engine.refresh, mpg_engine_refresh_values) from host and from
device values, the re-arm that follows, and the refill kernel alone between
HIP events beside the build (whose fill it replaces). A GPU tool, not a test.

Cases as tools/resolve_cost.py (mode mixed, CGS, GMRES(30), to 1e-10):
  lap1m    laplace:100, chebyshev with 4 sweeps
  band10m  band:1000000, jacobi, accum f32

usage: python tools/refresh_cost.py [--rounds 5] [--case lap1m --case band10m] [--out FILE]
One JSON line per case: medians with ranges, seconds. The parent commit's
setup_seconds comes from `tools/resolve_cost.py --what create --tree PARENT` in
the same session."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from resolve_cost import CASES, REPO, load, med, run_to_done  # noqa: E402


def refill_alone(mpg, A, rounds):
    """mpg_sell_refresh_values on a stand-alone fp32 copy between two HIP events on the context's stream,
    and mpg_sell_create (analysis + fill + column compaction) by the wall clock"""
    import numpy as np

    hip = mpg.hip_lib()
    rt = C.CDLL(mpg.hip_runtime() if mpg.hip_runtime() != "system" else "libamdhip64.so")
    ctx = C.c_void_p()
    assert hip.mpg_ctx_create(0, C.byref(ctx)) == 0
    stream = C.c_void_p(hip.mpg_ctx_stream(ctx))

    def dev(a):
        p = C.c_void_p()
        assert hip.mpg_malloc(ctx, max(a.nbytes, 1), C.byref(p)) == 0
        assert hip.mpg_memcpy_h2d(ctx, p, a.ctypes.data, a.nbytes) == 0
        return p

    rp, ci = dev(A.rowptr), dev(A.col)
    v1, v2 = dev(A.val.astype(np.float32)), dev(mpg.perturb_values(A, 0.1, 1).astype(np.float32))
    csr, sell = C.c_void_p(), C.c_void_p()
    assert hip.mpg_csr_create(ctx, A.nrows, A.ncols, A.nnz, A.rowptr.ctypes.data, rp, ci, C.byref(csr)) == 0
    build = []
    for r in range(rounds + 1):
        if sell:
            hip.mpg_sell_destroy(sell)
        hip.mpg_ctx_sync(ctx)
        t = time.perf_counter()
        assert hip.mpg_sell_create(ctx, csr, 1, v1, 2, C.byref(sell)) == 0
        if r:
            build.append(time.perf_counter() - t)
    stored = C.c_int64()
    hip.mpg_sell_layout(sell, None, None, C.byref(stored), None)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert rt.hipEventCreate(C.byref(e)) == 0
    times = []
    for r in range(rounds + 1):
        assert rt.hipEventRecord(ev[0], stream) == 0
        assert hip.mpg_sell_refresh_values(ctx, sell, csr, 1, v2 if r % 2 == 0 else v1) == 0
        assert rt.hipEventRecord(ev[1], stream) == 0
        assert rt.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert rt.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        if r:
            times.append(ms.value * 1e-3)
    # the refill's bytes: nnz values and the row starts read, every padded slot written (fp32)
    nbytes = A.nnz * 4 + stored.value * 4 + (A.nrows + 1) * 4
    for e in ev:
        rt.hipEventDestroy(e)
    hip.mpg_sell_destroy(sell)
    hip.mpg_csr_destroy(csr)
    for p in (rp, ci, v1, v2):
        hip.mpg_free(ctx, p)
    hip.mpg_ctx_destroy(ctx)
    m = med(times)
    return dict(refill_seconds=m, refill_bytes=nbytes, refill_fraction_of_8TBps=nbytes / m["median"] / 8e12,
                sell_create_wall_seconds=med(build), stored=stored.value)


def case(mpg, name, rounds):
    import torch

    spec, opts = CASES[name]
    A = mpg.gen_spec(spec)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    setup = []
    for r in range(rounds + 1):  # (round 0: the process's first engine, not counted)
        e = mpg.Engine(A, b, xt, **opts)
        e.sync()
        res = e.report()
        if r < rounds:
            e.close()
        if r:
            setup.append(res.setup_seconds)
    host, device, wall_host, wall_dev, arm, solve = [], [], [], [], [], []
    try:
        run_to_done(e)
        for r in range(rounds + 1):
            v = mpg.perturb_values(A, 1e-3, 1 + r)
            vd = torch.from_numpy(v).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            t = time.perf_counter()
            e.refresh(v)
            wh = time.perf_counter() - t
            h = e.refresh_seconds
            t = time.perf_counter()
            e.refresh(vd)
            wd = time.perf_counter() - t
            d = e.refresh_seconds
            Av = mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, v)
            e.rearm(mpg.host_spmv(Av, xt), x_true=xt)
            s = run_to_done(e)
            res = e.report()
            assert res.status == "converged", res.status
            if r:
                host.append(h), device.append(d), wall_host.append(wh), wall_dev.append(wd)
                arm.append(res.setup_seconds), solve.append(s)
        captures = e.graph_captures
    finally:
        e.close()
    out = dict(case=name, spec=spec, opts=opts, nnz=A.nnz, setup_seconds=med(setup), refresh_host_seconds=med(host),
               refresh_device_seconds=med(device), refresh_host_wall_seconds=med(wall_host),
               refresh_device_wall_seconds=med(wall_dev), rearm_setup_seconds=med(arm), solve_seconds=med(solve),
               graph_captures=captures)
    out["refresh_device_over_setup"] = out["refresh_device_seconds"]["median"] / out["setup_seconds"]["median"]
    out.update(refill_alone(mpg, A, rounds))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=list(CASES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    mpg = load(REPO)
    for name in args.case or list(CASES):
        line = json.dumps(case(mpg, name, args.rounds))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
