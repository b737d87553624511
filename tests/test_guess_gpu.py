"""The initial guess projected from earlier solutions on a live engine
(mpg_engine_guess_*, MPG_ARM_X0_PROJECT; Engine(guess_depth=), solve / rearm
(guess="project"), guess_info, guess_store; the CLI's --guess project
--rhs-path): the two kernels against fp64 on raw buffers, then recall, span,
the store's invariants, depth and restart, the re-imaging after a values
refresh, no change when off, determinism, the refusals and the CLI.

u = 2^-53 throughout. The bounds are the classical worst cases of the sums
involved (or follow from the projection being a least-squares fit), not
measurements."""
import ctypes as C
import dataclasses
import subprocess

import numpy as np
import pytest

from tests import guess_np as GS
from tests.test_cli_gpu import SUMMARY
from tests.test_resolve_gpu import BASE, _problem, _same

pytestmark = pytest.mark.gpu

U = GS.U
RLEN = BASE["rlen"]


# ---------------------------------------------------------------- 1. the kernels against fp64
def _ld(n):
    return (n + 32) // 32 * 32  # > n, even, a whole number of 256-byte lines


@pytest.mark.parametrize("nc", [1, 2, 7, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099, 70001])
def test_kernels_against_fp64(hip, n, nc):
    lib, ld = hip.lib, _ld(n)
    rng = np.random.default_rng(1000 * nc + n)
    G = lib.mpg_guess_groups(n)
    assert G >= 1
    SENT = -7.25  # what the padded rows hold: never read into a result, never written
    Qh = np.full((nc, ld), SENT)
    Zh = np.full((nc, ld), SENT)
    Qh[:, :n] = rng.standard_normal((nc, n))
    Zh[:, :n] = rng.standard_normal((nc, n)) * 10.0 ** rng.integers(-3, 3, (nc, 1))
    r = np.full(ld, SENT)
    xb = np.full(ld, SENT)
    wv = np.full(ld, SENT)
    r[:n], xb[:n], wv[:n] = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    Q, Z, rd = hip.buf(Qh), hip.buf(Zh), hip.buf(r)
    LD = np.longdouble

    def run():
        part, part2 = hip.buf((nc + 1) * G), hip.buf((nc + 1) * G)
        coef, coef2, info = hip.buf(nc + 1), hip.buf(nc + 1), hip.buf(3)
        y, y2, w = hip.buf(xb), hip.buf(xb), hip.buf(wv)
        qcol, zcol = hip.buf(np.full(ld, SENT)), hip.buf(np.full(ld, SENT))
        hip.call("mpg_guess_dots_f64", n, nc, ld, Q.p, rd.p, part.p)
        # project's form, in place: y = xbar + Z c
        hip.call("mpg_guess_update_f64", n, nc, ld, part.p, 1.0, Z.p, y.p, y.p, None, None, None, coef.p)
        # one Gram-Schmidt pass on (w, y2) with h = Q^T r, the next pass' dots in part2
        hip.call("mpg_guess_update_f64", n, nc, ld, part.p, -1.0, Z.p, y2.p, y2.p, Q.p, w.p, part2.p, None)
        # ... whose sums a further update reports (alpha = 0: y2 stays as it is)
        hip.call("mpg_guess_update_f64", n, nc, ld, part2.p, 0.0, Z.p, y2.p, y2.p, None, None, None, coef2.p)
        # the final form: nu^2 = ||w'||^2 (part2's last column), omega^2 = ||r||^2 (part's)
        hip.call("mpg_guess_scale_f64", n, part2.at(nc * G), part.at(nc * G), 1e-9, w.p, y2.p, qcol.p, zcol.p, info.p)
        hip.sync()
        out = [b.get() for b in (part, coef, y, y2, w, part2, coef2, qcol, zcol, info)]
        for b in (part, part2, coef, coef2, info, y, y2, w, qcol, zcol):
            b.free()
        return out

    first, again = run(), run()
    for a, b in zip(first, again):
        assert np.array_equal(a, b)  # two runs, the same bits
    part, coef, y, y2, w, part2, coef2, qcol, zcol, info = first
    Qn, Zn, rn = Qh[:, :n], Zh[:, :n], r[:n]

    # the dots: |c_j - q_j . r| <= n u sum_i |q_ij r_i|, and ||r||^2 likewise
    ref = (Qn.astype(LD) * rn.astype(LD)).sum(axis=1)
    cap = n * U * (np.abs(Qn) * np.abs(rn)).sum(axis=1)
    err = np.abs(coef[:nc].astype(LD) - ref).astype(np.float64)
    print(f"n {n} nc {nc}: dots err/cap {np.max(err / cap):.3g}")
    assert np.all(err <= cap)
    assert abs(float(coef[nc].astype(LD) - (rn.astype(LD) ** 2).sum())) <= n * U * float((rn * rn).sum())

    # the update, given the kernel's own c: |y_i - (xbar_i + sum_j z_ij c_j)| <= (nc + 1) u (|xbar_i| + sum_j |z_ij c_j|)
    c = coef[:nc]
    ref = xb[:n].astype(LD) + (Zn.astype(LD) * c.astype(LD)[:, None]).sum(axis=0)
    cap = (nc + 1) * U * (np.abs(xb[:n]) + (np.abs(Zn) * np.abs(c)[:, None]).sum(axis=0))
    err = np.abs(y[:n].astype(LD) - ref).astype(np.float64)
    print(f"n {n} nc {nc}: update err/cap {np.max(err / cap):.3g}")
    assert np.all(err <= cap)
    # the pair form: the same bound on d - Z h and on w - Q h
    for got, base, P in ((y2, xb, Zn), (w, wv, Qn)):
        ref = base[:n].astype(LD) - (P.astype(LD) * c.astype(LD)[:, None]).sum(axis=0)
        cap = (nc + 1) * U * (np.abs(base[:n]) + (np.abs(P) * np.abs(c)[:, None]).sum(axis=0))
        assert np.all(np.abs(got[:n].astype(LD) - ref).astype(np.float64) <= cap)
    # ... and its dots are those of the rows it wrote
    wn = w[:n]
    ref = (Qn.astype(LD) * wn.astype(LD)).sum(axis=1)
    assert np.all(np.abs(coef2[:nc].astype(LD) - ref).astype(np.float64) <= n * U * (np.abs(Qn) * np.abs(wn)).sum(axis=1))
    assert abs(float(coef2[nc].astype(LD) - (wn.astype(LD) ** 2).sum())) <= n * U * float((wn * wn).sum())
    # the final form: nu and omega (a square root of a sum within n u: one more rounding, half the relative error),
    # the columns w / nu and d / nu rounded once
    nu, om, kept = info
    assert kept == 1.0 and nu == np.sqrt(coef2[nc]) and om == np.sqrt(coef[nc])
    assert np.array_equal(qcol[:n], wn / nu) and np.array_equal(zcol[:n], y2[:n] / nu)
    # rows at and past n are left as found
    for v in (y, y2, w, qcol, zcol):
        assert np.all(v[n:] == SENT)


def test_kernel_argument_checks(hip):
    lib = hip.lib
    b = hip.buf(64)
    assert lib.mpg_guess_dots_f64(hip.ctx, 8, 17, 8, b.p, b.p, b.p) == -2  # more than a panel
    assert lib.mpg_guess_dots_f64(hip.ctx, 8, 1, 6, b.p, b.p, b.p) == -2  # ld < n
    assert lib.mpg_guess_dots_f64(hip.ctx, 8, 1, 9, b.p, b.p, b.p) == -2  # odd ld: columns off 16 bytes
    assert lib.mpg_guess_dots_f64(hip.ctx, 8, 1, 8, b.at(1), b.p, b.p) == -2  # a panel off 16 bytes
    assert lib.mpg_guess_update_f64(hip.ctx, 8, 0, 8, b.p, 1.0, b.p, None, b.p, None, None, None, None) == -2
    assert lib.mpg_guess_update_f64(hip.ctx, 8, 1, 8, b.p, 1.0, b.p, None, b.p, b.p, None, None, None) == -2  # half a pair
    b.free()


# ---------------------------------------------------------------- the engine
CASES = [("lap12", "mixed"), ("band4099", "mixed"), ("convdiff32", "mixed"), ("convdiff32", "baseline")]
IDS = [f"{k}-{m}" for k, m in CASES]
_rhs_cache = {}


def _setup(mpg, key, mode):
    """(A, the matrix of the residual prologue, [(b, x_true)] for four right-hand sides, the options)"""
    A, rhs = _problem(mpg, key)
    if key not in _rhs_cache:
        more = []
        for seed in (44, 45):
            xt = mpg.rand_vect(A.nrows, seed)
            more.append((mpg.host_spmv(A, xt), xt))
        _rhs_cache[key] = list(rhs) + more
    opts = dict(BASE, mode=mode)
    Ar = A if mode != "baseline" else dataclasses.replace(A, val=A.val.astype(np.float32).astype(np.float64))
    return A, Ar, _rhs_cache[key], opts


def _recall_cap(first, again, n):
    return (1 + 1e-6) * first.cyc_r_norm[-1] + n * U * again.cyc_normalization[0]


def _check_store(mpg, Ar, e):
    Z, Q = e.guess_store()
    n, p = Ar.nrows, Z.shape[1]
    assert p == e.guess_info()["held"] and p >= 1
    orth = GS.orth_defect(Q)
    print(f"held {p}: max|Q^T Q - I| {orth:.3g} (cap {p * n * U:.3g})")
    assert orth <= p * n * U
    for j, (err, znorm) in enumerate(GS.image_defects(lambda v: mpg.host_spmv(Ar, v), Z, Q)):
        cap = n * U * np.linalg.norm(Ar.val) * znorm
        print(f"  column {j}: ||q - A z|| {err:.3g} (cap {cap:.3g})")
        assert err <= cap
    return Z, Q


@pytest.mark.parametrize("key,mode", CASES, ids=IDS)
def test_recall(mpg, key, mode):
    A, Ar, rhs, opts = _setup(mpg, key, mode)
    b1, xt1 = rhs[0]
    e = mpg.Engine(A, b1, xt1, guess_depth=8, **opts)
    try:
        first = e.solve()
        assert first.status == "converged" and e.guess_info()["held"] == 1
        again = e.solve(b1, x_true=xt1, guess="project")
        info = e.guess_info()
        print(key, mode, "cold", first.total_iters, "recall", again.total_iters, "r0", again.cyc_r_norm[0], "cap",
              _recall_cap(first, again, A.nrows), info)
        assert again.status == "converged" and again.total_iters <= RLEN
        assert again.cyc_r_norm[0] <= _recall_cap(first, again, A.nrows)
        assert info["held"] == 1 and info["depth"] == 8  # the second keep found nothing new
        assert info["rho1"] <= info["rho0"] and info["seconds"] > 0
    finally:
        e.close()


@pytest.mark.parametrize("key,mode", CASES, ids=IDS)
def test_span(mpg, key, mode):
    A, Ar, rhs, opts = _setup(mpg, key, mode)
    (b1, xt1), (b2, xt2) = rhs[:2]
    b3, xt3 = 2 * b1 - 3 * b2, 2 * xt1 - 3 * xt2
    n = A.nrows
    e = mpg.Engine(A, b1, xt1, guess_depth=8, **opts)
    try:
        r1 = e.solve()
        r2 = e.solve(b2, x_true=xt2)
        assert e.guess_info()["held"] == 2
        x_prev = e.x()
        r3 = e.solve(b3, x_true=xt3, guess="project")
        cap = (1 + 1e-6) * (2 * r1.cyc_r_norm[-1] + 3 * r2.cyc_r_norm[-1]) + n * U * r3.cyc_normalization[0]
        print(key, mode, "r0", r3.cyc_r_norm[0], "cap", cap, "iters", r3.total_iters)
        assert r3.cyc_r_norm[0] <= cap
        assert r3.status == "converged" and r3.total_iters <= RLEN
        warm = e.solve(b3, x0=x_prev, x_true=xt3)  # the best guess without the store: the previous solution
        print("  from the previous solution:", warm.total_iters)
        assert warm.status == "converged" and warm.total_iters > r3.total_iters
    finally:
        e.close()


@pytest.mark.parametrize("key,mode", CASES, ids=IDS)
def test_store_invariants(mpg, key, mode):
    A, Ar, rhs, opts = _setup(mpg, key, mode)
    e = mpg.Engine(A, *rhs[0], guess_depth=8, **opts)
    try:
        e.solve()
        for b, xt in rhs[1:4]:
            e.solve(b, x_true=xt)
        assert e.guess_info()["held"] == 4
        _check_store(mpg, Ar, e)
    finally:
        e.close()


def test_depth_and_restart(mpg):
    A, Ar, rhs, opts = _setup(mpg, "lap12", "mixed")
    e = mpg.Engine(A, *rhs[0], guess_depth=2, **opts)
    try:
        e.solve()
        assert e.guess_info()["held"] == 1
        e.solve(*rhs[1][:1], x_true=rhs[1][1])
        assert e.guess_info()["held"] == 2
        third = e.solve(rhs[2][0], x_true=rhs[2][1])
        assert e.guess_info()["held"] == 1  # full on entry: the newest solution alone reseeds it
        again = e.solve(rhs[2][0], x_true=rhs[2][1], guess="project")
        assert again.total_iters <= RLEN and again.cyc_r_norm[0] <= _recall_cap(third, again, A.nrows)
        assert e.guess_info()["held"] == 1
        e.set_guess_depth(4)  # another depth empties it
        assert e.guess_info()["held"] == 0 and e.guess_info()["depth"] == 4
        Z, Q = e.guess_store()
        assert Z.shape == (A.nrows, 0) and Q.shape == (A.nrows, 0)
        cold = e.solve(rhs[2][0], x_true=rhs[2][1], guess="project")  # an empty store projects to xbar
        assert cold.total_iters == third.total_iters and e.guess_info()["held"] == 1
        e.set_guess_depth(0)  # frees it
        assert e.guess_info()["held"] == 0 and e.guess_info()["depth"] == 0
        with pytest.raises(RuntimeError, match=r"\(-5\).*depth"):
            e.solve(rhs[1][0], guess="project")
        assert e.solve(rhs[1][0], x_true=rhs[1][1]).status == "converged"
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            e.set_guess_depth(17)
    finally:
        e.close()


@pytest.mark.parametrize("key,mode", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_refresh_keeps_the_span(mpg, key, mode):
    A, Ar, rhs, opts = _setup(mpg, key, mode)
    e = mpg.Engine(A, *rhs[0], guess_depth=8, **opts)
    try:
        e.solve()
        e.solve(rhs[1][0], x_true=rhs[1][1])
        v2 = mpg.perturb_values(A, 1e-3, 1)
        A2 = dataclasses.replace(A, val=v2)
        A2r = A2 if mode != "baseline" else dataclasses.replace(A, val=v2.astype(np.float32).astype(np.float64))
        e.refresh(v2)
        t_refresh, s0 = e.refresh_seconds, e.guess_info()["seconds"]
        xt = rhs[2][1]
        b = mpg.host_spmv(A2, xt)
        e.rearm(b, x_true=xt, guess="project")
        info = e.guess_info()
        print(key, mode, info, "refresh", t_refresh)
        assert info["held"] == 2 and info["rho1"] <= info["rho0"]
        assert e.refresh_seconds == t_refresh and info["seconds"] > s0  # the re-imaging is the store's time
        _check_store(mpg, A2r, e)
        r = e.solve()
        assert r.status == "converged" and e.guess_info()["held"] == 3
        _check_store(mpg, A2r, e)
    finally:
        e.close()


def test_no_change_when_off(mpg):
    A, Ar, rhs, opts = _setup(mpg, "band4099", "mixed")
    (b1, xt1), (b2, xt2) = rhs[:2]
    with_store, without = mpg.Engine(A, b1, xt1, guess_depth=8, **opts), mpg.Engine(A, b1, xt1, **opts)
    try:
        for label, args in (("first", {}), ("second", dict(b=b2, x_true=xt2)), ("first again", dict(b=b1, x_true=xt1))):
            _same(with_store.solve(**args), without.solve(**args), label)
        assert with_store.guess_info()["held"] == 2 and without.guess_info() == dict(held=0, depth=0, rho0=0.0,
                                                                                      rho1=0.0, seconds=0.0)
    finally:
        with_store.close()
        without.close()


def test_determinism(mpg):
    A, Ar, rhs, opts = _setup(mpg, "convdiff32", "mixed")
    runs = []
    for _ in range(2):
        e = mpg.Engine(A, *rhs[0], guess_depth=8, **opts)
        try:
            res = [e.solve()]
            for b, xt in rhs[1:3]:
                res.append(e.solve(b, x_true=xt, guess="project"))
            res.append(e.solve(2 * rhs[0][0] + rhs[2][0], guess="project"))
            runs.append((res, e.guess_store(), e.guess_info()))
        finally:
            e.close()
    (ra, (Za, Qa), ia), (rb, (Zb, Qb), ib) = runs
    for j, (a, b) in enumerate(zip(ra, rb)):
        _same(a, b, f"solve {j}")
    assert np.array_equal(Za, Zb) and np.array_equal(Qa, Qb)
    assert {k: v for k, v in ia.items() if k != "seconds"} == {k: v for k, v in ib.items() if k != "seconds"}


def test_base_guess_is_honoured(mpg):
    """Engine.x right after rearm(b, x0 = xbar, guess = "project") is xbar + Z c of the restatement, c = Q^T (b -
    A xbar) on the engine's own store. Per element the update's bound of test 1, (p + 1) u (|xbar_i| + sum_j |z_ij
    c_j|), plus sum_j |z_ij| dc_j for the two sides' different c: dc_j <= 2 n u sum_i |q_ij r_i| (either side's dot,
    test 1's bound) + sum_i |q_ij| dr_i, dr_i <= 2 (row length + 1) u (|b_i| + (|A| |xbar|)_i) (either side's
    SpMV and subtraction)."""
    A, Ar, rhs, opts = _setup(mpg, "lap12", "mixed")
    n = A.nrows
    e = mpg.Engine(A, *rhs[0], guess_depth=8, **opts)
    try:
        e.solve()
        e.solve(rhs[1][0], x_true=rhs[1][1])
        Z, Q = e.guess_store()
        p = Z.shape[1]
        assert p == 2
        b, xt = rhs[2]
        xbar = xt + 1e-4 * mpg.rand_vect(n, 7)
        e.rearm(b, x0=xbar, x_true=xt, guess="project")
        x = e.x()
        st = GS.Store(lambda v: mpg.host_spmv(Ar, v), n, 8, opts["tol"])
        st.Z[:, :p], st.Q[:, :p], st.held = Z, Q, p
        want = st.project(b, xbar)
        r, c = st.coefficients(b, xbar)
        absA = dataclasses.replace(Ar, val=np.abs(Ar.val))
        rowlen = int(np.diff(Ar.rowptr).max())
        dr = 2 * (rowlen + 1) * U * (np.abs(b) + mpg.host_spmv(absA, np.abs(xbar)))
        dc = 2 * n * U * (np.abs(Q) * np.abs(r)[:, None]).sum(axis=0) + np.abs(Q).T @ dr
        cap = (p + 1) * U * (np.abs(xbar) + np.abs(Z) @ np.abs(c)) + np.abs(Z) @ dc
        err = np.abs(x - want)
        print("base guess: max err/cap", np.max(err / cap), "moved", np.abs(x - xbar).max())
        assert np.all(err <= cap) and not np.array_equal(x, xbar)
        info = e.guess_info()
        assert info["rho0"] == pytest.approx(st.rho0, rel=1e-9) and info["rho1"] <= info["rho0"]
        res = e.solve()
        assert res.status == "converged" and res.cyc_r_norm[0] == pytest.approx(info["rho1"], rel=1e-3)
    finally:
        e.close()


# ---------------------------------------------------------------- refusals
def test_refused_without_a_depth(mpg):
    A, Ar, rhs, opts = _setup(mpg, "lap12", "mixed")
    e = mpg.Engine(A, *rhs[0], **opts)
    try:
        first = e.solve()
        with pytest.raises(RuntimeError, match=r"\(-5\).*depth"):
            e.solve(rhs[1][0], guess="project")
        with pytest.raises(RuntimeError, match=r"\(-5\).*depth"):
            e.guess_keep()
        with pytest.raises(ValueError):
            e.solve(rhs[1][0], guess="previous")
        _same(e.solve(rhs[0][0], x_true=rhs[0][1]), first, "after the refusals")
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["single", "single-prec"])
def test_refused_in_the_fp32_modes(mpg, mode):
    A, Ar, rhs, opts = _setup(mpg, "lap12", "mixed")
    opts = dict(opts, mode=mode, tol=1e-5)
    with pytest.raises(RuntimeError, match=r"\(-5\).*" + mode):
        mpg.Engine(A, *rhs[0], guess_depth=4, **opts)
    e = mpg.Engine(A, *rhs[0], **opts)
    try:
        with pytest.raises(RuntimeError, match=r"\(-5\).*" + mode):
            e.set_guess_depth(4)
        assert e.guess_info()["depth"] == 0
        assert e.solve().status == "converged"
    finally:
        e.close()


def test_refused_after_measurement_launches(mpg):
    A, Ar, rhs, opts = _setup(mpg, "band4099", "mixed")
    e = mpg.Engine(A, *rhs[0], guess_depth=4, **opts)
    try:
        e.solve()
        e.time_phase("spmv", 2)
        with pytest.raises(RuntimeError, match=r"\(-5\).*measurement launches"):
            e.guess_keep()
        with pytest.raises(RuntimeError, match=r"\(-5\).*measurement launches"):
            e.solve(rhs[1][0], guess="project")
        with pytest.raises(RuntimeError, match=r"\(-5\).*measurement launches"):
            e.set_guess_depth(8)
        assert e.guess_info()["held"] == 1
    finally:
        e.close()


def test_refused_on_a_row_partitioned_engine(mpg):
    A = mpg.gen_band(20_000, 5, 4, seed=7)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    plan = mpg.HaloPlan(0, 1, [0, A.nrows], A)
    e = mpg.Engine.distributed(A, b, xt, plan, mpg.rccl_unique_id(), 1, 0, **BASE)
    try:
        with pytest.raises(RuntimeError, match=r"\(-5\).*row-partitioned"):
            e.set_guess_depth(4)
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            e.guess_keep()
        ran, done = e.run(40)
        assert done and e.report().status == "converged"
    finally:
        e.close()


# ---------------------------------------------------------------- the CLI
CLI_ARGS = ["--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec", "jacobi", "--tol",
            "1e-9", "--gpu", "--solves", "5", "--rhs-path", "2"]


def test_cli_guess_project(mpg):
    run = lambda extra: subprocess.run([str(mpg.CLI)] + CLI_ARGS + extra, capture_output=True, text=True,  # noqa: E731
                                       timeout=120)
    cold, proj = run([]), run(["--guess", "project"])
    assert cold.returncode == 0 and proj.returncode == 0, (cold.stderr, proj.stderr)
    fc, fp = SUMMARY.findall(cold.stdout), SUMMARY.findall(proj.stdout)
    assert len(fc) == 5 and len(fp) == 5, proj.stdout
    for out in (cold.stdout, proj.stdout):
        assert out.count("||x|| = ") == 5 and out.count("Doing Mixed Precision test") == 5
    # the same systems, the same lines: everything but the solve's own figures
    norms = lambda out: [ln for ln in out.splitlines() if ln.startswith("||")]  # noqa: E731
    assert norms(cold.stdout) == norms(proj.stdout) and len(norms(cold.stdout)) == 15
    assert "guess" not in proj.stdout and "guess" not in cold.stderr
    assert proj.stderr.count("guess: system") == 4 and " -> " in proj.stderr
    cyc_c, cyc_p = [int(f[2]) for f in fc], [int(f[2]) for f in fp]
    it_c, it_p = [int(f[3]) for f in fc], [int(f[3]) for f in fp]
    print("cycles cold", cyc_c, "projected", cyc_p, "iterations", it_c, it_p)
    assert cyc_c[0] == cyc_p[0] and it_c[0] == it_p[0]  # the first system has no guess
    for j in range(2, 5):
        assert cyc_p[j] <= cyc_c[j]
    for j in range(3, 5):
        assert cyc_p[j] < cyc_c[j]
