"""prec_values = "f16": the polynomial preconditioners' sweeps on an fp16 copy
of A (2 bytes per value, int8 row exponents), against the same sweeps on the
dequantised fp32 values (bit for bit), against an fp64 evaluation of the stated
formula, in whole solves (f16 = f16emu), on a live engine, the refusals, the CLI.

The matrices (tests/prec_values_np.py) have values that fp16 does not hold
exactly: the generators' Laplacian (6 and -1) would test nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import prec_values_np as pv
from tests.arnoldi_phase import MPG_F16, MPG_F32, PhaseWorkspace, gen_far33k, gen_far66k

pytestmark = pytest.mark.gpu

F32 = np.float32
PV_F32, PV_F16, PV_F16EMU = 0, 1, 2
POLY_STEP, POLY_PAIR = 0, 1
U32 = 2.0 ** -24  # unit roundoff of the vectors' type


# ---------------------------------------------------------------- helpers
_made = {}


def _matrix(mpg, name):
    if name not in _made:
        _made[name] = {"far33k": gen_far33k, "far66k": gen_far66k}.get(name, pv.MATRICES.get(name))(mpg)
    return _made[name]


def _problem(mpg, name):
    A = _matrix(mpg, name)
    xt = mpg.rand_vect(A.nrows, 42)
    return A, mpg.host_spmv(A, xt), xt


def _same(a, b, what):
    assert a.status == b.status and a.restarts == b.restarts and a.total_iters == b.total_iters, what
    np.testing.assert_array_equal(a.step_res, b.step_res, err_msg=what)
    np.testing.assert_array_equal(a.cyc_r_norm, b.cyc_r_norm, err_msg=what)
    np.testing.assert_array_equal(a.x, b.x, err_msg=what)


class Copies:
    """A on the device: the CSR structure, the fp16 copy of mpg_csr_half_values
    (scale = 1) with its exponents, the dequantised fp32 values of
    mpg_csr_half_dequant_f32, and on request SELL copies of both."""

    def __init__(self, hip, A, sell=False):
        self.hip, self.n, lib = hip, A.nrows, hip.lib
        self.rp, self.col = hip.buf(A.rowptr, np.int32), hip.buf(A.col, np.int32)
        self.csr = C.c_void_p()
        hip.call("mpg_csr_create", A.nrows, A.ncols, A.nnz, A.rowptr.ctypes.data, self.rp.p, self.col.p,
                 C.byref(self.csr))
        v64 = hip.buf(A.val)
        self.half, self.rexp, self.hat = hip.buf(A.nnz, np.uint16), hip.buf(A.nrows + 64, np.int8), hip.buf(A.nnz, F32)
        stats, bad = (C.c_int64 * 4)(), C.c_int64(-1)
        hip.call("mpg_csr_half_values", self.csr, v64.p, 1, self.half.p, self.rexp.p, stats)
        hip.call("mpg_csr_half_dequant_f32", self.csr, self.half.p, self.rexp.p, self.hat.p, C.byref(bad))
        v64.free()
        assert bad.value == 0
        self.scaled_rows = stats[0]
        self.sell16, self.sell32 = C.c_void_p(), C.c_void_p()
        if sell:
            hip.call("mpg_sell_create", self.csr, MPG_F16, self.half.p, 2, C.byref(self.sell16))
            hip.call("mpg_sell_create", self.csr, MPG_F32, self.hat.p, 2, C.byref(self.sell32))
            assert self.sell16.value and self.sell32.value

    def form(self):
        """(column form, CSR-summed slices, implicit slices) of the fp16 SELL copy."""
        form, exc, imp = C.c_int32(), C.c_int64(), C.c_int64()
        self.hip.check(self.hip.lib.mpg_sell_columns(self.sell16, C.byref(form), C.byref(exc), C.byref(imp)))
        return form.value, exc.value, imp.value

    def close(self):
        for s in (self.sell16, self.sell32):
            if s.value:
                self.hip.lib.mpg_sell_destroy(s)
        self.hip.lib.mpg_csr_destroy(self.csr)
        for b in (self.rp, self.col, self.half, self.rexp, self.hat):
            b.free()


def _vectors(n, seed, count=4):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.04, 0.25, n).astype(F32)] + [rng.standard_normal(n).astype(F32) for _ in range(count - 1)]


# ---------------------------------------------------------------- 0. the device's A^ is the restatement's
@pytest.mark.parametrize("name", sorted(pv.MATRICES))
def test_device_values_are_the_restatements(mpg, hip, name):
    A = _matrix(mpg, name)
    S = Copies(hip, A)
    try:
        h, e = pv.half_values(A)
        assert np.array_equal(S.half.get(), h.view(np.uint16))
        assert np.array_equal(S.rexp.get()[:A.nrows], e)
        hat = S.hat.get()
        assert np.array_equal(hat, pv.dequantised(h, e, A.rowptr))
        assert np.mean(hat != A.val.astype(F32)) >= 0.5
        assert (S.scaled_rows > 0) == (name == "band-stiff")
    finally:
        S.close()


# ---------------------------------------------------------------- 1. launch against emulation, bit for bit
def _launch_pairs(hip, S, on_sell, seed):
    """Every stand-alone f16f32 entry against its f32 sibling on the dequantised
    values, on the same vectors: (name, got, want) per launch and output."""
    lib, n = hip.lib, S.n
    d, r, z, zp = _vectors(n, seed)
    al, be, c0, c1 = F32(0.37), F32(1.21), F32(0.81), F32(-0.43)
    cf = C.c_float
    out = []

    def run(entry, kind, aliased=None, **kw):
        """kind: 16 (the fp16 copy) or 32 (the dequantised values)."""
        bufs = {k: hip.buf(v) for k, v in dict(d=d, r=r, z=z, zp=zp).items()}
        o = hip.buf(np.full(n, 7, F32))
        if on_sell:
            mat = [S.sell16, S.rexp.p] if kind == 16 else [S.sell32]
        else:
            mat = [S.csr, S.half.p, S.rexp.p] if kind == 16 else [S.csr, S.hat.p]
        suffix = "f16f32" if kind == 16 else "f32"
        st = "sell" if on_sell else "csr"
        if entry == "jacobi":
            zo = bufs["r"] if aliased else o
            hip.call(f"mpg_{st}_jacobi_sweep_{suffix}", *mat, bufs["d"].p, bufs["r"].p, bufs["z"].p, zo.p)
            res = [zo.get()]
        elif entry == "cheb":
            zo = bufs[aliased] if aliased else o
            prev = None if kw.get("first") else bufs["zp"].p
            hip.call(f"mpg_{st}_cheb_sweep_{suffix}", *mat, bufs["d"].p, bufs["r"].p, bufs["z"].p, prev, zo.p, cf(al),
                     cf(be))
            res = [zo.get()]
        else:  # poly: g gathered = z here, p = r, z in place = zp; a pair's second half stores out over p
            zo = None if kw.get("last") else (bufs["r"] if aliased else o)
            g = bufs["z"].p if kw.get("gather_other") else bufs["r"].p
            hip.call(f"mpg_{st}_poly_sweep_{suffix}", *mat, bufs["d"].p, g, bufs["r"].p, bufs["zp"].p,
                     zo.p if zo else None, kw["form"], int(kw.get("first", False)), int(kw.get("last", False)), cf(c0),
                     cf(c1))
            res = [bufs["zp"].get()] + ([zo.get()] if zo else [])
        for b in list(bufs.values()) + [o]:
            b.free()
        return res

    cases = [("jacobi", {}), ("jacobi", dict(aliased="r")),
             ("cheb", {}), ("cheb", dict(first=True)), ("cheb", dict(aliased="r")), ("cheb", dict(aliased="zp")),
             ("poly", dict(form=POLY_STEP)), ("poly", dict(form=POLY_STEP, first=True)),
             ("poly", dict(form=POLY_PAIR)), ("poly", dict(form=POLY_PAIR, first=True)),
             ("poly", dict(form=POLY_STEP, last=True)), ("poly", dict(form=POLY_PAIR, last=True, first=True)),
             ("poly", dict(form=POLY_STEP, gather_other=True, aliased="r"))]
    for entry, kw in cases:
        got, want = run(entry, 16, **kw), run(entry, 32, **kw)
        for q, (g, w) in enumerate(zip(got, want)):
            out.append((f"{entry} {kw} output {q}", g, w))
    return out


SELL_FORMS = {  # matrix -> (column form, CSR-summed slices > 0) of its fp16 copy
    "band4100": (1, False), "band4099": (1, False), "band8196": (1, False),  # int16 columns, implicit slices
    "band-stiff": (1, False),  # ... rows scaled up, down and left alone in every slice
    "far33k": (2, False),      # stepped int16 columns
    "far66k": (2, True),       # ... with a slice summed from the copy's CSR (xval read as fp16)
    "lap12p": (1, False),      # int16 columns, shared blocks
}
IMPLICIT = {"band4100", "band4099", "band8196", "band-stiff"}  # slices that read a shared column pattern


@pytest.mark.parametrize("name", ["band4100", "band4099", "band8196", "band-stiff", "lap12p"])
def test_csr_launches_equal_emulation(mpg, hip, name):
    S = Copies(hip, _matrix(mpg, name))
    try:
        for what, got, want in _launch_pairs(hip, S, False, seed=11):
            assert np.all(np.isfinite(want)), what
            assert np.array_equal(got, want), (what, int(np.sum(got != want)))
    finally:
        S.close()


@pytest.mark.parametrize("name", sorted(SELL_FORMS))
def test_sell_launches_equal_emulation(mpg, hip, name):
    S = Copies(hip, _matrix(mpg, name), sell=True)
    try:
        form, exc, imp = S.form()
        print(name, "form", form, "csr-summed", exc, "implicit", imp)
        assert (form, exc > 0) == SELL_FORMS[name] and (imp > 0 or name not in IMPLICIT)
        for what, got, want in _launch_pairs(hip, S, True, seed=12):
            assert np.array_equal(got, want), (what, int(np.sum(got != want)))
    finally:
        S.close()


def test_sell_int32_columns_equal_emulation(mpg, hip, monkeypatch):
    monkeypatch.setenv("MPG_SELL_STEPPED", "0")
    S = Copies(hip, _matrix(mpg, "far33k"), sell=True)
    try:
        assert S.form()[0] == 0
        for what, got, want in _launch_pairs(hip, S, True, seed=13):
            assert np.array_equal(got, want), (what, int(np.sum(got != want)))
    finally:
        S.close()


def test_launch_arguments_are_checked(mpg, hip):
    S = Copies(hip, _matrix(mpg, "band4099"), sell=True)
    lib, n = hip.lib, S.n
    d, r, z = (hip.buf(v) for v in _vectors(n, 1, 3))
    o = hip.buf(n, F32)
    try:
        assert lib.mpg_csr_jacobi_sweep_f16f32(hip.ctx, S.csr, S.half.p, None, d.p, r.p, z.p, o.p) == -2  # no exponents
        assert lib.mpg_csr_jacobi_sweep_f16f32(hip.ctx, S.csr, S.half.p, S.rexp.p, d.p, r.p, z.p, z.p) == -2
        assert lib.mpg_sell_jacobi_sweep_f16f32(hip.ctx, S.sell32, S.rexp.p, d.p, r.p, z.p, o.p) == -2  # an fp32 copy
        assert lib.mpg_sell_jacobi_sweep_f32(hip.ctx, S.sell16, d.p, r.p, z.p, o.p) == -2  # an fp16 copy
        assert lib.mpg_sell_cheb_sweep_f16f32(hip.ctx, S.sell16, None, d.p, r.p, z.p, None, o.p, C.c_float(1),
                                              C.c_float(1)) == -2
    finally:
        for b in (d, r, z, o):
            b.free()
        S.close()


# ---- both accumulation classes, through the workspace
class _Workspace(PhaseWorkspace):
    def applies(self, d, r):
        """w after each of the applications below, from the same r and diagonal d."""
        hip, lib, n = self.hip, self.hip.lib, self.n
        self._put(self.diag.p.value, d, F32)
        DP = C.POINTER(C.c_double)
        out = {}

        def run(name, fn):
            w, w0, w1 = hip.buf(r), hip.buf(np.zeros(n, F32)), hip.buf(np.zeros(n, F32))
            self._check(fn(w.p, w0.p, w1.p), name)
            out[name] = w.get()
            for b in (w, w0, w1):
                b.free()

        run("neumann3", lambda w, a, b: lib.mpg_arnoldi_neumann_apply(self.arn, 3, w, a, b))
        run("cheb4", lambda w, a, b: lib.mpg_arnoldi_cheb_apply(self.arn, 4, C.c_double(1.1), C.c_double(0.9), w, a, b))
        for label, roots in (("poly-real-pair-real", [1.7, 0.9 + 0.4j, 0.9 - 0.4j, 0.5, 1.2]),
                             ("poly-pair-first", [0.8 + 0.3j, 0.8 - 0.3j, 1.5]),
                             ("poly-pair-last", [1.3, 0.8 + 0.3j, 0.8 - 0.3j])):
            re = np.array([x.real for x in map(complex, roots)])
            im = np.array([x.imag for x in map(complex, roots)])
            run(label, lambda w, a, b: lib.mpg_arnoldi_poly_apply(self.arn, len(re), re.ctypes.data_as(DP),
                                                                   im.ctypes.data_as(DP), w, a, b))
        return out


@pytest.mark.parametrize("accum", [0, 1], ids=["acc64", "acc32"])
@pytest.mark.parametrize("fmt", [1, 2], ids=["csr", "sell"])
@pytest.mark.parametrize("name", ["band4100", "band4099", "band8196", "band-stiff"])
def test_workspace_applies_equal_emulation(mpg, hip, name, fmt, accum):
    """mpg_arnoldi_{neumann,cheb,poly}_apply with the fp16 copy set (every
    epilogue, the last sweep storing over r) = the same applications of a
    workspace whose Arnoldi matrix holds the dequantised values; on CSR also =
    the f16emu copy; and not what the fp32 values give."""
    A = _matrix(mpg, name)
    S = Copies(hip, A, sell=fmt == 2)
    Ahat = mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, S.hat.get().astype(np.float64))
    W16, Wemu = _Workspace(mpg, hip, A, "f32", fmt, accum), _Workspace(mpg, hip, Ahat, "f32", fmt, accum)
    lib = hip.lib
    try:
        assert W16.format == fmt and Wemu.format == fmt
        # (a diagonal of Jacobi's size, half the inverse of each row's largest entry: the chains stay in range)
        rowmax = np.maximum.reduceat(np.abs(A.val), A.rowptr[:-1].astype(np.int64))
        d, r = (0.5 / rowmax).astype(F32), _vectors(A.nrows, 21, 2)[1]
        plain = W16.applies(d, r)
        assert lib.mpg_arnoldi_prec_values(W16.arn) == PV_F32
        hip.check(lib.mpg_arnoldi_set_prec_copy(W16.arn, PV_F16, None if fmt == 2 else S.half.p, S.rexp.p,
                                                S.sell16 if fmt == 2 else None), "set_prec_copy")
        assert lib.mpg_arnoldi_prec_values(W16.arn) == PV_F16
        got, want = W16.applies(d, r), Wemu.applies(d, r)
        for k in want:
            assert np.all(np.isfinite(want[k])), k
            assert np.array_equal(got[k], want[k]), (k, int(np.sum(got[k] != want[k])))
            assert not np.array_equal(got[k], plain[k]), k
        if fmt == 1:
            hip.check(lib.mpg_arnoldi_set_prec_copy(W16.arn, PV_F16EMU, S.hat.p, None, None), "set_prec_copy")
            emu = W16.applies(d, r)
            for k in want:
                assert np.array_equal(emu[k], want[k]), k
        # surplus and missing arguments
        assert lib.mpg_arnoldi_set_prec_copy(W16.arn, PV_F16, S.half.p, None, None) == -2
        assert lib.mpg_arnoldi_set_prec_copy(W16.arn, PV_F16EMU, S.hat.p, S.rexp.p, None) == -2
        assert lib.mpg_arnoldi_set_prec_copy(W16.arn, 3, None, None, None) == -2
        hip.check(lib.mpg_arnoldi_set_prec_copy(W16.arn, PV_F32, None, None, None), "set_prec_copy")
        back = W16.applies(d, r)
        for k in plain:
            assert np.array_equal(back[k], plain[k]), k
    finally:
        W16.close(), Wemu.close(), S.close()


def test_fp64_workspace_refuses_the_copy(mpg, hip):
    A = _matrix(mpg, "band4099")
    S = Copies(hip, A)
    W = PhaseWorkspace(mpg, hip, A, "f64", 1, 0)
    try:
        assert hip.lib.mpg_arnoldi_set_prec_copy(W.arn, PV_F16, S.half.p, S.rexp.p, None) == -5
    finally:
        W.close(), S.close()


# ---------------------------------------------------------------- 2. launch against fp64
def _exact(A, h, e, d, r, z, zp, kind, coef):
    """The stated formula with A^ in fp64 and its forward-error bound per row,
    first order in the unit roundoffs. Row sum: the entries of the row (its
    width) each add at most 2^-53 of sum |a^_ij z_j| in the fp64 class, then
    one rounding to fp32; every epilogue operation adds one fp32 rounding of
    its own result and carries its operands' errors. e: the exponents used
    (the wrong ones of the CPU check, else the copy's own)."""
    rp = A.rowptr.astype(np.int64)
    rows = np.repeat(np.arange(A.nrows), np.diff(rp))
    hv = h.astype(np.float64)
    prod = hv * z.astype(np.float64)[A.col]
    ssum = np.add.reduceat(prod, rp[:-1])
    sabs = np.add.reduceat(np.abs(prod), rp[:-1])
    scale = np.ldexp(1.0, -e.astype(np.int64))
    s = ssum * scale
    width = np.diff(rp)
    e_s = width * 2.0 ** -53 * sabs * scale + U32 * np.abs(s)
    d, r, z, zp = (v.astype(np.float64) for v in (d, r, z, zp))
    if kind == "neumann":
        t = r - s
        u = d * t
        out = z + u
        err = np.abs(d) * (e_s + U32 * np.abs(t)) + U32 * np.abs(u) + U32 * np.abs(out)
        return [out], [err]
    if kind == "cheb":
        al, be = coef
        t = r - s
        u = d * t
        e_u = np.abs(d) * (e_s + U32 * np.abs(t)) + U32 * np.abs(u)
        v = be * u
        e_v = abs(be) * e_u + U32 * np.abs(v)
        p = z - zp
        q = al * p
        e_q = abs(al) * U32 * np.abs(p) + U32 * np.abs(q)
        y = z + q
        out = y + v
        err = e_q + U32 * np.abs(y) + e_v + U32 * np.abs(out)
        return [out], [err]
    c0, c1 = coef  # the pair's first half: p = r, z in place = zp
    u = d * s
    e_u = np.abs(d) * e_s + U32 * np.abs(u)
    q = c0 * r
    t = q - u
    e_t = U32 * np.abs(q) + e_u + U32 * np.abs(t)
    y = c1 * t
    znew = zp + y
    e_z = abs(c1) * e_t + U32 * np.abs(y) + U32 * np.abs(znew)
    return [znew, t], [e_z, e_t]


@pytest.mark.parametrize("kind", ["neumann", "cheb", "pair"])
def test_launch_against_fp64(mpg, hip, kind):
    """One sweep on gen_band_stiff(4099) against the formula in fp64. A dropped
    exponent, or the neighbouring row's, is more than four bounds away on the
    rows it changes (shown on the CPU), so the bound tells them apart."""
    A = _matrix(mpg, "band-stiff")
    h, e = pv.half_values(A)
    n = A.nrows
    d, r, z, zp = _vectors(n, 31)
    coef = (F32(0.37), F32(1.21)) if kind != "pair" else (F32(1.8), F32(1.03))
    want, bound = _exact(A, h, e, d, r, z, zp, kind, tuple(float(c) for c in coef))
    bound = [1.001 * b for b in bound]  # (the terms of second order)
    # the CPU part: wrong exponents
    for label, wrong in (("dropped", np.zeros_like(e)), ("neighbour", np.roll(e, -1))):
        changed = wrong != e
        assert changed.sum() > 100, label
        bad, _ = _exact(A, h, wrong, d, r, z, zp, kind, tuple(float(c) for c in coef))
        gap = np.abs(bad[0] - want[0])[changed] / bound[0][changed]
        print(kind, label, "rows", int(changed.sum()), "min gap / bound", float(gap.min()))
        assert np.all(gap > 4.0), (label, float(gap.min()))
    S = Copies(hip, A)
    bufs = [hip.buf(v) for v in (d, r, z, zp)]
    o = hip.buf(np.full(n, 7, F32))
    cf = C.c_float
    try:
        if kind == "neumann":
            hip.call("mpg_csr_jacobi_sweep_f16f32", S.csr, S.half.p, S.rexp.p, bufs[0].p, bufs[1].p, bufs[2].p, o.p)
            got = [o.get()]
        elif kind == "cheb":
            hip.call("mpg_csr_cheb_sweep_f16f32", S.csr, S.half.p, S.rexp.p, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p,
                     o.p, cf(coef[0]), cf(coef[1]))
            got = [o.get()]
        else:
            hip.call("mpg_csr_poly_sweep_f16f32", S.csr, S.half.p, S.rexp.p, bufs[0].p, bufs[2].p, bufs[1].p, bufs[3].p,
                     o.p, POLY_PAIR, 0, 0, cf(coef[0]), cf(coef[1]))
            got = [bufs[3].get(), o.get()]
        for g, w, b in zip(got, want, bound):
            ratio = np.abs(g.astype(np.float64) - w) / b
            print(kind, "max error / bound", float(ratio.max()))
            assert np.all(ratio <= 1.0), float(ratio.max())
    finally:
        for b in bufs + [o]:
            b.free()
        S.close()


# ---------------------------------------------------------------- 3. whole solves: f16 = f16emu
SOLVES = [  # (matrix, prec, sweeps, orth, accum, rlen)
    ("band4100", "neumann", 2, "cgs", "f64", 30), ("band4099", "neumann", 3, "mgs", "f32", 4),
    ("lap12p", "neumann", 4, "cgsr", "f32", 30), ("lap12p", "chebyshev", 2, "cgsr", "f64", 4),
    ("lap16p", "chebyshev", 3, "mgs", "f64", 30), ("lap16p", "chebyshev", 4, "cgs", "f32", 30),
    ("band8196", "chebyshev", 4, "cgs", "f64", 4), ("convdiff32", "gmres_poly", 2, "cgs", "f32", 4),
    ("convdiff32", "gmres_poly", 3, "cgsr", "f64", 30), ("convdiff32", "gmres_poly", 4, "cgs", "f32", 30),
    ("convdiff32", "gmres_poly", 4, "mgs", "f64", 30), ("band4100", "gmres_poly", 4, "cgs", "f64", 30),
    ("band-stiff", "gmres_poly", 3, "cgs", "f32", 30),
    # (convdiff32's roots are real up to s = 4; at s = 6 they hold a complex pair, test_complex_pair_case_holds_a_pair)
    ("convdiff32", "gmres_poly", 6, "cgs", "f64", 30), ("convdiff32", "gmres_poly", 6, "cgsr", "f32", 30),
]


def _opts(prec, s, orth="cgs", accum="f64", rlen=30, **kw):
    return dict(mode="mixed", orth=orth, prec=prec, jacobi_steps=s, rlen=rlen, tol=1e-10, max_restarts=20, accum=accum,
                engine="fused", **kw)


@pytest.mark.parametrize("name,prec,s,orth,accum,rlen", SOLVES, ids=["-".join(map(str, c)) for c in SOLVES])
def test_solves_f16_equals_emulation(mpg, name, prec, s, orth, accum, rlen):
    A, b, xt = _problem(mpg, name)
    opts = _opts(prec, s, orth, accum, rlen, spmv_format="csr")
    f16, emu = mpg.solve(A, b, xt, prec_values="f16", **opts), mpg.solve(A, b, xt, prec_values="f16emu", **opts)
    print(name, prec, s, orth, accum, rlen, f16.status, f16.restarts, f16.total_iters)
    assert f16.total_iters > 0 and np.all(np.isfinite(f16.x))
    _same(f16, emu, "f16 against f16emu")


def test_complex_pair_case_holds_a_pair(mpg):
    A, b, xt = _problem(mpg, "convdiff32")
    e = mpg.Engine(A, b, xt, prec_values="f16", **_opts("gmres_poly", 6, spmv_format="csr"))
    try:
        lay = e.spmv_layout()
        assert lay["prec_values"] == "f16" and any(t.imag != 0 for t in lay["prec_roots"]), lay
    finally:
        e.close()


def test_solves_beside_a_compressed_basis(mpg):
    A, b, xt = _problem(mpg, "lap12p")
    opts = _opts("chebyshev", 4, spmv_format="csr", basis="f16emu")
    _same(mpg.solve(A, b, xt, prec_values="f16", **opts), mpg.solve(A, b, xt, prec_values="f16emu", **opts), "basis f16emu")
    opts["basis"] = "f16"
    both = mpg.solve(A, b, xt, prec_values="f16", **opts)
    assert both.status == "converged"


@pytest.mark.parametrize("name", ["band8196", "lap12p"])
def test_storage_forms(mpg, name):
    """In the fp32 class the SELL and CSR sweeps (and SpMVs) give one another's
    bits, so cycle 0's step history is the same (tests/test_basis16_gpu.py)."""
    A, b, xt = _problem(mpg, name)
    opts = _opts("chebyshev", 4, accum="f32", prec_values="f16")
    opts.update(tol=0.0, max_restarts=3)
    got = {f: mpg.solve(A, b, xt, spmv_format=f, **opts) for f in ("csr", "sell")}
    np.testing.assert_array_equal(got["sell"].step_res[:30], got["csr"].step_res[:30])
    for f in got:
        e = mpg.Engine(A, b, xt, spmv_format=f, **opts)
        lay = e.spmv_layout()
        e.close()
        assert lay["format"] == f and lay["prec_values"] == "f16"


# ---------------------------------------------------------------- 4. the rounding happens
@pytest.mark.parametrize("name,prec", [("band8196", "gmres_poly"), ("convdiff32", "chebyshev")])
def test_emulation_differs_from_f32(mpg, name, prec, monkeypatch):
    monkeypatch.delenv("MPG_PREC_VALUES", raising=False)
    A, b, xt = _problem(mpg, name)
    opts = _opts(prec, 4, spmv_format="csr")
    emu, f32 = mpg.solve(A, b, xt, prec_values="f16emu", **opts), mpg.solve(A, b, xt, prec_values="f32", **opts)
    assert not np.array_equal(emu.x, f32.x) and not np.array_equal(emu.step_res[:30], f32.step_res[:30])
    _same(f32, mpg.solve(A, b, xt, **opts), "the keyword's default")
    e = mpg.Engine(A, b, xt, **opts)
    try:
        assert "prec_values" not in e.spmv_layout()
        e.solve()
        assert e.graph_captures == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 5. counts
@pytest.mark.parametrize("name,prec,s", pv.CASES, ids=[f"{c[0]}-{c[1]}{c[2]}" for c in pv.CASES])
def test_recorded_cycle_counts(mpg, name, prec, s):
    A, b, xt = _problem(mpg, name)
    for values in ("f32", "f16"):
        for accum in ("f64", "f32"):
            got = mpg.solve(A, b, xt, prec_values=values, **_opts(prec, s, accum=accum))
            print(name, prec, s, values, accum, got.status, got.restarts, got.total_iters)
            assert got.status == "converged" and got.restarts == pv.COUNTS[(name, prec, s)], (values, accum, got.restarts)


# ---------------------------------------------------------------- 6. live engine
@pytest.mark.parametrize("prec,captures", [("neumann", 1), ("chebyshev", 2)])
@pytest.mark.parametrize("fmt", ["csr", "sell"])
def test_refreshed_engine_is_a_new_engine(mpg, monkeypatch, fmt, prec, captures):
    for name in ("MPG_PIPELINE", "MPG_NO_GRAPH"):
        monkeypatch.delenv(name, raising=False)
    A, b, xt = _problem(mpg, "band8196")
    A2 = mpg.Csr(A.nrows, A.ncols, A.rowptr, A.col, mpg.perturb_values(A, 0.25, 5))
    b2 = mpg.host_spmv(A2, xt)
    opts = _opts(prec, 3, spmv_format=fmt, prec_values="f16")
    e = mpg.Engine(A, b, xt, **opts)
    try:
        r1 = e.solve()
        assert e.graph_captures == 1
        e.refresh(A2.val)
        r2 = e.solve(b2, x_true=xt)
        assert e.graph_captures == captures
        _same(r2, mpg.solve(A2, b2, xt, **opts), "refreshed against a new engine")
        assert not np.array_equal(r1.x, r2.x)
        # a value whose row leaves fp32's range once unscaled: refused, the old system's bits stay
        bad = A2.val.copy()
        bad[int(A.rowptr[17])] = 1e39
        with pytest.raises(RuntimeError, match="prec_values f16.*overflow fp32.*keeps its matrix"):
            e.refresh(bad)
        _same(e.solve(b2, x_true=xt), r2, "after the refused refresh")
    finally:
        e.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(mpg, monkeypatch):
    monkeypatch.delenv("MPG_PREC_VALUES", raising=False)
    A, b, xt = _problem(mpg, "lap12p")

    def refused(text, values="f16", **kw):
        opts = _opts("chebyshev", 4)
        opts.update(kw)
        with pytest.raises(RuntimeError, match=text):
            mpg.solve(A, b, xt, prec_values=values, **opts)

    for prec, extra in (("identity", {}), ("jacobi", {}), ("neumann", dict(jacobi_steps=1)), ("bjacobi", {}), ("ilu", {}),
                        ("ilu_jacobi", {})):
        refused("prec_values f16 needs a preconditioner that sweeps over A", prec=prec, **extra)
    for mode in ("baseline", "single", "single-prec", "mixed-half"):
        refused("prec_values f16 runs in mode mixed only|is not available in mode", mode=mode)
    refused("prec_values f16 runs in mode mixed only", mode="baseline")
    refused("prec_values f16 is not available on the operator-surface engine", engine="surface")
    refused("prec_values f16emu is built for the CSR row-block storage only", values="f16emu", spmv_format="sell")
    refused("MPG_PREC_VALUES = f8 is not f32, f16 or f16emu", values="f8")
    with pytest.raises(RuntimeError, match="prec_values f16 is not available on a row-partitioned solve"):
        mpg.solve_multi_gpu(A, b, xt, ngpus=1, prec_values="f16", **{k: v for k, v in _opts("chebyshev", 4).items()
                                                                        if k != "engine"})
    # the context solves afterwards, with and without the setting
    opts = _opts("chebyshev", 4)
    assert mpg.solve(A, b, xt, prec_values="f16", **opts).status == "converged"
    assert mpg.solve(A, b, xt, **opts).status == "converged"
    assert os.environ.get("MPG_PREC_VALUES") is None


# ---------------------------------------------------------------- 8. CLI
def test_cli(mpg):
    """--prec chebyshev --jacobi-steps 4 --prec-values f16 keeps the reference's
    stdout contract and reports the iterations of mpg.solve with the same options."""
    from tests.test_cli_gpu import SUMMARY

    cmd = [str(mpg.CLI), "--matrix", "laplace:12", "--rlen", "30", "--mode", "mixed", "--orth", "cgs", "--prec",
           "chebyshev", "--jacobi-steps", "4", "--tol", "1e-10", "--gpu"]
    env = {k: v for k, v in os.environ.items() if k != "MPG_PREC_VALUES"}
    A = mpg.gen_laplace3d(12)
    xt = mpg.rand_vect(A.nrows, 42)
    b = mpg.host_spmv(A, xt)
    for values in ("f32", "f16"):
        p = subprocess.run(cmd + ["--prec-values", values], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        m = SUMMARY.search(p.stdout)
        assert m, p.stdout
        assert float(m.group(1)) <= 1e-10
        assert p.stdout.startswith("||x|| = ") and "Doing Mixed Precision test" in p.stdout
        got = mpg.solve(A, b, xt, engine="fused", mode="mixed", orth="cgs", prec="chebyshev", jacobi_steps=4, rlen=30,
                        tol=1e-10, max_restarts=1_000_000, prec_values=values)
        assert int(m.group(4)) == got.total_iters > 0
    p = subprocess.run(cmd + ["--prec-values", "f8"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode != 0 and "MPG_PREC_VALUES = f8" in p.stdout + p.stderr
