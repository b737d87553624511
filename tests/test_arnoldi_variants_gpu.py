"""The fused Arnoldi SpMV launches on the storage variants that
tests/test_arnoldi_phases_gpu.py leaves out, each against the fp64 restatement
(tests/arnoldi_ref_np.py) under the bound written beside the check
(tests/test_arnoldi_ref_cpu.py shows each bound sees a wrong front offset, a
halo read as zero or from the other side, an ignored, neighbouring or missing
row exponent, a base of the neighbouring element, a wrapped or skipped
exception slice, a transposed or shifted block inverse).

Entry points x variants and the cases that cover them:
  spmv, givens_spmv, givens_partials_spmv      test_stepped: the stepped int16 SELL columns without (far33k) and
  prologue, prologue_finish_partials             with one CSR-summed slice (far66k), its int32 control
                                                 (MPG_SELL_STEPPED=0), Jacobi inside the launch
  spmv, givens_spmv                            test_halo: rows of one rank with n_front > 0 and / or n_ext > n
  prologue, reduce, prologue_finish              (band-ranks: csr, sell-pair, sell-single, the v_k window below
  dots, reduce, cgs_partials                     row 0; stencil-ranks: csr, sell gathered, node blocks), under
  step_dots_supported                            uniform_groups, the halo and the pad in front of it checked
  spmv, givens_spmv                            test_half_values: fp16 values, scaled per row (band-stiff) and
                                                 unscaled (band4099, stencil5), csr / sell-pair / sell-single /
                                                 sell gathered / node, with and without Jacobi
  spmv, givens_spmv                            test_half_values_halo: band-ranks rank 1 with scaled fp16 values
  spmv, prologue, prologue_wnorm               test_block_jacobi_node: block_dinv applied inside k_step_node_bj
                                                 and k_prologue_rows (prec_fused)
Every class (f32-acc64, f32-acc32, f64) where the form exists (fp16 values: an
fp32 Arnoldi). The output w is NaN before each SpMV launch (a row left out
fails whatever the bound), w_prev is compared bit for bit afterwards.
Not covered: spmv_dots / step_dots on these variants (refused with halo rows:
asserted; not built for fp16 values or stepped columns), the compressed basis
on them, SELL-C-sigma sorted copies, block sizes other than 3, the stepped
form's shared column blocks (MPG_SELL_SHARE), and more than one process."""
import functools

import numpy as np
import pytest

from tests import arnoldi_ref_np as R
from tests.arnoldi_phase import (CLASSES, FAR66_ROW, MATRICES, MPG_ERR_UNSUPPORTED, MPG_F16, RANK_SPLITS,
                                 PhaseWorkspace, RankBlock)
from tests.test_arnoldi_phases_gpu import check_givens_close, close_to, read_givens, same_bits

pytestmark = pytest.mark.gpu
CLS = sorted(CLASSES)
SENTINEL = 7.0  # what the halo entries of an output buffer hold before a launch (finite: compared bit for bit)


# ---------------------------------------------------------------- shared inputs, made once
def _mpg():
    from tests.conftest import load_package

    return load_package()


@functools.lru_cache(maxsize=None)
def _matrix(name):
    return MATRICES[name](_mpg())


@functools.lru_cache(maxsize=None)
def _block(name, rank):
    return RankBlock(_mpg(), _matrix(name), RANK_SPLITS[name], rank)


@functools.lru_cache(maxsize=None)
def _a64(name, t):
    """The T-valued matrix as fp64 (what a kernel with values of type T multiplies)."""
    return R.csr64(_matrix(name), np.float32 if t == "f32" else np.float64)


@functools.lru_cache(maxsize=None)
def _block64(name, rank, t):
    """_a64 of one rank's rows: n x (n_front + n_ext), columns shifted by n_front."""
    M = _block(name, rank).to_scipy()
    M.data = M.data.astype(np.float32 if t == "f32" else np.float64).astype(np.float64)
    return M


@functools.lru_cache(maxsize=None)
def _vec(n, seed, j, dtype):
    v = R.gen_vec(n, seed, j, dtype)
    v.setflags(write=False)
    return v


class _Ws:
    """Context manager around PhaseWorkspace on a given matrix (closed whatever the test does)."""

    def __init__(self, hip, A, cls, fmt, **kw):
        t, accum = CLASSES[cls]
        self.W = PhaseWorkspace(_mpg(), hip, A, t, fmt, accum, **kw)

    def __enter__(self):
        return self.W

    def __exit__(self, *exc):
        self.W.close()


def _pair_env(monkeypatch, pair):
    if pair is None:
        monkeypatch.delenv("MPG_SELL_PAIR", raising=False)
    else:
        monkeypatch.setenv("MPG_SELL_PAIR", pair)


def _layout(W):
    form, exc = W.sell_columns()
    return dict(format=W.format, window=W.window, spw=W.lib.mpg_arnoldi_slices_per_wave(W.arn), form=form,
                csr_slices=exc, prologue=W.lib.mpg_arnoldi_prologue_format(W.arn))


# ---------------------------------------------------------------- the checks
def check_spmv(W, A64, k, w_prev, inv, jacobi, what, n_front=0, rows=None):
    """tests/test_arnoldi_phases_gpu.py::_check_spmv on a given matrix: V(:,k)
    has the bits of T(w_prev * inv) on the rows [0, n); w = M(A v) against the
    fp64 row sums over the whole of v (halo included): tol_rows' sum term over
    the row's entries, and one rounding to T (three with Jacobi: the row sum,
    d * w and its store). rows: their worst ratio is printed separately (they
    are in the compared set either way)."""
    d = W.diag.get() if jacobi else None
    v, ref, scale = R.ref_spmv_step(A64, w_prev, inv, d, n_front)
    same_bits(W.get_V(k), v, what + ": V(:,k)")
    w1 = W.get_w(k + 1)
    tol = R.tol_spmv(ref, scale, int(np.diff(A64.indptr).max()), W.T, W.acc32, jacobi)
    if rows is not None:
        print(f"{what}: rows {rows[0]}..{rows[-1]}: worst |err|/tol = "
              f"{float(np.max(np.abs(w1[rows] - ref[rows]) / tol[rows])):.3g}")
    close_to(w1, ref, tol, what + ": w")
    return v, w1


def check_prologue(W, A64o, b, x, jacobi, n_front=0):
    """tests/test_arnoldi_phases_gpu.py::test_prologue's checks after prologue +
    finish, on a given fp64 matrix (halo columns included) and x (n_front +
    n_ext entries): the same bounds, x_norm over the rows [0, n)."""
    n, u = W.n, R.unit(W.T)
    P = R.ref_prologue(A64o, b, x, W.T, W.diag.get() if jacobi else None, n_front)
    w0 = W.get_w(0)
    dr = 2 * (P["nnz_row"] + 2) * 2.0 ** -53 * P["scale"]
    close_to(w0, P["w0"].astype(np.float64), R.tol_prologue_w0(P, W.T, W.diag.get() if jacobi else None), "w0")
    rep = W.get_report()
    # the norms: (n + 2) 2^-53 relative for the sum and the root, one rounding to T (X for x_norm); beta against
    # the norm of the device's own w0, r_norm (Jacobi: T(r) is not stored) against the restatement's
    sumtol = (n + 2) * 2.0 ** -53
    nw0 = float(np.sqrt((w0.astype(R.LD) ** 2).sum()))
    close_to(rep[1], nw0, (sumtol + u) * nw0, "beta")
    if jacobi:
        close_to(rep[0], P["r_norm"], (sumtol + 3 * u) * P["r_norm"] + float(np.linalg.norm(dr)), "r_norm")
    else:
        close_to(rep[0], nw0, (sumtol + u) * nw0, "r_norm")
    close_to(rep[2], P["x_norm"], (sumtol + 2.0 ** -53) * P["x_norm"], "x_norm")
    beta = W.T(rep[1])
    assert float(beta) == rep[1] and rep[3] == float(W.T(1) / beta), rep[:4]
    same_bits(W.get_inv(), W.T(1) / beta, "inv")
    s = np.zeros(W.m + 1, W.T)
    s[0] = beta
    same_bits(W.get_rot(2), s, "s = [beta, 0, ...]")
    close_to(np.sqrt(W.get_sums(3)), [rep[0], rep[1], rep[2]], u * np.abs(rep[:3]), "sums")


def run_spmv(W, A64, k, w_ext, jacobi, what, n_front=0, rows=None):
    """spmv(k) on w_prev = w_ext (n_front + n_ext entries; NaN in the pad in
    front of them): the output's rows NaN, its halo SENTINEL before the launch;
    afterwards the halo of the output and the whole of w_prev are untouched."""
    inv = W.T(0.37)
    out0 = _poison(W)
    W.put_inv(inv)
    W.put_w(k, w_ext, ext=True)
    W.put_w(k + 1, out0, ext=True)
    W.launch("spmv", k)
    check_spmv(W, A64, k, w_ext, inv, jacobi, what, n_front, rows)
    same_bits(W.get_w(k, ext=True), w_ext, what + ": w_prev untouched")
    _halo_untouched(W, k + 1, out0, what)


def _poison(W):
    """An output buffer's content before a launch: NaN in the rows [0, n), SENTINEL in the halo."""
    out = np.full(W.n_front + W.n_ext, SENTINEL, W.T)
    out[W.n_front:W.n_front + W.n] = np.nan
    return out


def _halo_untouched(W, kbuf, before, what):
    halo = np.ones(W.n_front + W.n_ext, bool)
    halo[W.n_front:W.n_front + W.n] = False
    same_bits(W.get_w(kbuf, ext=True)[halo], before[halo], what + ": the output's halo untouched")


def run_givens_spmv(W, A64, w_ext, jacobi, what, n_front=0, partials=False):
    """givens_spmv(1): the Givens step 0 on an injected column and sums[0] (bit
    for bit), 1/h into the SpMV of step 1 on w_prev = w_ext. partials:
    givens_partials_spmv(1) behind cgs(0, 0), as test_spmv_fold does (one GPU)."""
    n = W.n
    cs, sn, s = R.gen_rotations(W.m, 9, W.T)
    for q, v in enumerate((cs, sn, s)):
        W.put_rot(q, v)
    out0 = _poison(W)
    W.put_w(0, out0, ext=True)  # step 1 writes buffer 0
    if partials:
        Vfull = R.gen_basis(n, W.ld, W.m + 1, 11, W.T)
        W.put_V(Vfull)
        W.put_w(1, w_ext, ext=True)
        c64 = R.gen_coefs(1)
        W.put_sums(c64)
        W.launch("cgs", 0, 0)
        w1 = W.get_w(1, ext=True)
        own = w1[n_front:n_front + n]
        nrm = float(R.ref_dots(own[:, None], own)[0][0])
        for q, v in enumerate((cs, sn, s)):
            W.put_rot(q, v)
        W.launch("givens_partials_spmv", 1)
        G = R.ref_givens(0, np.array([c64[0], 0]).astype(W.T), None, cs, sn, s, nrm, W.T)
        got = read_givens(W, 0)
        check_givens_close(W, 0, G, got, R.tol_sum(nrm, nrm, n, W.T, W.acc32) / nrm, what)
    else:
        H0 = R.gen_upper(W.m, 1, 41, W.T)
        nrm = 1.75 + 1e-9
        W.put_H(H0)
        W.put_w(1, w_ext, ext=True)
        W.put_sums(np.array([nrm]))
        W.launch("givens_spmv", 1)
        G = R.ref_givens(0, H0[:2, 0], None, cs, sn, s, nrm, W.T)
        got = read_givens(W, 0)
        for key in ("col", "cs", "sn", "s", "inv"):
            same_bits(got[key], G[key], f"{what}: {key}")
        w1 = w_ext
    check_spmv(W, A64, 1, w1, got["inv"], jacobi, what + ": step 1", n_front)
    same_bits(W.get_w(1, ext=True), w1, what + ": w_prev untouched")
    _halo_untouched(W, 0, out0, what)


# ---------------------------------------------------------------- stepped int16 columns
# (matrix, MPG_SELL_STEPPED, MPG_SELL_IMPLICIT) -> (column form, CSR-summed slices). A tridiagonal matrix' inner
# slices are implicit (every row the same offsets: no columns read); "0" stores every slice's offsets
STEPPED = {("far33k", "1", "1"): (2, 0), ("far33k", "1", "0"): (2, 0), ("far66k", "1", "1"): (2, 1),
           ("far66k", "0", "1"): (0, 0)}


@pytest.mark.parametrize("name,stepped,implicit", sorted(STEPPED))
@pytest.mark.parametrize("cls", CLS)
def test_stepped(hip, monkeypatch, cls, name, stepped, implicit):
    """The SELL copy with one int16 offset per entry against a base per (slice,
    step, element): the SpMV (plain, both folds, with Jacobi) and the residual
    prologue. far66k's slice FAR66_ROW / 64 is summed from the copy's sub-CSR;
    MPG_SELL_STEPPED=0 (int32 columns) is the control under the same bound."""
    monkeypatch.setenv("MPG_SELL_STEPPED", stepped)
    monkeypatch.setenv("MPG_SELL_IMPLICIT", implicit)
    _pair_env(monkeypatch, None)
    A = _matrix(name)
    n = A.nrows
    x, b = _vec(n, 51, 2, np.float64), _vec(n, 52, 4, np.float64)
    exc = np.arange((FAR66_ROW // 64 - 1) * 64, (FAR66_ROW // 64 + 2) * 64) if name == "far66k" else None
    for jacobi in (0, 1):
        with _Ws(hip, A, cls, 2, m=6, jacobi=jacobi, x=x, b=b) as W:
            lay = _layout(W)
            assert (lay["format"], lay["window"], lay["form"], lay["csr_slices"]) == (2, 0) + STEPPED[name, stepped, implicit], lay
            assert lay["csr_slices"] * 100 <= -(-n // 64)
            A64 = _a64(name, W.t)
            for k in (0, 1) if not jacobi else (0,):
                run_spmv(W, A64, k, _vec(n, 25 + k, 5, W.T), jacobi, f"spmv {name} k={k} jacobi={jacobi}", rows=exc)
            if jacobi:
                continue
            w = _vec(n, 26, 5, W.T)
            run_givens_spmv(W, A64, w, 0, f"givens_spmv {name}")
            run_givens_spmv(W, A64, w, 0, f"givens_partials_spmv {name}", partials=True)
            assert lay["prologue"] == 2
            W.put_rot(2, np.full(W.m + 1, 9, W.T))
            W.put_w(0, np.full(n, np.nan, W.T))
            W.launch("prologue")
            W.launch("prologue_finish_partials")
            check_prologue(W, _a64(name, "f64"), b, x, 0)


# ---------------------------------------------------------------- halo rows
# storage -> (spmv_format, MPG_SELL_PAIR)
HALO_STORAGE = {"csr": (1, None), "sell-pair": (2, None), "sell-single": (2, "0"), "sell": (2, None), "node": (3, None)}
HALO_CASES = ([("band-ranks", st, r) for st in ("csr", "sell-pair", "sell-single") for r in (0, 1, 2)] +
              [("stencil-ranks", st, r) for st in ("csr", "sell", "node") for r in (0, 1)])


def _halo_layout(name, storage, rank, B):
    """(format, window, slices per wave, prologue format) of one rank's workspace."""
    if storage == "csr":
        return 1, 0, 0, 1
    if storage == "node":
        # node_prologue_build: the node prologue only without a lower halo (it reads x through the node copy's
        # columns; with n_front != 0 the workspace keeps the CSR prologue)
        return 3, 0, 0, 3 if B.n_front == 0 else 1
    if name == "stencil-ranks":
        return 2, 0, None, 2
    # the band: every column within the v_k window. Ranks 0 and 1 have an upper halo, so their last slice's rows
    # are as wide as the others' (uniform: the pair kernel); rank 2's last rows end at the matrix' last column
    return 2, 1, 2 if storage == "sell-pair" and rank < 2 else 1, 2


@pytest.mark.parametrize("name,storage,rank", HALO_CASES)
@pytest.mark.parametrize("cls", CLS)
def test_halo(hip, monkeypatch, cls, name, storage, rank):
    """One rank's rows of a row-partitioned matrix, the halo filled by hand from
    the global vector and NaN in the pad in front of -n_front (no correct launch
    multiplies a pad entry: the window form loads the pad rows below row 0 into
    LDS, where no column of the matrix points): the SpMV forms, the multi-rank
    prologue path, and the panel dots / update under uniform_groups."""
    fmt, pair = HALO_STORAGE[storage]
    _pair_env(monkeypatch, pair)
    monkeypatch.delenv("MPG_SELL_STEPPED", raising=False)
    B = _block(name, rank)
    N, n, nf = _matrix(name).nrows, B.n, B.n_front
    xg, bg = _vec(N, 51, 2, np.float64), _vec(N, 52, 4, np.float64)
    x_ext, b = xg[B.glob], bg[B.own]
    with _Ws(hip, B.A, cls, fmt, m=10, x=x_ext, b=b, n_ext=B.n_ext, n_front=nf) as W:
        W.uniform_groups()
        lay = _layout(W)
        xfmt, xwin, xspw, xpro = _halo_layout(name, storage, rank, B)
        assert (lay["format"], lay["window"], lay["prologue"]) == (xfmt, xwin, xpro), lay
        if xspw is not None:
            assert lay["spw"] == xspw, lay
        W.expect("step_dots_supported", (0,), MPG_ERR_UNSUPPORTED)
        A64 = _block64(name, rank, W.t)
        what = f"{name} {storage} rank {rank}"
        for k in (0, 1):
            run_spmv(W, A64, k, _vec(N, 25 + k, 5, W.T)[B.glob], 0, f"spmv {what} k={k}", nf)
            same_bits(W.get_x(ext=True), x_ext, "x untouched")
        run_givens_spmv(W, A64, _vec(N, 26, 5, W.T)[B.glob], 0, f"givens_spmv {what}", nf)
        # the multi-rank prologue: partials, reduce(3) (where the ranks would all-reduce), finish
        W.put_rot(2, np.full(W.m + 1, 9, W.T))
        out0 = _poison(W)
        W.put_w(0, out0, ext=True)
        W.launch("prologue")
        W.reduce(3)
        W.launch("prologue_finish")
        check_prologue(W, _block64(name, rank, "f64"), b, x_ext, 0, nf)
        _halo_untouched(W, 0, out0, "prologue")
        same_bits(W.get_x(ext=True), x_ext, "x untouched")
        # dots(8) + reduce(9), then dots(8) + cgs_partials(8): 256 partials per column whatever n
        nc, k = 9, 8
        w = _vec(n, R.W_SEED, 5, W.T)
        V = R.gen_basis_toward(w, n, W.ld, nc, 11, W.T)
        dref, dabs = R.ref_dots(V[:n], w)
        tol = R.tol_sum(dref, dabs, n, W.T, W.acc32)
        W.put_V(V)
        w_ext = out0.copy()
        w_ext[nf:nf + n] = w
        W.put_w(k + 1, w_ext, ext=True)
        W.put_sums(np.full(W.m + 4, np.nan))
        W.launch("dots", k)
        assert W.lib.mpg_arnoldi_partials_count(W.arn) == 256
        close_to(W.reduce(nc), dref, tol, f"dots {what}")
        same_bits(W.get_w(k + 1, ext=True), w_ext, "dots: w untouched")
        W.launch("dots", k)
        W.launch("cgs_partials", k)
        c = W.get_H()[:nc, k]
        close_to(c, dref, tol + 2 * R.unit(W.T) * np.abs(dref), f"cgs_partials {what}: coefficients")
        w1 = W.get_w(k + 1)
        ref, t, scale = R.ref_cgs_update(V[:n], c, w)
        close_to(w1, ref, R.tol_rows(ref, t, scale, nc, W.T, W.acc32), f"cgs_partials {what}: w'")
        nref, nabs = R.ref_dots(w1[:, None], w1)
        close_to(W.reduce(1), nref, R.tol_sum(nref, nabs, n, W.T, W.acc32), f"cgs_partials {what}: ||w'||^2")
        _halo_untouched(W, k + 1, w_ext, "cgs_partials")
        same_bits(W.get_x(ext=True), x_ext, "x untouched")
    # Jacobi inside the launches (what a row-partitioned solve runs by default): the inverse diagonal is found
    # among local columns, the lower halo's negative ones in front of it; one SpMV and the prologue
    with _Ws(hip, B.A, cls, fmt, m=4, jacobi=1, x=x_ext, b=b, n_ext=B.n_ext, n_front=nf) as W:
        W.uniform_groups()
        A64 = _block64(name, rank, W.t)
        dg = A64[np.arange(n), np.arange(n) + nf]
        same_bits(W.diag.get(), (W.T(1) / np.asarray(dg).ravel().astype(W.T)).astype(W.T), "1 / a_ii of the local rows")
        run_spmv(W, A64, 0, _vec(N, 25, 5, W.T)[B.glob], 1, f"spmv {what} jacobi", nf)
        out0 = _poison(W)
        W.put_w(0, out0, ext=True)
        W.launch("prologue")
        W.reduce(3)
        W.launch("prologue_finish")
        check_prologue(W, _block64(name, rank, "f64"), b, x_ext, 1, nf)
        _halo_untouched(W, 0, out0, "prologue with Jacobi")


# ---------------------------------------------------------------- fp16 matrix values
# case -> (matrix, spmv_format, MPG_SELL_PAIR, row scaling, (format, window, slices per wave))
HALF = {
    "stiff-csr": ("band-stiff", 1, None, 1, (1, 0, 0)),
    "stiff-sell-pair": ("band-stiff", 2, None, 1, (2, 1, 1)),    # (n = 4099: a ragged last slice, one slice per wave)
    "stiff-sell-single": ("band-stiff", 2, "0", 1, (2, 1, 1)),
    "stiff8197-sell-pair": ("band-stiff8197", 2, None, 1, (2, 1, 2)),  # k_step_sell2's two exponents per lane
    "plain-csr": ("band4099", 1, None, 0, (1, 0, 0)),
    "plain-sell-pair": ("band8197", 2, None, 0, (2, 1, 2)),
    "plain-sell-single": ("band8197", 2, "0", 0, (2, 1, 1)),
    "stencil-sell": ("stencil5", 2, None, 1, (2, 0, None)),
    "stencil-node": ("stencil5", 3, None, 1, (3, 0, 0)),
}


def _half_ws(hip, A, cls, fmt, scale, **kw):
    """A workspace on fp16 values, its device copy compared with the restatement. Returns (ws, fp64 matrix)."""
    n_front = kw.get("n_front", 0)
    bits, e, M = R.half_values(A, scale, n_front)
    ws = _Ws(hip, A, cls, fmt, inner_val=MPG_F16, row_exp=scale, **kw)
    W = ws.W
    try:
        assert np.array_equal(W.half_bits(), bits), int(np.sum(W.half_bits() != bits))
        if scale:
            assert np.array_equal(W.row_exp().astype(np.int64), e)
        assert W.half_stats[0] == int(np.count_nonzero(e)) and W.half_stats[1:] == [0, 0, 0], W.half_stats
    except BaseException:
        W.close()
        raise
    return ws, M


@pytest.mark.parametrize("jacobi", [0, 1])
@pytest.mark.parametrize("case", sorted(HALF))
@pytest.mark.parametrize("cls", ["f32-acc32", "f32-acc64"])
def test_half_values(hip, monkeypatch, cls, case, jacobi):
    """inner_val = MPG_F16: the copy's bits and exponents against half_values,
    then the SpMV against the fp64 row sums over float(h_ij) 2^-e_i: the
    unscaling is a power of two, so _check_spmv's bound holds unchanged."""
    name, fmt, pair, scale, xlay = HALF[case]
    _pair_env(monkeypatch, pair)
    monkeypatch.delenv("MPG_SELL_STEPPED", raising=False)
    A = _matrix(name)
    n = A.nrows
    ws, M = _half_ws(hip, A, cls, fmt, scale, m=6, jacobi=jacobi)
    with ws as W:
        lay = _layout(W)
        assert (lay["format"], lay["window"]) == xlay[:2] and xlay[2] in (None, lay["spw"]), lay
        for k in (0, 1):
            run_spmv(W, M, k, _vec(n, 25 + k, 5, W.T), jacobi, f"spmv {case} k={k} jacobi={jacobi}")
        run_givens_spmv(W, M, _vec(n, 26, 5, W.T), jacobi, f"givens_spmv {case}")


def test_half_values_need_an_fp32_arnoldi(hip):
    """The f64 class is not built on fp16 values: mpg_arnoldi_create answers MPG_ERR_UNSUPPORTED."""
    with pytest.raises(RuntimeError, match="mpg_arnoldi_create: unsupported operation"):
        PhaseWorkspace(_mpg(), hip, _matrix("band4099"), "f64", 1, 0, inner_val=MPG_F16, row_exp=0)


@pytest.mark.parametrize("storage", ["csr", "sell-pair"])
@pytest.mark.parametrize("cls", ["f32-acc32", "f32-acc64"])
def test_half_values_halo(hip, monkeypatch, cls, storage):
    """Scaled fp16 values on rows with a halo on both sides (band-ranks rank 1,
    rows scaled as band-stiff's): the exponent belongs to the local row, the
    column to the local numbering."""
    fmt, pair = HALO_STORAGE[storage]
    _pair_env(monkeypatch, pair)
    B = _block("band-stiff-ranks", 1)
    N = _matrix("band-stiff-ranks").nrows
    ws, M = _half_ws(hip, B.A, cls, fmt, 1, m=6, n_ext=B.n_ext, n_front=B.n_front)
    with ws as W:
        W.uniform_groups()
        assert W.half_stats[0] > 0 and (W.format, W.window) == (fmt, int(fmt == 2))
        for k in (0, 1):
            run_spmv(W, M, k, _vec(N, 25 + k, 5, W.T)[B.glob], 0, f"spmv half halo {storage} k={k}", B.n_front)
        run_givens_spmv(W, M, _vec(N, 26, 5, W.T)[B.glob], 0, f"givens_spmv half halo {storage}", B.n_front)


# ---------------------------------------------------------------- block Jacobi inside the node launches
@pytest.mark.parametrize("name", ["stencil5", "stencil5-rows"])
@pytest.mark.parametrize("cls", CLS)
def test_block_jacobi_node(hip, cls, name):
    """block_dinv on node blocks (prec_block 3): k_step_node_bj's w = Dinv (A
    v) against ref_node_bj under tol_node_bj, and where the prologue applies
    the inverses too, w0 = Dinv T(b - A x) by the same rule (the caller then
    re-forms ||w0||^2: prologue_wnorm). stencil5-rows: unsymmetric diagonal
    blocks (on stencil5 a transposed read of an inverse changes nothing)."""
    A = _matrix(name)
    n = A.nrows
    x, b = _vec(n, 51, 2, np.float64), _vec(n, 52, 4, np.float64)
    with _Ws(hip, A, cls, 3, m=6, prec_block=3, x=x, b=b) as W:
        assert W.format == 3 and W.prec_fused(0) == 1
        A64 = _a64(name, W.t)
        terms = int(np.diff(A64.indptr).max())
        dinv = W.block_dinv()
        # (the set-up is tests/test_bjacobi_gpu.py's subject; here its restatement makes the reference stand alone)
        from tests.test_bjacobi_gpu import np_block_inverse

        dref, bad = np_block_inverse(A, 3, W.T)
        assert not bad.any()
        same_bits(dinv, dref, "block_dinv = the NumPy Gauss-Jordan's inverses")
        for k in (0, 1):
            inv, w_prev = W.T(0.37), _vec(n, 25 + k, 5, W.T)
            W.put_inv(inv)
            W.put_w(k, w_prev)
            W.put_w(k + 1, np.full(n, np.nan, W.T))
            W.launch("spmv", k)
            Rj = R.ref_node_bj(A64, w_prev, inv, dinv)
            same_bits(W.get_V(k), Rj["v"], f"bj spmv k={k}: V(:,k)")
            close_to(W.get_w(k + 1), Rj["w"], R.tol_node_bj(Rj, terms, W.T, W.T, W.acc32), f"bj spmv k={k}: w")
            same_bits(W.get_w(k), w_prev, "w_prev untouched")
        if W.prec_fused(1) == 1:
            W.put_w(0, np.full(n, np.nan, W.T))
            W.launch("prologue")
            W.launch("prologue_wnorm")
            W.launch("prologue_finish_partials")
            # t = T(b - A x) per row as check_prologue bounds it: dr + u |r|; through |Dinv|, then the three products
            # and two adds in P and the store (tol_node_bj's terms, with delta = dr + u |r|)
            u = R.unit(W.T)
            P = R.ref_prologue(_a64(name, "f64"), b, x, W.T)
            D = np.asarray(dinv, np.float64).reshape(-1, 3, 3)
            blk = lambda M, v: np.einsum("bij,bj->bi", M, v.reshape(-1, 3)).reshape(-1)
            ref = blk(D, P["r"])
            delta = 2 * (P["nnz_row"] + 2) * 2.0 ** -53 * P["scale"] + u * np.abs(P["r"])
            absDt, Dd = blk(np.abs(D), np.abs(P["r"])), blk(np.abs(D), delta)
            w0 = W.get_w(0)
            close_to(w0, ref, (Dd + 3 * u * (absDt + Dd) + u * np.abs(ref)) * (1 + 2.0 ** -20) + 3 * 2.0 ** -53 * absDt,
                     "bj prologue: w0")
            nw0 = float(np.sqrt((w0.astype(R.LD) ** 2).sum()))
            close_to(W.get_report()[1], nw0, ((n + 2) * 2.0 ** -53 + u) * nw0, "bj prologue: beta")
