"""Every fused Arnoldi phase launch (include/mpgmres/arnoldi.h) against the
fp64 restatement of the operation it performs (tests/arnoldi_ref_np.py).

The workspace state is injected (tests/arnoldi_phase.py), one launch runs, and
what it left is compared with the restatement under a derived bound (written
beside each check; tests/test_arnoldi_ref_cpu.py shows each bound sees a
dropped row, swapped columns, a shifted coefficient, k off by one and ld taken
as n). Where a launch reads what another launch wrote (a coefficient, w'), the
reference is fed with the device's own value, so every bound stays tight.

Entry points and the cases that cover them:
  prologue, prologue_finish, prologue_finish_partials   test_prologue
  spmv                                                  test_spmv_step (csr, sell-pair, sell-single, sell-ragged,
                                                        sell-gather, sell-stencil, node; jacobi)
  givens_spmv, givens_partials_spmv                     test_spmv_fold
  spmv_dots                                             test_spmv_dots
  step_dots                                             test_step_dots
  dots (one panel, k_dots_panels, row grid; MGS)        test_dots
  dots_sums                                             test_dots
  cgs (pass 0, pass 1), cgs_givens                      test_cgs_from_sums, test_cgsr
  cgs_partials (plain, prefetch, stream, wide)          test_cgs_partials
  cgsr_wide_pass                                        test_cgsr_wide
  mgs, mgs_partials                                     test_mgs
  givens                                                test_givens_bits, test_cgsr, test_cgsr_wide
  givens_partials                                       test_cgs_from_sums
  update                                                test_update
  update_tail                                           test_update_tail
  reduce                                                every sum below
  compressed basis (dots, cgs_partials, update)         test_basis16
Not covered here (one rank, fp32 / fp64 values, plain int16 or int32 SELL
columns): the stepped int16 column form of the SELL copy, halo rows (n_front
> 0, n_ext > n), fp16 matrix values and block Jacobi inside the node launches
are tests/test_arnoldi_variants_gpu.py's, by the same method; its header
lists what remains uncovered after both files."""
import functools

import numpy as np
import pytest

from tests import arnoldi_ref_np as R
from tests.arnoldi_phase import CLASSES, MATRICES, MPG_ERR_UNSUPPORTED, PhaseWorkspace
from tests.basis16_np import pack_f16, round_f16

pytestmark = pytest.mark.gpu

BANDS = ["band260", "band4099", "band4100", "band8197"]
CLS = sorted(CLASSES)


# ---------------------------------------------------------------- shared inputs, made once
@functools.lru_cache(maxsize=None)
def _matrix(name):
    from tests.conftest import load_package

    return MATRICES[name](load_package())


@functools.lru_cache(maxsize=None)
def _a64(name, t):
    return R.csr64(_matrix(name), np.float32 if t == "f32" else np.float64)


@functools.lru_cache(maxsize=None)
def _basis(n, ld, ncols, dtype):
    V = R.gen_basis(n, ld, ncols, 11, dtype)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def _pbasis(n, ld, ncols, dtype):
    """R.gen_basis_toward of the shared w (R.W_SEED): the cases whose coefficients are the dots themselves."""
    V = R.gen_basis_toward(R.gen_vec(n, R.W_SEED, 5, dtype), n, ld, ncols, 11, dtype)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def _pdots(n, ld, ncols, dtype):
    return R.ref_dots(_pbasis(n, ld, ncols, dtype)[:n], _vec(n, R.W_SEED, 5, dtype))


@functools.lru_cache(maxsize=None)
def _vec(n, seed, j, dtype):
    v = R.gen_vec(n, seed, j, dtype)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _dots_of(n, ld, ncols, dtype, seed):
    """ref_dots of the shared basis with the shared w (seed), all columns at once."""
    return R.ref_dots(_basis(n, ld, ncols, dtype)[:n], _vec(n, seed, 5, dtype))


class _Ws:
    """Context manager around PhaseWorkspace (closed whatever the test does)."""

    def __init__(self, hip, name, cls, **kw):
        from tests.conftest import load_package

        t, accum = CLASSES[cls]
        self.W = PhaseWorkspace(load_package(), hip, _matrix(name), t, kw.pop("fmt", 1), accum, **kw)

    def __enter__(self):
        return self.W

    def __exit__(self, *exc):
        self.W.close()


def close_to(got, ref, tol, what):
    """|got - ref| <= tol elementwise; the worst ratio is printed first."""
    got, ref, tol = np.atleast_1d(got).astype(np.float64), np.atleast_1d(ref), np.atleast_1d(tol)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (what, got.shape, ref.shape)
    ratio = np.abs(got - ref) / np.maximum(tol, 1e-300)
    i = int(np.argmax(ratio))
    print(f"{what}: worst |err|/tol = {ratio[i]:.3g} at {i}")
    assert ratio[i] <= 1.0, (what, i, float(got[i]), float(ref[i]), float(tol[i]))


def same_bits(got, ref, what):
    got, ref = np.atleast_1d(got), np.atleast_1d(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), (what, int(np.sum(got != ref)), got[got != ref][:4], ref[got != ref][:4])


def check_norm2(W, w_dev, what):
    """reduce(1) of the ||w'||^2 partials a launch emitted against the exact
    sum over the device's own w' (tol_sum: the dot bound)."""
    ref, abs_sum = R.ref_dots(w_dev[:, None], w_dev)
    close_to(W.reduce(1), ref, R.tol_sum(ref, abs_sum, W.n, W.T, W.acc32), what)
    return float(ref[0])


def check_givens_close(W, k, G, got, nrm_tol_rel, what):
    """Givens outputs formed from a norm the device summed itself: hn within
    the dot bound's square-root image (d sqrt(x) = dx / (2 sqrt(x)), plus the
    rounding to T); every other output within 8 eps_T of its scale (the
    column's largest entry, 1 for cs / sn, |s_k| + |s_k+1| for s), eps_T = 2 u_T:
    a relative change d of hn moves r, c, s and the rotated s by at most d
    times that scale, and the step itself is under ten roundings."""
    eps = 2 * R.unit(W.T)
    u = R.unit(W.T)
    hn = float(G["hn"])
    inv_ref = 1.0 / hn
    close_to(got["inv"], inv_ref, (0.5 * nrm_tol_rel + 3 * u) * inv_ref, what + " inv")
    cscale = float(np.max(np.abs(G["col"].astype(np.float64))) + hn)
    close_to(got["col"], G["col"].astype(np.float64), np.full(k + 2, 8 * eps * cscale), what + " H(:,k)")
    close_to([got["cs"], got["sn"]], [float(G["cs"]), float(G["sn"])], np.full(2, 8 * eps), what + " cs, sn")
    ss = float(np.sum(np.abs(G["s"].astype(np.float64))))
    close_to(got["s"], G["s"].astype(np.float64), np.full(2, 8 * eps * ss), what + " s")
    close_to(got["report"], G["report"], 8 * eps * ss, what + " report")


def read_givens(W, k, staged_col=None):
    H = W.get_H() if staged_col is None else None
    s = W.get_rot(2)
    return dict(col=H[:k + 2, k] if H is not None else staged_col, cs=W.get_rot(0)[k], sn=W.get_rot(1)[k],
                s=s[k:k + 2], inv=W.get_inv(), report=W.get_report()[4 + k])


# ---------------------------------------------------------------- dots
# (orth, launch, k + 1): one panel (<= 32), k_dots_panels (33 .. 128), the row-grid passes (129)
DOTS = ([("cgs", "dots", nc) for nc in (1, 8, 9, 32, 33, 64, 128, 129)] +
        [("cgsr", "dots", nc) for nc in (1, 8, 9, 32, 33, 64, 128, 129)] +
        [("mgs", "dots", 1), ("mgs", "dots", 4)] +  # (MGS: one column, <v_0, w>, whatever k)
        [("cgs", "dots_sums", nc) for nc in (1, 9, 32)])


@pytest.mark.parametrize("orth", ["cgs", "cgsr", "mgs"])
@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_dots(hip, cls, name, orth):
    """The partials of <v_j, w>, j <= k, summed by reduce (dots) or by the
    launch's last workgroup (dots_sums): tol_sum."""
    with _Ws(hip, name, cls, m=130, orth=orth) as W:
        n = W.n
        assert W.groups() * 1024 >= n  # the row-grid forms: at most one quad of rows per lane (tol_sum's depth)
        V, w = _basis(n, W.ld, 130, W.T), _vec(n, R.W_SEED, 5, W.T)
        ref, abs_sum = _dots_of(n, W.ld, 130, W.T, R.W_SEED)
        W.put_V(V)
        for o, launch, nc in DOTS:
            if o != orth:
                continue
            k = nc - 1
            W.put_w(k + 1, w)
            W.put_sums(np.full(W.m + 4, np.nan))
            W.launch(launch, k)
            ncols = 1 if orth == "mgs" else nc
            got = W.get_sums(ncols) if launch == "dots_sums" else W.reduce(ncols)
            close_to(got, ref[:ncols], R.tol_sum(ref[:ncols], abs_sum[:ncols], n, W.T, W.acc32),
                     f"{launch} {orth} nc={nc}")
            same_bits(W.get_w(k + 1), w, "w untouched")


# ---------------------------------------------------------------- CGS update
_coefs = R.gen_coefs


def _check_update(W, V, c_dev, w_old, w_new, what):
    """w' against ref_cgs_update fed with the coefficients the device stored: tol_rows."""
    ref, t, scale = R.ref_cgs_update(V, c_dev, w_old)
    close_to(w_new, ref, R.tol_rows(ref, t, scale, len(c_dev), W.T, W.acc32), what)


# launch -> (restart length, k + 1): cgs_givens exists up to mpg_arnoldi_fold_max_m() = 128
CGS_SUMS = {"cgs": (130, (1, 8, 9, 32, 33, 129)), "cgs_givens": (40, (1, 9, 32, 33))}


@pytest.mark.parametrize("launch", sorted(CGS_SUMS))
@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_cgs_from_sums(hip, cls, name, launch):
    """cgs(k, 0) from injected sums, then givens_partials(k) on its partials;
    cgs_givens(k, 0), the two in one launch."""
    m, ncs = CGS_SUMS[launch]
    with _Ws(hip, name, cls, m=m) as W:
        n = W.n
        Vfull, w = _basis(n, W.ld, m, W.T), _vec(n, 22, 5, W.T)
        W.put_V(Vfull)
        cs, sn, s = R.gen_rotations(W.m, 5, W.T)
        for nc in ncs:
            k, c64 = nc - 1, _coefs(nc)
            c = c64.astype(W.T)
            W.put_w(k + 1, w)
            W.put_sums(c64)
            for q, v in enumerate((cs, sn, s)):
                W.put_rot(q, v)
            W.launch(launch, k, 0)
            w1 = W.get_w(k + 1)
            if launch == "cgs":
                same_bits(W.get_H()[:nc, k], c, f"cgs nc={nc}: H(:,k) = T(sums)")
            _check_update(W, Vfull[:n, :nc], c, w, w1, f"{launch} nc={nc}: w'")
            if launch == "cgs":
                nrm = check_norm2(W, w1, f"cgs nc={nc}: ||w'||^2")
                W.launch("givens_partials", k)  # right behind its producer
            else:
                nrm = float(R.ref_dots(w1[:, None], w1)[0][0])
            G = R.ref_givens(k, np.concatenate([c, [0]]).astype(W.T), None, cs, sn, s, nrm, W.T)
            rel = R.tol_sum(nrm, nrm, n, W.T, W.acc32) / nrm
            check_givens_close(W, k, G, read_givens(W, k), rel, f"{launch} nc={nc}: givens")


# (MPG_CGS_PREFETCH, k + 1) -> the form cgs_stream_at must name (1: the streaming form), per class
def _stream_expected(cls, pref, nc):
    if cls != "f32-acc32" or pref == "0" or nc > 32:
        return 0
    return 1 if pref == "1" or nc >= 9 else 0


@pytest.mark.parametrize("pref", [None, "0", "1"])
@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_cgs_partials(hip, monkeypatch, cls, name, pref):
    """dots(k), then cgs_partials(k), which sums the coefficients itself: the
    plain, prefetch and streaming forms (<= 32 columns) and k_cgs_update_wide
    (33, 128)."""
    if pref is None:
        monkeypatch.delenv("MPG_CGS_PREFETCH", raising=False)
    else:
        monkeypatch.setenv("MPG_CGS_PREFETCH", pref)
    with _Ws(hip, name, cls, m=130) as W:
        n = W.n
        Vfull, w = _pbasis(n, W.ld, 130, W.T), _vec(n, R.W_SEED, 5, W.T)
        dref, dabs = _pdots(n, W.ld, 130, W.T)
        W.put_V(Vfull)
        for nc in (1, 4, 5, 8, 9, 10, 18, 32) + ((33, 128) if pref is None else ()):
            k = nc - 1
            W.expect("cgs_stream_at", (k,), _stream_expected(cls, pref, nc))
            W.put_w(k + 1, w)
            W.launch("dots", k)
            W.launch("cgs_partials", k)
            c = W.get_H()[:nc, k]
            # the dot bound plus the rounding of the stored coefficient to T (eps_T)
            close_to(c, dref[:nc], R.tol_sum(dref[:nc], dabs[:nc], n, W.T, W.acc32) + 2 * R.unit(W.T) * np.abs(dref[:nc]),
                     f"cgs_partials nc={nc}: coefficients")
            w1 = W.get_w(k + 1)
            _check_update(W, Vfull[:n, :nc], c, w, w1, f"cgs_partials nc={nc}: w'")
            check_norm2(W, w1, f"cgs_partials nc={nc}: ||w'||^2")


def _read_corr(W, k):
    """The CGSR correction the last pass-1 launch left in the workspace, exactly:
    givens(k) on a zero column with identity rotations and ||w||^2 = 0 stores
    0 + 1 * corr_j below the diagonal and rotg(corr_k, 0) = corr_k on it."""
    H = W.get_H()
    H[:, k] = 0
    W.put_H(H)
    one = np.zeros(W.m + 1, W.T)
    W.put_rot(0, one + 1)
    W.put_rot(1, one)
    W.put_rot(2, one)
    W.put_sums(np.zeros(1))
    W.launch("givens", k)
    return W.get_H()[:k + 1, k].copy()


def _check_givens_corr(W, k, h, corr):
    """givens(k) under CGSR adds the correction: bit equality with ref_givens on h + corr."""
    cs, sn, s = R.gen_rotations(W.m, 6, W.T)
    H = W.get_H()
    H[:k + 1, k] = h
    W.put_H(H)
    for q, v in enumerate((cs, sn, s)):
        W.put_rot(q, v)
    nrm = 2.7182818
    W.put_sums(np.array([nrm]))
    W.launch("givens", k)
    G = R.ref_givens(k, np.concatenate([h, [0]]).astype(W.T), corr, cs, sn, s, nrm, W.T)
    got = read_givens(W, k)
    for key in ("col", "cs", "sn", "s", "inv"):
        same_bits(got[key], G[key], f"givens k={k} with correction: {key}")


@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_cgsr(hip, cls, name):
    """CGSR from sums: pass 0 (coefficients, update, the next dots' partials)
    and pass 1 (the correction, seen through givens(k), and ||w''||^2)."""
    with _Ws(hip, name, cls, m=40, orth="cgsr") as W:
        n = W.n
        Vfull, w = _basis(n, W.ld, 41, W.T), _vec(n, 23, 5, W.T)
        W.put_V(Vfull)
        for nc in (9, 32, 33):
            k, V = nc - 1, Vfull[:n, :nc]
            c64 = _coefs(nc)
            W.put_w(k + 1, w)
            W.put_sums(c64)
            W.launch("cgs", k, 0)
            h = W.get_H()[:nc, k].copy()
            same_bits(h, c64.astype(W.T), f"cgsr pass 0 nc={nc}: H(:,k)")
            w1 = W.get_w(k + 1)
            _check_update(W, V, h, w, w1, f"cgsr pass 0 nc={nc}: w'")
            ref, abs_sum = R.ref_dots(V, w1)
            close_to(W.reduce(nc), ref, R.tol_sum(ref, abs_sum, n, W.T, W.acc32), f"cgsr pass 0 nc={nc}: next dots")
            c2 = _coefs(nc, seed=32)
            W.put_sums(c2)
            W.launch("cgs", k, 1)
            w2 = W.get_w(k + 1)
            check_norm2(W, w2, f"cgsr pass 1 nc={nc}: ||w''||^2")
            same_bits(W.get_H()[:nc, k], h, "pass 1 leaves H(:,k)")
            corr = _read_corr(W, k)
            same_bits(corr, c2.astype(W.T), f"cgsr pass 1 nc={nc}: correction = T(sums)")
            _check_update(W, V, corr, w1, w2, f"cgsr pass 1 nc={nc}: w''")
            _check_givens_corr(W, k, h, corr)


@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_cgsr_wide(hip, cls, name):
    """CGSR at 32 < k + 1 <= 128: dots, cgsr_wide_pass(k, 0), dots,
    cgsr_wide_pass(k, 1), each pass summing its coefficients from the
    preceding k_dots_panels partials."""
    with _Ws(hip, name, cls, m=130, orth="cgsr") as W:
        n = W.n
        Vfull, w = _pbasis(n, W.ld, 130, W.T), _vec(n, R.W_SEED, 5, W.T)
        dref, dabs = _pdots(n, W.ld, 130, W.T)
        W.put_V(Vfull)
        for nc in (33, 128):
            k, V = nc - 1, Vfull[:n, :nc]
            W.put_w(k + 1, w)
            W.launch("dots", k)
            W.launch("cgsr_wide_pass", k, 0)
            h = W.get_H()[:nc, k].copy()
            close_to(h, dref[:nc], R.tol_sum(dref[:nc], dabs[:nc], n, W.T, W.acc32) + 2 * R.unit(W.T) * np.abs(dref[:nc]),
                     f"wide pass 0 nc={nc}: coefficients")
            w1 = W.get_w(k + 1)
            _check_update(W, V, h, w, w1, f"wide pass 0 nc={nc}: w'")
            check_norm2(W, w1, f"wide pass 0 nc={nc}: ||w'||^2")
            W.launch("dots", k)
            W.launch("cgsr_wide_pass", k, 1)
            w2 = W.get_w(k + 1)
            check_norm2(W, w2, f"wide pass 1 nc={nc}: ||w''||^2")
            corr = _read_corr(W, k)
            ref, abs_sum = R.ref_dots(V, w1)
            close_to(corr, ref, R.tol_sum(ref, abs_sum, n, W.T, W.acc32) + 2 * R.unit(W.T) * np.abs(ref),
                     f"wide pass 1 nc={nc}: correction")
            _check_update(W, V, corr, w1, w2, f"wide pass 1 nc={nc}: w''")
            _check_givens_corr(W, k, h, corr)


# ---------------------------------------------------------------- MGS
@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_mgs(hip, cls, name):
    """mgs(k, j) from sums, and the chain dots -> mgs_partials(k, 0 .. k):
    h_jk, w' (one term, in T: tol_rows) and the next partial, <v_j+1, w'> or
    ||w'||^2 for j = k."""
    with _Ws(hip, name, cls, m=4, orth="mgs") as W:
        n = W.n
        Vfull, w = _basis(n, W.ld, 5, W.T), _vec(n, R.W_SEED, 5, W.T)
        W.put_V(Vfull)

        def after(k, j, h, w_old, what):
            w1 = W.get_w(k + 1)
            ref, t, scale = R.ref_mgs_update(Vfull[:n, j], h, w_old)
            close_to(w1, ref, R.tol_rows(ref, t, scale, 1, W.T, W.acc32), what + ": w'")
            nxt = w1 if j == k else Vfull[:n, j + 1]
            dref, dabs = R.ref_dots(nxt[:, None], w1)
            return w1, dref, R.tol_sum(dref, dabs, n, W.T, W.acc32)

        for k, j in ((0, 0), (3, 0), (3, 2), (3, 3)):
            h64 = 0.15 + 1e-9
            W.put_w(k + 1, w)
            W.put_sums(np.array([h64]))
            W.launch("mgs", k, j)
            h = W.get_H()[j, k]
            same_bits(h, W.T(h64), f"mgs({k},{j}): h = T(sums[0])")
            _, dref, tol = after(k, j, h, w, f"mgs({k},{j})")
            close_to(W.reduce(1), dref, tol, f"mgs({k},{j}): next partial")
        Vfull = _pbasis(n, W.ld, 5, W.T)  # (the chain's coefficients are the dots themselves)
        W.put_V(Vfull)
        for k in (0, 3):
            W.put_w(k + 1, w)
            W.launch("dots", k)
            cur = w
            dref, dabs = R.ref_dots(Vfull[:n, :1], cur)
            tol = R.tol_sum(dref, dabs, n, W.T, W.acc32)
            for j in range(k + 1):
                W.launch("mgs_partials", k, j)
                h = W.get_H()[j, k]
                close_to(h, dref, tol + 2 * R.unit(W.T) * np.abs(dref), f"mgs_partials({k},{j}): h")
                cur, dref, tol = after(k, j, h, cur, f"mgs_partials({k},{j})")
            close_to(W.reduce(1), dref, tol, f"mgs_partials({k},{k}): ||w'||^2")


# ---------------------------------------------------------------- Givens
@pytest.mark.parametrize("cls", CLS)
def test_givens_bits(hip, cls):
    """givens(k) from sums[0]: every output has the bits of ref_givens (the
    step is a fixed sequence of T operations with no contraction), and
    nothing else of H, cs, sn, s moves."""
    with _Ws(hip, "band260", cls, m=100) as W:
        m = W.m
        cs, sn, s = R.gen_rotations(m, 7, W.T)
        H0 = np.asfortranarray(R.gen_vec((m + 1) * m, 8, 0, W.T).reshape((m + 1, m), order="F"))
        for k in (0, 1, 7, 31, 99):
            nrm = 1.75 + 0.01 * k + 1e-9
            W.put_H(H0)
            for q, v in enumerate((cs, sn, s)):
                W.put_rot(q, v)
            W.put_sums(np.array([nrm]))
            W.put_report(np.zeros(m + 4))
            W.launch("givens", k)
            G = R.ref_givens(k, H0[:k + 2, k], None, cs, sn, s, nrm, W.T)
            got = read_givens(W, k)
            for key in ("col", "cs", "sn", "s", "inv"):
                same_bits(got[key], G[key], f"givens k={k}: {key}")
            assert got["report"] == G["report"], (k, got["report"], G["report"])
            H, Hx = W.get_H(), H0.copy()
            Hx[:k + 2, k] = G["col"]
            same_bits(H, Hx, f"givens k={k}: the rest of H")
            for q, v in enumerate((cs, sn, s)):
                x = v.copy()
                x[k:k + (2 if q == 2 else 1)] = G["s"] if q == 2 else G["cs" if q == 0 else "sn"]
                same_bits(W.get_rot(q), x, f"givens k={k}: rotations {q}")


# ---------------------------------------------------------------- SpMV step
# storage -> (matrix, spmv_format, MPG_SELL_PAIR, expected format, window, slices per wave, SELL column form)
STORAGE = {
    "csr": ("band4099", 1, None, 1, 0, 0, -1),
    "csr-stencil": ("stencil5", 1, None, 1, 0, 0, -1),
    "sell-pair": ("band8197", 2, None, 2, 1, 2, 1),     # k_step_sell2 with the v_k window
    "sell-single": ("band8197", 2, "0", 2, 1, 1, 1),    # k_step_sell, one slice per wave
    # (band4099's last slice, rows 4096 .. 4098, is 8 entries wide, not 10: slices of unequal width)
    "sell-ragged": ("band4099", 2, None, 2, 1, 1, 1),
    "sell-gather": ("lap12", 2, None, 2, 0, None, 1),   # no window: v_k gathered from memory
    "sell-stencil": ("stencil5", 2, None, 2, 0, None, 1),  # 81 entries per row, gathered
    "node": ("stencil5", 3, None, 3, 0, 0, -1),
}


def _storage_ws(hip, monkeypatch, storage, cls, **kw):
    name, fmt, pair, xfmt, xwin, xspw, xform = STORAGE[storage]
    if pair is None:
        monkeypatch.delenv("MPG_SELL_PAIR", raising=False)
    else:
        monkeypatch.setenv("MPG_SELL_PAIR", pair)
    ws = _Ws(hip, name, cls, fmt=fmt, **kw)
    W = ws.W
    try:
        assert (W.format, W.window) == (xfmt, xwin), (storage, W.format, W.window)
        if xspw is not None:
            assert W.lib.mpg_arnoldi_slices_per_wave(W.arn) == xspw, storage
        if xform is not None:
            assert W.sell_form() == xform, (storage, W.sell_form())
    except BaseException:
        W.close()
        raise
    return ws, name


def _check_spmv(W, name, k, w_prev, inv, jacobi, what):
    """V(:,k) has the bits of T(w_prev * inv); w = M(A v) against the fp64 row
    sums: tol_rows' sum term over the row's entries, and one rounding to T
    (three with Jacobi: the row sum, d * w and its store)."""
    A64 = _a64(name, W.t)
    d = W.diag.get() if jacobi else None
    v, ref, scale = R.ref_spmv_step(A64, w_prev, inv, d)
    same_bits(W.get_V(k), v, what + ": V(:,k)")
    terms = int(np.diff(A64.indptr).max())
    ua = 2.0 ** -24 if W.acc32 else 2.0 ** -53
    w1 = W.get_w(k + 1)
    # (and the restatement's own fp64 row sums: (terms + 1) 2^-53 scale)
    close_to(w1, ref, ((3 if jacobi else 1) * R.unit(W.T) * np.abs(ref) + (terms + 1) * (ua + 2.0 ** -53) * scale)
             * (1 + 2.0 ** -20), what + ": w")
    return v, w1


# (storage, jacobi): Jacobi inside the launch on the band's forms
SPMV_CASES = [(st, 0) for st in sorted(STORAGE)] + [(st, 1) for st in ("csr", "sell-pair", "sell-single", "sell-ragged")]


@pytest.mark.parametrize("storage,jacobi", SPMV_CASES)
@pytest.mark.parametrize("cls", CLS)
def test_spmv_step(hip, monkeypatch, cls, storage, jacobi):
    """spmv(k), k = 0, 1, on every storage form."""
    ws, name = _storage_ws(hip, monkeypatch, storage, cls, jacobi=jacobi)
    with ws as W:
        inv = W.T(0.37)
        for k in (0, 1):
            w_prev = _vec(W.n, 25 + k, 5, W.T)
            W.put_inv(inv)
            W.put_w(k, w_prev)
            W.put_w(k + 1, np.full(W.n, np.nan, W.T))  # a row the launch leaves out stays NaN (close_to refuses it)
            W.launch("spmv", k)
            _check_spmv(W, name, k, w_prev, inv, jacobi, f"spmv {storage} k={k}")
            same_bits(W.get_w(k), w_prev, "w_prev untouched")


@pytest.mark.parametrize("storage", ["csr", "sell-pair", "sell-single", "sell-ragged", "node"])
@pytest.mark.parametrize("cls", CLS)
def test_spmv_fold(hip, monkeypatch, cls, storage):
    """givens_spmv(1) (||w||^2 from sums[0]: the Givens outputs bit for bit)
    and givens_partials_spmv(1) behind a real producer, cgs(0, 0)."""
    ws, name = _storage_ws(hip, monkeypatch, storage, cls, m=6)
    with ws as W:
        n = W.n
        Vfull, w = _basis(n, W.ld, 7, W.T), _vec(n, 26, 5, W.T)
        cs, sn, s = R.gen_rotations(W.m, 9, W.T)
        for fold in (1, 2):
            W.put_V(Vfull)
            W.put_w(1, w)
            c64 = _coefs(1)
            W.put_sums(c64)
            W.launch("cgs", 0, 0)
            w1 = W.get_w(1)
            nrm = float(R.ref_dots(w1[:, None], w1)[0][0])
            for q, v in enumerate((cs, sn, s)):
                W.put_rot(q, v)
            if fold == 1:
                W.put_sums(np.array([nrm]))
                W.launch("givens_spmv", 1)
            else:
                W.launch("givens_partials_spmv", 1)
            G = R.ref_givens(0, np.array([c64[0], 0]).astype(W.T), None, cs, sn, s, nrm, W.T)
            got = read_givens(W, 0)
            if fold == 1:
                for key in ("col", "cs", "sn", "s", "inv"):
                    same_bits(got[key], G[key], f"givens_spmv {storage}: {key}")
            else:
                check_givens_close(W, 0, G, got, R.tol_sum(nrm, nrm, n, W.T, W.acc32) / nrm,
                                   f"givens_partials_spmv {storage}")
            _check_spmv(W, name, 1, w1, got["inv"], 0, f"fold {fold} {storage}")


def _check_fused_dots(W, name, k, Vfull, w_prev, inv, what):
    v, w1 = _check_spmv(W, name, k, w_prev, inv, 0, what)
    V = np.column_stack([Vfull[:W.n, :k], v]) if k else v[:, None]
    ref, abs_sum = R.ref_dots(V, w1)
    close_to(W.reduce(k + 1), ref, R.tol_sum(ref, abs_sum, W.n, W.T, W.acc32), what + ": dots")


@pytest.mark.parametrize("name", BANDS)
def test_spmv_dots(hip, monkeypatch, name):
    """spmv_dots(k, 0): the SELL step with the panel dots in its launch (fp64 class only)."""
    monkeypatch.delenv("MPG_SELL_PAIR", raising=False)
    with _Ws(hip, name, "f32-acc64", fmt=2, m=32) as W:
        assert (W.format, W.window) == (2, 1)
        Vfull = _basis(W.n, W.ld, 33, W.T)
        inv = W.T(0.37)
        for k in (0, 1, 8, 16, 31):
            w_prev = _vec(W.n, 27, 5, W.T)
            W.put_V(Vfull)
            W.put_inv(inv)
            W.put_w(k, w_prev)
            W.launch_if("spmv_dots", "spmv_dots_supported", (k,), k, 0)
            _check_fused_dots(W, name, k, Vfull, w_prev, inv, f"spmv_dots k={k}")
    with _Ws(hip, name, "f32-acc32", fmt=2, m=32) as W:
        W.expect("spmv_dots_supported", (0,), MPG_ERR_UNSUPPORTED)


@pytest.mark.parametrize("name", ["band260", "band4100", "band8196"])
def test_step_dots(hip, monkeypatch, name):
    """step_dots(k, fold) in the fp32 class: the SpMV inside the panel dots'
    launch; fold 2 takes the Givens step k - 1 from cgs(k - 1, 0)'s partials."""
    monkeypatch.delenv("MPG_SELL_PAIR", raising=False)
    with _Ws(hip, name, "f32-acc32", fmt=2, m=32) as W:
        n = W.n
        Vfull = _basis(n, W.ld, 33, W.T)
        cs, sn, s = R.gen_rotations(W.m, 9, W.T)
        for k in (0, 1, 8, 31):
            for fold in (0, 2):
                if fold and k == 0:
                    continue
                w_prev = _vec(n, 28, 5, W.T)
                W.put_V(Vfull)
                W.put_w(k, w_prev)
                if fold:
                    c64 = _coefs(k)
                    W.put_sums(c64)
                    W.launch("cgs", k - 1, 0)  # w_prev of step k is its w'
                    w_prev = W.get_w(k)
                    nrm = float(R.ref_dots(w_prev[:, None], w_prev)[0][0])
                    for q, v in enumerate((cs, sn, s)):
                        W.put_rot(q, v)
                else:
                    W.put_inv(W.T(0.37))
                W.launch_if("step_dots", "step_dots_supported", (k,), k, fold)
                inv = W.get_inv()
                if fold:
                    G = R.ref_givens(k - 1, np.concatenate([c64, [0]]).astype(W.T), None, cs, sn, s, nrm, W.T)
                    check_givens_close(W, k - 1, G, read_givens(W, k - 1), R.tol_sum(nrm, nrm, n, W.T, True) / nrm,
                                       f"step_dots k={k} fold")
                _check_fused_dots(W, name, k, Vfull, w_prev, inv, f"step_dots k={k} fold={fold}")
    with _Ws(hip, name, "f32-acc64", fmt=2, m=32) as W:
        W.expect("step_dots_supported", (0,), MPG_ERR_UNSUPPORTED)


# ---------------------------------------------------------------- update
def _update_inputs(W, k, ncols):
    H = R.gen_upper(W.m, k, 41, W.T)
    s = _vec(W.m + 1, 42, 0, W.T)
    x0 = _vec(W.n, 43, 3, np.float64)
    return H, s, x0, _basis(W.n, W.ld, ncols, W.T)


@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_update(hip, cls, name):
    """update(k): x + X(T(V y)), y = H(0:k,0:k)^-1 s(0:k): the one-panel
    form (<= 32), k_update_x with the wave solve (<= 64), and the separate
    solves k_trsv_upper_lds / k_trsv_upper (fp64: 127 against 128): tol_update."""
    with _Ws(hip, name, cls, m=130) as W:
        V = _basis(W.n, W.ld, 130, W.T)
        W.put_V(V)
        for k in (1, 8, 32, 33, 64, 65, 127, 128, 130):
            H, s, x0, _ = _update_inputs(W, k, 130)
            W.put_H(H)
            W.put_rot(2, s)
            W.put_x(x0)
            W.launch("update", k)
            U = R.ref_update(V[:W.n], H, s, k, x0)
            close_to(W.get_x(), U["x"], R.tol_update(U, k, U["x"], W.T, np.float64, W.acc32), f"update k={k}")


@pytest.mark.parametrize("m", [1, 9, 32])
@pytest.mark.parametrize("name", BANDS)
@pytest.mark.parametrize("cls", CLS)
def test_update_tail(hip, cls, name, m):
    """update_tail(m, flags) behind cgs(m - 1, 0): Givens step m - 1 from the
    partials, the solve, the update and (flags 1) the x snapshot in one
    launch; the rotated column reaches H in the next finish launch."""
    with _Ws(hip, name, cls, m=m) as W:
        n, k = W.n, m - 1
        H0, s, x0, V = _update_inputs(W, m, m + 1)
        cs, sn, _ = R.gen_rotations(m, 9, W.T)
        w = _vec(n, 29, 5, W.T)
        W.put_V(V)
        for flags in (0, 1):
            _tail_case(hip, W, m, flags, H0, s, x0, V, cs, sn, w)


def _tail_case(hip, W, m, flags, H0, s, x0, V, cs, sn, w):
    n, k = W.n, m - 1
    snap = hip.buf(np.full(n, 7.0))
    try:
        W.put_H(H0)
        for q, v in enumerate((cs, sn, s)):
            W.put_rot(q, v)
        W.put_x(x0)
        W.put_w(m, w)
        c64 = _coefs(m)
        W.put_sums(c64)
        W.launch("cgs", k, 0)
        w1 = W.get_w(m)
        nrm = float(R.ref_dots(w1[:, None], w1)[0][0])
        hip.check(W.lib.mpg_arnoldi_set_x_snapshot(W.arn, snap.p if flags else None), "set_x_snapshot")
        W.launch_if("update_tail", "update_tail_supported", (), m, flags)
        G = R.ref_givens(k, np.concatenate([c64, [0]]).astype(W.T), None, cs, sn, s, nrm, W.T)
        rel = R.tol_sum(nrm, nrm, n, W.T, W.acc32) / nrm
        x1 = W.get_x()
        if flags:
            same_bits(snap.get(), x0, "the snapshot is the old x")
        # the solve runs on the rotated column and s_k
        Hr, sr = H0.copy(), s.copy()
        Hr[:m + 1, k] = G["col"]
        sr[k] = G["s"][0]
        U = R.ref_update(V[:n], Hr, sr, m, x0)
        # ... which the device formed from its own norm: a relative change e of the column and of s_k moves y
        # by at most e |H^-1| (|H| |y| + |s|) <= 2 e g; e = check_givens_close's 8 eps_T
        tol = R.tol_update(U, m, U["x"], W.T, np.float64, W.acc32) + 2 * 16 * R.unit(W.T) * U["absVg"]
        close_to(x1, U["x"], tol, f"update_tail m={m} flags={flags}: x")
        # cs, sn, 1/h and the report entry are stored in place (check_givens_close's bounds). The rotated
        # column is staged (checked below, once the finish launch has put it into H) and the rotated s is
        # not stored at all: it is seen through x only
        eps = 2 * R.unit(W.T)
        hn = float(G["hn"])
        close_to(W.get_inv(), 1.0 / hn, (0.5 * rel + 3 * R.unit(W.T)) / hn, f"update_tail m={m}: inv")
        close_to([W.get_rot(0)[k], W.get_rot(1)[k]], [float(G["cs"]), float(G["sn"])], np.full(2, 8 * eps),
                 f"update_tail m={m}: cs, sn")
        ss = float(np.sum(np.abs(G["s"].astype(np.float64))))
        close_to(W.get_report()[4 + k], G["report"], 8 * eps * ss, f"update_tail m={m}: report")
        W.launch("prologue")
        W.launch("prologue_finish_partials")
        close_to(W.get_H()[:m + 1, k], G["col"].astype(np.float64),
                 np.full(m + 1, 16 * R.unit(W.T) * float(np.max(np.abs(G["col"])) + G["hn"])),
                 f"update_tail m={m}: staged column in H")
        same_bits(W.get_H()[:, :k], H0[:, :k], "the other columns of H")
    finally:
        snap.free()


# ---------------------------------------------------------------- prologue
@pytest.mark.parametrize("finish", ["partials", "reduce"])
@pytest.mark.parametrize("jacobi", [0, 1])
@pytest.mark.parametrize("storage", ["csr", "sell-pair", "node"])
@pytest.mark.parametrize("cls", CLS)
def test_prologue(hip, monkeypatch, cls, storage, jacobi, finish):
    """prologue + finish: w0 = M(T(b - A x)) with a nonzero x, the three norms,
    beta, 1/beta and s = [beta, 0, ...]; mixed (fp64 residual, fp32 Arnoldi)
    and baseline."""
    name = STORAGE[storage][0]
    A = _matrix(name)
    x, b = _vec(A.nrows, 51, 2, np.float64), _vec(A.nrows, 52, 4, np.float64)
    ws, name = _storage_ws(hip, monkeypatch, storage, cls, jacobi=jacobi, x=x, b=b)
    with ws as W:
        n, u = W.n, R.unit(W.T)
        assert W.lib.mpg_arnoldi_prologue_format(W.arn) == STORAGE[storage][3]
        W.put_rot(2, np.full(W.m + 1, 9, W.T))
        W.put_w(0, np.full(n, np.nan, W.T))  # a row the launch leaves out stays NaN
        W.launch("prologue")
        if finish == "partials":
            W.launch("prologue_finish_partials")
        else:
            W.reduce(3)
            W.launch("prologue_finish")
        P = R.ref_prologue(_a64(name, "f64"), b, x, W.T, W.diag.get() if jacobi else None)
        w0 = W.get_w(0)
        # r: an fp64 sum of nnz products and one subtraction, (nnz + 2) 2^-53 (|b| + |A| |x|) whatever the order;
        # then T(r), and with Jacobi d * T(r) rounded to T (the diagonal scales the whole bound)
        # (twice: the device's fp64 evaluation and the restatement's own)
        dr = 2 * (P["nnz_row"] + 2) * 2.0 ** -53 * P["scale"]
        d = np.abs(W.diag.get().astype(np.float64)) if jacobi else 1.0
        close_to(w0, P["w0"].astype(np.float64), (d * (dr + u * np.abs(P["r"])) * (1 + 2 * u) + u * np.abs(P["w0"])),
                 "w0")
        rep = W.get_report()
        # the norms: (n + 2) 2^-53 relative for the sum and the root, one rounding to T (X for x_norm). beta is
        # compared with the norm of the device's own w0; r_norm, whose vector T(r) is not stored when Jacobi
        # follows it, with the restatement's, which may differ from the device's by dr and one rounding per
        # entry: ||T(r)_dev - T(r)_ref|| <= ||dr|| + 2 u ||r||
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
        sums = W.get_sums(3)
        close_to(np.sqrt(sums), [rep[0], rep[1], rep[2]], u * np.abs(rep[:3]), "sums")


# ---------------------------------------------------------------- compressed basis
@pytest.mark.parametrize("storage", ["csr", "sell-pair"])
@pytest.mark.parametrize("cls", ["f32-acc64", "f32-acc32"])
def test_basis16(hip, monkeypatch, cls, storage):
    """MPG_BASIS_F16: V injected as the fp16 bits rne(2^14 v) at the
    documented ld (a multiple of 128 entries); the references read
    2^-14 float(h). dots, cgs_partials and update, one case each."""
    ws, name = _storage_ws(hip, monkeypatch, storage, cls, m=12, basis=1)
    with ws as W:
        n, nc = W.n, 9
        assert W.ld % 128 == 0 and W.ld >= n and W.ld - n < 128, W.ld
        Vv = R.gen_basis_toward(_vec(n, R.W_SEED, 5, W.T), n, W.ld, 13, 11, np.float32)
        W.put_V(np.asfortranarray(pack_f16(Vv)))
        V = round_f16(Vv)[:n]
        w, k = _vec(n, R.W_SEED, 5, W.T), nc - 1
        W.put_w(k + 1, w)
        W.launch("dots", k)
        dref, dabs = R.ref_dots(V[:, :nc], w)
        tol = R.tol_sum(dref, dabs, n, W.T, W.acc32)
        close_to(W.reduce(nc), dref, tol, "f16 dots")
        W.launch("dots", k)
        W.launch("cgs_partials", k)
        c = W.get_H()[:nc, k]
        close_to(c, dref, tol + 2 * R.unit(W.T) * np.abs(dref), "f16 cgs_partials: coefficients")
        w1 = W.get_w(k + 1)
        _check_update(W, V[:, :nc], c, w, w1, "f16 cgs_partials: w'")
        check_norm2(W, w1, "f16 cgs_partials: ||w'||^2")
        H, s, x0, _ = _update_inputs(W, nc, 13)
        W.put_H(H)
        W.put_rot(2, s)
        W.put_x(x0)
        W.launch("update", nc)
        U = R.ref_update(V, H, s, nc, x0)
        close_to(W.get_x(), U["x"], R.tol_update(U, nc, U["x"], W.T, np.float64, W.acc32), "f16 update")
