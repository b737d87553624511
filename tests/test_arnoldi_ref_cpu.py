"""The fp64 restatement of the fused Arnoldi phases (tests/arnoldi_ref_np.py),
without a GPU.

(a) Chained, the restatement is GMRES: it reproduces the Arnoldi relation and
    |s(k+1)| = ||b - A x_k||, which fixes the layouts and the rotation order
    independently of the kernels.
(b) Every bound the GPU tests use (tests/test_arnoldi_phases_gpu.py) can see
    the defects it is there for. Each GPU case's inputs are built again here
    from the same generators and seeds (where a launch reads what an earlier
    one wrote -- a coefficient, w', 1/h -- the restatement's value rounded to
    T stands in for the device's), and a dropped row (the last, row 4096,
    the last of a full quad), two swapped basis columns, a coefficient taken
    from the column before, k off by one and ld taken as n must each move the
    restatement by at least 4 x the bound:
      test_dots                        test_dots_inputs
      test_cgs_from_sums               test_cgs_from_sums_inputs (with the Givens step's 1/h)
      test_cgsr                        test_cgsr_inputs (pass 0, its next dots, pass 1)
      test_cgs_partials, _cgsr_wide    test_partial_fed_inputs (the dots as coefficients, both wide passes)
      test_mgs                         test_mgs_inputs (from sums, and the partials chain)
      test_update, test_update_tail    test_update_inputs (the tail: cgs, Givens, the rotated column and s)
      test_basis16                     test_basis16_inputs
      test_spmv_dots, test_step_dots   test_spmv_dots_inputs, test_step_dots_inputs (w = T(A v), fold 2's 1/h)
      test_spmv_fold                   test_spmv_fold_inputs (the norm under the folded Givens step)
      test_prologue                    test_prologue_inputs (the three norms)
      the Givens bounds                test_givens_tolerance_sees_defects
    Not a matter of a bound: test_givens_bits and the stored V(:,k) are bit
    comparisons, and the SpMV's and the prologue's output vectors are filled
    with NaN before the launch, so a row left out fails whatever the bound.
    "At every output the check covers" is read per mutation: the outputs it
    reaches (a swap of columns j, j + 1 reaches dots j and j + 1; a dropped
    row reaches that row of a vector). A check of a vector fails when any
    one row leaves its bound; a column mutation must move at least a quarter
    of the rows by 4 bounds (not every row can: two entries of random
    magnitude may lie close, and with 130 columns in the fp32 class the row
    bound is (terms + 1) u_32 wide).
(c) The storage variants (tests/test_arnoldi_variants_gpu.py). The generators
    give what the GPU cases rely on: front_pad is arnoldi.h's macro; far33k
    and far66k reach the stepped form with 0 and exactly 1 CSR-summed slice by
    a NumPy restatement of k_sell_span / k_sell_classify; HaloPlan gives the
    band's reach as n_front / n_ext - n; half_values scales up, down and not at
    all within one slice, and nothing rounds to 0 or Inf. And the SpMV and
    prologue bounds see each variant's own defects, on the GPU cases' inputs:
      test_halo                        test_halo_inputs (local columns off by one, halo zero / swapped)
      test_half_values, _halo          test_half_inputs (e_i ignored, e_i+-1, the unscaled cast)
      test_stepped                     test_stepped_inputs (base of k+-1, wrapped offsets, slice skipped)
      test_block_jacobi_node           test_block_jacobi_inputs (not applied, block +-1, transposed)"""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

from tests import arnoldi_ref_np as R
from tests.arnoldi_phase import CLASSES, FAR66_ROW, MATRICES, RANK_SPLITS, RankBlock, front_pad, ld_of

TT = {"f32": np.float32, "f64": np.float64}
BAND_N = [260, 4099, 4100, 8197]
CLS = sorted(CLASSES)


# ---------------------------------------------------------------- (a) the restatement is GMRES
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_chain_is_gmres(t):
    T, n, m = TT[t], 40, 6
    u = R.unit(T)
    rng = np.random.default_rng(3)
    A = sp.csr_matrix(4.0 * np.eye(n) + rng.standard_normal((n, n)) / np.sqrt(n))
    A64 = sp.csr_matrix(A.toarray().astype(T).astype(np.float64))  # the T-valued Arnoldi matrix
    b, x0 = R.gen_vec(n, 1, 0, np.float64), R.gen_vec(n, 2, 0, np.float64) * 0.1
    P = R.ref_prologue(A64, b, x0, T)
    np.testing.assert_allclose(P["beta"], np.linalg.norm(b - A64 @ x0), rtol=(n + 4) * u)
    V = np.zeros((n, m + 1), T, order="F")
    H = np.zeros((m + 1, m), T, order="F")
    Hbar = np.zeros((m + 1, m))
    cs, sn, s = np.zeros(m + 1, T), np.zeros(m + 1, T), np.zeros(m + 1, T)
    s[0] = T(P["beta"])
    w, inv = P["w0"], T(P["inv_beta"])
    AV = np.zeros((n, m))
    absAV = np.zeros((n, m))
    for k in range(m):
        v, w64, scale = R.ref_spmv_step(A64, w, inv)
        V[:, k], AV[:, k], absAV[:, k] = v, w64, scale
        w = w64.astype(T)
        dots, _ = R.ref_dots(V[:, :k + 1], w)
        H[:k + 1, k] = dots.astype(T)
        w = R.ref_cgs_update(V[:, :k + 1], H[:k + 1, k], w)[0].astype(T)
        G = R.ref_givens(k, H[:k + 2, k], None, cs, sn, s, R.ref_dots(w[:, None], w)[0][0], T)
        Hbar[:k + 1, k], Hbar[k + 1, k] = H[:k + 1, k], G["hn"]
        H[:k + 2, k], cs[k], sn[k], s[k:k + 2], inv = G["col"], G["cs"], G["sn"], G["s"], G["inv"]
        assert G["report"] == abs(float(s[k + 1]))
    V[:, m] = (w * inv).astype(T)
    # H-bar again from the rotated H, the rotations undone last to first: the rotation order and the layout
    Hun = H.astype(np.float64)
    for k in range(m):
        for j in range(k, -1, -1):
            a, bb = Hun[j, k], Hun[j + 1, k]
            Hun[j, k], Hun[j + 1, k] = cs[j] * a - sn[j] * bb, sn[j] * a + cs[j] * bb
    # (each rotation and its inverse: a few roundings of entries bounded by the column's norm)
    assert np.max(np.abs(Hun - Hbar)) <= 8 * (m + 1) * u * np.max(np.abs(Hbar))
    assert np.all(np.tril(H[:m, :m], -1) == 0) and np.all(H[m, :] == 0)
    # A V_m = V_m+1 H-bar: per column, T(A v) is one rounding, w' = T(w - V c) one (the relation holds for
    # whatever c was taken), v_k+1 = T(w' T(1 / T(hn))) three: 5 roundings of entries below |A||v| + |V||h|,
    # taken with 4 (m + 2) >= 5 to cover the fp64 evaluation here as well
    V64 = V.astype(np.float64)
    res = np.abs(AV - V64 @ Hun)
    bound = 4 * (m + 2) * u * (absAV + np.abs(V64) @ np.abs(Hun))
    assert np.all(res <= bound), float(np.max(res / bound))
    # |s(k+1)| = ||b - A x_k|| up to the basis' loss of orthogonality (measured on the restatement's own V)
    # and the n m roundings of the relation above
    loss = np.linalg.norm(V64.T @ V64 - np.eye(m + 1), 2)
    for k in range(1, m + 1):
        sk = _rot_s(P, cs, sn, k, T)  # s after k steps
        U = R.ref_update(V, H, sk, k, x0)
        rk = np.linalg.norm(b - A64 @ U["x"])
        sk1 = abs(float(sk[k]))
        assert abs(rk - sk1) <= (loss + 20 * m * n * u) * P["beta"], (k, rk, sk1)
    assert abs(float(s[m])) < 1e-2 * P["beta"]  # and it did converge


def _rot_s(P, cs, sn, k, T):
    """beta e_1 rotated k times."""
    s = np.zeros(len(cs), T)
    s[0] = T(P["beta"])
    for j in range(k):
        a1, a2 = s[j], s[j + 1]
        s[j], s[j + 1] = cs[j] * a1 + sn[j] * a2, cs[j] * a2 - sn[j] * a1
    return s


def test_givens_restates_rotg():
    """ref_givens on a zero column with identity rotations and a zero norm
    returns the correction itself (what the GPU test reads it back with)."""
    T = np.float32
    corr = R.gen_vec(5, 4, 0, T)
    one = np.zeros(6, T)
    G = R.ref_givens(4, np.zeros(6, T), corr, one + 1, one, one, 0.0, T)
    assert np.array_equal(G["col"][:5], corr) and G["col"][5] == 0


# ---------------------------------------------------------------- (b) the bounds see the defects
def drop_rows(n):
    """The last row, row 4096, the last row of a full quad."""
    return sorted({n - 1, (n & ~3) - 1} | ({4096} if n > 4096 else set()))


def moved_everywhere(ref, mut, tol, what, idx=None):
    d, tol = np.abs(np.atleast_1d(mut) - np.atleast_1d(ref)), np.atleast_1d(tol)
    if idx is not None:
        d, tol = d[idx], tol[idx]
    assert np.all(d >= 4 * tol), (what, float(np.min(d / tol)))


def moved_mostly(ref, mut, tol, what):
    frac = np.mean(np.abs(mut - ref) >= 4 * tol)
    assert frac >= 0.25, (what, float(frac))


def flat_ld_as_n(V, n):
    """The columns a reader finds that steps through the padded buffer with ld = n."""
    flat = np.asarray(V).ravel(order="F")
    return np.column_stack([flat[j * n:j * n + n] for j in range(V.shape[1])])


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("cls", CLS)
def test_dots_inputs(cls, n):
    """test_dots (and dots_sums, MGS' one column): the basis and w of R.W_SEED."""
    check_dots(cls, n)


def check_dots(cls, n):
    T, acc32 = _cls(cls)
    Vp, w = _basis(n, T), R.gen_vec(n, R.W_SEED, 5, T)
    for nc in (1, 8, 9, 32, 33, 64, 128, 129):
        dots_case(Vp[:, :nc], w, n, T, acc32, f"dots nc={nc}")


_coefs = R.gen_coefs


def _row_mutations(Vp, n, c, base, evaluate, tol, what):
    """The column mutations of a row update evaluate(V, c) whose unmutated value is base."""
    V, nc = Vp[:n], len(c)
    # k off by one: the last column's term is missing, in every row
    moved_everywhere(base, evaluate(V[:, :nc - 1], c[:nc - 1]) if nc > 1 else evaluate(V[:, :1], 0 * c), tol,
                     what + " k off by one")
    if nc > 1:
        for j in sorted({0, nc // 2 - 1 if nc > 3 else 0, nc - 2}):
            p = np.arange(nc)
            p[j], p[j + 1] = j + 1, j
            moved_mostly(base, evaluate(V[:, p], c), tol, what + f" columns {j}, {j + 1} swapped")
        moved_mostly(base, evaluate(V, np.concatenate([c[:1], c[:-1]])), tol, what + " coefficient shift")
        moved_mostly(base, evaluate(flat_ld_as_n(Vp[:, :nc], n), c), tol, what + " ld = n")


def norm2_sees_rows(w1, n, T, acc32, what, givens=False):
    """check_norm2 on the ||w'||^2 a launch emits: a row left out of the sum.
    givens: the norm also feeds a Givens step (check_givens_close): 1/h moves
    by half the row's share, against half the dot bound plus three roundings."""
    nr, na = R.ref_dots(w1[:, None], w1)
    ntol = R.tol_sum(nr, na, n, T, acc32)
    for i in drop_rows(n):
        moved_everywhere(nr, nr - float(w1[i]) ** 2, ntol, f"{what}: ||w'||^2 without row {i}")
        if givens:
            inv_tol = 0.5 * float(ntol[0] / nr[0]) + 3 * R.unit(T)
            assert 0.5 * float(w1[i]) ** 2 / nr[0] >= 4 * inv_tol, (what, "1/h without row", i)


def update_case(Vp, n, w, c, T, acc32, what, givens=False):
    """One CGS update w' = w - V c on a GPU case's inputs: tol_rows against
    every mutation, then the emitted ||w'||^2. Returns T(w')."""
    nc = len(c)
    ref, tt, scale = R.ref_cgs_update(Vp[:n, :nc], c, w)
    tol = R.tol_rows(ref, tt, scale, nc, T, acc32)
    # a dropped row keeps its old value
    moved_everywhere(ref, w.astype(np.float64), tol, f"{what}: rows dropped", idx=drop_rows(n))
    _row_mutations(Vp[:, :nc], n, c, ref, lambda V, cc: R.ref_cgs_update(V, cc, w)[0], tol, what)
    w1 = ref.astype(T)
    norm2_sees_rows(w1, n, T, acc32, what, givens)
    return w1


def dots_case(Vp, w, n, T, acc32, what, coef=True):
    """The dots <v_j, w>, j < nc = Vp.shape[1], on a GPU case's inputs: tol_sum
    (coef: plus eps_T |ref|, the form the stored coefficients are checked
    with) against every mutation. Returns the dots."""
    V, nc = Vp[:n], Vp.shape[1]
    r, a = R.ref_dots(V, w)
    tol = R.tol_sum(r, a, n, T, acc32) + (2 * R.unit(T) * np.abs(r) if coef else 0)
    for i in drop_rows(n):
        keep = np.arange(n) != i
        moved_everywhere(r, R.ref_dots(V[keep], w[keep])[0], tol, f"{what}: row {i} dropped")
    # k off by one: column k is not formed (the tests also poison the sums); no dot is zero by accident
    moved_everywhere(r, np.zeros(nc), tol, f"{what}: k off by one")
    if nc > 1:
        # columns j, j + 1 swapped, for every j: output j holds dot j + 1 and output j + 1 dot j
        moved_everywhere(r[:-1], r[1:], np.maximum(tol[:-1], tol[1:]), f"{what}: swap")
        # coefficient j from column j - 1
        moved_everywhere(r[1:], r[:-1], tol[1:], f"{what}: shift")
        moved_everywhere(r, R.ref_dots(flat_ld_as_n(Vp, n), w)[0], tol, f"{what}: ld = n", idx=np.arange(1, nc))
    return r


def _basis(n, T, ncols=130):
    return R.gen_basis(n, ld_of(n, np.dtype(T).itemsize), ncols, 11, T)


def _pbasis(w, n, T, ncols=130):
    return R.gen_basis_toward(w, n, ld_of(n, np.dtype(T).itemsize), ncols, 11, T)


def _cls(cls):
    t, accum = CLASSES[cls]
    return TT[t], accum == 1


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("cls", CLS)
def test_cgs_from_sums_inputs(cls, n):
    """test_cgs_from_sums: w seed 22, gen_coefs; the norm feeds a Givens step."""
    T, acc32 = _cls(cls)
    Vp, w = _basis(n, T), R.gen_vec(n, 22, 5, T)
    for nc in (1, 8, 9, 32, 33, 129):
        update_case(Vp, n, w, _coefs(nc).astype(T), T, acc32, f"cgs nc={nc}", givens=True)


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("cls", CLS)
def test_cgsr_inputs(cls, n):
    """test_cgsr: w seed 23; pass 0 (update, next dots), pass 1 on T(w') with the coefficients of seed 32."""
    T, acc32 = _cls(cls)
    Vp, w = _basis(n, T, 41), R.gen_vec(n, 23, 5, T)
    for nc in (9, 32, 33):
        w1 = update_case(Vp, n, w, _coefs(nc).astype(T), T, acc32, f"cgsr pass 0 nc={nc}")
        dots_case(Vp[:, :nc], w1, n, T, acc32, f"cgsr next dots nc={nc}", coef=False)
        update_case(Vp, n, w1, _coefs(nc, seed=32).astype(T), T, acc32, f"cgsr pass 1 nc={nc}", givens=True)


def check_partial_fed(cls, n):
    """test_cgs_partials and test_cgsr_wide: gen_basis_toward, w of R.W_SEED, the
    coefficients the dots themselves."""
    T, acc32 = _cls(cls)
    w = R.gen_vec(n, R.W_SEED, 5, T)
    Vp = _pbasis(w, n, T)
    for nc in (1, 4, 5, 8, 9, 10, 18, 32, 33, 128):
        c = dots_case(Vp[:, :nc], w, n, T, acc32, f"partials nc={nc}").astype(T)
        w1 = update_case(Vp, n, w, c, T, acc32, f"cgs_partials nc={nc}")
        if nc > 32:  # cgsr_wide_pass(k, 1) on w'
            c2 = dots_case(Vp[:, :nc], w1, n, T, acc32, f"wide pass 1 nc={nc}").astype(T)
            update_case(Vp, n, w1, c2, T, acc32, f"wide pass 1 nc={nc}", givens=True)


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("cls", CLS)
def test_partial_fed_inputs(cls, n):
    check_partial_fed(cls, n)


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("cls", CLS)
def test_mgs_inputs(cls, n):
    """test_mgs: mgs(k, j) from sums (h = 0.15, w seed 24) and the chain dots ->
    mgs_partials(k, 0 .. k) on gen_basis_toward, h the dots themselves."""
    T, acc32 = _cls(cls)
    w = R.gen_vec(n, R.W_SEED, 5, T)

    def step(Vp, j, last, h, cur, what):
        ref, tt, scale = R.ref_mgs_update(Vp[:n, j], h, cur)
        tol = R.tol_rows(ref, tt, scale, 1, T, acc32)
        moved_everywhere(ref, cur.astype(np.float64), tol, what + ": rows dropped", idx=drop_rows(n))
        moved_mostly(ref, R.ref_mgs_update(Vp[:n, j + 1], h, cur)[0], tol, what + ": column j + 1 for j")
        moved_mostly(ref, R.ref_mgs_update(flat_ld_as_n(Vp[:, :5], n)[:, j + 1], h, cur)[0], tol, what + ": ld = n")
        w1 = ref.astype(T)
        if last:
            norm2_sees_rows(w1, n, T, acc32, what)
            return w1, None
        nxt = Vp[:n, j + 1]
        dr, da = R.ref_dots(nxt[:, None], w1)
        dtol = R.tol_sum(dr, da, n, T, acc32) + 2 * R.unit(T) * np.abs(dr)
        for i in drop_rows(n):
            moved_everywhere(dr, dr - float(nxt[i]) * float(w1[i]), dtol, f"{what}: next partial without row {i}")
        moved_everywhere(dr, R.ref_dots(Vp[:n, j:j + 1], w1)[0], dtol, what + ": next partial on column j")
        moved_everywhere(dr, 0 * dr, dtol, what + ": next partial not formed")
        return w1, T(dr[0])

    Vp = _basis(n, T, 5)
    for k, j in ((0, 0), (3, 0), (3, 2), (3, 3)):
        step(Vp, j, j == k, T(0.15 + 1e-9), w, f"mgs({k},{j})")
    Vs = _pbasis(w, n, T, 5)
    for k in (0, 3):
        cur, h = w, T(dots_case(Vs[:, :1], w, n, T, acc32, f"mgs dots k={k}")[0])
        for j in range(k + 1):
            cur, h = step(Vs, j, j == k, h, cur, f"mgs_partials({k},{j})")


def _update_mutations(Vp, n, H, s, k, x0, T, acc32, what, extra=0.0):
    U = R.ref_update(Vp[:n], H, s, k, x0)
    tol = R.tol_update(U, k, U["x"], T, np.float64, acc32) + extra * R.unit(T) * U["absVg"]
    moved_everywhere(U["x"], x0, tol, f"{what}: rows dropped", idx=drop_rows(n))
    _row_mutations(Vp[:, :k], n, U["y"], U["x"], lambda V, yy: x0 + V.astype(np.float64) @ yy, tol, what)
    if k > 1:  # the solve taken one column short
        moved_everywhere(U["x"], R.ref_update(Vp[:n], H, s, k - 1, x0)["x"], tol, f"{what}: solve with k - 1")


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("cls", CLS)
def test_update_inputs(cls, n):
    """test_update (tol_update) and test_update_tail: cgs(m - 1, 0) on w seed
    29, the Givens step on its norm, the solve on the rotated column and s."""
    T, acc32 = _cls(cls)
    Vp = _basis(n, T)
    x0, s = R.gen_vec(n, 43, 3, np.float64), R.gen_vec(131, 42, 0, T)
    for k in (1, 8, 32, 33, 64, 65, 127, 128, 130):
        _update_mutations(Vp, n, R.gen_upper(130, k, 41, T), s, k, x0, T, acc32, f"update k={k}")
    for m in (1, 9, 32):
        k = m - 1
        c = _coefs(m).astype(T)
        w1 = update_case(Vp, n, R.gen_vec(n, 29, 5, T), c, T, acc32, f"tail m={m}: cgs", givens=True)
        cs, sn, _ = R.gen_rotations(m, 9, T)
        sm = R.gen_vec(m + 1, 42, 0, T)
        G = R.ref_givens(k, np.concatenate([c, [0]]).astype(T), None, cs, sn, sm, R.ref_dots(w1[:, None], w1)[0][0], T)
        H = R.gen_upper(m, m, 41, T)
        H[:m + 1, k] = G["col"]
        sm[k] = G["s"][0]
        _update_mutations(Vp, n, H, sm, m, x0, T, acc32, f"update_tail m={m}", extra=32)


@pytest.mark.parametrize("cls", ["f32-acc64", "f32-acc32"])
def test_basis16_inputs(cls):
    """test_basis16: gen_basis_toward as 2^-14 float(fp16 bits), n = 4099 (csr) and 8197 (sell-pair)."""
    from tests.basis16_np import round_f16

    T, acc32 = _cls(cls)
    for n in (4099, 8197):
        ld = (n + 127) // 128 * 128
        w = R.gen_vec(n, R.W_SEED, 5, T)
        Vp = round_f16(R.gen_basis_toward(w, n, ld, 13, 11, T))
        c = dots_case(Vp[:, :9], w, n, T, acc32, "f16 dots").astype(T)
        update_case(Vp, n, w, c, T, acc32, "f16 cgs_partials")
        _update_mutations(Vp, n, R.gen_upper(12, 9, 41, T), R.gen_vec(13, 42, 0, T), 9, R.gen_vec(n, 43, 3, np.float64),
                          T, acc32, "f16 update")


def _padded(cols, n, ld, T):
    Vp = np.full((ld, len(cols)), 3.0, T, order="F")
    for j, c in enumerate(cols):
        Vp[:n, j] = c
    return Vp


def check_fused_dots(mpg, name, cls, ks, seed, folds):
    """test_spmv_dots / test_step_dots: the dots of [V(:, :k), v_k] with w =
    T(A v_k); fold 2: w_prev is cgs(k - 1, 0)'s w' and 1/h its Givens step's."""
    T, acc32 = _cls(cls)
    A = MATRICES[name](mpg)
    n, A64 = A.nrows, R.csr64(A, T)
    Vp = _basis(n, T, 33)
    cs, sn, s = R.gen_rotations(32, 9, T)
    for k in ks:
        for fold in folds:
            if fold and k == 0:
                continue
            w_prev, inv = R.gen_vec(n, seed, 5, T), T(0.37)
            if fold:
                c = _coefs(k).astype(T)
                w_prev = update_case(Vp, n, w_prev, c, T, acc32, f"fold: cgs({k - 1})", givens=True)
                inv = R.ref_givens(k - 1, np.concatenate([c, [0]]).astype(T), None, cs, sn, s,
                                   R.ref_dots(w_prev[:, None], w_prev)[0][0], T)["inv"]
            v, w64, _ = R.ref_spmv_step(A64, w_prev, inv)
            cols = [Vp[:n, j] for j in range(k)] + [v]
            dots_case(_padded(cols, n, Vp.shape[0], T), w64.astype(T), n, T, acc32,
                      f"fused dots {name} k={k} fold={fold}", coef=False)


@pytest.mark.parametrize("name", ["band260", "band4099", "band4100", "band8197"])
def test_spmv_dots_inputs(mpg, name):
    check_fused_dots(mpg, name, "f32-acc64", (0, 1, 8, 16, 31), 27, (0,))


@pytest.mark.parametrize("name", ["band260", "band4100", "band8196"])
def test_step_dots_inputs(mpg, name):
    check_fused_dots(mpg, name, "f32-acc32", (0, 1, 8, 31), 28, (0, 2))


@pytest.mark.parametrize("storage", ["csr", "sell-pair", "sell-single", "sell-ragged", "node"])
@pytest.mark.parametrize("cls", CLS)
def test_spmv_fold_inputs(mpg, cls, storage):
    """test_spmv_fold: the ||w'||^2 of cgs(0, 0) on w seed 26 feeds the folded Givens step."""
    T, acc32 = _cls(cls)
    n = MATRICES[{"csr": "band4099", "sell-ragged": "band4099", "node": "stencil5"}.get(storage, "band8197")](mpg).nrows
    update_case(_basis(n, T, 7), n, R.gen_vec(n, 26, 5, T), _coefs(1).astype(T), T, acc32, "fold: cgs(0)", givens=True)


@pytest.mark.parametrize("jacobi", [0, 1])
@pytest.mark.parametrize("name", ["band4099", "band8197", "stencil5"])
@pytest.mark.parametrize("t", ["f32", "f64"])
def test_prologue_inputs(mpg, t, name, jacobi):
    """test_prologue's norms: a row left out of ||T(r)||^2, ||w0||^2 or ||x||^2
    moves the norm by half its share, against the bounds the test uses."""
    T = TT[t]
    A = MATRICES[name](mpg)
    n, u = A.nrows, R.unit(T)
    x, b = R.gen_vec(n, 51, 2, np.float64), R.gen_vec(n, 52, 4, np.float64)
    A64 = R.csr64(A, np.float64)
    d = (1.0 / A64.diagonal()).astype(T) if jacobi else None
    P = R.ref_prologue(A64, b, x, T, d)
    sumtol = (n + 2) * 2.0 ** -53
    dr = 2 * (P["nnz_row"] + 2) * 2.0 ** -53 * P["scale"]
    tr = P["r"].astype(T).astype(np.float64)
    w0 = P["w0"].astype(np.float64)
    rn_tol = (sumtol + 3 * u) + float(np.linalg.norm(dr)) / P["r_norm"] if jacobi else sumtol + u
    for vec, rel, what in ((tr, rn_tol, "r_norm"), (w0, sumtol + u, "beta"), (x, sumtol + 2.0 ** -53, "x_norm")):
        tot = float((vec ** 2).sum())
        for i in drop_rows(n):
            assert 0.5 * vec[i] ** 2 / tot >= 4 * rel, (what, i, 0.5 * vec[i] ** 2 / tot / rel)
    # w0 itself: a dropped row keeps the poison the test stores there first (not a matter of the bound)


@pytest.mark.parametrize("t", ["f32", "f64"])
def test_givens_tolerance_sees_defects(t):
    """check_givens_close's 8 eps_T: a rotation skipped, the rotations applied
    in the other order, or cs and sn exchanged move the rotated column by more
    than 4 x the bound. (A row missing from the ||w||^2 that feeds the step:
    norm2_sees_rows, on each case's own w'.)"""
    T = TT[t]
    eps = 2 * R.unit(T)
    cs, sn, s = R.gen_rotations(40, 5, T)
    for nc in (9, 32, 33):
        k = nc - 1
        col = np.concatenate([_coefs(nc), [0]]).astype(T)
        nrm = 0.8 * 4099.0
        G = R.ref_givens(k, col, None, cs, sn, s, nrm, T)
        cscale = float(np.max(np.abs(G["col"].astype(np.float64))) + float(G["hn"]))
        tol = 8 * eps * cscale
        for name, (c2, s2) in {"cs / sn exchanged": (sn, cs), "rotations shifted": (np.roll(cs, 1), np.roll(sn, 1))}.items():
            M = R.ref_givens(k, col, None, c2, s2, s, nrm, T)
            assert np.max(np.abs(M["col"].astype(np.float64) - G["col"])) >= 4 * tol, name
        M = R.ref_givens(k - 1, col, None, cs, sn, s, nrm, T)
        assert abs(float(M["col"][k - 1]) - float(G["col"][k - 1])) >= 4 * tol, "k off by one"


# ---------------------------------------------------------------- (c) the storage variants
# tests/test_arnoldi_variants_gpu.py: the generators give what the GPU cases rely on, and the SpMV bound
# (R.tol_spmv, R.tol_node_bj, R.tol_prologue_w0) sees the defects of each variant's own address arithmetic.
# A mutation reaches the rows whose operands it changes; at least a quarter of them must move by 4 bounds
# (a defect confined to one slice: a quarter of the rows it reaches there).
def test_front_pad_restates_the_header():
    """front_pad against MPG_FRONT_PAD as include/mpgmres/arnoldi.h defines it (the macro's text, evaluated)."""
    text = (Path(__file__).resolve().parent.parent / "include/mpgmres/arnoldi.h").read_text()
    m = re.search(r"#define MPG_FRONT_PAD\(n_front\) \((.*)\)\n", text)
    cond, yes, no = re.fullmatch(r"(.*) \? (.*) : (.*)", m.group(1)).groups()
    expr = f"({yes.replace('/', '//')}) if ({cond}) else ({no})"
    for nf in (0, 1, 5, 63, 64, 65, 108, 128, 1000):
        assert front_pad(nf) == eval(expr, {"n_front": nf}), (nf, expr)
    assert front_pad(5) == 128 and front_pad(108) == 192  # the GPU cases' pads


def sell_span(A):
    """k_sell_span (csrc/sell.hip): min and max of col - (first row of the row's slice)."""
    r = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    d = A.col.astype(np.int64) - (r & ~63)
    return int(d.min()), int(d.max())


def sell_bases(A):
    """k_sell_classify: per (slice, entry index k) the min and max of col - row over the slice's rows that
    have an entry k, base = floor((lo + hi) / 2); a slice is CSR-summed (stepped form) when some hi - base or
    base - lo exceeds 32767. Returns (lo, hi, base, present, bad slices)."""
    n = A.nrows
    r = np.repeat(np.arange(n), np.diff(A.rowptr))
    k = np.arange(A.nnz) - A.rowptr[r]
    s, ns, width = r // 64, -(-n // 64), int(np.diff(A.rowptr).max())
    d = A.col.astype(np.int64) - r
    lo = np.full((ns, width), np.iinfo(np.int64).max)
    hi = np.full((ns, width), np.iinfo(np.int64).min)
    np.minimum.at(lo, (s, k), d)
    np.maximum.at(hi, (s, k), d)
    present = hi >= lo
    base = np.where(present, (np.where(present, lo, 0) + np.where(present, hi, 0)) >> 1, 0)
    bad = np.flatnonzero(np.any(present & ((hi - base > 32767) | (lo - base < -32767)), axis=1))
    return lo, hi, base, present, bad


def test_far_matrices_reach_the_stepped_form(mpg):
    A = MATRICES["far33k"](mpg)
    lo, hi = sell_span(A)
    assert A.nrows == 33_280 and (lo < -32767 or hi > 32767), (lo, hi)
    assert len(sell_bases(A)[4]) == 0
    B = MATRICES["far66k"](mpg)
    lo, hi = sell_span(B)
    ns = -(-B.nrows // 64)
    assert B.nrows == 66_048 and ns == 1032 and (lo < -32767 or hi > 32767)
    bad = sell_bases(B)[4]
    assert bad.tolist() == [FAR66_ROW // 64] and len(bad) * 100 <= ns
    # element 0 of the two rows: r - 33,000 and r + 33,000
    for row, off in ((FAR66_ROW, -33_000), (FAR66_ROW + 1, 33_000)):
        assert B.col[B.rowptr[row]] - row == off
    assert B.rowptr[FAR66_ROW + 2] - B.rowptr[FAR66_ROW + 1] == 1


def test_halo_plan_of_the_band(mpg):
    """band-ranks' three row blocks: the halo a rank needs is the band's reach below (n_front) and above
    (n_ext - n) its rows, read from the matrix' own offsets."""
    A = MATRICES["band-ranks"](mpg)
    off = A.col.astype(np.int64) - np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    below, above = int(-off.min()), int(off.max())
    assert (below, above) == (5, 4)  # gen_band(n, 5, 4): five sub-diagonals, four super-diagonals
    want = [(0, 4099 + above), (below, 4099 + above), (below, 4099)]
    for rank in range(3):
        B = RankBlock(mpg, A, RANK_SPLITS["band-ranks"], rank)
        assert (B.n_front, B.n_ext) == want[rank], (rank, B.n_front, B.n_ext)
        assert B.A.col.min() == -B.n_front and B.A.col.max() == B.n_ext - 1
        # the local numbering keeps the band: local col - local row = global col - global row
        lrow = np.repeat(np.arange(B.n), np.diff(B.A.rowptr))
        assert np.array_equal(B.glob[B.A.col + B.n_front] - B.glob[lrow + B.n_front], B.A.col - lrow)
    S = MATRICES["stencil-ranks"](mpg)
    for rank, (nf, ne) in enumerate([(0, 324 + 108), (108, 324)]):  # one plane of 36 nodes, 3 dof each
        B = RankBlock(mpg, S, RANK_SPLITS["stencil-ranks"], rank)
        assert (B.n_front, B.n_ext) == (nf, ne)


HALF_MATRICES = {"band-stiff": 1, "band-stiff8197": 1, "band4099": 0, "band8197": 0, "stencil5": 1}


@pytest.mark.parametrize("name", sorted(HALF_MATRICES))
def test_half_values_rule(mpg, name):
    A = MATRICES[name](mpg)
    scale = HALF_MATRICES[name]
    bits, e, M = R.half_values(A, scale)
    h = bits.view(np.float16)
    assert np.all(np.isfinite(h)) and not np.any((h == 0) & (A.val != 0)), "an entry rounds to 0 or Inf"
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    rmax = np.maximum.reduceat(np.abs(h.astype(np.float64)), A.rowptr[:-1])
    assert np.all((rmax >= 2.0 ** -2) & (rmax <= 2.0 ** 15))  # (a maximum just under 2^15 may round up to it)
    # the copy is within fp16's rounding of A, entry by entry (normal range), whatever the row's scale
    big = np.abs(np.ldexp(A.val, e[rows])) >= 2.0 ** -14
    assert np.all(np.abs(M.data - A.val)[big] <= 2.0 ** -11 * (1 + 2.0 ** -20) * np.abs(A.val)[big])
    if name.startswith("band-stiff"):
        sl = np.arange(A.nrows) // 64
        both = [s for s in range(sl.max() + 1) if np.any(e[sl == s] > 0) and np.any(e[sl == s] < 0)
                and np.any(e[sl == s] == 0)]
        assert len(both) > 0 and np.count_nonzero(e) > A.nrows // 7
    else:
        assert not e.any()


def moved_fraction(ref, mut, tol, reached, what, everywhere=False):
    """At least a quarter (everywhere: all) of the rows the mutation reaches move by 4 bounds; a row that
    turns Inf or NaN has moved."""
    reached = np.flatnonzero(reached) if np.asarray(reached).dtype == bool else np.asarray(reached)
    assert len(reached) > 0, (what, "reaches no row")
    with np.errstate(invalid="ignore"):
        moved = ~(np.abs(mut[reached] - ref[reached]) < 4 * tol[reached])
    frac = float(np.mean(moved))
    assert frac >= (1.0 if everywhere else 0.25), (what, frac, len(reached))


def _rows_of(M, cols_mask):
    """Rows of M with an entry in a masked column."""
    return np.flatnonzero(np.diff(M.indptr) > 0) if cols_mask is None else \
        np.unique(np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))[cols_mask[M.indices]])


def _recol(M, newcol):
    """M with its column indices replaced (clipped into range; duplicates are summed, as a kernel would)."""
    return sp.csr_matrix((M.data.copy(), np.clip(newcol, 0, M.shape[1] - 1), M.indptr.copy()), shape=M.shape)


def _spmv_and_prologue(M64, Mo64, w_ext, x_ext, b, T, acc32, n_front):
    """The two row-sum launches of a variant on a GPU case's inputs: evaluate(M, Mo, w, x) -> [(w, tol), (w0, tol)]."""
    terms = int(np.diff(M64.indptr).max())

    def evaluate(M, Mo, w, x):
        _, ref, scale = R.ref_spmv_step(M, w, T(0.37), None, n_front)
        P = R.ref_prologue(Mo, b, x, T, None, n_front)
        return [(ref, R.tol_spmv(ref, scale, terms, T, acc32)), (P["w0"].astype(np.float64), R.tol_prologue_w0(P, T))]

    return evaluate


HALO_BLOCKS = [("band-ranks", 0), ("band-ranks", 1), ("band-ranks", 2), ("stencil-ranks", 0), ("stencil-ranks", 1)]


@pytest.mark.parametrize("name,rank", HALO_BLOCKS)
@pytest.mark.parametrize("cls", CLS)
def test_halo_inputs(mpg, cls, name, rank):
    """test_halo's SpMV (w_prev seed 25) and prologue (x seed 51, b seed 52): the local column index off by
    one either way (a wrong front offset), the upper halo read as zero, the lower halo taken from the upper."""
    T, acc32 = _cls(cls)
    A = MATRICES[name](mpg)
    B = RankBlock(mpg, A, RANK_SPLITS[name], rank)
    n, nf, N = B.n, B.n_front, A.nrows
    M64 = B.to_scipy()
    Mo = M64.copy()
    M64.data = M64.data.astype(T).astype(np.float64)
    w = R.gen_vec(N, 25, 5, T)[B.glob]
    x, b = R.gen_vec(N, 51, 2, np.float64)[B.glob], R.gen_vec(N, 52, 4, np.float64)[B.own]
    ev = _spmv_and_prologue(M64, Mo, w, x, b, T, acc32, nf)
    base = ev(M64, Mo, w, x)
    allrows = np.arange(n)
    for sh in (1, -1):
        mut = ev(_recol(M64, M64.indices + sh), _recol(Mo, Mo.indices + sh), w, x)
        for (r0, tol), (r1, _), what in zip(base, mut, ("spmv", "prologue")):
            moved_fraction(r0, r1, tol, allrows, f"{what}: columns shifted by {sh}")
    cols = np.arange(nf + B.n_ext)
    if B.n_ext > n:
        up = cols >= nf + n
        wz, xz = np.where(up, 0, w).astype(T), np.where(up, 0, x)
        for (r0, tol), (r1, _), what in zip(base, ev(M64, Mo, wz, xz), ("spmv", "prologue")):
            moved_fraction(r0, r1, tol, _rows_of(M64, up), f"{what}: upper halo read as zero")
    if nf and B.n_ext > n:
        lo = cols < nf
        src = nf + n + np.arange(nf) % (B.n_ext - n)
        wl, xl = w.copy(), x.copy()
        wl[:nf], xl[:nf] = w[src], x[src]
        for (r0, tol), (r1, _), what in zip(base, ev(M64, Mo, wl, xl), ("spmv", "prologue")):
            moved_fraction(r0, r1, tol, _rows_of(M64, lo), f"{what}: lower halo taken from the upper")
    # x_norm over the halo as well would count rows twice across the ranks: the bound sees it
    xn = float(np.sqrt((x[nf:nf + n] ** 2).sum()))
    if B.n_ext > n or nf:
        assert abs(float(np.sqrt((x ** 2).sum())) - xn) >= 4 * ((n + 2) * 2.0 ** -53 + 2.0 ** -53) * xn


HALF_CASES = [("band-stiff", None), ("band-stiff8197", None), ("band-stiff-ranks", 1)]


@pytest.mark.parametrize("name,rank", HALF_CASES)
@pytest.mark.parametrize("acc32", [False, True])
def test_half_inputs(mpg, acc32, name, rank):
    """test_half_values / test_half_values_halo on scaled rows: e_i ignored, e_i of the neighbouring row,
    and the fp16 values read as the unscaled cast (which overflows the rows scaled down, and loses the small
    entries of the rows scaled up to fp16's subnormal range)."""
    T = np.float32
    A = MATRICES[name](mpg)
    N, nf = A.nrows, 0
    glob = np.arange(N)
    if rank is not None:
        B = RankBlock(mpg, A, RANK_SPLITS[name], rank)
        A, nf, glob = B.A, B.n_front, B.glob
    bits, e, M = R.half_values(A, 1, nf)
    terms = int(np.diff(M.indptr).max())
    w = R.gen_vec(N, 25, 5, T)[glob]
    _, ref, scale = R.ref_spmv_step(M, w, T(0.37), None, nf)
    tol = R.tol_spmv(ref, scale, terms, T, acc32)
    moved_fraction(ref, np.ldexp(ref, e), tol, e != 0, "e_i ignored", everywhere=True)
    for sh in (1, -1):
        en = np.roll(e, sh)
        moved_fraction(ref, np.ldexp(ref, e - en), tol, e != en, f"e_i of row i {-sh:+d}", everywhere=True)
    with np.errstate(over="ignore"):
        plain = A.val.astype(np.float32).astype(np.float16).astype(np.float64)
    Mp = sp.csr_matrix((plain, M.indices.copy(), M.indptr.copy()), shape=M.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        _, mut, _ = R.ref_spmv_step(Mp, w, T(0.37), None, nf)
    reached = np.flatnonzero(np.add.reduceat((Mp.data != M.data).astype(np.int64), M.indptr[:-1]) > 0)
    assert set(np.flatnonzero(e < 0)) <= set(reached)  # every row scaled down overflows
    moved_fraction(ref, mut, tol, reached, "the unscaled cast")


@pytest.mark.parametrize("name", ["far33k", "far66k"])
@pytest.mark.parametrize("cls", CLS)
def test_stepped_inputs(mpg, cls, name):
    """test_stepped's SpMV and prologue: a stepped column is row + base(slice, k) + int16 offset. The base of
    entry k taken from entry k - 1 or k + 1 of the slice; the CSR-summed slice decoded from its offsets
    wrapped to int16 (reaches the two rows whose offsets leave int16: both move); that slice skipped."""
    T, acc32 = _cls(cls)
    A = MATRICES[name](mpg)
    n = A.nrows
    M64, Mo = R.csr64(A, T), R.csr64(A, np.float64)
    w = R.gen_vec(n, 25, 5, T)
    x, b = R.gen_vec(n, 51, 2, np.float64), R.gen_vec(n, 52, 4, np.float64)
    ev = _spmv_and_prologue(M64, Mo, w, x, b, T, acc32, 0)
    base0 = ev(M64, Mo, w, x)
    lo, hi, base, present, bad = sell_bases(A)
    r = np.repeat(np.arange(n), np.diff(A.rowptr))
    k = np.arange(A.nnz) - A.rowptr[r]
    s = r // 64
    col = A.col.astype(np.int64)
    for sh in (1, -1):
        kk = np.clip(k + sh, 0, base.shape[1] - 1)
        other = np.where(present[s, kk], base[s, kk], base[s, k])  # (no neighbouring element: its own base)
        newcol = col - base[s, k] + other
        reached = np.unique(r[np.clip(newcol, 0, n - 1) != col])
        assert len(reached) > n // 2
        mut = ev(_recol(M64, newcol), _recol(Mo, newcol), w, x)
        for (r0, tol), (r1, _), what in zip(base0, mut, ("spmv", "prologue")):
            moved_fraction(r0, r1, tol, reached, f"{what}: base of element k {sh:+d}")
    if name == "far66k":
        sb = int(bad[0])
        off = col - r - base[s, k]
        wrapped = (off + 32768) % 65536 - 32768
        newcol = np.where(s == sb, r + base[s, k] + wrapped, col)
        reached = np.unique(r[newcol != col])
        assert reached.tolist() == [FAR66_ROW, FAR66_ROW + 1]
        mut = ev(_recol(M64, newcol), _recol(Mo, newcol), w, x)
        for (r0, tol), (r1, _), what in zip(base0, mut, ("spmv", "prologue")):
            moved_fraction(r0, r1, tol, reached, f"{what}: wrapped offsets", everywhere=True)
        rows = np.arange(64 * sb, 64 * sb + 64)
        for (r0, tol), what in zip(base0, ("spmv", "prologue")):  # (the GPU test also stores NaN there first)
            moved_fraction(r0, np.zeros(n), tol, rows, f"{what}: slice skipped", everywhere=True)


@pytest.mark.parametrize("name", ["stencil5", "stencil5-rows"])
@pytest.mark.parametrize("cls", CLS)
def test_block_jacobi_inputs(mpg, cls, name):
    """test_block_jacobi_node: the inverses not applied, those of the neighbouring block, and the 3 x 3
    inverses transposed. stencil5's diagonal blocks are symmetric, and so are their inverses up to the
    set-up's rounding: a transposed read is no defect there, and no bound can see it. stencil5-rows (each
    row scaled by its own factor) has unsymmetric blocks: the transposition is asserted there."""
    from tests.test_bjacobi_gpu import np_block_inverse

    T, acc32 = _cls(cls)
    A = MATRICES[name](mpg)
    n = A.nrows
    A64 = R.csr64(A, T)
    dinv, badb = np_block_inverse(A, 3, T)
    assert not badb.any()
    w = R.gen_vec(n, 25, 5, T)
    Rj = R.ref_node_bj(A64, w, T(0.37), dinv)
    tol = R.tol_node_bj(Rj, int(np.diff(A64.indptr).max()), T, T, acc32)
    D = dinv.reshape(-1, 3, 3)
    plain = A64 @ Rj["v"].astype(np.float64)
    moved_fraction(Rj["w"], plain, tol, np.arange(n), "inverses not applied")
    muts = [("block + 1", np.roll(D, -1, axis=0)), ("block - 1", np.roll(D, 1, axis=0))]
    if name == "stencil5":
        assert np.all(np.abs(D - D.transpose(0, 2, 1)) <= 4 * R.unit(T) * np.abs(D).max(axis=(1, 2), keepdims=True))
    else:
        muts.append(("transposed", D.transpose(0, 2, 1)))
    for what, Dm in muts:
        mut = R.ref_node_bj(A64, w, T(0.37), np.ascontiguousarray(Dm).reshape(-1))["w"]
        moved_fraction(Rj["w"], mut, tol, np.arange(n), f"block Jacobi: {what}")
