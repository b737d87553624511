"""k_step_dots at the boundaries of its waves (mpg_arnoldi_step_dots;
MPG_STEP_DOTS).

A wave of the one launch owns four SELL-64 slices, 256 rows: it forms
||w||^2 and the scale itself, fills its own window of v_k (its rows and 64 on
either side, which the neighbouring wave or workgroup owns), and hands its
rows of w and v_k to its own lanes' panel dots. The shapes here put a wave
boundary, a workgroup boundary and a partly live wave where those steps could
go wrong; as in tests/test_step_dots_gpu.py every case runs two restart cycles
of BAND (gen_band(n, 5, 4, seed=7)) at tol = 0 and compares MPG_STEP_DOTS=2
with =0 by array_equal.
"""
import numpy as np
import pytest

from tests.test_step_dots_gpu import _run, _same

pytestmark = pytest.mark.gpu


# 64: one slice, 15 dead waves; 256: exactly one live wave; 260: a second wave
# with one row group, whose window's low side is the first wave's rows; 508: a
# wave whose last slice is partly live; 4352 = 4096 + 256: a second workgroup
# with one full wave, whose window crosses the workgroup boundary; 8196: two
# full workgroups plus one row group
@pytest.mark.parametrize("fold", ["0", "1"])
@pytest.mark.parametrize("prec", ["identity", "jacobi"])
@pytest.mark.parametrize("rlen", [30, 32])
@pytest.mark.parametrize("n", [64, 256, 260, 508, 4352, 8196])
def test_same_bits_as_split_at_wave_boundaries(mpg, monkeypatch, n, rlen, prec, fold):
    """x, the per-step residuals, the cycles' true residuals and the final
    residual of the one-launch steps are those of the split launches, and
    every step of the cycle took the one launch."""
    monkeypatch.setenv("MPG_FOLD_GIVENS", fold)
    opts = dict(mode="mixed", prec=prec, rlen=rlen, spmv_format="sell")
    ref, lay0 = _run(mpg, monkeypatch, n, 0, want_fused=0, **opts)
    got, lay = _run(mpg, monkeypatch, n, 2, want_fused=rlen, **opts)
    assert lay["dots_fused"] == rlen and "dots_fused" not in lay0
    assert lay["accum"] == "f32" and lay["givens_folded"] == (fold == "1")
    assert ref.total_iters == 2 * rlen and got.total_iters == 2 * rlen
    _same(got, ref, (n, rlen, prec, fold))


EDGE_OFFSETS = (-64, -33, -7, -1, 0, 1, 9, 30, 47, 63)


def _edge_matrix(mpg, n, seed=11):
    """10 entries per row at EDGE_OFFSETS (dropped where they leave the
    matrix): the first and the last entry of every slice's window are read.
    Seeded values, a dominant diagonal."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n, dtype=np.int64), len(EDGE_OFFSETS))
    cols = rows + np.tile(np.asarray(EDGE_OFFSETS, dtype=np.int64), n)
    vals = rng.uniform(-1.0, 1.0, rows.size)
    vals[cols == rows] = 12.0 + rng.uniform(0.0, 1.0, n)
    keep = (cols >= 0) & (cols < n)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    rowptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return mpg.Csr(n, n, rowptr, cols.astype(np.int32), np.ascontiguousarray(vals, dtype=np.float64))


def _run_csr(mpg, monkeypatch, A, xt, b, step_dots, rlen, fold, cycles=2):
    monkeypatch.setenv("MPG_STEP_DOTS", str(step_dots))
    monkeypatch.setenv("MPG_FOLD_GIVENS", fold)
    eng = mpg.Engine(A, b, xt, mode="mixed", orth="cgs", prec="identity", rlen=rlen, tol=0.0, max_restarts=cycles,
                     accum="f32", spmv_format="sell")
    try:
        lay = eng.spmv_layout()
        eng.run(cycles)
        eng.sync()
        return eng.report(), lay
    finally:
        eng.close()


@pytest.mark.parametrize("fold", ["0", "1"])
@pytest.mark.parametrize("rlen", [30, 32])
def test_entries_at_the_windows_edges(mpg, monkeypatch, rlen, fold):
    """A matrix whose rows reach 64 below and 63 above the diagonal, n = 4352
    (a second workgroup of one wave): its storage takes the window form and
    every step the one launch, with the bits of the split launches."""
    n = 4352
    A = _edge_matrix(mpg, n)
    xt = mpg.rand_vect(n, 42)
    b = mpg.host_spmv(A, xt)
    ref, lay0 = _run_csr(mpg, monkeypatch, A, xt, b, 0, rlen, fold)
    got, lay = _run_csr(mpg, monkeypatch, A, xt, b, 2, rlen, fold)
    assert lay["format"] == "sell" and lay["window"], lay
    assert lay.get("dots_fused", 0) == rlen and "dots_fused" not in lay0, (lay, lay0)
    assert ref.total_iters == 2 * rlen and got.total_iters == 2 * rlen
    _same(got, ref, ("edges", rlen, fold))
