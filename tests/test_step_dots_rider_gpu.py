"""The folded Givens step of k_step_dots on a workgroup of its own (the rider).

With the fold, the SpMV + dots launch has one workgroup more than the dots'
grid: the last block index runs Givens step k - 1 beside the others' SpMV
phase and stores no partials. Every case here is BAND (gen_band(n, 5, 4,
seed=7)), tol = 0, MPG_FOLD_GIVENS=1, and compares MPG_STEP_DOTS=2 (required)
against =0 (split launches, workgroup 0's fold) with array_equal; the layout
says which form ran. The sizes place the rider: beside one mostly dead
workgroup (Gd = 1), one full workgroup, a last real workgroup of one row
group, the largest grid with a free CU (Gd = 255) and the full grid (Gd = 256),
where the rider is the 257th workgroup and starts behind a retiring one.
"""
import pytest

from tests.test_step_dots_gpu import _run, _same

pytestmark = pytest.mark.gpu


def _compare(mpg, monkeypatch, n, cycles, fused, step_dots=2, **opts):
    monkeypatch.setenv("MPG_FOLD_GIVENS", "1")
    opts.setdefault("spmv_format", "sell")  # (auto leaves the smallest to CSR)
    ref, lay0 = _run(mpg, monkeypatch, n, 0, cycles=cycles, want_fused=0, **opts)
    got, lay = _run(mpg, monkeypatch, n, step_dots, cycles=cycles, want_fused=fused, **opts)
    assert lay["givens_rider"] is True and lay["dots_fused"] == fused, lay
    assert lay["givens_folded"] and lay0["givens_folded"] and "givens_rider" not in lay0, (lay, lay0)
    assert got.total_iters == ref.total_iters == cycles * opts["rlen"]
    _same(got, ref, (n, opts))


@pytest.mark.parametrize("prec", ["identity", "jacobi"])
@pytest.mark.parametrize("rlen", [30, 32])
@pytest.mark.parametrize("n", [64, 4096, 4100])
def test_rider_same_bits_small(mpg, monkeypatch, n, rlen, prec):
    """Two cycles; rlen 32 runs the rotation chain up to k = 31."""
    _compare(mpg, monkeypatch, n, 2, rlen, rlen=rlen, prec=prec)


@pytest.mark.parametrize("prec", ["identity", "jacobi"])
@pytest.mark.parametrize("n", [255 * 4096, 256 * 4096])
def test_rider_same_bits_full_grid(mpg, monkeypatch, n, prec):
    """Gd = 255 (the rider takes a free CU) and Gd = 256 (it waits for one): one cycle of rlen 30."""
    _compare(mpg, monkeypatch, n, 1, 30, rlen=30, prec=prec)


def test_rider_under_restart_100(mpg, monkeypatch):
    """GMRES(100), CGS: the steps with k + 1 <= 32 take the launch under the m <= 128 fold,
    with the split kernels' fold after them. (MPG_STEP_DOTS=1: =2 refuses a cycle with steps
    past 32 columns, tests/test_step_dots_gpu.py; dots_fused == 32 shows the launch ran.)"""
    _compare(mpg, monkeypatch, 4100, 2, 32, step_dots=1, rlen=100, orth="cgs")
