"""The streaming form of the in-launch-sum CGS update
(k_cgs_update_nc<..., STREAM>; MPG_CGS_PREFETCH).

Every lane requests its row quad of w and of up to 9 basis columns right
behind the coefficient partials, the columns into a ring of LDS slots that is
refilled as it is consumed, and adds the products in the plain form's order.
Every case runs two restart cycles at tol = 0 in mixed mode with accum="f32"
and compares MPG_CGS_PREFETCH=1 (the streaming form wherever it is built)
with =0 (the plain product form) by array_equal on x, the per-step residuals
and the cycles' true residuals: a lane reading a neighbour's slot, or a slot's
previous column, would still give finite numbers, so nothing weaker would see
it. The basis differs per column and per row in every solve here.
"""
import numpy as np
import pytest

from tests.test_step_dots_gpu import _same

pytestmark = pytest.mark.gpu

RING = 9  # kStreamSlots (csrc/lds_ring.hpp)
_PROBLEMS = {}


def _problem(mpg, key):
    if key not in _PROBLEMS:
        A = mpg.gen_laplace3d(12) if key == "lap12" else mpg.gen_band(key, 5, 4, seed=7)
        xt = mpg.rand_vect(A.nrows, 42)
        _PROBLEMS[key] = (A, xt, mpg.host_spmv(A, xt))
    return _PROBLEMS[key]


def _run(mpg, monkeypatch, key, prefetch, step_dots=None, keep=True, **opts):
    """Two restart cycles under MPG_CGS_PREFETCH=prefetch: (report, spmv_layout)."""
    A, xt, b = _problem(mpg, key)
    if not keep:
        del _PROBLEMS[key]
    monkeypatch.setenv("MPG_CGS_PREFETCH", prefetch)
    if step_dots is None:
        monkeypatch.delenv("MPG_STEP_DOTS", raising=False)
    else:
        monkeypatch.setenv("MPG_STEP_DOTS", step_dots)
    kw = dict(mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=2, accum="f32")
    kw.update(opts)
    eng = mpg.Engine(A, b, xt, **kw)
    try:
        lay = eng.spmv_layout()
        eng.run(2)
        eng.sync()
        return eng.report(), lay
    finally:
        eng.close()


def _check(mpg, monkeypatch, key, step_dots=None, **opts):
    rlen = opts.get("rlen", 30)
    ref, lay0 = _run(mpg, monkeypatch, key, "0", step_dots, **opts)
    got, lay = _run(mpg, monkeypatch, key, "1", step_dots, **opts)
    assert "cgs_stream" not in lay0 and lay["cgs_stream"] == rlen, (lay0, lay)
    assert ref.total_iters == got.total_iters == 2 * rlen
    _same(got, ref, (key, step_dots, opts))


# 64: one live wave, 960 lanes whose clamped requests contribute nothing;
# 4096: one full workgroup; 4100: a second workgroup with one live lane;
# 8196: two full workgroups plus one row group
@pytest.mark.parametrize("n", [64, 4096, 4100, 8196])
def test_same_bits_as_plain(mpg, monkeypatch, n):
    _check(mpg, monkeypatch, n)


@pytest.mark.parametrize("n", [4099, 8197])
def test_tail_rows(mpg, monkeypatch, n):
    """n % 4 != 0 (k_step_dots needs n % 4 = 0: split launches): the update's tail loop."""
    _check(mpg, monkeypatch, n, step_dots="0")


def test_split_launches_on_another_storage(mpg, monkeypatch):
    _check(mpg, monkeypatch, "lap12")


def test_second_grid_stride_iteration(mpg, monkeypatch):
    """n = 4096 * 256 + 4096 + 8: the first workgroup's lanes own a second row
    group, which the ring does not cover (the plain path after the stream)."""
    n = 4096 * 256 + 4096 + 8
    ref, lay0 = _run(mpg, monkeypatch, n, "0", "0")
    got, lay = _run(mpg, monkeypatch, n, "1", "0", keep=False)
    assert "cgs_stream" not in lay0 and lay["cgs_stream"] == 30
    _same(got, ref, n)


# 8 / 9: the last NC of the register prefetch and the first beyond it; 9 / 10:
# NC = the ring's depth (no refill) and one past it (one refill); 17 / 18: the
# second lap of the ring ends / begins; 30: the bench's; 32: NC = kNC
@pytest.mark.parametrize("rlen", [8, RING, RING + 1, 17, 2 * RING, 30, 32])
def test_restart_lengths(mpg, monkeypatch, rlen):
    _check(mpg, monkeypatch, 8196, rlen=rlen)


def test_wrong_slot(mpg, monkeypatch):
    """rlen 32 on n = 260: every slot refilled up to three times; two live
    waves, the second with one live lane."""
    _check(mpg, monkeypatch, 260, rlen=32)


@pytest.mark.parametrize("step_dots", [None, "0"])
@pytest.mark.parametrize("prec", ["identity", "jacobi"])
def test_prec_and_step_dots(mpg, monkeypatch, prec, step_dots):
    _check(mpg, monkeypatch, 8196, step_dots=step_dots, prec=prec)


def test_two_ranks_same_bits(mpg, monkeypatch):
    """The multi-rank engine takes the same form: its update sums the
    all-reduced partials in-launch, as on one GPU. Two loopback ranks of 4098
    rows each (a full workgroup plus a row group of two live rows and the
    tail), =1 against =0, and every rank reports what it ran."""
    A, xt, b = _problem(mpg, 8196)
    monkeypatch.delenv("MPG_STEP_DOTS", raising=False)
    opts = dict(mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=2, accum="f32")
    res, lays = {}, {}
    for v in ("0", "1"):
        monkeypatch.setenv("MPG_CGS_PREFETCH", v)
        lays[v] = []
        res[v] = mpg.solve_loopback(A, b, xt, nranks=2, layouts=lays[v], **opts)
    assert [L["cgs_stream"] for L in lays["0"]] == [0, 0], lays["0"]
    assert [L["cgs_stream"] for L in lays["1"]] == [30, 30], lays["1"]
    assert res["0"].total_iters == res["1"].total_iters == 60
    _same(res["1"], res["0"], "two ranks")


def test_engine_reports_what_it_ran(mpg, monkeypatch):
    """spmv_layout()["cgs_stream"]: the update launches per cycle that take the
    streaming form -- rlen under =1 in the fp32 class, absent under =0, in the
    fp64 class (not built: it runs what it ran before) and under MGS."""
    A, xt, b = _problem(mpg, 8196)
    monkeypatch.delenv("MPG_STEP_DOTS", raising=False)

    def layout(prefetch, **opts):
        if prefetch is None:
            monkeypatch.delenv("MPG_CGS_PREFETCH", raising=False)
        else:
            monkeypatch.setenv("MPG_CGS_PREFETCH", prefetch)
        kw = dict(mode="mixed", orth="cgs", prec="identity", rlen=30, tol=0.0, max_restarts=1, accum="f32")
        kw.update(opts)
        eng = mpg.Engine(A, b, xt, **kw)
        try:
            return eng.spmv_layout()
        finally:
            eng.close()

    assert layout("1")["cgs_stream"] == 30
    assert layout("1", rlen=12)["cgs_stream"] == 12
    assert "cgs_stream" not in layout("0")
    assert "cgs_stream" not in layout("1", accum="f64")
    assert "cgs_stream" not in layout(None, accum="f64")
    assert "cgs_stream" not in layout("1", orth="mgs")
    unset = layout(None)
    assert unset.get("cgs_stream", 0) == UNSET_DEFAULT_STEPS, unset


# update launches of GMRES(30)'s cycle that stream when MPG_CGS_PREFETCH is
# unset (cgs_update_form, csrc/arnoldi_launch.hpp: NC >= kCgsStreamFrom)
UNSET_DEFAULT_STEPS = 22  # NC = 9 .. 30
