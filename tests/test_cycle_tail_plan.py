"""The cycle's tail in one launch, as plan_cycle lists it (host/cycle_plan.cpp,
mpg_cycle_policy.tail_fold). CPU only.

With tail_fold set, on one GPU and m <= 32, a givens_partials(m-1) directly
ahead of update(m) becomes givens+update(m,flags), in the folded and in the
unfolded plan; with `pipeline` the op's flag 1 says it also keeps the x it
read, and the list has no x_snapshot. Everything else is today's list.
"""
from tests.test_cycle_plan import CGSR, MGS, ONES, describe, names, policy


def test_folded(mpg):
    got = describe(mpg, policy(mpg, tail_fold=1))
    assert names(got) == ("spmv(0) dots(0) cgs_partials(0) "
                          "givens+spmv(1) dots(1) cgs_partials(1) "
                          "givens+spmv(2) dots(2) cgs_partials(2) "
                          "givens+update(3,1) prologue prologue_finish_partials").split()
    # the new op is no timed site, and the others keep their tags
    assert got[-3] == "givens+update(3,1)" and got[-2] == "prologue@1"
    assert got[:3] == ["spmv(0)@0+dup", "dots(0)@3+dup", "cgs_partials(0)@2+dup<1"]
    # not pipelined: no snapshot either way, flag 0
    got = describe(mpg, policy(mpg, tail_fold=1, pipeline=0))
    assert got[-3:] == ["givens+update(3,0)", "prologue@1", "prologue_finish_partials"]
    assert "x_snapshot" not in got


def test_step_dots_cycle(mpg):
    """The bench's cycle: every step on the one launch, then the one tail launch."""
    got = describe(mpg, policy(mpg, tail_fold=1, step_dots=-1, step_dots_ok=ONES))
    assert got == ("step_dots(0,0)@0+dup cgs_partials(0)@2+dup<1 "
                   "step_dots(1,2)@0+dup cgs_partials(1)@2+dup<1 "
                   "step_dots(2,2)@0+dup cgs_partials(2)@2+dup<1 "
                   "givens+update(3,1) prologue@1 prologue_finish_partials").split()


def test_unfolded(mpg):
    got = describe(mpg, policy(mpg, tail_fold=1, fold=0, m=2))
    assert names(got) == ("spmv(0) dots(0) cgs_partials(0) givens_partials(0) "
                          "spmv(1) dots(1) cgs_partials(1) "
                          "givens+update(2,1) prologue prologue_finish_partials").split()
    # m = 1: the only Givens step is the tail's
    got = describe(mpg, policy(mpg, tail_fold=1, fold=0, m=1, pipeline=0))
    assert names(got) == "spmv(0) dots(0) cgs_partials(0) givens+update(1,0) prologue prologue_finish_partials".split()


def test_mgs(mpg):
    got = describe(mpg, policy(mpg, tail_fold=1, orth=MGS, m=2, fold=0, cgs_partials=0, pipeline=0))
    assert names(got) == ("spmv(0) dots(0) mgs_partials(0,0) givens_partials(0) "
                          "spmv(1) dots(1) mgs_partials(1,0) mgs_partials(1,1) "
                          "givens+update(2,0) prologue prologue_finish_partials").split()


def test_cgsr(mpg):
    got = describe(mpg, policy(mpg, tail_fold=1, orth=CGSR, m=2, cgs_partials=0))
    assert names(got) == ("spmv(0) dots(0) reduce(1) cgs(0,0) reduce(1) cgs(0,1) "
                          "givens+spmv(1) dots(1) reduce(2) cgs(1,0) reduce(2) cgs(1,1) "
                          "givens+update(2,1) prologue prologue_finish_partials").split()


def test_a_separate_preconditioner_keeps_its_launches(mpg):
    ilu = dict(sep_prec=1, sep_prec_step=1, sep_prec_prologue=1)
    got = describe(mpg, policy(mpg, tail_fold=1, m=2, **ilu))
    assert names(got)[-5:] == ["givens+update(2,1)", "prologue", "apply_prec(w0)", "prologue_wnorm",
                               "prologue_finish_partials"]


def test_todays_lists(mpg):
    """Ranks, m = 33, the combining launches and tail_fold = 0: word for word
    what the same policy gives without the field."""
    for kw in (dict(ranks=2, m=2), dict(ranks=1, m=2), dict(m=33), dict(m=40, orth=CGSR, cgs_partials=0),
               dict(m=2, combine=1, cgs_partials=0, fold=0), dict(ranks=2, m=2, orth=MGS, fold=0, cgs_partials=0)):
        want = describe(mpg, policy(mpg, **kw))
        assert describe(mpg, policy(mpg, tail_fold=1, **kw)) == want, kw
        assert "givens+update" not in " ".join(want)
    got33 = describe(mpg, policy(mpg, tail_fold=1, m=33))
    assert got33[0] == "x_snapshot" and got33[-4:-2] == ["givens_partials(32)", "update(33)"]
    # 32 is the last restart length that takes the form
    got32 = describe(mpg, policy(mpg, tail_fold=1, m=32))
    assert got32[-3] == "givens+update(32,1)" and "x_snapshot" not in got32
    for kw in (dict(), dict(fold=0), dict(orth=MGS, fold=0, cgs_partials=0), dict(pipeline=0),
               dict(step_dots=-1, step_dots_ok=ONES)):
        got = describe(mpg, policy(mpg, tail_fold=0, **kw))
        assert got[-4:-2] == ["givens_partials(2)", "update(3)"], kw
        assert (got[0] == "x_snapshot") == bool(kw.get("pipeline", 1)), kw
