"""The fused engine's restart cycle as an op list (host/cycle_plan.cpp,
mpg_cycle_plan_describe): the launches and collectives a policy gives, in
order, with the phase timers' tags. CPU only: the plan is a pure function of
mpg_cycle_policy, and nothing here touches a device.

Every expected list is read off the engine's step / Givens / prologue
sequence: SpMV (with Givens(k-1) folded in from step 1), an optional
preconditioner launch, the orthogonalisation's launches, then the Givens step
unless it is folded into the next SpMV; after step m-1 the trailing Givens of
a folded cycle, update(m) and the residual prologue.
"""
import ctypes as C

import pytest

UNSUPPORTED = -5  # MPG_ERR_UNSUPPORTED (include/mpgmres/capi.h)
CGS, MGS, CGSR = 0, 1, 2


def policy(mpg, **kw):
    from mpgmres_amd._abi import CyclePolicy
    f = dict(ranks=0, orth=CGS, m=3, graph=1, pipeline=1, fold=1, combine=0, cgs_partials=1, fuse_dots=0,
             fuse_dots_required=0, fuse_dots_k0=32, step_dots=0, step_dots_lo=1, step_dots_hi=32, sep_prec=0,
             sep_prec_step=0, sep_prec_prologue=0, partials_max_cols=128, fold_max_m=128)
    step_ok, spmv_ok = kw.pop("step_dots_ok", ()), kw.pop("spmv_dots_ok", ())
    f.update(kw)
    p = CyclePolicy(**f)
    for k, v in enumerate(step_ok):
        p.step_dots_ok[k] = v
    for k, v in enumerate(spmv_ok):
        p.spmv_dots_ok[k] = v
    return p


def describe(mpg, p):
    """The tokens of plan_cycle(p), or the negative status."""
    lib = mpg.host_lib()
    need = lib.mpg_cycle_plan_describe(C.byref(p), None, 0)
    if need < 0:
        return need
    buf = C.create_string_buffer(need + 1)
    assert lib.mpg_cycle_plan_describe(C.byref(p), buf, need + 1) == need
    return buf.value.decode().split(" ")


def names(tokens):
    return [t.split("@")[0] for t in tokens]


def tags(tokens):
    return {t.split("@")[0]: t.split("@")[1] for t in tokens if "@" in t}


ONES = [1] * 32
SPLIT_1 = ("x_snapshot "
           "spmv(0) dots(0) cgs_partials(0) "
           "givens+spmv(1) dots(1) cgs_partials(1) "
           "givens+spmv(2) dots(2) cgs_partials(2) "
           "givens_partials(2) update(3) prologue prologue_finish_partials").split()


def test_one_gpu_cgs_folded(mpg):
    got = describe(mpg, policy(mpg))
    assert names(got) == SPLIT_1
    assert got[1:4] == ["spmv(0)@0+dup", "dots(0)@3+dup", "cgs_partials(0)@2+dup<1"]
    assert got[4] == "givens+spmv(1)@0+dup" and got[-2] == "prologue@1"
    assert set(tags(got)) == set(SPLIT_1[1:10]) | {"prologue"}


def test_buffer_contract(mpg):
    lib, p = mpg.host_lib(), policy(mpg)
    whole = " ".join(describe(mpg, p))
    buf = C.create_string_buffer(12)
    assert lib.mpg_cycle_plan_describe(C.byref(p), buf, 12) == len(whole)
    assert buf.value.decode() == whole[:11]
    assert lib.mpg_cycle_plan_describe(None, buf, 12) == -2
    assert describe(mpg, policy(mpg, m=0)) == -2


def test_step_dots(mpg):
    got = describe(mpg, policy(mpg, step_dots=-1, step_dots_ok=ONES))
    assert got == ("x_snapshot "
                   "step_dots(0,0)@0+dup cgs_partials(0)@2+dup<1 "
                   "step_dots(1,2)@0+dup cgs_partials(1)@2+dup<1 "
                   "step_dots(2,2)@0+dup cgs_partials(2)@2+dup<1 "
                   "givens_partials(2) update(3) prologue@1 prologue_finish_partials").split()
    # unfolded: fold form 0 at every step, and the step's own Givens launch
    got = describe(mpg, policy(mpg, step_dots=1, fold=0, m=2, step_dots_ok=ONES))
    assert names(got) == ("x_snapshot step_dots(0,0) cgs_partials(0) givens_partials(0) step_dots(1,0) "
                          "cgs_partials(1) givens_partials(1) update(2) prologue prologue_finish_partials").split()
    # a step the workspace refuses reverts alone to the three launches
    got = describe(mpg, policy(mpg, step_dots=-1, step_dots_ok=[1, 0, 1]))
    assert names(got) == (SPLIT_1[:1] + ["step_dots(0,0)", "cgs_partials(0)"] + SPLIT_1[4:7] +
                          ["step_dots(2,2)", "cgs_partials(2)"] + SPLIT_1[10:])
    # the measured policy's range, moved
    got = describe(mpg, policy(mpg, step_dots=-1, step_dots_lo=2, step_dots_hi=2, step_dots_ok=ONES))
    assert names(got) == SPLIT_1[:4] + ["step_dots(1,2)", "cgs_partials(1)"] + SPLIT_1[7:]
    # never; and wherever supported, with nothing supported
    assert names(describe(mpg, policy(mpg, step_dots=0, step_dots_ok=ONES))) == SPLIT_1
    assert names(describe(mpg, policy(mpg, step_dots=1))) == SPLIT_1
    # required: an engine or a step that cannot take it is an error
    assert describe(mpg, policy(mpg, step_dots=2, step_dots_ok=ONES)) == describe(
        mpg, policy(mpg, step_dots=1, step_dots_ok=ONES))
    assert describe(mpg, policy(mpg, step_dots=2, step_dots_ok=ONES, sep_prec=1)) == UNSUPPORTED
    assert describe(mpg, policy(mpg, step_dots=2, step_dots_ok=[1, 0, 1])) == UNSUPPORTED
    for other in (dict(ranks=2), dict(orth=CGSR), dict(orth=MGS, cgs_partials=0), dict(cgs_partials=0),
                  dict(combine=1, cgs_partials=0, fold=0)):
        assert describe(mpg, policy(mpg, step_dots=2, step_dots_ok=ONES, **other)) == UNSUPPORTED, other
        assert "step_dots" not in " ".join(describe(mpg, policy(mpg, step_dots=1, step_dots_ok=ONES, **other))), other


def test_two_ranks_cgs(mpg):
    got = describe(mpg, policy(mpg, ranks=2, m=2))
    assert names(got) == ("x_snapshot "
                          "halo(0) spmv(0) dots(0) allreduce_partials(1) cgs_partials(0) "
                          "allreduce_partials+halo(1) givens+spmv(1) dots(1) allreduce_partials(2) cgs_partials(1) "
                          "reduce(1) allreduce_sums(1) givens(1) "
                          "update(2) "
                          "halo(x) prologue reduce(3) allreduce_sums(3) prologue_finish").split()
    # the duplicate update re-runs the dots, not the all-reduce between them
    assert tags(got) == {"spmv(0)": "0+dup", "dots(0)": "3+dup", "cgs_partials(0)": "2+dup<2",
                         "givens+spmv(1)": "0+dup", "dots(1)": "3+dup", "cgs_partials(1)": "2+dup<2", "prologue": "1"}
    # a communicator of one rank runs the ranks' sequence
    assert names(describe(mpg, policy(mpg, ranks=1, m=2))) == names(got)
    # unfolded: one sum reduced and all-reduced ahead of every Givens launch
    got = describe(mpg, policy(mpg, ranks=2, m=1, fold=0, pipeline=0))
    assert names(got) == ("halo(0) spmv(0) dots(0) allreduce_partials(1) cgs_partials(0) reduce(1) allreduce_sums(1) "
                          "givens(0) update(1) halo(x) prologue reduce(3) allreduce_sums(3) prologue_finish").split()
    # past 32 columns the ranks' update takes the reduced sums
    got = names(describe(mpg, policy(mpg, ranks=2, m=34)))
    i = got.index("givens+spmv(33)")
    assert got[i - 1:i + 6] == ["allreduce_partials+halo(33)", "givens+spmv(33)", "dots(33)", "reduce(34)",
                                "allreduce_sums(34)", "cgs(33,0)", "reduce(1)"]


def test_mgs(mpg):
    got = describe(mpg, policy(mpg, orth=MGS, m=2, fold=0, cgs_partials=0, pipeline=0))
    assert names(got) == ("spmv(0) dots(0) mgs_partials(0,0) givens_partials(0) "
                          "spmv(1) dots(1) mgs_partials(1,0) mgs_partials(1,1) givens_partials(1) "
                          "update(2) prologue prologue_finish_partials").split()
    assert tags(got) == {"spmv(0)": "0+dup", "spmv(1)": "0+dup", "prologue": "1"}  # no MGS op is a timed site
    got = describe(mpg, policy(mpg, orth=MGS, m=2, fold=0, cgs_partials=0, pipeline=0, ranks=2))
    assert names(got) == ("halo(0) spmv(0) dots(0) allreduce_partials(1) mgs_partials(0,0) "
                          "reduce(1) allreduce_sums(1) givens(0) "
                          "halo(1) spmv(1) dots(1) allreduce_partials(1) mgs_partials(1,0) allreduce_partials(1) "
                          "mgs_partials(1,1) reduce(1) allreduce_sums(1) givens(1) "
                          "update(2) halo(x) prologue reduce(3) allreduce_sums(3) prologue_finish").split()


def test_cgsr(mpg):
    got = describe(mpg, policy(mpg, orth=CGSR, m=2, cgs_partials=0))
    assert names(got) == ("x_snapshot "
                          "spmv(0) dots(0) reduce(1) cgs(0,0) reduce(1) cgs(0,1) "
                          "givens+spmv(1) dots(1) reduce(2) cgs(1,0) reduce(2) cgs(1,1) "
                          "givens_partials(1) update(2) prologue prologue_finish_partials").split()
    # only the SpMV, the dots and the last pass are timed sites
    assert tags(got) == {"spmv(0)": "0+dup", "dots(0)": "3+dup", "cgs(0,1)": "2+dup", "givens+spmv(1)": "0+dup",
                         "dots(1)": "3+dup", "cgs(1,1)": "2+dup", "prologue": "1"}
    # MPG_CGS_PARTIALS=1: the first pass sums the dots' partials itself
    got = describe(mpg, policy(mpg, orth=CGSR, m=1, cgs_partials=1, pipeline=0))
    assert got == ("spmv(0)@0+dup dots(0)@3+dup cgs_partials(0)@2+dup<1 reduce(1) cgs(0,1)@2+dup givens_partials(0) "
                   "update(1) prologue@1 prologue_finish_partials").split()


def test_cgsr_past_32_columns(mpg):
    got = describe(mpg, policy(mpg, orth=CGSR, m=40, cgs_partials=0))
    for k in range(32, 40):
        i = got.index(f"givens+spmv({k})@0+dup")
        assert got[i + 1:i + 5] == [f"dots({k})", f"cgsr_wide_pass({k},0)", f"dots({k})", f"cgsr_wide_pass({k},1)"]
    assert got[got.index("givens+spmv(31)@0+dup") + 1] == "dots(31)@3+dup"
    assert sum(t.startswith("cgsr_wide_pass") for t in got) == 16 and got[-4] == "givens_partials(39)"
    # past the wide update's columns: the reduced form again
    got = names(describe(mpg, policy(mpg, orth=CGSR, m=40, cgs_partials=0, partials_max_cols=36)))
    assert got[got.index("givens+spmv(36)") + 1:][:5] == ["dots(36)", "reduce(37)", "cgs(36,0)", "reduce(37)",
                                                           "cgs(36,1)"]
    # plain CGS there: the wide update sums the panel dots' partials itself, up to the same limit
    got = names(describe(mpg, policy(mpg, m=40, partials_max_cols=36)))
    assert got[got.index("dots(35)") + 1] == "cgs_partials(35)"
    assert got[got.index("dots(36)") + 1:][:2] == ["reduce(37)", "cgs(36,0)"]


@pytest.mark.parametrize("mode", [-1, 0, 1])
def test_separate_preconditioner(mpg, mode):
    ilu = dict(sep_prec=1, sep_prec_step=1, sep_prec_prologue=1)
    got = describe(mpg, policy(mpg, m=2, step_dots=mode, step_dots_ok=ONES, spmv_dots_ok=ONES, fuse_dots=1, **ilu))
    assert names(got) == ("x_snapshot "
                          "spmv(0) apply_prec(w1) dots(0) cgs_partials(0) "
                          "givens+spmv(1) apply_prec(w2) dots(1) cgs_partials(1) "
                          "givens_partials(1) update(2) "
                          "prologue apply_prec(w0) prologue_wnorm prologue_finish_partials").split()
    # block Jacobi applied inside the prologue: only the norm again
    got = describe(mpg, policy(mpg, m=1, step_dots=mode, step_dots_ok=ONES, sep_prec=1, sep_prec_step=1))
    assert names(got)[-5:] == ["givens_partials(0)", "update(1)", "prologue", "prologue_wnorm",
                               "prologue_finish_partials"]
    # ... and inside the SpMV: no launch of its own, and still no one-launch step
    got = describe(mpg, policy(mpg, m=1, step_dots=mode, step_dots_ok=ONES, sep_prec=1))
    assert names(got)[:4] == ["x_snapshot", "spmv(0)", "dots(0)", "cgs_partials(0)"]


def test_combine(mpg):
    got = describe(mpg, policy(mpg, m=2, combine=1, cgs_partials=0, fold=0))
    assert got == ("x_snapshot spmv(0)@0+dup dots_sums(0) cgs_givens(0,0) spmv(1)@0+dup dots_sums(1) cgs_givens(1,0) "
                   "update(2) prologue@1 prologue_finish_partials").split()
    got = names(describe(mpg, policy(mpg, orth=CGSR, m=1, combine=1, cgs_partials=0, fold=0, pipeline=0)))
    assert got[:5] == ["spmv(0)", "dots_sums(0)", "cgs(0,0)", "reduce(1)", "cgs_givens(0,1)"]


def test_fuse_dots(mpg):
    got = describe(mpg, policy(mpg, m=2, fuse_dots=1, fuse_dots_k0=1, spmv_dots_ok=ONES))
    assert got == ("x_snapshot spmv_dots(0,0)@0 cgs_partials(0) "
                   "givens+spmv(1)@0+dup dots(1)@3+dup cgs_partials(1)@2+dup<1 "
                   "givens_partials(1) update(2) prologue@1 prologue_finish_partials").split()
    got = describe(mpg, policy(mpg, m=2, fuse_dots=1, spmv_dots_ok=ONES))
    assert got[1:5] == ["spmv_dots(0,0)@0", "cgs_partials(0)", "spmv_dots(1,2)@0", "cgs_partials(1)"]
    # storage that does not support it: the separate launches, or an error when required
    assert names(describe(mpg, policy(mpg, fuse_dots=1))) == SPLIT_1
    assert describe(mpg, policy(mpg, fuse_dots=1, fuse_dots_required=1)) == UNSUPPORTED
    assert describe(mpg, policy(mpg, fuse_dots=1, fuse_dots_required=1, fuse_dots_k0=0)) == describe(mpg, policy(mpg))


def _dup_counts(tokens):
    """(added launches per phase, duplicates that re-issue an earlier op) as time_phase_dup counts them"""
    added = {ph: sum(f"@{ph}+dup" in t for t in tokens) for ph in (0, 2, 3)}
    return added, sum("<" in t for t in tokens)


def test_duplicate_counts(mpg):
    assert _dup_counts(describe(mpg, policy(mpg))) == ({0: 3, 2: 3, 3: 3}, 3)
    # every step on the one launch: no dots launch left to double
    assert _dup_counts(describe(mpg, policy(mpg, step_dots=-1, step_dots_ok=ONES))) == ({0: 3, 2: 3, 3: 0}, 3)
    assert _dup_counts(describe(mpg, policy(mpg, orth=CGSR, m=2, cgs_partials=0))) == ({0: 2, 2: 2, 3: 2}, 0)
    # the bench's cycle: m added launches per phase
    assert _dup_counts(describe(mpg, policy(mpg, m=30)))[0] == {0: 30, 2: 30, 3: 30}
