// The fused engine's restart cycle as data: pure functions of the resolved
// policy (mpg_cycle_policy, include/mpgmres/solve.h) that list the launches
// and collectives of a step, of the residual prologue and of a whole cycle.
// The engine issues the list (FusedEngine::issue); the phase timers walk it.
// Host C++ only: the schedule is tested on a CPU (tests/test_cycle_plan.py).
#ifndef MPGMRES_CYCLE_PLAN_HPP
#define MPGMRES_CYCLE_PLAN_HPP

#include <string>
#include <vector>

#include "mpgmres/solve.h"

namespace mpg {

using CyclePolicy = mpg_cycle_policy;

// One kind per distinct call of the cycle: FusedEngine::issue maps each to
// its mpg_arnoldi_* / Comm call, kOpNames (cycle_plan.cpp, this order) to
// its spelling. Halo: of w_prev(a), a < 0: of x. ApplyPrec: M^-1 on w_prev(a).
// GivensUpdate(m, flags): Givens step m-1 and update(m) in one launch
// (policy.tail_fold); flags bit 0: the launch also keeps the x it read (the
// cycle then has no XSnapshot).
enum class OpKind : uint8_t {
    XSnapshot, Halo, AllreducePartialsHalo, Spmv, GivensSpmv, SpmvDots, StepDots, ApplyPrec, Dots, DotsSums,
    AllreducePartials, Reduce, AllreduceSums, CgsPartials, Cgs, CgsGivens, CgsrWidePass, MgsPartials, Givens,
    GivensPartials, Update, Prologue, PrologueWnorm, PrologueFinish, PrologueFinishPartials, GivensUpdate,
};

struct Op {
    OpKind kind;
    int8_t phase;  // the C-ABI's `which` (0 SpMV, 1 prologue, 2 CGS update, 3 dots) of a timed site; -1: none
    bool dup;      // time_phase_dup issues the op twice
    uint8_t redo;  // ... after issuing the op this far back once more (0: none)
    int a, b;      // the step k or a column count; the pass, the column j or the fold form
};

// Append step k's ops (fold: Givens(k-1) rides this step's SpMV launch and
// step k's own Givens is left to the next step / the caller), the residual
// prologue's, a whole cycle's (snapshot, steps 0..m-1, the trailing Givens
// step if folded, update(m), prologue; with policy.tail_fold on one GPU and
// m <= 32, a givens_partials(m-1) directly ahead of update(m) and the
// snapshot go into the one givens+update launch). MPG_OK, or MPG_ERR_UNSUPPORTED where
// a required launch (step_dots / fuse_dots = 2) cannot be taken.
int plan_step(const CyclePolicy& p, int k, bool fold, std::vector<Op>& out);
void plan_prologue(const CyclePolicy& p, std::vector<Op>& out);
int plan_cycle(const CyclePolicy& p, std::vector<Op>& out);
std::string describe(const std::vector<Op>& ops);  // the grammar of mpg_cycle_plan_describe (solve.h)

}  // namespace mpg

#endif  // MPGMRES_CYCLE_PLAN_HPP
