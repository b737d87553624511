// The restart cycle's op list (cycle_plan.hpp) and its text form.
#include "cycle_plan.hpp"

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "mpgmres/capi.h"

namespace mpg {
namespace {

// in OpKind's order
constexpr struct {
    const char* name;
    int nargs;
} kOpNames[] = {
    {"x_snapshot", 0}, {"halo", 1}, {"allreduce_partials+halo", 1}, {"spmv", 1}, {"givens+spmv", 1},
    {"spmv_dots", 2}, {"step_dots", 2}, {"apply_prec", 1}, {"dots", 1}, {"dots_sums", 1},
    {"allreduce_partials", 1}, {"reduce", 1}, {"allreduce_sums", 1}, {"cgs_partials", 1}, {"cgs", 2},
    {"cgs_givens", 2}, {"cgsr_wide_pass", 2}, {"mgs_partials", 2}, {"givens", 1}, {"givens_partials", 1},
    {"update", 1}, {"prologue", 0}, {"prologue_wnorm", 0}, {"prologue_finish", 0}, {"prologue_finish_partials", 0},
    {"givens+update", 2},
};
static_assert(sizeof kOpNames / sizeof kOpNames[0] == (size_t)OpKind::GivensUpdate + 1, "one name per kind");

struct Builder {
    const CyclePolicy& p;
    std::vector<Op>& out;
    bool ranks() const { return p.ranks > 0; }
    void op(OpKind kind, int a = 0, int b = 0) { out.push_back(Op{kind, -1, false, 0, a, b}); }
    // a site of the phase timers; dup: time_phase_dup doubles it, after the op `redo` back once more
    void site(int phase, bool dup, OpKind kind, int a = 0, int b = 0, int redo = 0) {
        out.push_back(Op{kind, (int8_t)phase, dup, (uint8_t)redo, a, b});
    }
    void reduce(int nc) {
        op(OpKind::Reduce, nc);
        if (ranks()) op(OpKind::AllreduceSums, nc);
    }
    // ||w||^2: one GPU folds the partial sums into the Givens kernel; ranks of
    // a partitioned solve reduce + all-reduce first
    void givens(int k) {
        if (ranks()) reduce(1);
        op(ranks() ? OpKind::Givens : OpKind::GivensPartials, k);
    }
};

bool at(const uint8_t* ok, int k) { return k < MPG_CYCLE_POLICY_STEPS && ok[k]; }

}  // namespace

int plan_step(const CyclePolicy& p, int k, bool fold, std::vector<Op>& out) {
    Builder B{p, out};
    const bool ranks = B.ranks();
    const int f = fold && k > 0 ? 2 : 0;
    // one GPU, plain CGS whose update sums the dots' partials itself, no
    // preconditioner launch between the SpMV and the dots
    const bool one_launch_ok = !ranks && !p.sep_prec && p.orth == MPG_ORTH_CGS && p.cgs_partials && !p.combine;
    // SpMV and panel dots in one launch (MPG_FUSE_DOTS); where the storage
    // does not support it: the separate launches below
    if (p.fuse_dots && one_launch_ok && k + 1 <= p.fuse_dots_k0) {
        if (at(p.spmv_dots_ok, k)) {
            B.site(0, false, OpKind::SpmvDots, k, f);
            B.op(OpKind::CgsPartials, k);
            if (!fold) B.givens(k);
            return MPG_OK;
        }
        if (p.fuse_dots_required) return MPG_ERR_UNSUPPORTED;
    }
    // the SpMV inside the panel dots' launch, then straight to the update
    // that sums the dots' partials itself (MPG_STEP_DOTS; same bits)
    const bool can = one_launch_ok && at(p.step_dots_ok, k);
    if (p.step_dots == 2 && !can) return MPG_ERR_UNSUPPORTED;
    if (can && (p.step_dots > 0 || (p.step_dots < 0 && k + 1 >= p.step_dots_lo && k + 1 <= p.step_dots_hi))) {
        B.site(0, true, OpKind::StepDots, k, f);
        // (the update's own partials replaced nothing the launch before it
        // reads, but its duplicate needs w = A v_k and the dots again: the
        // one launch is re-run ahead, and time_phase_dup takes its share out)
        B.site(2, true, OpKind::CgsPartials, k, 0, 1);
        if (!fold) B.givens(k);
        return MPG_OK;
    }
    // (folded: the ||w||^2 partials' all-reduce and the w_prev halo in one RCCL group)
    if (ranks) B.op(f ? OpKind::AllreducePartialsHalo : OpKind::Halo, k);
    B.site(0, true, f ? OpKind::GivensSpmv : OpKind::Spmv, k);
    if (p.sep_prec_step) B.op(OpKind::ApplyPrec, k + 1);  // w = M(A v_k)
    if (p.orth == MPG_ORTH_MGS) {
        B.op(OpKind::Dots, k);
        // each update sums the previous launch's partials itself (ranks:
        // all-reduced in place first)
        for (int j = 0; j <= k; ++j) {
            if (ranks) B.op(OpKind::AllreducePartials, 1);
            B.op(OpKind::MgsPartials, k, j);
        }
        if (!fold) B.givens(k);
        return MPG_OK;
    }
    // (one GPU, plain CGS: up to partials_max_cols columns -- GMRES(100) --
    // the wide update sums the one-launch panel dots' partials itself)
    const bool small = k + 1 <= 32 || (!ranks && p.orth == MPG_ORTH_CGS && k + 1 <= p.partials_max_cols);
    if (!ranks && !p.combine && p.orth == MPG_ORTH_CGSR && k + 1 > 32 && k + 1 <= p.partials_max_cols) {
        // CGSR at GMRES(100): dots, pass 0, dots again on the updated w, pass 1
        for (int pass = 0; pass < 2; ++pass) {
            B.op(OpKind::Dots, k);
            B.op(OpKind::CgsrWidePass, k, pass);
        }
        if (!fold) B.givens(k);
        return MPG_OK;
    }
    const int last_pass = p.orth == MPG_ORTH_CGSR ? 1 : 0;
    bool pass0_done = false;
    if (p.combine && k + 1 <= 32) {
        // the dots' last workgroup writes the sums
        B.op(OpKind::DotsSums, k);
    } else {
        B.site(3, true, OpKind::Dots, k);
        if (p.cgs_partials && small) {
            if (ranks) B.op(OpKind::AllreducePartials, k + 1);
            // (the in-launch sums read the dots' partials, which the first
            // update's own partials replaced: the duplicate re-runs the dots
            // first -- not the all-reduce -- and time_phase_dup takes their
            // share back out)
            B.site(2, true, OpKind::CgsPartials, k, 0, ranks ? 2 : 1);
            pass0_done = true;
        } else {
            B.reduce(k + 1);
        }
    }
    if (last_pass == 1) {
        if (!pass0_done) B.op(OpKind::Cgs, k, 0);
        B.reduce(k + 1);
    } else if (pass0_done) {
        if (!fold) B.givens(k);
        return MPG_OK;
    }
    if (p.combine) {  // ... and the last CGS pass's last workgroup runs the Givens step
        B.op(OpKind::CgsGivens, k, last_pass);
        return MPG_OK;
    }
    B.site(2, true, OpKind::Cgs, k, last_pass);
    if (!fold) B.givens(k);
    return MPG_OK;
}

void plan_prologue(const CyclePolicy& p, std::vector<Op>& out) {
    Builder B{p, out};
    if (B.ranks()) B.op(OpKind::Halo, -1);
    B.site(1, false, OpKind::Prologue);
    if (p.sep_prec) {  // w = M(T(r)) outside the kernel, then ||w||^2 again
        // (block Jacobi inside the prologue: only the norm, in the order the
        // separate form sums it, so both forms give one beta)
        if (p.sep_prec_prologue) B.op(OpKind::ApplyPrec, 0);
        B.op(OpKind::PrologueWnorm);
    }
    if (B.ranks()) B.reduce(3);  // (one GPU: the 3 column sums inside the finish launch, same bits)
    B.op(B.ranks() ? OpKind::PrologueFinish : OpKind::PrologueFinishPartials);
}

int plan_cycle(const CyclePolicy& p, std::vector<Op>& out) {
    if (p.m < 1) return MPG_ERR_ARG;
    const size_t head = out.size();
    for (int k = 0; k < p.m; ++k)
        if (int st = plan_step(p, k, p.fold != 0, out)) return st;
    Builder B{p, out};
    if (p.fold) B.givens(p.m - 1);
    // the cycle's tail in one launch: the last Givens step, the update and
    // the snapshot of the x it overwrites (the next cycle's undo)
    const bool tail = p.tail_fold && !B.ranks() && p.m <= 32 && out.size() > head &&
                      out.back().kind == OpKind::GivensPartials && out.back().a == p.m - 1;
    if (tail) {
        out.pop_back();
        B.op(OpKind::GivensUpdate, p.m, p.pipeline ? 1 : 0);
    } else {
        if (p.pipeline) out.insert(out.begin() + (std::ptrdiff_t)head, Op{OpKind::XSnapshot, -1, false, 0, 0, 0});
        B.op(OpKind::Update, p.m);
    }
    plan_prologue(p, out);
    return MPG_OK;
}

std::string describe(const std::vector<Op>& ops) {
    std::string s;
    for (const Op& o : ops) {
        const auto& t = kOpNames[(size_t)o.kind];
        if (!s.empty()) s += ' ';
        s += t.name;
        const std::string a = o.kind == OpKind::ApplyPrec ? "w" + std::to_string(o.a) : o.a < 0 ? "x" : std::to_string(o.a);
        if (t.nargs) s += "(" + a + (t.nargs == 2 ? "," + std::to_string(o.b) : "") + ")";
        if (o.phase >= 0) s += '@' + std::to_string(o.phase);
        if (o.dup) s += "+dup";
        if (o.redo) s += '<' + std::to_string(o.redo);
    }
    return s;
}

}  // namespace mpg

extern "C" int mpg_cycle_plan_describe(const mpg_cycle_policy* p, char* buf, int len) {
    if (!p || len < 0 || (len && !buf)) return MPG_ERR_ARG;
    std::vector<mpg::Op> ops;
    if (int st = mpg::plan_cycle(*p, ops)) return st;
    const std::string s = mpg::describe(ops);
    if (len) std::snprintf(buf, (size_t)len, "%s", s.c_str());
    return (int)s.size();
}
