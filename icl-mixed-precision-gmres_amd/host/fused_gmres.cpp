// Fused Arnoldi engine (see fused_gmres.hpp) and its C-ABI (mpg_engine_*,
// mpg_solve with engine = MPG_ENGINE_FUSED).
#include "fused_gmres.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <thread>

#include "gmres.hpp"
#include "types_hip.hpp"

namespace mpg {

// ---------------------------------------------------------------- DevMem
DevMem::DevMem(mpg_ctx_t c, size_t b) : ctx(c), bytes(b) { check(mpg_malloc(c, b, &p), "mpg_malloc", c); }
DevMem::~DevMem() {
    if (p) mpg_free(ctx, p);
}
DevMem& DevMem::operator=(DevMem&& o) noexcept {
    if (this != &o) {
        if (p) mpg_free(ctx, p);
        ctx = o.ctx;
        p = o.p;
        bytes = o.bytes;
        o.p = nullptr;
        o.bytes = 0;
    }
    return *this;
}

void hipck(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("mpgmres: ") + what + ": " + hipGetErrorString(e));
}

namespace {

using clk = std::chrono::steady_clock;

// the driver's working types for a mode (gmres_perf_test.cpp:240-305)
struct ModeTypes {
    int T, X, P, VI;  // mpg_dtype_t
    bool single_scalars;  // host scalars in float (mode single)
};
ModeTypes types_for(int mode) {
    switch (mode) {
        case MPG_MODE_MIXED: return {MPG_F32, MPG_F64, MPG_F32, MPG_F32, false};
        case MPG_MODE_MIXED_HALF: return {MPG_F32, MPG_F64, MPG_F32, MPG_F16, false};
        case MPG_MODE_BASELINE: return {MPG_F64, MPG_F64, MPG_F64, MPG_F64, false};
        case MPG_MODE_SINGLE_PREC: return {MPG_F64, MPG_F64, MPG_F32, MPG_F64, false};
        case MPG_MODE_SINGLE: return {MPG_F32, MPG_F32, MPG_F32, MPG_F32, true};
        default: throw std::invalid_argument("unknown mode");
    }
}
size_t dsize(int t) { return t == MPG_F64 ? 8 : t == MPG_F32 ? 4 : 2; }

// LostOrthogonality (IterUtil.hpp:172-227) on the fused engine's basis. The
// base check (count, restart at m) comes first, as in the reference; the
// V^T v / S-column update is the engine's (orth_loss_step), which returns
// dot(s_col, s_col) rounded to the basis precision.
class LostOrthogonalityFused : public Convergence<double, void> {
    using Base = Convergence<double, void>;
    const double restart_tol_squared_;
    double current_loss_squared_ = 0;

public:
    std::function<double(size_t)> step_loss;
    LostOrthogonalityFused(double tol, double restart_tol, size_t m, size_t max_restarts)
        : Base(tol, m, max_restarts), restart_tol_squared_(restart_tol * restart_tol) {}
    iteration_action check_initial(double r, double nrm, double pr, double pb) override {
        current_loss_squared_ = 0;
        return Base::check_initial(r, nrm, pr, pb);
    }
    iteration_action check(size_t k, double res, double bnorm) override {
        const iteration_action a = Base::check(k, res, bnorm);
        if (a != iteration_next) return a;
        current_loss_squared_ += step_loss(k);
        return current_loss_squared_ >= restart_tol_squared_ ? iteration_restart : iteration_next;
    }
    bool needs_arnoldi_residual() const override { return true; }
};

// the unset MPG_STEP_DOTS policy: the steps (k + 1 in [lo, hi]) that take the
// SpMV inside the dots' launch; lo > hi: none. BAND-10M, kernel trace of the
// bench (profiles/r07_step_dots/): the one launch took less than k_step_sell2
// + k_dots_nc at every k (12.5 against 14.6 us at k = 0, 29.7 against 30.4 at
// k = 29) and saves the launch boundary between them, so every step takes it
constexpr int kStepDotsLo = 1, kStepDotsHi = 32;

}  // namespace

int basis_setting() {
    const char* e = std::getenv("MPG_BASIS");
    if (!e || !*e) return MPG_BASIS_F32;
    const std::string v = e;
    if (v == "f32") return MPG_BASIS_F32;
    if (v == "f16") return MPG_BASIS_F16;
    if (v == "f16emu") return MPG_BASIS_F16EMU;
    throw StatusError(MPG_ERR_ARG, "MPG_BASIS = " + v + " is not f32, f16 or f16emu");
}

const char* basis_name(int basis) {
    return basis == MPG_BASIS_F16 ? "f16" : basis == MPG_BASIS_F16EMU ? "f16emu" : "f32";
}

void check_basis_args(const mpg_solve_args& a, int basis, bool surface, bool ranks) {
    if (basis == MPG_BASIS_F32) return;
    const std::string name = std::string("basis ") + basis_name(basis);
    auto refuse = [&](const std::string& why) { throw StatusError(MPG_ERR_UNSUPPORTED, name + " " + why); };
    if (surface)
        refuse("is not available on the operator-surface engine: the compressed basis lives in the fused engine's "
               "Arnoldi kernels");
    if (ranks)
        refuse("is not available on a row-partitioned solve: the halo carries the raw w_prev, and the receiver's "
               "rounding giving the owner's bits is untested");
    if (a.mode != MPG_MODE_MIXED)
        refuse("runs in mode mixed only (fp32 Arnoldi on fp32 values, fp64 residual)");
    if (a.orth == MPG_ORTH_MGS)
        refuse("runs with orth cgs and cgsr only, not orth mgs: the MGS update has no compressed form");
    if (a.rlen > 32)
        refuse("needs rlen <= 32 (one panel of basis columns): rlen = " + std::to_string(a.rlen) +
               " would take the wide launches, which have no compressed form");
    if (a.orthloss) refuse("is not available with --orthloss: the loss estimate reads the basis as fp32");
    if (a.spmv_format == 3) refuse("is not available on node-block storage: node blocks are not built for it");
    if (basis == MPG_BASIS_F16EMU && a.spmv_format == 2)
        refuse("is built for the CSR row-block SpMV only (it exists for the tests): not SELL storage");
}

int prec_values_setting() {
    const char* e = std::getenv("MPG_PREC_VALUES");
    if (!e || !*e) return MPG_PREC_VALUES_F32;
    const std::string v = e;
    if (v == "f32") return MPG_PREC_VALUES_F32;
    if (v == "f16") return MPG_PREC_VALUES_F16;
    if (v == "f16emu") return MPG_PREC_VALUES_F16EMU;
    throw StatusError(MPG_ERR_ARG, "MPG_PREC_VALUES = " + v + " is not f32, f16 or f16emu");
}

const char* prec_values_name(int kind) {
    return kind == MPG_PREC_VALUES_F16 ? "f16" : kind == MPG_PREC_VALUES_F16EMU ? "f16emu" : "f32";
}

void check_prec_values_args(const mpg_solve_args& a, int kind, bool surface, bool ranks) {
    if (kind == MPG_PREC_VALUES_F32) return;
    const std::string name = std::string("prec_values ") + prec_values_name(kind);
    auto refuse = [&](const std::string& why) { throw StatusError(MPG_ERR_UNSUPPORTED, name + " " + why); };
    if (surface)
        refuse("is not available on the operator-surface engine: the sweeps on an fp16 copy of A are the fused "
               "engine's");
    if (ranks) refuse("is not available on a row-partitioned solve: the polynomial preconditioners are not either");
    const bool sweeps = (a.prec == MPG_PREC_NEUMANN && a.jacobi_steps > 1) || a.prec == MPG_PREC_CHEBYSHEV ||
                        a.prec == MPG_PREC_GMRES_POLY;
    if (!sweeps)
        refuse("needs a preconditioner that sweeps over A (prec neumann with two steps or more, chebyshev, "
               "gmres_poly): this one reads no copy of A's values in the sweeps' slot");
    if (a.mode != MPG_MODE_MIXED)
        refuse("runs in mode mixed only (fp32 sweeps beside an fp32 Arnoldi matrix and an fp64 residual)");
    if (kind == MPG_PREC_VALUES_F16EMU && a.spmv_format != 0 && a.spmv_format != 1)
        refuse("is built for the CSR row-block storage only (it exists for the tests): not SELL or node-block storage");
}

struct FusedEngine::Impl {
    mpg_ctx_t ctx = nullptr;
    mpg_solve_args args{};
    Comm* comm = nullptr;
    ModeTypes ty{};
    int n = 0, n_ext = 0, m = 0, orth = 0;
    int front = 0;       // MPG_FRONT_PAD(n_front): entries of x / x64 before row 0
    void* xp = nullptr;  // row 0 of x (x.p + front entries)
    int64_t nnz = 0;
    DevMem rowptr, col, val64, val_outer_own, val_inner_own, diag, b, x, tmp_t, tmp_p, scal;
    DevMem row_exp;                 // mixed-half: per-row exponents of the scaled fp16 values
    int64_t half_stats[4] = {0, 0, 0, 0};
    bool half_scaled = false;       // ... and the workspace runs the scaled kernels (chosen at create, kept for good)
    const void* val_outer = nullptr;
    const void* val_inner = nullptr;
    mpg_csr_t csr = nullptr;
    mpg_arnoldi_t arn = nullptr;
    double* rep[2] = {nullptr, nullptr};  // pinned report buffers (two: pipelined cycles)
    double* report_host = nullptr;       // = rep[0] or rep[1]: the report the host works on
    int report_len = 0;
    // pipelined cycles: the next cycle's graph is launched before this
    // cycle's report is read; it starts by saving x, so a cycle launched past
    // a stop decision is undone by restoring x
    DevMem x_snap;
    // arming (FusedEngine::arm): host fp64 vectors pass through stage64 where x
    // is not fp64; x_true is kept on the device for finish_report
    DevMem stage64, xt;
    bool have_xt = false;
    hipEvent_t report_ev[2] = {nullptr, nullptr};
    CyclePolicy pol{};      // what decides the cycle's launches (resolve_policy)
    std::vector<Op> cycle;  // plan_cycle(pol): the ops of one restart cycle
    CapturedGraph graph;    // ... captured (ensure_graph)
    void resolve_policy();
    bool step_dots_at(int k) const {  // step k runs the SpMV inside the dots' launch (mpg_arnoldi_step_dots)
        return std::any_of(cycle.begin(), cycle.end(), [k](const Op& o) { return o.kind == OpKind::StepDots && o.a == k; });
    }
    mpg_ilu_t ilu = nullptr;  // ILU(0) factors (prec ilu / ilu_jacobi), applied between phase kernels
    // block Jacobi (prec bjacobi): bs x bs inverses of the nodes' diagonal blocks in the
    // preconditioner precision (mpg_bjacobi_setup_*), applied by a launch of
    // its own in the slot ILU's solves take
    int bj_bs = 0;  // unknowns per node; 0: another preconditioner
    DevMem bj_dinv;
    // MPG_BJACOBI_FUSE=1: the Arnoldi SpMV / the residual prologue apply the
    // inverses themselves where the storage supports it (mpg_arnoldi_prec_fused:
    // node blocks, bs = 3; the same bits). Unset or 0: the launch of its own,
    // the faster form as measured -- C4 stand-in, mixed CGS: 454 us per step
    // against 540 fused (k_step_node_bj holds 80 VGPRs where k_step_node holds
    // 54: 6 waves per SIMD instead of 8), point Jacobi 451
    // (profiles/r08_bjacobi/bjacobi_bench.json)
    bool bj_fused_step = false, bj_fused_prologue = false;
    // Jacobi-sweep polynomial (prec neumann): nm_steps sweeps on A z = w from
    // z = 0 with Jacobi's inverse diagonal (`diag`), on the workspace's Arnoldi
    // matrix (mpg_arnoldi_neumann_apply), in the slot ILU's solves take.
    // One sweep is point Jacobi and runs as point Jacobi: the product inside
    // the SpMV and the prologue (nm_steps stays 0), so that it has prec jacobi's
    // bits in every class -- the launch of its own would sum the prologue's
    // ||w||^2 in prologue_wnorm's order, other last bits under an fp64 Arnoldi.
    int nm_steps = 0;   // sweeps applied between the phase kernels; 0: none (another preconditioner, or one sweep)
    int nm_asked = 0;   // jacobi_steps of prec neumann; 0: another preconditioner
    DevMem nm_work0, nm_work1;
    // Chebyshev polynomial (prec chebyshev): the same slot, vectors and counts
    // (nm_steps = nm_asked for every count: one step is Jacobi scaled by
    // 1 / theta, not jacobi's bits), through mpg_arnoldi_cheb_apply on the
    // interval read at set-up
    bool cheb = false;
    ChebInterval cheb_iv{};
    // GMRES polynomial (prec gmres_poly): again that slot and those vectors,
    // through mpg_arnoldi_poly_apply on the roots of the set-up (nm_steps =
    // nm_asked = their count, which an invariant subspace makes smaller than
    // jacobi_steps; one root is Jacobi scaled by 1 / theta)
    bool poly = false;
    PolyRoots poly_roots{};
    bool jacobi_inside() const { return args.prec == MPG_PREC_JACOBI || (nm_asked == 1 && !cheb && !poly); }
    int basis = MPG_BASIS_F32;  // the basis' storage (MPG_BASIS, read at create; mpg_arnoldi_set_basis)
    // The copy of A the sweeps read (MPG_PREC_VALUES, read at create;
    // mpg_arnoldi_set_prec_copy). f16: the row exponents and, where the Arnoldi
    // runs on a SELL copy, an MPG_F16 SELL copy, else the fp16 bits in CSR
    // order. f16emu: the dequantised fp32 values in CSR order. f32: nothing.
    int prec_values = MPG_PREC_VALUES_F32;
    DevMem pv_vals, pv_exp;
    mpg_sell_t pv_sell = nullptr;
    // the initial-guess store (FusedEngine::guess_*): g_L columns of capacity,
    // g_p held, panels of leading dimension g_ld (padded to 256 B like the
    // basis); nothing is allocated while g_L == 0
    int g_L = 0, g_p = 0;
    int64_t g_ld = 0;
    bool g_stale = false;  // refresh_values changed A: Q is no longer A Z
    DevMem g_Z, g_Q, g_w, g_d, g_r, g_part, g_info;
    bool orthloss = false;    // LostOrthogonality: v_{k+1} stored each step, S / u below
    DevMem loss_S, loss_u;    // (m+1) x (m+1) and m+2 of T, zero-filled (IterUtil.hpp:185-191)

    ~Impl() {
        if (ilu) mpg_ilu_destroy(ilu);
        if (arn) mpg_arnoldi_destroy(arn);
        if (pv_sell) mpg_sell_destroy(pv_sell);
        if (csr) mpg_csr_destroy(csr);
        for (double* r : rep)
            if (r) (void)hipHostFree(r);
        for (hipEvent_t e : report_ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipStream_t stream() const { return static_cast<hipStream_t>(mpg_ctx_stream(ctx)); }

    // cast-copy between device arrays of runtime dtypes
    void cast(const void* src, int st, void* dst, int dt, int64_t count) {
        if (count == 0) return;
        if (st == MPG_F64 && dt == MPG_F64) check(mpg_copy_f64f64(ctx, count, (const double*)src, (double*)dst), "copy", ctx);
        else if (st == MPG_F64 && dt == MPG_F32) check(mpg_copy_f64f32(ctx, count, (const double*)src, (float*)dst), "copy", ctx);
        else if (st == MPG_F32 && dt == MPG_F64) check(mpg_copy_f32f64(ctx, count, (const float*)src, (double*)dst), "copy", ctx);
        else if (st == MPG_F32 && dt == MPG_F32) check(mpg_copy_f32f32(ctx, count, (const float*)src, (float*)dst), "copy", ctx);
        else if (st == MPG_F64 && dt == MPG_F16) check(mpg_copy_f64f16(ctx, count, (const double*)src, (uint16_t*)dst), "copy", ctx);
        else throw std::invalid_argument("unsupported cast");
    }
    // fp64 accumulator of <u, v> over local rows, summed across ranks
    double dot_acc(const void* u, const void* v, int t, int64_t count) {
        double* acc = scal.as<double>();
        if (t == MPG_F64) check(mpg_dot_acc_f64(ctx, count, (const double*)u, (const double*)v, acc), "dot", ctx);
        else check(mpg_dot_acc_f32(ctx, count, (const float*)u, (const float*)v, acc), "dot", ctx);
        if (comm) comm->allreduce_sum(acc, 1, stream());
        double h = 0;
        check(mpg_memcpy_d2h(ctx, &h, acc, sizeof h), "d2h", ctx);
        return h;
    }
    // x <- Dinv x on a vector of T (the casts to and from P inside the launch)
    void apply_bjacobi(void* w) {
        int st;
        if (ty.T == MPG_F32) st = mpg_bjacobi_apply_f32(ctx, n, bj_bs, bj_dinv.as<float>(), (float*)w);
        else if (ty.P == MPG_F64) st = mpg_bjacobi_apply_f64(ctx, n, bj_bs, bj_dinv.as<double>(), (double*)w);
        else st = mpg_bjacobi_apply_f64_p32(ctx, n, bj_bs, bj_dinv.as<float>(), (double*)w);
        check(st, "block Jacobi apply", ctx);
    }
    // M^-1 w for the preconditioners applied between the phase kernels: block
    // Jacobi, the Jacobi sweeps, or ILU with typesafe_apply's casts when the preconditioner
    // precision differs (gmres.cpp:12-22)
    void apply_neumann(void* w) {
        if (poly)
            return check(mpg_arnoldi_poly_apply(arn, poly_roots.count, poly_roots.re, poly_roots.im, w, nm_work0.p,
                                                nm_work1.p),
                         "GMRES-polynomial apply", ctx);
        if (cheb)
            return check(mpg_arnoldi_cheb_apply(arn, nm_steps, cheb_iv.theta(), cheb_iv.delta(), w, nm_work0.p,
                                                nm_work1.p),
                         "Chebyshev apply", ctx);
        check(mpg_arnoldi_neumann_apply(arn, nm_steps, w, nm_work0.p, nm_work1.p), "Jacobi-sweep apply", ctx);
    }
    void apply_ilu(void* w) {
        if (bj_bs) return apply_bjacobi(w);
        if (nm_steps) return apply_neumann(w);
        void* wp = w;
        if (ty.P != ty.T) {
            cast(w, ty.T, tmp_p.p, ty.P, n);
            wp = tmp_p.p;
        }
        solve_ilu(wp);
        if (ty.P != ty.T) cast(tmp_p.p, ty.P, w, ty.T, n);
    }
    void solve_ilu(void* wp) {
        if (args.prec == MPG_PREC_ILU) check(mpg_ilu_solve(ctx, ilu, wp), "ilusv", ctx);
        else check(mpg_ilu_jacobi_solve(ctx, ilu, args.jacobi_steps, wp), "ilusv_jacobi", ctx);
    }
    // nrm2 rounded to the vector's precision
    double nrm2(const void* u, int t, int64_t count) {
        const double s = std::sqrt(dot_acc(u, u, t, count));
        return t == MPG_F64 ? s : (double)(float)s;
    }
};

// What decides the cycle's launches, read once: the environment, the ranks,
// the preconditioner and what the workspace supports (mpg_cycle_policy, solve.h).
void FusedEngine::Impl::resolve_policy() {
    CyclePolicy& P = pol;
    P.ranks = comm ? comm->size() : 0;
    P.orth = orth;
    P.m = m;
    P.sep_prec = ilu || bj_bs || nm_steps;  // a preconditioner applied between the phase kernels, not inside them
    P.sep_prec_step = ilu || (bj_bs && !bj_fused_step) || nm_steps;
    P.sep_prec_prologue = ilu || (bj_bs && !bj_fused_prologue) || nm_steps;
    P.partials_max_cols = mpg_arnoldi_partials_max_cols();
    P.fold_max_m = mpg_arnoldi_fold_max_m();
    for (int k = 0; k < std::min(m, MPG_CYCLE_POLICY_STEPS); ++k) {
        P.step_dots_ok[k] = mpg_arnoldi_step_dots_supported(arn, k) == MPG_OK;
        P.spmv_dots_ok[k] = mpg_arnoldi_spmv_dots_supported(arn, k) == MPG_OK;
    }
    // the first character of a setting; 0: unset or empty
    auto env = [](const char* name) { const char* v = std::getenv(name); return v ? *v : '\0'; };
    // A compressed or emulated basis takes the plain launches, as under
    // MPG_STEP_DOTS=0 MPG_CGS_PREFETCH=0 MPG_TAIL_FOLD=0 whatever those say:
    // the workspace reports none of the fused forms as supported
    // (mpg_arnoldi_set_basis), so the plan below holds none. Asking for one
    // of them is an error, not a silent fall-back.
    const bool plain_only = basis != MPG_BASIS_F32;
    if (plain_only) {
        const char* asked = env("MPG_STEP_DOTS") == '2'      ? "MPG_STEP_DOTS=2"
                            : env("MPG_FUSE_DOTS") == '2'    ? "MPG_FUSE_DOTS=2"
                            : env("MPG_FUSE_DOTS") == '1'    ? "MPG_FUSE_DOTS=1"
                            : env("MPG_CGS_PREFETCH") == '1' ? "MPG_CGS_PREFETCH=1"
                            : env("MPG_TAIL_FOLD") == '1'    ? "MPG_TAIL_FOLD=1"
                            : env("MPG_COMBINE") == '1'      ? "MPG_COMBINE=1"
                                                             : nullptr;
        if (asked)
            throw StatusError(MPG_ERR_UNSUPPORTED, std::string("basis ") + basis_name(basis) + ": " + asked +
                                                       " asks for a fused launch form, which reads an fp32 basis; "
                                                       "the compressed basis runs the plain forms only");
    }
    P.pipeline = env("MPG_PIPELINE") != '0';  // 0: read each cycle's report before the next launch
    P.graph = env("MPG_NO_GRAPH") != '1' && (!comm || comm->capturable());
    // Givens(k-1) is folded into SpMV(k) by default (MPG_FOLD_GIVENS=0: its
    // own launch): every SpMV workgroup sums the 256 ||w||^2 partials of the
    // 1024-thread CGS update itself (+1.9 us per SpMV, -4.6 us Givens launch
    // and its boundary: 19.3k vs 18.7k it/s on BAND-10M). Experiments, off:
    // MPG_COMBINE=1 (one GPU, CGS/CGSR) does last-arriver combines in the dots
    // and CGS launches: 15.1k it/s (1024 tickets on one counter serialise).
    // One GPU, by default (MPG_CGS_PARTIALS=0: off): every CGS workgroup sums
    // the 256 dots partials per column itself (8 branch-free loads per lane,
    // one latency) instead of the reduce launch: 21.6k vs 21.1k it/s on
    // BAND-10M (tools/ab_bench.sh, 4 interleaved runs each).
    P.combine = !comm && env("MPG_COMBINE") == '1' && orth != MPG_ORTH_MGS && m <= P.fold_max_m;
    // (CGSR's first pass also emits the next dots: its in-launch form is the
    // older runtime-count kernel, slower than reduce + update; on only with =1)
    // (ranks: the dots' partials are all-reduced in place first, so the
    // update still sums them itself -- no reduce launch per step)
    P.cgs_partials = !P.combine && orth != MPG_ORTH_MGS &&
                     (orth == MPG_ORTH_CGSR ? env("MPG_CGS_PARTIALS") == '1' && !plain_only  // (the runtime-count kernel)
                                            : env("MPG_CGS_PARTIALS") != '0');
    // MPG_FUSE_DOTS=1: the panel dots inside the SELL SpMV launch (SellDots)
    // (=2: required -- an error where the storage does not support it; tests)
    const char denv = env("MPG_FUSE_DOTS");
    P.fuse_dots = P.cgs_partials && orth == MPG_ORTH_CGS && (denv == '1' || denv == '2');
    P.fuse_dots_required = P.fuse_dots && denv == '2';
    // MPG_FUSE_DOTS_K0=K: fuse only the steps with k + 1 <= K (the first
    // steps, whose per-row basis loads are few; VERDICT r3 item 5's policy)
    const char* kenv = std::getenv("MPG_FUSE_DOTS_K0");
    P.fuse_dots_k0 = kenv && *kenv ? std::max(0, std::min(32, std::atoi(kenv))) : 32;
    // MPG_STEP_DOTS: the SpMV inside the panel dots' launch (k_step_dots).
    // 0 never, 1 wherever the launch is supported, 2 required (an unsupported
    // step is an error; tests); unset: the steps with kStepDotsLo <= k + 1 <=
    // kStepDotsHi, where the one launch measured faster than the two on
    // BAND-10M in the fp32 accumulation class, the only one it is built for
    // (profiles/r07_step_dots/). MPG_STEP_DOTS_LO / _HI move the range.
    const char senv = env("MPG_STEP_DOTS");
    P.step_dots = senv >= '0' && senv <= '2' ? senv - '0' : -1;
    const char* lo = std::getenv("MPG_STEP_DOTS_LO");
    const char* hi = std::getenv("MPG_STEP_DOTS_HI");
    P.step_dots_lo = lo && *lo ? std::atoi(lo) : kStepDotsLo;
    P.step_dots_hi = hi && *hi ? std::atoi(hi) : kStepDotsHi;
    // MPG_FOLD_GIVENS: 0 never, 1 always (m permitting), unset: where it pays
    // (mpg_arnoldi_fold_pays: up to ~4k SpMV workgroups)
    const char fenv = env("MPG_FOLD_GIVENS");
    bool fold_on = fenv ? fenv != '0' : mpg_arnoldi_fold_pays(arn) != 0;
    if (comm && !fenv) {
        // ranks of one solve must run the same collective sequence (a folding
        // rank all-reduces the ||w||^2 partials with the halo, a non-folding
        // one reduces + all-reduces one sum after it): every rank's row block
        // and SELL layout differ, so the fold is taken only if it pays on
        // EVERY rank (all-reduce max of "does not pay")
        double* flag = scal.as<double>() + 6;
        const double no = fold_on ? 0.0 : 1.0;
        check(mpg_memcpy_h2d(ctx, flag, &no, sizeof no), "h2d", ctx);
        comm->allreduce_max(flag, 1, stream());
        double any_no = 0;
        check(mpg_memcpy_d2h(ctx, &any_no, flag, sizeof any_no), "d2h", ctx);
        fold_on = any_no == 0.0;
    }
    P.fold = !P.combine && fold_on && m <= P.fold_max_m;
    // MPG_TAIL_FOLD: the last Givens step, update(m) and the x snapshot in
    // the one givens+update launch, where the workspace builds it (one GPU,
    // m <= 32). 0 never, 1 wherever built; unset: in the fp32 accumulation
    // class, where it was measured (BAND-10M, profiles/r13_cycle_tail/) and
    // the columns stream through LDS; the fp64 class keeps the launches it had.
    const char tenv = env("MPG_TAIL_FOLD");
    const bool tail_on = tenv ? tenv != '0' : mpg_arnoldi_accum(arn) == MPG_ACCUM_F32;
    P.tail_fold = !comm && tail_on && mpg_arnoldi_update_tail_supported(arn) == MPG_OK;
    if (int st = plan_cycle(P, cycle))
        throw StatusError(st, "MPG_STEP_DOTS=2 / MPG_FUSE_DOTS=2: a step of the cycle cannot take the required SpMV + "
                              "dots launch (one GPU, plain CGS with in-launch sums, no preconditioner launch -- ILU, "
                              "block Jacobi, Jacobi, Chebyshev or GMRES-polynomial sweeps -- between the SpMV and the dots, storage the "
                              "launch supports)");
}

FusedEngine::FusedEngine(mpg_ctx_t ctx, const mpg_solve_args& a, Comm* comm, int n_ext, int n_front, const double* x0)
    : p_(new Impl) {
    auto t0 = clk::now();
    Impl& I = *p_;
    I.ctx = ctx;
    I.args = a;
    I.comm = comm;
    I.ty = types_for(a.mode);
    I.n = a.n;
    I.n_ext = n_ext < 0 ? a.n : n_ext;
    if (n_front < 0) throw std::invalid_argument("n_front < 0");
    I.front = MPG_FRONT_PAD(n_front);
    I.m = a.rlen;
    I.orth = a.orth;
    I.nnz = a.nnz;
    I.basis = basis_setting();
    check_basis_args(a, I.basis, false, comm != nullptr);
    I.prec_values = prec_values_setting();
    check_prec_values_args(a, I.prec_values, false, comm != nullptr);
    const bool ilu = a.prec == MPG_PREC_ILU || a.prec == MPG_PREC_ILU_JACOBI;
    if (ilu && comm)
        throw std::invalid_argument("ILU / ILU-Jacobi factor the whole matrix: not available on a row-partitioned solve");
    const bool bjacobi = a.prec == MPG_PREC_BLOCK_JACOBI;
    const bool chebyshev = a.prec == MPG_PREC_CHEBYSHEV;
    const bool gmres_poly = a.prec == MPG_PREC_GMRES_POLY;
    const bool neumann = a.prec == MPG_PREC_NEUMANN || chebyshev || gmres_poly;  // (the sweeps' set-up, whichever polynomial)
    if (!ilu && !bjacobi && !neumann && a.prec != MPG_PREC_IDENTITY && a.prec != MPG_PREC_JACOBI)
        throw std::invalid_argument("Unknown prec type");
    if (neumann) {
        gmres_poly ? check_gmres_poly_args(a) : chebyshev ? check_cheb_args(a) : check_neumann_args(a);
        if (comm)
            throw StatusError(MPG_ERR_UNSUPPORTED,
                              std::string("prec ") + (gmres_poly ? "gmres_poly" : chebyshev ? "chebyshev" : "neumann") +
                                  " is not available on a row-partitioned solve: every sweep needs a halo "
                                  "exchange of z (the follow-up that would make it the first preconditioner stronger "
                                  "than Jacobi on more than one GPU)");
        I.cheb = chebyshev;
        I.poly = gmres_poly;
        I.nm_asked = a.jacobi_steps;
        I.nm_steps = a.jacobi_steps > 1 || chebyshev || gmres_poly ? a.jacobi_steps : 0;
    }
    if (bjacobi) {
        const int bs = a.prec_block == 0 ? 3 : a.prec_block;
        if (bs < 2 || bs > 4) throw std::invalid_argument("prec bjacobi: prec_block must be 2, 3 or 4 (0: 3)");
        if (comm)
            throw std::invalid_argument("prec bjacobi is not available on a row-partitioned solve (a rank's diagonal "
                                        "blocks are not set up across the partition)");
        if (a.n % bs != 0)
            throw std::invalid_argument("prec bjacobi: n = " + std::to_string(a.n) + " is not a multiple of the block size " +
                                        std::to_string(bs));
        I.bj_bs = bs;
    }
    I.orthloss = a.orthloss && a.rtol != 0 && !a.repeat_iter;  // alloc_convergence order (gmres_perf_test.cpp:184-195)
    if (I.orthloss && comm)
        throw std::invalid_argument("LostOrthogonality restarts are not available on a row-partitioned solve");
    if (a.rowptr[a.n] != a.nnz) throw std::invalid_argument("rowptr[n] != nnz");

    // structure + analysed schedule
    const size_t n1 = (size_t)I.n + 1, nz = (size_t)I.nnz;
    I.rowptr = DevMem(ctx, n1 * 4);
    I.col = DevMem(ctx, std::max<size_t>(nz, 1) * 4);
    check(mpg_memcpy_h2d(ctx, I.rowptr.p, a.rowptr, n1 * 4), "h2d", ctx);
    if (nz) check(mpg_memcpy_h2d(ctx, I.col.p, a.col, nz * 4), "h2d", ctx);
    check(mpg_csr_create(ctx, I.n, I.n_ext, I.nnz, a.rowptr, I.rowptr.as<int32_t>(), I.col.as<int32_t>(), &I.csr),
          "mpg_csr_create", ctx);

    // everything that reads the values (load_values: a values refresh comes through it again)
    I.scal = DevMem(ctx, 64);
    I.tmp_t = DevMem(ctx, (size_t)I.n * dsize(I.ty.T) + 64);
    if (I.ty.P != I.ty.T) I.tmp_p = DevMem(ctx, (size_t)I.n * dsize(I.ty.P) + 64);
    load_values(a.val, false);
    const ModeTypes& ty = I.ty;

    // b and x (outer type, x with halo tail), the work vectors of the arm
    // (tmp_t: T(b), tmp_p: typesafe_apply's P copy, above); their values are arm()'s
    I.b = DevMem(ctx, (size_t)I.n * dsize(ty.X) + 8);
    if (ty.X != MPG_F64) I.stage64 = DevMem(ctx, (size_t)I.n * 8 + 8);
    I.x = DevMem(ctx, (size_t)(I.front + I.n_ext) * dsize(ty.X) + 64);
    I.xp = static_cast<char*>(I.x.p) + (size_t)I.front * dsize(ty.X);

    mpg_arnoldi_desc d{};
    d.n = I.n;
    d.n_ext = I.n_ext;
    d.m = I.m;
    d.orth = I.orth;
    d.vec_type = ty.T;
    d.outer_type = ty.X;
    d.prec_type = ty.P;
    d.inner_val = ty.VI;
    d.jacobi = I.jacobi_inside();
    d.A = I.csr;
    d.val_outer = I.val_outer;
    d.val_inner = I.val_inner;
    // (the sweeps' diagonal rides in the descriptor with jacobi = 0: the phase
    // kernels apply no preconditioner, mpg_arnoldi_neumann_apply reads it)
    d.diag = d.jacobi || neumann ? I.diag.p : nullptr;
    d.b = I.b.p;
    d.x = I.xp;
    d.spmv_format = a.spmv_format;
    // a compressed basis: auto picks among CSR row blocks and the SELL copy
    // (no node blocks); the emulated one is built for the CSR kernel
    if (I.basis != MPG_BASIS_F32 && a.spmv_format == 0) d.spmv_format = I.basis == MPG_BASIS_F16EMU ? 1 : 4;
    if (I.prec_values == MPG_PREC_VALUES_F16EMU) d.spmv_format = 1;  // (auto or csr: check_prec_values_args)
    d.n_front = n_front;
    {
        const char* benv = std::getenv("MPG_BJACOBI_FUSE");
        if (I.bj_bs && benv && *benv == '1') {
            d.block_dinv = I.bj_dinv.p;
            d.prec_block = I.bj_bs;
        }
    }
    // rows all in range: the unscaled kernels (no exponent loads, same bits)
    I.half_scaled = I.half_stats[0] > 0;
    d.inner_row_exp = I.half_scaled ? I.row_exp.as<int8_t>() : nullptr;
    check(mpg_arnoldi_create(ctx, &d, &I.arn), "mpg_arnoldi_create", ctx);
    I.bj_fused_step = mpg_arnoldi_prec_fused(I.arn, 0) == 1;
    I.bj_fused_prologue = mpg_arnoldi_prec_fused(I.arn, 1) == 1;
    // fp32 Arnoldi: the reference's fp32 accumulation class on request (arnoldi.h)
    if (a.accum) check(mpg_arnoldi_set_accum(I.arn, MPG_ACCUM_F32), "mpg_arnoldi_set_accum", ctx);
    if (I.basis != MPG_BASIS_F32) check(mpg_arnoldi_set_basis(I.arn, I.basis), "mpg_arnoldi_set_basis", ctx);
    if (I.prec_values == MPG_PREC_VALUES_F16) {
        // the storage form of the Arnoldi SpMV decides the sweeps': a SELL copy
        // of the fp16 bits beside a SELL Arnoldi matrix (load_values left the
        // bits in pv_vals for it; the copy owns its own), else the bits in CSR order
        int32_t fmt = 0;
        check(mpg_arnoldi_spmv_layout(I.arn, &fmt, nullptr, nullptr, nullptr, nullptr), "layout", ctx);
        if (fmt == 2) {
            check(mpg_sell_create(ctx, I.csr, MPG_F16, I.pv_vals.p, 2, &I.pv_sell), "fp16 SELL copy for the sweeps", ctx);
            check(mpg_ctx_sync(ctx), "sync", ctx);
            I.pv_vals = DevMem();
        }
        check(mpg_arnoldi_set_prec_copy(I.arn, I.prec_values, I.pv_sell ? nullptr : I.pv_vals.p, I.pv_exp.as<int8_t>(),
                                        I.pv_sell),
              "mpg_arnoldi_set_prec_copy", ctx);
    } else if (I.prec_values == MPG_PREC_VALUES_F16EMU) {
        check(mpg_arnoldi_set_prec_copy(I.arn, I.prec_values, I.pv_vals.p, nullptr, nullptr),
              "mpg_arnoldi_set_prec_copy", ctx);
    }
    // (the GMRES polynomial: for the asked degree, so that the root count of refreshed values fits)
    const int nm_cap = I.poly ? a.jacobi_steps : I.nm_steps;
    if (nm_cap >= 2) I.nm_work0 = DevMem(ctx, (size_t)I.n * dsize(ty.T) + 64);
    if (nm_cap >= 3) I.nm_work1 = DevMem(ctx, (size_t)I.n * dsize(ty.T) + 64);
    // ranks all-reduce per-workgroup partials in place: same count on every rank
    // (MPG_UNIFORM_GROUPS=1 gives one GPU the ranks' partial counts: a P = 1
    // RCCL solve then has the single-GPU solve's bits, tests/test_dist_gpu.py)
    const char* uenv = std::getenv("MPG_UNIFORM_GROUPS");
    if (comm || (uenv && *uenv == '1')) check(mpg_arnoldi_uniform_groups(I.arn), "uniform groups", ctx);
    I.report_len = mpg_arnoldi_report_len(I.arn);
    for (double*& r : I.rep) hipck(hipHostMalloc((void**)&r, (size_t)I.report_len * sizeof(double), 0), "hipHostMalloc");
    I.report_host = I.rep[0];
    for (hipEvent_t& e : I.report_ev) hipck(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");

    if (I.orthloss) {
        const size_t mm = (size_t)a.rlen;
        I.loss_S = DevMem(ctx, (size_t)(mm + 1) * (mm + 1) * dsize(ty.T));
        I.loss_u = DevMem(ctx, (size_t)(mm + 2) * dsize(ty.T));
    }
    breakdown.stop = a.stop_on_breakdown != 0;

    I.resolve_policy();
    if (I.pol.pipeline) I.x_snap = DevMem(ctx, I.x.bytes);
    if (I.pol.pipeline && tail_fold())
        check(mpg_arnoldi_set_x_snapshot(I.arn, static_cast<char*>(I.x_snap.p) + (size_t)I.front * dsize(I.ty.X)),
              "x snapshot", ctx);
    arm(a.b, x0, a.x_true, 0);
    check(mpg_ctx_sync(ctx), "sync", ctx);
    setup_seconds = std::chrono::duration<double>(clk::now() - t0).count();
    start();
}

namespace {
const char* const kMeasuredText =
    "the engine ran measurement launches (mpg_engine_time_*), which change its Krylov basis, "
    "Hessenberg column and iterate; create a new engine to continue a solve";
}

// Everything the set-up derives from the values of A, from fp64 values in CSR
// order (host memory, or the engine's device): the fp64 copy, the residual
// and the Arnoldi matrix in their types, Jacobi's diagonal, the Chebyshev
// interval, the GMRES-polynomial roots, the block-Jacobi inverses, the ILU
// factors and ||A||_F. The constructor and refresh_values() both come through
// here, so a refreshed engine runs a new engine's launches on a new engine's
// numbers. On a live engine (the workspace exists) no buffer moves, the
// workspace's storage copies are refilled (mpg_arnoldi_refresh_values) and a
// captured cycle whose launch arguments changed is released. It reads none of
// args' pointers: they are the caller's of create time and may be gone.
void FusedEngine::load_values(const double* val, bool on_device) {
    Impl& I = *p_;
    const mpg_ctx_t ctx = I.ctx;
    const mpg_solve_args& a = I.args;  // (its scalars only)
    const ModeTypes& ty = I.ty;
    Comm* const comm = I.comm;
    const size_t nz = (size_t)I.nnz, nz1 = std::max<size_t>(nz, 1);
    const bool live = I.arn != nullptr;
    const bool ilu = a.prec == MPG_PREC_ILU || a.prec == MPG_PREC_ILU_JACOBI;
    const bool neumann = a.prec == MPG_PREC_NEUMANN || I.cheb || I.poly;
    auto need = [&](DevMem& m, size_t bytes) {
        if (!m.p) m = DevMem(ctx, bytes);
    };
    const bool rounded_outer = a.mode != MPG_MODE_MIXED && a.mode != MPG_MODE_MIXED_HALF;
    const bool half = !rounded_outer && ty.VI == MPG_F16;
    const bool scale = a.half_unscaled == 0;

    // A live mixed-half engine chose scaled or unscaled kernels when it was
    // created: the fp16 conversion of the new values goes into scratch first,
    // and values the engine's kernels cannot take are refused with the old
    // matrix untouched
    DevMem staged, half_new, exp_new;
    int64_t stats_new[4] = {0, 0, 0, 0};
    if (live && half) {
        if (!on_device) {
            staged = DevMem(ctx, nz1 * 8);
            if (nz) check(mpg_memcpy_h2d(ctx, staged.p, val, nz * 8), "h2d", ctx);
            val = staged.as<double>();
            on_device = true;
        }
        half_new = DevMem(ctx, nz1 * 2);
        if (scale) exp_new = DevMem(ctx, (size_t)I.n + 64);
        const int st = mpg_csr_half_values(ctx, I.csr, val, scale ? 1 : 0, half_new.as<uint16_t>(),
                                           scale ? exp_new.as<int8_t>() : nullptr, stats_new);
        if (st == MPG_ERR_RANGE)
            throw StatusError(MPG_ERR_RANGE,
                              "mixed-half: the new values do not fit the fp16 Arnoldi copy (" +
                                  std::to_string(stats_new[2]) + " entries overflow, " + std::to_string(stats_new[1]) +
                                  " round to 0" + (scale ? "" : " under half_unscaled") +
                                  "); the engine keeps its matrix");
        check(st, "fp16 Arnoldi values", ctx);
        if (!I.half_scaled && stats_new[0] > 0)
            throw StatusError(MPG_ERR_UNSUPPORTED,
                              "mixed-half: " + std::to_string(stats_new[0]) +
                                  " rows of the new values need row scaling, and this engine was created on values "
                                  "that needed none, with the unscaled kernels; the engine keeps its matrix -- create "
                                  "a new engine for these values");
    }
    // The sweeps' fp16 copy (prec_values): converted into scratch first too,
    // and refused with the old matrix untouched when an entry does not fit --
    // fp16 after the row scaling, the int8 exponent, or fp32 once unscaled
    DevMem pv_half, pv_exp_new;
    if (I.prec_values != MPG_PREC_VALUES_F32) {
        if (!on_device) {
            staged = DevMem(ctx, nz1 * 8);
            if (nz) check(mpg_memcpy_h2d(ctx, staged.p, val, nz * 8), "h2d", ctx);
            val = staged.as<double>();
            on_device = true;
        }
        pv_half = DevMem(ctx, nz1 * 2);
        pv_exp_new = DevMem(ctx, (size_t)I.n + 64);
        int64_t st4[4] = {0, 0, 0, 0}, bad = 0;
        const std::string name = std::string("prec_values ") + prec_values_name(I.prec_values);
        const int st = mpg_csr_half_values(ctx, I.csr, val, 1, pv_half.as<uint16_t>(), pv_exp_new.as<int8_t>(), st4);
        if (st == MPG_ERR_RANGE)
            throw StatusError(MPG_ERR_RANGE, name + ": the values do not fit the sweeps' fp16 copy (" +
                                                 std::to_string(st4[2]) + " entries overflow, " +
                                                 std::to_string(st4[3]) + " row exponents outside int8)" +
                                                 (live ? "; the engine keeps its matrix" : ""));
        check(st, "fp16 values for the sweeps", ctx);
        check(mpg_csr_half_dequant_f32(ctx, I.csr, pv_half.as<uint16_t>(), pv_exp_new.as<int8_t>(), nullptr, &bad),
              "fp16 values for the sweeps", ctx);
        if (bad)
            throw StatusError(MPG_ERR_RANGE, name + ": " + std::to_string(bad) +
                                                 " entries of the sweeps' fp16 copy overflow fp32 once unscaled" +
                                                 (live ? "; the engine keeps its matrix" : ""));
    }
    values_dirty_ = live;  // from here on a failure leaves a live engine without a consistent matrix

    // values: the original fp64 A, the residual matrix (outer type) and the
    // Arnoldi matrix (inner type) — gmres_perf_test.cpp:66 (baseline solves with
    // double(float(A))) and :136 (mixed: fp64 residual, fp32 Arnoldi)
    need(I.val64, nz1 * 8);
    if (nz && on_device) check(mpg_memcpy_d2d(ctx, I.val64.p, val, nz * 8), "d2d", ctx);
    else if (nz) check(mpg_memcpy_h2d(ctx, I.val64.p, val, nz * 8), "h2d", ctx);
    if (rounded_outer) {
        if (ty.X == MPG_F64) {
            DevMem f32(ctx, nz1 * 4);
            I.cast(I.val64.p, MPG_F64, f32.p, MPG_F32, (int64_t)nz);
            need(I.val_outer_own, nz1 * 8);
            I.cast(f32.p, MPG_F32, I.val_outer_own.p, MPG_F64, (int64_t)nz);
        } else {
            need(I.val_outer_own, nz1 * 4);
            I.cast(I.val64.p, MPG_F64, I.val_outer_own.p, MPG_F32, (int64_t)nz);
        }
        I.val_outer = I.val_outer_own.p;
        I.val_inner = I.val_outer;  // the same matrix drives the Arnoldi cycle
    } else {
        I.val_outer = I.val64.p;
        need(I.val_inner_own, nz1 * dsize(ty.VI));
        if (half && live) {
            if (nz) check(mpg_memcpy_d2d(ctx, I.val_inner_own.p, half_new.p, nz * 2), "d2d", ctx);
            // (a scaled engine takes any exponents: all zero gives the unscaled bits)
            if (I.half_scaled) check(mpg_memcpy_d2d(ctx, I.row_exp.p, exp_new.p, (size_t)I.n), "d2d", ctx);
            std::copy(stats_new, stats_new + 4, I.half_stats);
        } else if (half) {
            // fp16 values, scaled per row by powers of two where a row's
            // magnitude falls outside fp16's range (mpg_csr_half_values);
            // with a.half_unscaled such a matrix fails here (MPG_ERR_RANGE)
            if (scale) I.row_exp = DevMem(ctx, (size_t)I.n + 64);
            check(mpg_csr_half_values(ctx, I.csr, I.val64.as<double>(), scale ? 1 : 0,
                                      I.val_inner_own.as<uint16_t>(), scale ? I.row_exp.as<int8_t>() : nullptr,
                                      I.half_stats),
                  "fp16 Arnoldi values", ctx);
        } else {
            I.cast(I.val64.p, MPG_F64, I.val_inner_own.p, ty.VI, (int64_t)nz);
        }
        // a row whose own range exceeds fp16's (~2^39 below its largest
        // entry) loses its smallest entries to 0 even when scaled: not an
        // error (the plain cast's MPG_ERR_RANGE case), but said
        if (half && I.half_stats[1] > 0 && a.verbose)
            std::fprintf(stderr,
                         "mpgmres: mixed-half: %lld nonzero entries rounded to 0 in the fp16 Arnoldi copy "
                         "(rows spanning more than fp16's range; %lld rows scaled)\n",
                         (long long)I.half_stats[1], (long long)I.half_stats[0]);
        I.val_inner = I.val_inner_own.p;
    }

    // the sweeps' copy, in place on a live engine: the exponents; the bits in
    // CSR order (f16 without a SELL copy, which is refilled from the scratch
    // below) or the dequantised values (f16emu)
    if (I.prec_values != MPG_PREC_VALUES_F32) {
        need(I.pv_exp, (size_t)I.n + 64);
        if (I.n) check(mpg_memcpy_d2d(ctx, I.pv_exp.p, pv_exp_new.p, (size_t)I.n), "d2d", ctx);
        if (I.prec_values == MPG_PREC_VALUES_F16EMU) {
            int64_t bad = 0;
            need(I.pv_vals, nz1 * 4);
            check(mpg_csr_half_dequant_f32(ctx, I.csr, pv_half.as<uint16_t>(), I.pv_exp.as<int8_t>(),
                                           I.pv_vals.as<float>(), &bad),
                  "fp16 values for the sweeps", ctx);
        } else if (!I.pv_sell) {
            need(I.pv_vals, nz1 * 2);
            if (nz) check(mpg_memcpy_d2d(ctx, I.pv_vals.p, pv_half.p, nz * 2), "d2d", ctx);
        }
    }

    // Jacobi<P>(A): fp64 original A for P = double (baseline), else the A
    // converted to float (types.hpp:393-431 on SparseMatrix<P>)
    // (max row sum all-reduced across ranks: ||A||_inf of the whole matrix)
    if (a.prec == MPG_PREC_JACOBI || neumann) {
        need(I.diag, (size_t)I.n * dsize(ty.P) + 16);
        double* rowmax = I.scal.as<double>() + 4;
        if (ty.P == MPG_F64) {
            check(mpg_jacobi_rowmax_f64(ctx, I.csr, I.val64.as<double>(), rowmax), "jacobi", ctx);
            if (comm) comm->allreduce_max(rowmax, 1, I.stream());
            check(mpg_jacobi_diag_f64(ctx, I.csr, I.val64.as<double>(), rowmax, I.diag.as<double>()), "jacobi", ctx);
        } else {
            DevMem f32(ctx, std::max<size_t>(nz, 1) * 4);
            I.cast(I.val64.p, MPG_F64, f32.p, MPG_F32, (int64_t)nz);
            check(mpg_jacobi_rowmax_f32(ctx, I.csr, f32.as<float>(), rowmax), "jacobi", ctx);
            if (comm) comm->allreduce_max(rowmax, 1, I.stream());
            check(mpg_jacobi_diag_f32(ctx, I.csr, f32.as<float>(), rowmax, I.diag.as<float>()), "jacobi", ctx);
            check(mpg_ctx_sync(ctx), "sync", ctx);
        }
    }

    if (I.cheb) {
        // the interval, from the Gershgorin bound of D A on the matrix the sweeps run on (P = T = its value type)
        I.cheb_iv = cheb_interval([&] {
            double bound = 0.0;
            check(ty.P == MPG_F64 ? mpg_csr_jacobi_bound_f64(ctx, I.csr, static_cast<const double*>(I.val_inner),
                                                             I.diag.as<double>(), &bound)
                                  : mpg_csr_jacobi_bound_f32(ctx, I.csr, static_cast<const float*>(I.val_inner),
                                                             I.diag.as<float>(), &bound),
                  "Gershgorin bound", ctx);
            return bound;
        });
        double al[64], be[64];
        cheb_coefficients(I.nm_steps, I.cheb_iv, al, be);  // (refused here, not at the first application)
    }

    if (I.poly) {
        // the roots, from the Arnoldi steps on D A with the matrix the sweeps run on (P = T = its value type)
        I.poly_roots = ty.P == MPG_F64
                           ? gmres_poly_setup<double>(ctx, I.csr, static_cast<const double*>(I.val_inner),
                                                      I.diag.as<double>(), I.n, a.jacobi_steps)
                           : gmres_poly_setup<float>(ctx, I.csr, static_cast<const float*>(I.val_inner),
                                                     I.diag.as<float>(), I.n, a.jacobi_steps);
        // (a refresh may change the count, always >= 1. The cycle policy reads
        // nm_steps only as "a preconditioner launch sits between the phase
        // kernels" -- sep_prec* in resolve_policy, true for every count -- and
        // jacobi_inside() is false under poly whatever nm_asked says, so the
        // plan made at create holds; the count itself is an argument of
        // apply_neumann's launches, which the re-captured graph takes anew)
        I.nm_asked = I.nm_steps = I.poly_roots.count;
    }

    // block Jacobi in the preconditioner precision, from the matrix Jacobi<P>
    // takes above: the fp64 A for P = double, else its fp32 copy
    if (I.bj_bs) {
        need(I.bj_dinv, (size_t)I.n * I.bj_bs * dsize(ty.P) + 16);
        int st;
        if (ty.P == MPG_F64) {
            st = mpg_bjacobi_setup_f64(ctx, I.csr, I.val64.as<double>(), I.bj_bs, I.bj_dinv.as<double>(), nullptr);
        } else {
            DevMem f32(ctx, std::max<size_t>(nz, 1) * 4);
            I.cast(I.val64.p, MPG_F64, f32.p, MPG_F32, (int64_t)nz);
            st = mpg_bjacobi_setup_f32(ctx, I.csr, f32.as<float>(), I.bj_bs, I.bj_dinv.as<float>(), nullptr);
        }
        check(st, "block Jacobi set-up", ctx);
    }

    // ILU(0) of the fp64 A in the preconditioner precision (gmres_perf_test.cpp:70-79, 140-149)
    // (new values: the factor object again, its level schedule included; no in-place refactorisation.
    // A factorisation that fails returns its status here, inside the refresh; the fault word
    // check_ilu_fault reads belongs to the triangular solves, which run from the re-arm on)
    if (ilu && I.ilu) {
        check(mpg_ctx_sync(ctx), "sync", ctx);
        mpg_ilu_destroy(I.ilu);
        I.ilu = nullptr;
    }
    if (ilu) check(mpg_ilu0_create(ctx, I.csr, I.val64.as<double>(), ty.P == MPG_F64 ? 0 : 1, &I.ilu), "ilu0", ctx);

    // ||A||_F of the matrix the driver was given (A_single in mixed mode)
    {
        const bool mixed = !rounded_outer;
        const void* av = mixed ? nullptr : I.val_outer;
        int at = ty.X;
        DevMem f32;
        if (mixed) {  // A_single values (fp32) even in mixed-half mode
            f32 = DevMem(ctx, std::max<size_t>(nz, 1) * 4);
            I.cast(I.val64.p, MPG_F64, f32.p, MPG_F32, (int64_t)nz);
            av = f32.p;
            at = MPG_F32;
        }
        a_norm = I.nrm2(av, at, (int64_t)nz);
    }

    if (!live) return;
    // the workspace's storage copies, from the arrays rewritten above (the
    // descriptor's pointers are unchanged)
    check(mpg_arnoldi_refresh_values(I.arn), "mpg_arnoldi_refresh_values", ctx);
    if (I.pv_sell)
        check(mpg_sell_refresh_values(ctx, I.pv_sell, I.csr, MPG_F16, pv_half.p), "fp16 SELL copy for the sweeps", ctx);
    // The captured cycle holds its launch arguments by value. Identity,
    // Jacobi, block Jacobi and the Jacobi sweeps pass addresses only, which
    // did not move: the graph stays. Chebyshev's theta / delta and the
    // GMRES-polynomial roots are arguments by value, and the ILU factors are
    // a new object: those cycles are captured again at the next solve.
    if (I.cheb || I.poly || ilu) {
        check(mpg_ctx_sync(ctx), "sync", ctx);
        I.graph.reset();
    }
    values_dirty_ = false;
}

void FusedEngine::refresh_values(const double* val, int64_t nnz, int flags) {
    Impl& I = *p_;
    if (nnz != I.nnz || (nnz > 0 && !val))
        throw StatusError(MPG_ERR_ARG, "mpg_engine_refresh_values: " + std::to_string(nnz) +
                                           " values for an engine whose matrix stores " + std::to_string(I.nnz) +
                                           " (the sparsity pattern is the engine's: one fp64 value per stored "
                                           "entry, in CSR order)");
    if (I.comm)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          "refreshing the values of a row-partitioned engine is not available: Jacobi's row "
                          "maximum and ||A||_F would have to cross the ranks again, and the re-arm that must follow "
                          "is not available there either");
    if (measured) throw StatusError(MPG_ERR_UNSUPPORTED, kMeasuredText);
    auto t0 = clk::now();
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
    load_values(val, (flags & MPG_REFRESH_VAL_DEVICE) != 0);
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
    armed_ = false;  // ||M^-1 b|| and the first residual belong to the old matrix: rearm() must follow
    I.g_stale = I.g_p > 0;  // the guess store's images too: the next project or keep makes them again
    refresh_seconds = std::chrono::duration<double>(clk::now() - t0).count();
}

// What a solve takes from b and x: the vectors in the outer type, the drivers'
// one-time norms of b and M^-1 b, x_true for the report, and the host's
// per-solve state. The constructor and rearm() both come through here, so a
// re-armed solve runs a fresh engine's launches on a fresh engine's values.
// b: nullptr keeps the current right-hand side (rearm only); x0: nullptr is
// zeros; flags: MPG_ARM_B_DEVICE / MPG_ARM_X0_DEVICE (solve.h).
void FusedEngine::arm(const double* b, const double* x0, const double* x_true, int flags) {
    Impl& I = *p_;
    const mpg_ctx_t ctx = I.ctx;
    const ModeTypes& ty = I.ty;
    const size_t n8 = (size_t)I.n * 8;
    // an fp64 vector of n, in host memory or on the device, into a device vector of the outer type
    auto put = [&](const double* src, bool on_device, void* dst) {
        if (on_device) {
            if (ty.X == MPG_F64) check(mpg_memcpy_d2d(ctx, dst, src, n8), "d2d", ctx);
            else I.cast(src, MPG_F64, dst, ty.X, I.n);
            return;
        }
        void* to = ty.X == MPG_F64 ? dst : I.stage64.p;
        check(mpg_memcpy_h2d(ctx, to, src, n8), "h2d", ctx);
        if (ty.X != MPG_F64) I.cast(I.stage64.p, MPG_F64, dst, ty.X, I.n);
    };
    if (b) put(b, (flags & MPG_ARM_B_DEVICE) != 0, I.b.p);
    // x: zeros in the front pad, the halo and the tail, X(x0) over rows [0, n)
    // (the first arm finds the allocation's zeros)
    if (solves_ > 0) check(mpg_memset(ctx, I.x.p, 0, I.x.bytes), "memset", ctx);
    if (x0) put(x0, (flags & MPG_ARM_X0_DEVICE) != 0, I.xp);
    if (flags & MPG_ARM_X0_PROJECT) guess_project(x0 != nullptr);
    I.have_xt = x_true != nullptr;
    if (x_true) {
        if (!I.xt.p) I.xt = DevMem(ctx, n8 + 8);  // (the first x_true this engine is given)
        check(mpg_memcpy_h2d(ctx, I.xt.p, x_true, n8), "h2d", ctx);
    }

    // one-time norms of the drivers (gmres.cpp:51-58, 162-168)
    b_norm = I.nrm2(I.b.p, ty.X, I.n);
    {
        I.cast(I.b.p, ty.X, I.tmp_t.p, ty.T, I.n);              // copy(b, w)
        if (ty.P != ty.T) I.cast(I.tmp_t.p, ty.T, I.tmp_p.p, ty.P, I.n);  // typesafe_apply
        void* wp = ty.P != ty.T ? I.tmp_p.p : I.tmp_t.p;
        if (I.jacobi_inside()) {
            if (ty.P == MPG_F64)
                check(mpg_gdmv_f64(ctx, I.n, 1.0, I.diag.as<double>(), (double*)wp, 0.0, (double*)wp), "gdmv", ctx);
            else
                check(mpg_gdmv_f32(ctx, I.n, 1.0f, I.diag.as<float>(), (float*)wp, 0.0f, (float*)wp), "gdmv", ctx);
        }
        if (I.ilu) I.solve_ilu(wp);
        if (ty.P != ty.T) I.cast(I.tmp_p.p, ty.P, I.tmp_t.p, ty.T, I.n);
        if (I.bj_bs) I.apply_bjacobi(I.tmp_t.p);  // (on the vector of T, casting inside)
        // the sweeps: ||M^-1 b|| through the launches every application takes (tmp_t holds T(b))
        if (I.nm_steps) I.apply_neumann(I.tmp_t.p);
        minvb_norm = I.nrm2(I.tmp_t.p, ty.T, I.n);
    }
    if (I.pol.pipeline && tail_fold()) {
        // the givens+update launch keeps rows [0, n) of the x it reads; the
        // restore copies the whole array, so its padding is filled here
        hipck(hipMemcpyAsync(I.x_snap.p, I.x.p, I.x.bytes, hipMemcpyDeviceToDevice, I.stream()), "x snapshot");
    }

    // the host's state of a solve
    cycles.clear();
    step_res.clear();
    step_cycle.clear();
    status = 0;
    restarts = 0;
    inner_k = 0;
    const bool stop = breakdown.stop;
    breakdown = BreakdownLog();
    breakdown.stop = stop;
    I.report_host = I.rep[0];
    // convergence strategy (gmres_perf_test.cpp:185-196)
    const mpg_solve_args& a = I.args;
    const size_t mm = (size_t)a.rlen, mr = (size_t)a.max_restarts;
    if (a.rtol == 0) conv_ = std::make_unique<Convergence<double, void>>(a.tol, mm, mr);
    else if (a.repeat_iter) conv_ = std::make_unique<RepeatIteration_Convergence<double, void>>(a.tol, a.rtol, mm, mr);
    else if (I.orthloss) {
        auto lo = std::make_unique<LostOrthogonalityFused>(a.tol, a.rtol, mm, mr);
        lo->step_loss = [this](size_t k) { return orth_loss_step(k); };
        if (solves_ > 0) {
            // S, u and the basis as a new engine has them: the loss estimate
            // reads the basis column after the newest one (orth_loss_step)
            int64_t ld = 0;
            void* V = const_cast<void*>(mpg_arnoldi_basis_dev(I.arn, &ld));
            check(mpg_memset(ctx, V, 0, (size_t)ld * (mm + 1) * dsize(ty.T)), "memset", ctx);
            check(mpg_memset(ctx, I.loss_S.p, 0, I.loss_S.bytes), "memset", ctx);
            check(mpg_memset(ctx, I.loss_u.p, 0, I.loss_u.bytes), "memset", ctx);
        }
        conv_ = std::move(lo);
    } else conv_ = std::make_unique<RelPrecRes_Convergence<double, void>>(a.tol, a.rtol, mm, mr);
    conv_->total_iters = 0;
    ++solves_;
    armed_ = true;
}

void FusedEngine::start() {
    prologue();
    read_report(4);
    if (p_->ilu) check_ilu_fault(p_->ilu);
}

void FusedEngine::rearm(const double* b, const double* x0, const double* x_true, int flags) {
    Impl& I = *p_;
    if (I.comm)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          "re-arming a row-partitioned engine is not available: the norms of the new vectors and "
                          "the halo of the initial guess would have to cross the ranks");
    if (measured) throw StatusError(MPG_ERR_UNSUPPORTED, kMeasuredText);
    if ((flags & MPG_ARM_X0_PROJECT) && I.g_L == 0)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          "MPG_ARM_X0_PROJECT needs a guess store and this engine has none (depth 0): "
                          "mpg_engine_guess_depth comes first");
    auto t0 = clk::now();
    arm(b, x0, x_true, flags);
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
    setup_seconds = std::chrono::duration<double>(clk::now() - t0).count();
    start();
}

void FusedEngine::copy_x(double* dst, bool dst_on_device) {
    Impl& I = *p_;
    const size_t n8 = (size_t)I.n * 8;
    if (dst_on_device) {
        if (I.ty.X == MPG_F64) check(mpg_memcpy_d2d(I.ctx, dst, I.xp, n8), "d2d", I.ctx);
        else I.cast(I.xp, I.ty.X, dst, MPG_F64, I.n);
    } else {
        const void* from = I.xp;
        if (I.ty.X != MPG_F64) {
            I.cast(I.xp, I.ty.X, I.stage64.p, MPG_F64, I.n);
            from = I.stage64.p;
        }
        check(mpg_memcpy_d2h(I.ctx, dst, from, n8), "d2h", I.ctx);
    }
    sync();
}

// ---------------------------------------------------------------- the initial-guess store
//  Z and Q = A Z with Q^T Q = I, fp64, A = val_outer on csr: the
// matrix of the residual prologue. project: the least-squares guess in
// xbar + span Z; keep: the newest solution orthogonalised in by two passes of
// classical Gram-Schmidt on the images. Launches: project = dots + update
// (+ the SpMV of b - A xbar where xbar != 0); keep = SpMV, dots, two update
// passes, scale.
void FusedEngine::guess_check(const char* what) const {
    const Impl& I = *p_;
    const std::string w = std::string(what) + ": the guess store ";
    if (I.comm)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          w + "is not available on a row-partitioned engine: Q^T r and the norms would have to "
                              "cross the ranks, and the re-arm that projects is not available there either");
    if (measured) throw StatusError(MPG_ERR_UNSUPPORTED, w + "is not available: " + kMeasuredText);
    if (I.ty.X != MPG_F64)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          w + "is not available in the modes whose outer type is fp32 (single): solutions "
                              "resolved to 1e-7 cannot make guesses worth a cycle");
    if (I.args.mode == MPG_MODE_SINGLE_PREC)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          w + "is not available in mode single-prec: its fp32 preconditioner bounds what the "
                              "solves resolve, and the store is not tested there");
}

int FusedEngine::guess_held() const { return p_->g_p; }
int FusedEngine::guess_L() const { return p_->g_L; }

void FusedEngine::guess_depth(int L) {
    Impl& I = *p_;
    if (L < 0 || L > MPG_GUESS_MAX_DEPTH)
        throw StatusError(MPG_ERR_ARG, "mpg_engine_guess_depth: depth " + std::to_string(L) + " is outside [0, " +
                                           std::to_string(MPG_GUESS_MAX_DEPTH) + "]");
    if (L > 0) guess_check("mpg_engine_guess_depth");
    if (L == I.g_L) return;
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
    I.g_Z = DevMem(), I.g_Q = DevMem(), I.g_w = DevMem(), I.g_d = DevMem(), I.g_r = DevMem();
    I.g_part = DevMem(), I.g_info = DevMem();
    I.g_L = I.g_p = 0;
    I.g_stale = false;
    guess_rho0 = guess_rho1 = 0;
    if (L == 0) return;
    const int G = mpg_guess_groups(I.n);
    if (G < 1) throw StatusError(MPG_ERR_ARG, "mpg_engine_guess_depth: an engine without rows");
    I.g_ld = ((int64_t)I.n + 31) / 32 * 32;
    const size_t col = (size_t)I.g_ld * 8;
    I.g_Z = DevMem(I.ctx, col * L);
    I.g_Q = DevMem(I.ctx, col * L);
    I.g_w = DevMem(I.ctx, col);
    I.g_d = DevMem(I.ctx, col);
    I.g_r = DevMem(I.ctx, col);
    I.g_part = DevMem(I.ctx, (size_t)3 * (L + 1) * G * 8);
    I.g_info = DevMem(I.ctx, 64 * 8);
    I.g_L = L;
}

void FusedEngine::guess_project(bool have_base) {
    Impl& I = *p_;
    const mpg_ctx_t ctx = I.ctx;
    auto t0 = clk::now();
    if (I.g_stale) guess_reimage();
    const int n = I.n, p = I.g_p;
    const double* r = I.b.as<double>();
    if (have_base) {  // r = b - A xbar
        check(mpg_memcpy_d2d(ctx, I.g_r.p, I.b.p, (size_t)n * 8), "d2d", ctx);
        check(mpg_csr_spmv_f64(ctx, I.csr, -1.0, static_cast<const double*>(I.val_outer),
                               static_cast<const double*>(I.xp), 1.0, I.g_r.as<double>()),
              "guess residual", ctx);
        r = I.g_r.as<double>();
    }
    if (p == 0) {
        guess_rho0 = guess_rho1 = I.nrm2(r, MPG_F64, n);
    } else {
        double* part = I.g_part.as<double>();
        double* coef = I.g_info.as<double>();
        check(mpg_guess_dots_f64(ctx, n, p, I.g_ld, I.g_Q.as<double>(), r, part), "mpg_guess_dots_f64", ctx);
        check(mpg_guess_update_f64(ctx, n, p, I.g_ld, part, 1.0, I.g_Z.as<double>(), static_cast<const double*>(I.xp),
                                   static_cast<double*>(I.xp), nullptr, nullptr, nullptr, coef),
              "mpg_guess_update_f64", ctx);
        double h[MPG_GUESS_MAX_DEPTH + 1];
        check(mpg_memcpy_d2h(ctx, h, coef, (size_t)(p + 1) * 8), "d2h", ctx);
        double cc = 0;
        for (int j = 0; j < p; ++j) cc += h[j] * h[j];
        guess_rho0 = std::sqrt(h[p]);
        guess_rho1 = std::sqrt(std::max(0.0, h[p] - cc));
    }
    check(mpg_ctx_sync(ctx), "sync", ctx);
    guess_seconds += std::chrono::duration<double>(clk::now() - t0).count();
}

void FusedEngine::guess_keep_vec(const double* x) {
    Impl& I = *p_;
    const mpg_ctx_t ctx = I.ctx;
    const int n = I.n;
    if (I.g_p == I.g_L) I.g_p = 0;  // Fischer's restart: the newest solution alone reseeds the store
    const int p = I.g_p;
    const int G = mpg_guess_groups(n);
    const int64_t ld = I.g_ld;
    double *Z = I.g_Z.as<double>(), *Q = I.g_Q.as<double>(), *w = I.g_w.as<double>(), *d = I.g_d.as<double>();
    double* pa = I.g_part.as<double>();
    double* pb = pa + (size_t)(I.g_L + 1) * G;
    double* pc = pb + (size_t)(I.g_L + 1) * G;
    double* info = I.g_info.as<double>() + 32;
    check(mpg_csr_spmv_f64(ctx, I.csr, 1.0, static_cast<const double*>(I.val_outer), x, 0.0, w), "guess image", ctx);
    check(mpg_guess_dots_f64(ctx, n, p, ld, Q, w, pa), "mpg_guess_dots_f64", ctx);  // Q^T w, omega^2
    const double* dv = x;
    const double* nu2 = pa + (size_t)p * G;
    if (p > 0) {
        check(mpg_guess_update_f64(ctx, n, p, ld, pa, -1.0, Z, x, d, Q, w, pb, nullptr), "mpg_guess_update_f64", ctx);
        check(mpg_guess_update_f64(ctx, n, p, ld, pb, -1.0, Z, d, d, Q, w, pc, nullptr), "mpg_guess_update_f64", ctx);
        dv = d;
        nu2 = pc + (size_t)p * G;
    }
    const double thr = std::max(I.args.tol, (double)n * 0x1p-53);
    check(mpg_guess_scale_f64(ctx, n, nu2, pa + (size_t)p * G, thr, w, dv, Q + (size_t)p * ld, Z + (size_t)p * ld,
                              info),
          "mpg_guess_scale_f64", ctx);
    double h[3] = {0, 0, 0};
    check(mpg_memcpy_d2h(ctx, h, info, sizeof h), "d2h", ctx);
    if (h[2] != 0.0) I.g_p = p + 1;
}

void FusedEngine::guess_reimage() {
    Impl& I = *p_;
    const int p = I.g_p;
    I.g_stale = false;
    if (p == 0) return;
    const size_t col = (size_t)I.g_ld * 8;
    DevMem old(I.ctx, col * p);
    check(mpg_memcpy_d2d(I.ctx, old.p, I.g_Z.p, col * p), "d2d", I.ctx);
    I.g_p = 0;
    for (int j = 0; j < p; ++j) guess_keep_vec(old.as<double>() + (size_t)j * I.g_ld);
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
}

void FusedEngine::guess_keep() {
    Impl& I = *p_;
    guess_check("mpg_engine_guess_keep");
    if (I.g_L == 0)
        throw StatusError(MPG_ERR_UNSUPPORTED, "mpg_engine_guess_keep: this engine has no guess store (depth 0): "
                                               "mpg_engine_guess_depth comes first");
    auto t0 = clk::now();
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
    if (I.g_stale) guess_reimage();
    guess_keep_vec(static_cast<const double*>(I.xp));
    check(mpg_ctx_sync(I.ctx), "sync", I.ctx);
    guess_seconds += std::chrono::duration<double>(clk::now() - t0).count();
}

void FusedEngine::guess_store(double* Z, double* Q) {
    Impl& I = *p_;
    guess_check("mpg_engine_guess_store");
    if (I.g_stale) {
        auto t0 = clk::now();
        guess_reimage();
        guess_seconds += std::chrono::duration<double>(clk::now() - t0).count();
    }
    const size_t n8 = (size_t)I.n * 8;
    for (int j = 0; j < I.g_p; ++j) {
        if (Z) check(mpg_memcpy_d2h(I.ctx, Z + (size_t)j * I.n, I.g_Z.as<double>() + (size_t)j * I.g_ld, n8), "d2h", I.ctx);
        if (Q) check(mpg_memcpy_d2h(I.ctx, Q + (size_t)j * I.n, I.g_Q.as<double>() + (size_t)j * I.g_ld, n8), "d2h", I.ctx);
    }
    sync();
}

FusedEngine::~FusedEngine() = default;

void FusedEngine::sync() { check(mpg_ctx_sync(p_->ctx), "sync", p_->ctx); }

// One op of the cycle's list (cycle_plan.hpp): the only place the cycle's
// launches and collectives are made.
void FusedEngine::issue(const Op& o) {
    Impl& I = *p_;
    const mpg_arnoldi_t A = I.arn;
    const hipStream_t s = I.stream();
    switch (o.kind) {
        case OpKind::XSnapshot:  // the cycle may run past a stop decision: keep the x it started from
            return hipck(hipMemcpyAsync(I.x_snap.p, I.x.p, I.x.bytes, hipMemcpyDeviceToDevice, s), "x snapshot");
        case OpKind::Halo:
            if (o.a < 0) return I.comm->halo(I.xp, (int)dsize(I.ty.X), s);
            return I.comm->halo(mpg_arnoldi_wprev_dev(A, o.a), mpg_arnoldi_vec_bytes(A), s);
        case OpKind::AllreducePartialsHalo:
            return I.comm->allreduce_sum_and_halo(mpg_arnoldi_partials_dev(A), mpg_arnoldi_partials_count(A),
                                                  mpg_arnoldi_wprev_dev(A, o.a), mpg_arnoldi_vec_bytes(A), s);
        case OpKind::Spmv: return check(mpg_arnoldi_spmv(A, o.a), "spmv", I.ctx);
        case OpKind::GivensSpmv: return check(mpg_arnoldi_givens_partials_spmv(A, o.a), "givens+spmv", I.ctx);
        case OpKind::SpmvDots: return check(mpg_arnoldi_spmv_dots(A, o.a, o.b), "spmv+dots", I.ctx);
        case OpKind::StepDots: return check(mpg_arnoldi_step_dots(A, o.a, o.b), "spmv+dots", I.ctx);
        case OpKind::ApplyPrec: return I.apply_ilu(mpg_arnoldi_wprev_dev(A, o.a));
        case OpKind::Dots: return check(mpg_arnoldi_dots(A, o.a), "dots", I.ctx);
        case OpKind::DotsSums: return check(mpg_arnoldi_dots_sums(A, o.a), "dots+sums", I.ctx);
        case OpKind::AllreducePartials:
            // the last launch's partials, [column][workgroup] (uniform workgroup
            // counts on every rank: mpg_arnoldi_uniform_groups), summed in place
            // (bit-identical on every rank), for a consumer that sums them itself
            return I.comm->allreduce_sum(mpg_arnoldi_partials_dev(A), (int64_t)o.a * mpg_arnoldi_partials_count(A), s);
        case OpKind::Reduce: return check(mpg_arnoldi_reduce(A, o.a), "reduce", I.ctx);
        case OpKind::AllreduceSums: return I.comm->allreduce_sum(mpg_arnoldi_sums_dev(A), o.a, s);
        case OpKind::CgsPartials: return check(mpg_arnoldi_cgs_partials(A, o.a), "cgs", I.ctx);
        case OpKind::Cgs: return check(mpg_arnoldi_cgs(A, o.a, o.b), "cgs", I.ctx);
        case OpKind::CgsGivens: return check(mpg_arnoldi_cgs_givens(A, o.a, o.b), "cgs+givens", I.ctx);
        case OpKind::CgsrWidePass: return check(mpg_arnoldi_cgsr_wide_pass(A, o.a, o.b), "cgsr", I.ctx);
        case OpKind::MgsPartials: return check(mpg_arnoldi_mgs_partials(A, o.a, o.b), "mgs", I.ctx);
        case OpKind::Givens: return check(mpg_arnoldi_givens(A, o.a), "givens", I.ctx);
        case OpKind::GivensPartials: return check(mpg_arnoldi_givens_partials(A, o.a), "givens", I.ctx);
        case OpKind::Update: return check(mpg_arnoldi_update(A, o.a), "update", I.ctx);
        case OpKind::GivensUpdate: return check(mpg_arnoldi_update_tail(A, o.a, o.b), "givens+update", I.ctx);
        case OpKind::Prologue: return check(mpg_arnoldi_prologue(A), "prologue", I.ctx);
        case OpKind::PrologueWnorm: return check(mpg_arnoldi_prologue_wnorm(A), "prologue wnorm", I.ctx);
        case OpKind::PrologueFinish: return check(mpg_arnoldi_prologue_finish(A), "prologue_finish", I.ctx);
        case OpKind::PrologueFinishPartials:
            return check(mpg_arnoldi_prologue_finish_partials(A), "prologue_finish", I.ctx);
    }
}

void FusedEngine::issue(const std::vector<Op>& ops) {
    for (const Op& o : ops) issue(o);
}

void FusedEngine::prologue() {
    std::vector<Op> ops;
    plan_prologue(p_->pol, ops);
    issue(ops);
}

// Arnoldi step k on its own (the stepwise strategies). fold as in plan_step.
void FusedEngine::step(int k, bool fold) {
    std::vector<Op> ops;
    check(plan_step(p_->pol, k, fold, ops), "step plan", p_->ctx);
    issue(ops);
}

// v_{k+1} = T(w * (1/h_{k+1,k})) into V(:,k+1) right after step k, as the
// reference's add_vector does (Orthogonalization.hpp:51-60); the next SpMV
// forms and stores the same value again. Only LostOrthogonality needs it
// early: it reads the basis column after the newest one.
void FusedEngine::store_next_basis(int k) {
    Impl& I = *p_;
    int64_t ld = 0;
    void* V = const_cast<void*>(mpg_arnoldi_basis_dev(I.arn, &ld));
    const void* inv = mpg_arnoldi_inv_dev(I.arn);
    const void* w = mpg_arnoldi_wprev_dev(I.arn, k + 1);
    const size_t off = (size_t)(k + 1) * (size_t)ld;
    if (I.ty.T == MPG_F64)
        check(mpg_scal_copy_dev_f64(I.ctx, I.n, (const double*)inv, (const double*)w, (double*)V + off), "v_k+1", I.ctx);
    else
        check(mpg_scal_copy_dev_f32(I.ctx, I.n, (const float*)inv, (const float*)w, (float*)V + off), "v_k+1", I.ctx);
}

// LostOrthogonality_Convergence::check body (IterUtil.hpp:206-216) for
// check(k): u = V(:,0:k+1)^T V(:,k+1); s_col = S(0:k+1,k+1) = u - S(0:k+1,
// 0:k+1) u; returns dot(s_col, s_col). V(:,k+1) is the column after the
// newest basis vector: what an earlier cycle left there, or zeros.
double FusedEngine::orth_loss_step(size_t kk) {
    Impl& I = *p_;
    const int64_t k = (int64_t)kk, ldS = I.m + 1;
    int64_t ld = 0;
    const void* V = mpg_arnoldi_basis_dev(I.arn, &ld);
    if (I.ty.T == MPG_F64) {
        const double* Vd = (const double*)V;
        double *u = I.loss_u.as<double>(), *S = I.loss_S.as<double>(), *scol = S + (k + 1) * ldS;
        check(mpg_gemv_f64(I.ctx, 1, I.n, k + 1, 1.0, Vd, ld, Vd + (k + 1) * ld, 0.0, u), "gemv", I.ctx);
        check(mpg_copy_f64f64(I.ctx, k + 1, u, scol), "copy", I.ctx);
        check(mpg_gemv_f64(I.ctx, 0, k + 1, k + 1, -1.0, S, ldS, u, 1.0, scol), "gemv", I.ctx);
        double d = 0;
        check(mpg_dot_f64_host(I.ctx, k + 1, scol, scol, &d), "dot", I.ctx);
        return d;
    }
    const float* Vf = (const float*)V;
    float *u = I.loss_u.as<float>(), *S = I.loss_S.as<float>(), *scol = S + (k + 1) * ldS;
    check(mpg_gemv_f32(I.ctx, 1, I.n, k + 1, 1.0f, Vf, ld, Vf + (k + 1) * ld, 0.0f, u), "gemv", I.ctx);
    check(mpg_copy_f32f32(I.ctx, k + 1, u, scol), "copy", I.ctx);
    check(mpg_gemv_f32(I.ctx, 0, k + 1, k + 1, -1.0f, S, ldS, u, 1.0f, scol), "gemv", I.ctx);
    float d = 0;
    check(mpg_dot_f32_host(I.ctx, k + 1, scol, scol, &d), "dot", I.ctx);
    return (double)d;
}

void FusedEngine::update(int k) { issue(Op{OpKind::Update, -1, false, 0, k, 0}); }

void FusedEngine::read_report(int count) {
    Impl& I = *p_;
    hipck(hipMemcpyAsync(I.report_host, mpg_arnoldi_report_dev(I.arn), (size_t)count * sizeof(double),
                         hipMemcpyDeviceToHost, I.stream()),
          "report d2h");
    if (I.comm && I.comm->async()) {
        hipck(hipEventRecord(I.report_ev[0], I.stream()), "event record");
        wait_event(I.report_ev[0], (int64_t)cycles.size(), "the step collectives (halo send/recv, all-reduces)");
    }
    hipck(hipStreamSynchronize(I.stream()), "report sync");
}

// Host wait for the device. With an asynchronous transport (RCCL) a peer
// that never arrives would hang the rank in hipEventSynchronize, and the
// driver's 8-GPU run would only end at its time limit with no message: poll
// instead, check the communicator's asynchronous error, and after
// MPG_COMM_TIMEOUT_S seconds (default 120) without completion abort the
// communicator and fail with the rank, the restart cycle and the collectives
// in flight named (MPG_ERR_RCCL).
void FusedEngine::wait_event(hipEvent_t ev, int64_t cycle, const char* what) {
    Impl& I = *p_;
    if (!I.comm || !I.comm->async()) {
        hipck(hipEventSynchronize(ev), "wait");
        return;
    }
    const char* env = std::getenv("MPG_COMM_TIMEOUT_S");
    const double limit = env && *env ? std::atof(env) : 120.0;
    const auto t0 = clk::now();
    for (int polls = 0;; ++polls) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return;
        if (q != hipErrorNotReady) hipck(q, "event query");
        const double waited = std::chrono::duration<double>(clk::now() - t0).count();
        std::string why = I.comm->async_error();
        if (why.empty() && waited > limit)
            why = "no progress for " + std::to_string(waited) + " s (MPG_COMM_TIMEOUT_S " + std::to_string(limit) + ")";
        if (!why.empty()) {
            // a grace period first: work that still completes was slow, not
            // hung, and is not torn down under running kernels (the
            // communicator stays intact); otherwise abort it
            bool done_late = false;
            const bool async_err = waited <= limit;
            if (!async_err) {
                const auto g0 = clk::now();
                while (std::chrono::duration<double>(clk::now() - g0).count() < 5.0)
                    if (hipEventQuery(ev) == hipSuccess) {
                        done_late = true;
                        break;
                    }
            }
            const std::string where = "rank " + std::to_string(I.comm->rank()) + " of " +
                                      std::to_string(I.comm->size()) + ": restart cycle " + std::to_string(cycle) +
                                      ", waiting for " + what + ": " + why;
            if (done_late) {
                // slow but healthy (e.g. a huge or time-shared solve): say so
                // and go on; only an async error or a real hang ends the solve
                // 
                std::fprintf(stderr, "mpgmres: warning: %s; it completed within the 5 s grace period, continuing\n",
                             where.c_str());
                return;
            }
            I.comm->abort();
            throw StatusError(MPG_ERR_RCCL, where + "; communicator aborted");
        }
        // spin for the first ~ms (a cycle is ~1 ms), then back off
        if (polls > 2000) std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// check_initial on the report of the last prologue (gmres.cpp:171-190)
bool FusedEngine::check_start(int64_t i) {
    Impl& I = *p_;
    const double* r = I.report_host;
    double r_norm = r[0], beta = r[1], x_norm = r[2];
    double normalization;
    if (I.ty.single_scalars) normalization = (double)((float)b_norm + (float)a_norm * (float)x_norm);
    else normalization = b_norm + a_norm * x_norm;
    cycles.push_back(CycleRecord{r_norm, normalization, beta, minvb_norm});
    restarts = i;
    breakdown.cycle(r_norm, beta, i);
    switch (conv_->check_initial(r_norm, normalization, beta, minvb_norm)) {
        case iteration_converged: {
            const double rel = I.ty.single_scalars ? (double)(float)((float)beta / (float)minvb_norm)
                             : I.ty.T == MPG_F64 ? beta / minvb_norm
                                                 : (double)((float)beta / minvb_norm);
            out() << "Found solution with rel prec res norm = " << rel << " when k = 0 and i = " << i << std::endl;
            out() << "  total iterations = " << conv_->total_iterations() << std::endl;
            status = MPG_RESULT_CONVERGED;
            return true;
        }
        case iteration_aborted:
            out() << "Aborting after " << conv_->total_iterations() << " iterations" << std::endl;
            status = MPG_RESULT_ABORTED;
            return true;
        default: return false;
    }
}

// capture the cycle program once; if the runtime refuses (e.g. a collective
// that cannot be captured) fall back to eager launches for good
void FusedEngine::ensure_graph() {
    Impl& I = *p_;
    if (!I.pol.graph || I.graph.exec) return;
    try {
        I.graph = CapturedGraph(I.stream(), [this] { issue(p_->cycle); });
        ++graph_captures_;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "mpgmres: cycle capture failed (%s); running eagerly\n", ex.what());
        I.pol.graph = 0;
    }
}

// the base strategy's per-step bookkeeping for one cycle's report
void FusedEngine::record_steps(int64_t i) {
    Impl& I = *p_;
    for (int k = 0; k < I.m; ++k) {
        const double res = I.report_host[4 + k];
        step_res.push_back(res);
        step_cycle.push_back((int)i);
        breakdown.step(res, (int64_t)step_res.size() - 1, i, (size_t)k);
        conv_->check((size_t)k + 1, res, minvb_norm);  // base strategy: counts, restarts at m
    }
}

// Graph cycles with the host round trip hidden: cycle i+1 is launched before
// cycle i's report is read, so the GPU never waits for the host's
// check_initial (≈ 38 us per cycle on BAND-10M: the report copy, the
// stream synchronisation and the next launch). A cycle launched past a stop
// decision (converged or aborted at check_initial) is undone by restoring the
// x it started from (it cannot have changed anything else the result reads);
// no cycle is ever left in flight when run() returns.
int FusedEngine::run_pipelined(int max_cycles, bool& done) {
    Impl& I = *p_;
    int64_t i = (int64_t)cycles.size();
    if (check_start(i)) {
        done = true;
        return 0;
    }
    if (max_cycles <= 0) return 0;
    // one replay of the captured cycle, then its report into rep[p], marked by report_ev[p]
    auto launch = [&](int p) {
        hipck(hipGraphLaunch(I.graph.exec, I.stream()), "graph launch");
        hipck(hipMemcpyAsync(I.rep[p], mpg_arnoldi_report_dev(I.arn), (size_t)I.report_len * sizeof(double),
                             hipMemcpyDeviceToHost, I.stream()),
              "report d2h");
        hipck(hipEventRecord(I.report_ev[p], I.stream()), "event record");
    };
    // the buffer not holding the report check_start just read
    int p = I.report_host == I.rep[0] ? 1 : 0, ran = 0;
    launch(p);
    for (;;) {
        const bool more = ran + 1 < max_cycles;
        if (more) launch(p ^ 1);  // speculative: decided by this cycle's report
        wait_event(I.report_ev[p], i, "the step collectives (halo send/recv, all-reduces)");
        if (I.ilu) check_ilu_fault(I.ilu);  // every apply of this cycle is valid
        I.report_host = I.rep[p];
        record_steps(i);
        ++ran;
        ++i;
        if (!more) return ran;
        if (check_start(i)) {  // stop: undo the cycle launched past it
            done = true;
            sync();
            hipck(hipMemcpyAsync(I.x.p, I.x_snap.p, I.x.bytes, hipMemcpyDeviceToDevice, I.stream()), "x restore");
            sync();
            return ran;
        }
        p ^= 1;
    }
}

// --stop-on-breakdown: the first non-finite value ends the solve with
// MPG_ERR_BREAKDOWN (nothing left in flight: a pipelined cycle may be)
int FusedEngine::run(int max_cycles, bool& done) {
    if (measured)
        throw StatusError(MPG_ERR_UNSUPPORTED, kMeasuredText);
    if (!armed_)
        throw StatusError(MPG_ERR_ARG,
                          "the engine's matrix values were refreshed and no solve is armed on them: ||M^-1 b|| and the "
                          "first residual depend on the new matrix, so mpg_engine_rearm must come before "
                          "mpg_engine_run (b == NULL keeps the right-hand side)");
    try {
        return run_cycles(max_cycles, done);
    } catch (const BreakdownError& e) {
        (void)hipStreamSynchronize(p_->stream());
        done = true;
        status = MPG_RESULT_ERROR;
        throw StatusError(MPG_ERR_BREAKDOWN, e.what());
    }
}

int FusedEngine::run_cycles(int max_cycles, bool& done) {
    Impl& I = *p_;
    done = false;
    int ran = 0;
    const bool stepwise = conv_->needs_arnoldi_residual();
    if (!stepwise) ensure_graph();
    if (!stepwise && I.pol.graph && I.pol.pipeline) return run_pipelined(max_cycles, done);
    for (; ran < max_cycles; ++ran) {
        const int64_t i = (int64_t)cycles.size();
        if (check_start(i)) {
            done = true;
            return ran;
        }
        if (!stepwise) {
            if (I.pol.graph) hipck(hipGraphLaunch(I.graph.exec, I.stream()), "graph launch");
            else issue(I.cycle);  // steps 0..m-1, solution update with k = m, next residual prologue
            read_report(I.report_len);
            if (I.ilu) check_ilu_fault(I.ilu);
            record_steps(i);
            continue;
        }
        // adaptive restart strategies: one host read of |s(k+1)| per step
        for (int k = 0;; ++k) {
            step(k, false);
            if (I.orthloss) store_next_basis(k);
            read_report(4 + k + 1);
            if (I.ilu) check_ilu_fault(I.ilu);
            const double res = I.report_host[4 + k];
            step_res.push_back(res);
            step_cycle.push_back((int)i);
            breakdown.step(res, (int64_t)step_res.size() - 1, i, (size_t)k);
            const iteration_action act = conv_->check((size_t)k + 1, res, minvb_norm);
            if (act == iteration_converged) {
                update(k + 1);
                out() << "Found solution with rel prec res norm = " << res / minvb_norm << " when k = " << k + 1
                      << " and i = " << i << std::endl;
                out() << "  total iterations = " << conv_->total_iterations() << std::endl;
                status = MPG_RESULT_CONVERGED;
                inner_k = k + 1;
                done = true;
                sync();
                return ran + 1;
            }
            if (act == iteration_aborted) {
                out() << "Aborting after " << conv_->total_iterations() << " iterations" << std::endl;
                status = MPG_RESULT_ABORTED;
                done = true;
                return ran + 1;
            }
            if (act == iteration_restart) {
                update(k + 1);
                prologue();
                read_report(4);
                if (I.ilu) check_ilu_fault(I.ilu);
                break;
            }
        }
    }
    return ran;
}

void FusedEngine::finish_report(mpg_solve_result* r) {
    Impl& I = *p_;
    const int n = I.n;
    // x and b widened to fp64 (DoBaselineProblem copies x_type / b_type to double)
    DevMem x64m(I.ctx, (size_t)(I.front + I.n_ext) * 8 + 8), r64(I.ctx, (size_t)n * 8 + 8), b64(I.ctx, (size_t)n * 8 + 8);
    double* x64 = x64m.as<double>() + I.front;  // row 0
    I.cast(I.xp, I.ty.X, x64, MPG_F64, n);
    I.cast(I.b.p, I.ty.X, b64.p, MPG_F64, n);
    if (r->x_out) check(mpg_memcpy_d2h(I.ctx, r->x_out, x64, (size_t)n * 8), "d2h", I.ctx);
    if (I.comm) I.comm->halo(x64, 8, I.stream());
    check(mpg_memcpy_d2d(I.ctx, r64.p, b64.p, (size_t)n * 8), "d2d", I.ctx);
    check(mpg_csr_spmv_f64(I.ctx, I.csr, -1.0, I.val64.as<double>(), x64, 1.0, r64.as<double>()), "spmv", I.ctx);
    r->res_norm = std::sqrt(I.dot_acc(r64.p, r64.p, MPG_F64, n));
    if (I.have_xt) {  // (the copy arm() made: the caller's array may be gone)
        check(mpg_axpy_f64(I.ctx, n, -1.0, I.xt.as<double>(), x64), "axpy", I.ctx);
        r->err_norm = std::sqrt(I.dot_acc(x64, x64, MPG_F64, n));
    }
}

double FusedEngine::phase_bytes(int which) const {
    const Impl& I = *p_;
    const double n = I.n, z = (double)I.nnz, sT = (double)dsize(I.ty.T), sX = (double)dsize(I.ty.X);
    const double sV = (double)dsize(I.ty.VI), sP = (double)dsize(I.ty.P);
    const double sB = I.basis == MPG_BASIS_F16 ? 2.0 : sT;  // an entry of V (2 bytes compressed)
    // Jacobi's diagonal read inside the launch; block Jacobi's own launch
    // after it (w read and written again, bs inverse entries per row)
    const bool bjf = which == 1 ? I.bj_fused_prologue : I.bj_fused_step;
    const double jac = I.jacobi_inside() ? 1.0 : I.bj_bs ? (bjf ? 0.0 : 2 * sT / sP) + I.bj_bs : 0.0;
    // the Jacobi sweeps' launches after the SpMV: the gdmv (w read, z written,
    // the diagonal), then per sweep the matrix again, z read and written and
    // three more n-vectors (r, the diagonal, z's own entry); a Chebyshev sweep
    // after the first reads z_prev too. A GMRES-polynomial sweep: the gathered
    // vector, the diagonal and p read, z read and written, the second output
    // written (six n-vectors), less z's read in the first sweep and the second
    // output in the last: with k roots (k - 1) * 6 - 2 n-vectors beside the
    // matrix, k >= 2
    // (prec_values f16: 2 bytes per value and the n row exponents in each sweep)
    const double sW = I.prec_values == MPG_PREC_VALUES_F16 ? 2.0 : sV;
    const double ex = I.prec_values == MPG_PREC_VALUES_F16 ? n : 0.0;
    const double nm = I.nm_steps ? (2 * sT + sP) * n + (I.nm_steps - 1) * (z * (sW + 4) + ex + (n + 1) * 4 + 5 * n * sT) +
                                       (I.cheb && I.nm_steps > 2 ? (I.nm_steps - 2) * n * sT : 0.0) +
                                       (I.poly && I.nm_steps > 2 ? (I.nm_steps - 3) * n * sT : 0.0) -
                                       (I.poly && I.nm_steps == 2 ? n * sT : 0.0)
                                 : 0.0;
    if (which == 0) {
        // SURVEY §8(d) B_spmv, the same for every storage: CSR values + int32
        // columns + row pointers, x read once, y written (the SELL-64 copy
        // moves fewer bytes; profiles/ PMC traffic shows the actual ones),
        // plus the Jacobi diagonal when the preconditioner is fused in
        return z * (sV + 4) + (n + 1) * 4 + 2 * n * sT + jac * n * sP + nm;
    }
    if (which == 1) return z * (sX + 4) + (n + 1) * 4 + 3 * n * sX + n * sT + jac * n * sP;
    if (which == 4) {
        // the bytes the Arnoldi SpMV's own storage moves per launch: SELL-64
        // slots (column offset + value), slice offsets and step bases, or CSR
        // values + int32 columns + row pointers; then w_prev read once, v_k
        // stored to V(:,k), w written, the Jacobi diagonal when fused
        int32_t fmt = 0, W = 0, cb = 0, win = 0;
        int64_t stored = 0;
        check(mpg_arnoldi_spmv_layout(I.arn, &fmt, &W, &cb, &stored, &win), "layout", I.ctx);
        // (steps that run the SpMV inside the dots' launch also read
        // V(:,0..k-1) there: their columns, averaged over the cycle's steps)
        double cols = 0;
        for (int k = 0; k < I.m; ++k)
            if (I.step_dots_at(k)) cols += k;
        const double vec = 2 * n * sT + n * sB + jac * n * sP + cols / I.m * n * sT;
        if (fmt == 2 || fmt == 3) return (double)mpg_arnoldi_sell_matrix_bytes(I.arn) + vec;  // (3: node blocks)
        return z * (sV + 4) + (n + 1) * 4 + vec;
    }
    if (which == 3) {
        // panel dots, mean over k: V(:,0..k) and w read (per step of the
        // cycle: a step whose dots ride in the SpMV's launch adds nothing here)
        double cols = 0, launches = 0;
        for (int k = 0; k < I.m; ++k)
            if (!I.step_dots_at(k)) {
                cols += (I.orth == MPG_ORTH_MGS ? 1 : k + 1);
                launches += 1;
            }
        return cols / I.m * n * sB + launches / I.m * n * sT;
    }
    // CGS update at mean k: read V(:,0..k), read + write w
    return ((I.m - 1) / 2.0 + 1) * n * sB + 2 * n * sT;
}

mpg_arnoldi_t FusedEngine::arnoldi() const { return p_->arn; }
int FusedEngine::basis() const { return p_->basis; }
int FusedEngine::prec_values() const { return p_->prec_values; }
const int64_t* FusedEngine::half_stats() const { return p_->half_stats; }
int FusedEngine::prec_fused() const { return p_->bj_bs ? (p_->bj_fused_step ? 1 : 0) : -1; }
int FusedEngine::prec_sweeps() const { return p_->nm_asked ? p_->nm_asked : -1; }
int FusedEngine::prec_roots(double* re, double* im, int cap) const {
    if (!p_->poly) return -1;
    for (int i = 0; i < p_->poly_roots.count && i < cap; ++i) {
        if (re) re[i] = p_->poly_roots.re[i];
        if (im) im[i] = p_->poly_roots.im[i];
    }
    return p_->poly_roots.count;
}
bool FusedEngine::prec_interval(double* a, double* b) const {
    if (!p_->cheb) return false;
    if (a) *a = p_->cheb_iv.a;
    if (b) *b = p_->cheb_iv.b;
    return true;
}
int FusedEngine::step_dots_steps() const {
    return (int)std::count_if(p_->cycle.begin(), p_->cycle.end(), [](const Op& o) { return o.kind == OpKind::StepDots; });
}
bool FusedEngine::givens_rider() const {  // (StepDots: a = k, b = the fold)
    return std::any_of(p_->cycle.begin(), p_->cycle.end(), [](const Op& o) { return o.kind == OpKind::StepDots && o.b != 0; });
}
bool FusedEngine::tail_fold() const {
    return std::any_of(p_->cycle.begin(), p_->cycle.end(), [](const Op& o) { return o.kind == OpKind::GivensUpdate; });
}
int FusedEngine::cgs_stream_steps() const {
    return (int)std::count_if(p_->cycle.begin(), p_->cycle.end(), [&](const Op& o) {
        return o.kind == OpKind::CgsPartials && mpg_arnoldi_cgs_stream_at(p_->arn, o.a) == 1;
    });
}
const CyclePolicy& FusedEngine::policy() const { return p_->pol; }
const std::vector<Op>& FusedEngine::cycle_ops() const { return p_->cycle; }
hipStream_t FusedEngine::stream() const { return p_->stream(); }
mpg_ctx_t FusedEngine::ctx() const { return p_->ctx; }

// ---------------------------------------------------------------- mpg_solve (fused)
void fill_history(const FusedEngine& e, mpg_solve_result* r) {
    r->status = e.status;
    r->restarts = e.restarts;
    r->inner_k = e.inner_k;
    r->total_iters = (int64_t)e.total_iters();
    r->minvb_norm = e.minvb_norm;
    r->setup_seconds = e.setup_seconds;
    r->n_cycles = (int64_t)e.cycles.size();
    for (size_t c = 0; c < e.cycles.size() && (int64_t)c < r->cycle_cap; ++c) {
        if (r->cyc_r_norm) r->cyc_r_norm[c] = e.cycles[c].r_norm;
        if (r->cyc_normalization) r->cyc_normalization[c] = e.cycles[c].normalization;
        if (r->cyc_beta) r->cyc_beta[c] = e.cycles[c].beta;
    }
    r->nonfinite_steps = e.breakdown.steps;
    r->nonfinite_cycles = e.breakdown.cycles;
    r->first_nonfinite_step = e.breakdown.first_step;
    r->n_steps = (int64_t)e.step_res.size();
    for (size_t s = 0; s < e.step_res.size() && (int64_t)s < r->step_cap; ++s) {
        if (r->step_res) r->step_res[s] = e.step_res[s];
        if (r->step_cycle) r->step_cycle[s] = e.step_cycle[s];
    }
}

int solve_fused(const mpg_solve_args& a, mpg_solve_result* r, const double* x0) {
    mpg_ctx_t ctx = current_ctx();
    const char* banner = a.mode == MPG_MODE_MIXED || a.mode == MPG_MODE_MIXED_HALF ? "Doing Mixed Precision test"
                                                                                     : "Doing Baseline test";
    out() << banner << std::endl;
    FusedEngine e(ctx, a, nullptr, -1, 0, x0);
    auto t1 = clk::now();
    bool done = false;
    while (!done) e.run(1 << 20, done);
    e.sync();
    const double gmres_s = std::chrono::duration<double>(clk::now() - t1).count();
    fill_history(e, r);
    r->gmres_seconds = gmres_s;
    e.finish_report(r);
    out() << "  ilu took " << (float)r->setup_seconds << "s; gmres took " << (float)gmres_s << "s" << std::endl;
    out() << "  resNorm = " << r->res_norm << "; errNorm = " << r->err_norm << std::endl;
    return 0;
}

}  // namespace mpg

// ---------------------------------------------------------------- engine C-ABI

extern "C" {

int mpg_engine_create(const mpg_solve_args* a, mpg_engine_t* out, char* err, int errlen) {
    if (!a || !out) return MPG_ERR_ARG;
    *out = nullptr;
    auto* e = new mpg_engine();
    try {
        mpg::set_quiet(!a->verbose);
        mpg::check(mpg_ctx_create(a->device, &e->ctx), "mpg_ctx_create");
        mpg::ScopedContext scope(e->ctx);
        e->eng = std::make_unique<mpg::FusedEngine>(e->ctx, *a);
    } catch (const std::exception& ex) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", ex.what());
        mpg_engine_destroy(e);
        return MPG_ERR_ARG;
    }
    *out = e;
    return MPG_OK;
}

int mpg_engine_run(mpg_engine_t e, int max_cycles, int* done) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        bool d = false;
        const int ran = e->eng->run(max_cycles, d);
        if (done) *done = d ? 1 : 0;
        return ran;
    });
}

const char* mpg_engine_last_error(mpg_engine_t e) { return e ? e->last_error.c_str() : ""; }

int mpg_engine_rearm(mpg_engine_t e, const double* b, const double* x0, const double* x_true, int flags) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        e->eng->rearm(b, x0, x_true, flags);
        return (int)MPG_OK;
    });
}

int mpg_engine_refresh_values(mpg_engine_t e, const double* val, int64_t nnz, int flags) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    const int st = mpg::engine_call(e, [&] {
        e->eng->refresh_values(val, nnz, flags);
        return (int)MPG_OK;
    });
    if (st && !e->dead && e->eng->values_dirty()) {
        e->dead = st;
        e->dead_error = "the engine is dead: a values refresh failed after it began overwriting the matrix (" +
                        e->last_error + "); destroy it";
        e->last_error = e->dead_error;
    }
    return st;
}

int mpg_engine_guess_depth(mpg_engine_t e, int depth) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        e->eng->guess_depth(depth);
        return (int)MPG_OK;
    });
}

int mpg_engine_guess_keep(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        e->eng->guess_keep();
        return (int)MPG_OK;
    });
}

int mpg_engine_guess_info(mpg_engine_t e, int* held, int* depth, double* rho0, double* rho1, double* seconds) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    if (held) *held = e->eng->guess_held();
    if (depth) *depth = e->eng->guess_L();
    if (rho0) *rho0 = e->eng->guess_rho0;
    if (rho1) *rho1 = e->eng->guess_rho1;
    if (seconds) *seconds = e->eng->guess_seconds;
    return MPG_OK;
}

int mpg_engine_guess_store(mpg_engine_t e, double* Z, double* Q) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        e->eng->guess_store(Z, Q);
        return e->eng->guess_held();
    });
}

double mpg_engine_refresh_seconds(mpg_engine_t e) { return e && e->eng ? e->eng->refresh_seconds : -1.0; }

int mpg_engine_x(mpg_engine_t e, double* dst, int dst_on_device) {
    if (!e || !e->eng || !dst) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        e->eng->copy_x(dst, dst_on_device != 0);
        return (int)MPG_OK;
    });
}

int mpg_engine_solves(mpg_engine_t e) { return e && e->eng ? e->eng->solves() : MPG_ERR_ARG; }
int mpg_engine_graph_captures(mpg_engine_t e) { return e && e->eng ? e->eng->graph_captures() : MPG_ERR_ARG; }

int mpg_engine_sync(mpg_engine_t e) {
    if (!e) return MPG_ERR_ARG;
    return mpg_ctx_sync(e->ctx);
}

int64_t mpg_engine_total_iters(mpg_engine_t e) { return e && e->eng ? (int64_t)e->eng->total_iters() : -1; }

int mpg_engine_report(mpg_engine_t e, mpg_solve_result* r) {
    if (!e || !e->eng || !r) return MPG_ERR_ARG;
    const int st = mpg::engine_call(e, [&] {
        e->eng->sync();
        mpg::fill_history(*e->eng, r);
        e->eng->finish_report(r);
        return (int)MPG_OK;
    });
    if (st) std::snprintf(r->message, sizeof r->message, "%s", e->last_error.c_str());
    return st;
}

double mpg_engine_phase_bytes(mpg_engine_t e, int which) {
    return e && e->eng ? e->eng->phase_bytes(which) : 0.0;
}

int mpg_engine_spmv_layout(mpg_engine_t e, int32_t* format, int32_t* vec_width, int32_t* col_bytes,
                           int64_t* stored, int32_t* window) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_spmv_layout(e->eng->arnoldi(), format, vec_width, col_bytes, stored, window);
}

int mpg_engine_sell_columns(mpg_engine_t e, int32_t* form, int64_t* csr_slices, int64_t* implicit_slices) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_sell_columns(e->eng->arnoldi(), form, csr_slices, implicit_slices);
}

int mpg_engine_prec_fused(mpg_engine_t e) { return e && e->eng ? e->eng->prec_fused() : -1; }
int mpg_engine_prec_sweeps(mpg_engine_t e) { return e && e->eng ? e->eng->prec_sweeps() : -1; }
int mpg_engine_prec_roots(mpg_engine_t e, double* re, double* im, int32_t cap) {
    return e && e->eng ? e->eng->prec_roots(re, im, cap) : -1;
}
int mpg_engine_prec_interval(mpg_engine_t e, double* a, double* b) {
    return e && e->eng && e->eng->prec_interval(a, b) ? 0 : -1;
}
int mpg_engine_accum(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_accum(e->eng->arnoldi());
}
int mpg_engine_basis(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_basis(e->eng->arnoldi());
}
int mpg_engine_prec_values(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_prec_values(e->eng->arnoldi());
}

int mpg_engine_prologue_format(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_prologue_format(e->eng->arnoldi());
}

int mpg_engine_givens_folded(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return e->eng->policy().fold;
}

int mpg_engine_step_dots_steps(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return e->eng->step_dots_steps();
}

int mpg_engine_givens_rider(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return e->eng->givens_rider() ? 1 : 0;
}

int mpg_engine_tail_fold(mpg_engine_t e) {
    return e && e->eng ? (e->eng->tail_fold() ? 1 : 0) : -1;
}
int mpg_engine_cgs_stream_steps(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return e->eng->cgs_stream_steps();
}

int mpg_engine_cycle_policy(mpg_engine_t e, mpg_cycle_policy* out) {
    if (!e || !e->eng || !out) return MPG_ERR_ARG;
    *out = e->eng->policy();
    return MPG_OK;
}

int mpg_engine_step_dots_status(mpg_engine_t e, int k) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_step_dots_supported(e->eng->arnoldi(), k);
}

int mpg_engine_comm_ranks(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return e->comm ? e->comm->transport_ranks() : 1;
}

int64_t mpg_engine_sell_shared_slices(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_sell_shared_slices(e->eng->arnoldi());
}

int mpg_engine_sell_sigma(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_sell_sigma(e->eng->arnoldi());
}

int mpg_engine_slices_per_wave(mpg_engine_t e) {
    if (!e || !e->eng) return MPG_ERR_ARG;
    return mpg_arnoldi_slices_per_wave(e->eng->arnoldi());
}

int mpg_engine_half_stats(mpg_engine_t e, int64_t* stats) {
    if (!e || !e->eng || !stats) return MPG_ERR_ARG;
    for (int q = 0; q < 4; ++q) stats[q] = e->eng->half_stats()[q];
    return MPG_OK;
}

int mpg_engine_destroy(mpg_engine_t e) {
    if (!e) return MPG_OK;
    if (e->ctx) {
        {
            mpg::ScopedContext scope(e->ctx);
            e->eng.reset();
            e->comm.reset();
        }
        mpg_ctx_destroy(e->ctx);
    }
    delete e;
    return MPG_OK;
}

}  // extern "C"
