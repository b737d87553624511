// Fused Arnoldi engine: restarted GMRES(m) on one GPU (or one rank of a
// row-partitioned solve) with one host synchronisation per restart cycle.
//
// Same outer control flow as the drivers in gmres_impl.hpp (and the
// reference gmres.cpp:24-245): check_initial on the true residual at every
// restart, m Arnoldi steps, solution update. The cycle itself is the phase
// program of include/mpgmres/arnoldi.h, captured once into a hipGraph and
// replayed every cycle (steps 0..m-1, the solution update and the next
// residual prologue); the host reads back one small report block per cycle
// (r_norm, beta, ||x||, |s(k+1)| for every step). Strategies that look at
// |s(k+1)| inside a cycle run the same program step by step instead.
#ifndef MPGMRES_FUSED_GMRES_HPP
#define MPGMRES_FUSED_GMRES_HPP

#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "IterUtil.hpp"
#include "cycle_plan.hpp"
#include "mpgmres/arnoldi.h"
#include "mpgmres/capi.h"
#include "mpgmres/solve.h"
#include "types_hip.hpp"

namespace mpg {

// prec neumann, prec chebyshev and prec gmres_poly (MPG_PREC_NEUMANN,
// MPG_PREC_CHEBYSHEV, MPG_PREC_GMRES_POLY; `name`
// in the messages): the sweep count and the modes they run in,
// checked by both engines before any set-up. The sweeps run in the Arnoldi
// precision on the Arnoldi matrix, so the preconditioner precision has to be
// that precision (not mode single-prec) and the matrix has to exist in it
// (not mode mixed-half, whose inner operator is the fp16 copy).
inline void check_sweep_prec_args(const mpg_solve_args& a, const std::string& name) {
    if (a.jacobi_steps < 1 || a.jacobi_steps > 64)
        throw std::invalid_argument("prec " + name + ": jacobi_steps = " + std::to_string(a.jacobi_steps) +
                                    " is outside [1, 64]");
    if (a.mode == MPG_MODE_SINGLE_PREC)
        throw StatusError(MPG_ERR_UNSUPPORTED,
                          "prec " + name + " is not available in mode single-prec: the sweeps run in the Arnoldi "
                          "precision and would need A in a second precision");
    if (a.mode == MPG_MODE_MIXED_HALF)
        throw StatusError(MPG_ERR_UNSUPPORTED, "prec " + name + " is not available in mode mixed-half: the inner "
                                               "operator is the fp16 copy of A");
}
inline void check_neumann_args(const mpg_solve_args& a) { check_sweep_prec_args(a, "neumann"); }
inline void check_cheb_args(const mpg_solve_args& a) { check_sweep_prec_args(a, "chebyshev"); }
inline void check_gmres_poly_args(const mpg_solve_args& a) { check_sweep_prec_args(a, "gmres_poly"); }

// The Krylov basis' storage (mpg_arnoldi_set_basis), from the setting
// MPG_BASIS = f32 (default) / f16 / f16emu, read once when an engine is
// created; any other value is MPG_ERR_ARG naming it.
int basis_setting();
const char* basis_name(int basis);
// A compressed or emulated basis runs on the fused engine on one GPU, mode
// mixed, CGS / CGSR, rlen <= 32, CSR or SELL storage (f16emu: CSR), without
// --orthloss: anything else is MPG_ERR_UNSUPPORTED naming the reason.
// surface / ranks: the caller is the operator-surface engine / a rank of a
// row-partitioned solve.
void check_basis_args(const mpg_solve_args& a, int basis, bool surface, bool ranks);

// The matrix values the polynomial preconditioners' sweeps read
// (mpg_arnoldi_set_prec_copy), from the setting MPG_PREC_VALUES = f32 (default)
// / f16 / f16emu, read once when an engine is created; any other value is
// MPG_ERR_ARG naming it.
int prec_values_setting();
const char* prec_values_name(int kind);
// An fp16 or emulated copy runs on the fused engine on one GPU, mode mixed,
// under prec neumann (two sweeps or more), chebyshev and gmres_poly (f16emu:
// CSR row blocks): anything else is MPG_ERR_UNSUPPORTED naming the reason.
void check_prec_values_args(const mpg_solve_args& a, int kind, bool surface, bool ranks);

// Communication seam of the row-partitioned solve: a single-GPU engine has
// no communicator; a multi-GPU rank supplies one (see comm.hpp).
class Comm {
public:
    virtual ~Comm() {}
    virtual int size() const = 0;
    virtual int rank() const = 0;
    // in-place sum / max of `count` doubles across ranks (bit-identical on every rank)
    virtual void allreduce_sum(double* dev, int count, hipStream_t s) = 0;
    virtual void allreduce_max(double* dev, int count, hipStream_t s) = 0;
    // fill the halo entries [-n_front, 0) and [n, n_ext) of a vector of
    // `elem_bytes` elements (passed as a pointer to its row 0)
    virtual void halo(void* dev_vec, int elem_bytes, hipStream_t s) = 0;
    // allreduce_sum and halo together (independent inputs): one RCCL group,
    // i.e. one collective launch per Arnoldi step instead of two
    virtual void allreduce_sum_and_halo(double* dev, int count, void* dev_vec, int elem_bytes, hipStream_t s) {
        allreduce_sum(dev, count, s);
        halo(dev_vec, elem_bytes, s);
    }
    // whether the collectives may be captured into a hipGraph (no host waits)
    virtual bool capturable() const = 0;
    // device-side transport (RCCL) whose collectives can hang or fail
    // asynchronously: the engine then waits with a bounded poll
    // (FusedEngine::wait_event) instead of a blocking synchronise
    virtual bool async() const { return false; }
    // "" or the transport's asynchronous error (ncclCommGetAsyncError)
    virtual std::string async_error() { return {}; }
    // tear the communicator down so that pending collectives return
    // (ncclCommAbort); called on the owning rank's thread only
    virtual void abort() {}
    // another rank failed: from any thread, ask the owning rank to abort
    // (RCCL: a flag its bounded wait polls, then abort() on its own thread)
    virtual void request_abort() { abort(); }
    // ranks the transport itself reports (RCCL: ncclCommCount), -1 when it
    // cannot say; the caller's size() otherwise
    virtual int transport_ranks() { return size(); }
};

// RAII device buffer through the C-ABI allocator
struct DevMem {
    mpg_ctx_t ctx = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    DevMem() = default;
    DevMem(mpg_ctx_t c, size_t b);
    ~DevMem();
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept { *this = std::move(o); }
    DevMem& operator=(DevMem&& o) noexcept;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

void hipck(hipError_t e, const char* what);  // throws std::runtime_error on a HIP runtime error

// What `build` issues on the stream, captured and instantiated: the graph
// pair is owned here and destroyed on every path. The constructor throws
// when the capture, the build or the instantiation fails (nothing is left
// capturing and the runtime's error state is cleared).
struct CapturedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    CapturedGraph() = default;
    CapturedGraph(hipStream_t s, const std::function<void()>& build);
    ~CapturedGraph() { reset(); }
    CapturedGraph(const CapturedGraph&) = delete;
    CapturedGraph& operator=(CapturedGraph&& o) noexcept {
        std::swap(graph, o.graph), std::swap(exec, o.exec);
        return *this;
    }
    void reset();
};

class FusedEngine {
public:
    // `rows`/`halo` describe the local row block of a partitioned matrix
    // (global columns already remapped to [0, n_ext)); a single GPU passes the
    // whole matrix and no communicator.
    // n_front: halo rows of lower ranks, local ids [-n_front, 0) (dist.h)
    // x0: the initial guess (host fp64, n; one GPU only), nullptr: zeros
    FusedEngine(mpg_ctx_t ctx, const mpg_solve_args& args, Comm* comm = nullptr, int n_ext = -1, int n_front = 0,
                const double* x0 = nullptr);
    ~FusedEngine();

    // Advance the solve by up to max_cycles outer iterations; returns the
    // number run. `done` is set on convergence or abort.
    int run(int max_cycles, bool& done);
    void finish_report(mpg_solve_result* r);  // resNorm/errNorm + x with the original fp64 A

    // Start another solve on this engine (mpg_engine_rearm, solve.h): a new
    // right-hand side (b == nullptr: keep the current one), an initial guess
    // (x0 == nullptr: zeros) and a new x_true (host, may be nullptr), through
    // the code the constructor arms its own solve with. b / x0 are fp64
    // arrays of n in host memory, or on the engine's device where `flags`
    // says so (MPG_ARM_B_DEVICE, MPG_ARM_X0_DEVICE). The matrix copies, the
    // preconditioner, the policy, the captured cycle and every buffer stay as
    // they are. Refused (MPG_ERR_UNSUPPORTED) on a row-partitioned engine and
    // after measurement launches.
    void rearm(const double* b, const double* x0, const double* x_true, int flags);
    // New values of A on the unchanged sparsity pattern (mpg_engine_refresh_values,
    // solve.h): nnz fp64 values in CSR order, in host memory or on the
    // engine's device (MPG_REFRESH_VAL_DEVICE), through the code the
    // constructor loads its own values with. The CSR analysis, the storage
    // layouts, the workspace, the policy and every address stay; the engine is
    // left unarmed (rearm must follow). Refused with nothing touched: a wrong
    // nnz (MPG_ERR_ARG), a row-partitioned or measured engine, mixed-half
    // values the engine's kernels cannot take. A failure after that
    // (values_dirty()) leaves the engine without a consistent matrix.
    void refresh_values(const double* val, int64_t nnz, int flags);
    bool values_dirty() const { return values_dirty_; }
    double refresh_seconds = 0;  // the last refresh_values, wall clock (0: none yet)
    // rows [0, n) of x widened to fp64 into dst (host, or the engine's device); synchronises
    void copy_x(double* dst, bool dst_on_device);
    // ---- the initial-guess store (mpg_engine_guess_*, solve.h) ----
    // fp64 panels Z, Q = A Z with Q^T Q = I of the last few solutions, A the
    // residual prologue's matrix. Off (depth 0) until guess_depth(L) allocates
    // it: no buffer and no launch otherwise. Every entry point is refused
    // (MPG_ERR_UNSUPPORTED) on a row-partitioned engine, after measurement
    // launches and in the modes whose outer type is fp32.
    void guess_depth(int L);  // 0 frees the store; another L empties it
    void guess_keep();        // keep() on the x the engine holds
    void guess_store(double* Z, double* Q);  // the held columns to host, n x held each, column-major, ld = n
    int guess_held() const;
    int guess_L() const;
    double guess_rho0 = 0, guess_rho1 = 0;  // the last projection: ||b - A xbar|| and the predicted ||b - A x0||
    double guess_seconds = 0;               // wall clock of every project, keep and re-imaging so far
    int solves() const { return solves_; }                  // arms so far, the constructor's included
    int graph_captures() const { return graph_captures_; }  // cycle graphs captured so far

    size_t total_iters() const { return conv_->total_iterations(); }
    double time_phase(int which, int reps, bool inplace = false, std::vector<double>* per_launch = nullptr);
    double time_phase_graph(int which, int reps, std::vector<double>* per_launch = nullptr);
    double time_phase_stamps(int which, int reps, std::vector<double>* per_launch = nullptr);
    double time_phase_dup(int which, int reps, int64_t* launches = nullptr, bool step_dots_only = false);
    double phase_bytes(int which) const;
    mpg_arnoldi_t arnoldi() const;
    int basis() const;  // mpg_engine_basis
    int prec_values() const;  // mpg_engine_prec_values
    // mixed-half: what the fp16 cast of the Arnoldi values did (stats of
    // mpg_csr_half_values, capi.h; zeros in other modes)
    const int64_t* half_stats() const;
    int prec_fused() const;  // mpg_engine_prec_fused
    int prec_sweeps() const;  // mpg_engine_prec_sweeps
    bool prec_interval(double* a, double* b) const;  // mpg_engine_prec_interval
    int prec_roots(double* re, double* im, int cap) const;  // mpg_engine_prec_roots
    int cgs_stream_steps() const;      // CGS update launches of a cycle that take the streaming form
    int step_dots_steps() const;       // steps of a cycle that run the SpMV inside the dots' launch
    bool givens_rider() const;         // ... and one of them folds the Givens step (k_step_dots' rider workgroup)
    bool tail_fold() const;            // the cycle ends with the givens+update launch (mpg_arnoldi_update_tail)
    void sync();
    const CyclePolicy& policy() const;  // mpg_engine_cycle_policy

    // history (per restart / per step)
    std::vector<CycleRecord> cycles;
    std::vector<double> step_res;
    std::vector<int> step_cycle;
    int status = 0;          // MPG_RESULT_*
    int64_t restarts = 0;
    int64_t inner_k = 0;
    double minvb_norm = 0, b_norm = 0, a_norm = 0;
    double setup_seconds = 0;
    BreakdownLog breakdown;  // non-finite |s(k+1)| / restart residuals (IterUtil.hpp)
    // set by every time_phase*: the measurement launches (duplicated kernels,
    // cycles run without the host's checks) change V, H, w and x, so run()
    // refuses to continue the solve afterwards
    bool measured = false;

private:
    struct Impl;
    std::unique_ptr<Impl> p_;
    std::unique_ptr<Convergence<double, void>> conv_;
    int solves_ = 0, graph_captures_ = 0;
    bool armed_ = false;         // a solve is armed on the engine's current matrix (arm; refresh_values clears it)
    bool values_dirty_ = false;  // load_values began overwriting a live engine's matrix and has not finished
    // what depends on the values of A: the constructor's and refresh_values' one code path
    void load_values(const double* val, bool on_device);
    // what depends on b and x: the constructor's and rearm's one code path
    void arm(const double* b, const double* x0, const double* x_true, int flags);
    void start();  // the first residual prologue of a solve and its report
    void guess_check(const char* what) const;  // the refusals of the guess store's entry points
    void guess_project(bool have_base);        // x <- x + Z Q^T (b - A x) (arm, MPG_ARM_X0_PROJECT)
    void guess_keep_vec(const double* x_dev);  // keep() on a device vector of n
    void guess_reimage();                      // after refresh_values: Q = A Z again, column by column
    void prologue();
    void step(int k, bool fold);
    void issue(const Op& op);
    void issue(const std::vector<Op>& ops);
    // the phase timers (fused_timing.cpp) walk the cycle's op list themselves
    const std::vector<Op>& cycle_ops() const;
    hipStream_t stream() const;
    mpg_ctx_t ctx() const;
    void require_captured_phase(int which);
    void update(int k);
    void store_next_basis(int k);
    double orth_loss_step(size_t k);
    void read_report(int count);
    void wait_event(hipEvent_t ev, int64_t cycle, const char* what);
    void ensure_graph();
    void record_steps(int64_t i);
    int run_pipelined(int max_cycles, bool& done);
    int run_cycles(int max_cycles, bool& done);
    bool check_start(int64_t i);
};

// x0: the initial guess (host fp64, n), nullptr: zeros (mpg_solve_from)
int solve_fused(const mpg_solve_args& args, mpg_solve_result* result, const double* x0 = nullptr);
// status, counts and the per-cycle / per-step history of an engine into r
void fill_history(const FusedEngine& e, mpg_solve_result* r);

}  // namespace mpg

// handle behind mpg_engine_t (solve.h / dist.h)
struct mpg_engine {
    mpg_ctx_t ctx = nullptr;
    std::unique_ptr<mpg::Comm> comm;          // declared first: destroyed after eng
    std::unique_ptr<mpg::FusedEngine> eng;
    std::string last_error;  // the text of the last failed mpg_engine_run
    // a values refresh that failed after it began overwriting the matrix: the
    // engine is dead, and every call that works on the solve returns this
    int dead = 0;
    std::string dead_error;
};

namespace mpg {
// A C-ABI call into the engine on its context: what `f` returns (>= 0), or
// the status of what it threw, with the text kept for mpg_engine_last_error.
template <class F>
int engine_call(mpg_engine_t e, F&& f) {
    if (e->dead) {
        e->last_error = e->dead_error;
        return e->dead;
    }
    e->last_error.clear();
    try {
        ScopedContext scope(e->ctx);
        return f();
    } catch (const StatusError& ex) {
        e->last_error = ex.what();
        return ex.status;
    } catch (const std::exception& ex) {
        e->last_error = ex.what();
        return MPG_ERR_HIP;
    }
}
}  // namespace mpg

#endif  // MPGMRES_FUSED_GMRES_HPP
