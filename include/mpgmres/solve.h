/*
 * mpgmres solve C-ABI: one call = one restarted GMRES(m) solve of A x = b,
 * set up and reported the way the reference's perf-test driver does
 * (gmres_perf_test.cpp:53-182 DoBaselineProblem / DoMixedPrecisionProblem):
 * x0 = 0, timer around the GMRES call only, then resNorm = ||b - A x|| with
 * the original fp64 A and errNorm = ||x - x_true||.
 *
 * Beyond the reference (additions): mpg_solve_from starts from an initial
 * guess, and a live fused engine takes further systems with the same matrix
 * (mpg_engine_rearm: a new b, an initial guess, vectors in host or device
 * memory; mpg_engine_x reads the iterate back) without repeating the set-up --
 * the matrix copies, the preconditioner, the cycle policy and the captured
 * cycle graph are kept.
 *
 * The same argument/result structs are used by the HIP path
 * (libmpgmres_host.so: mpg_solve) and by the CPU oracle under oracle/
 * (liboracle.so: oracle_solve), so parity tests can run both on one input.
 */
#ifndef MPGMRES_SOLVE_H
#define MPGMRES_SOLVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gmres_perf_test.cpp:31-36 test_mode_t, plus a new fp16-value mode */
typedef enum {
    MPG_MODE_MIXED = 0,       /* fp64 residual/update, fp32 Arnoldi (gmres_singleUpdate) */
    MPG_MODE_BASELINE = 1,    /* fp64 GMRES on double(float(A)) (gmres_baseline<d,d>) */
    MPG_MODE_SINGLE_PREC = 2, /* fp64 GMRES, fp32 preconditioner (gmres_baseline<d,f>) */
    MPG_MODE_SINGLE = 3,      /* fp32 GMRES (gmres_baseline<f,f>) */
    MPG_MODE_MIXED_HALF = 4   /* like MIXED, but the inner SpMV reads fp16 values (new) */
} mpg_mode_t;

/* gmres_perf_test.cpp:17-22 orth_t */
typedef enum { MPG_ORTH_CGS = 0, MPG_ORTH_MGS = 1, MPG_ORTH_CGSR = 2 } mpg_orth_t;

/* gmres_perf_test.cpp:24-29 prec_t (same numbering) */
typedef enum {
    MPG_PREC_ILU = 0,
    MPG_PREC_ILU_JACOBI = 1,
    MPG_PREC_JACOBI = 2,
    MPG_PREC_IDENTITY = 3,
    MPG_PREC_BLOCK_JACOBI = 4, /* new: the inverse of each node's diagonal block (mpg_bjacobi_*, capi.h) */
    MPG_PREC_NEUMANN = 5, /* new: jacobi_steps Jacobi sweeps on A z = r from z = 0, the truncated Neumann series
                             sum_{j<s} (I - D A)^j D with Jacobi's D (mpg_*_jacobi_sweep_*, capi.h); s = 1 is
                             MPG_PREC_JACOBI's bits */
    MPG_PREC_CHEBYSHEV = 6, /* new: the Chebyshev polynomial of degree jacobi_steps - 1 in D A applied to D r, for a
                              spectrum of D A near [b / ratio, b] (mpg_*_cheb_sweep_*, capi.h; mpg_cheb_coeffs and
                              mpg_engine_prec_interval below). b: the Gershgorin bound of D A, or MPG_CHEB_LMAX
                              (a real > 0); ratio: MPG_CHEB_RATIO (a real > 1, default 30); both read once when the
                              preconditioner is set up. For spectra on the positive real axis: a banded matrix whose
                              D A has a disc around 1 wants a small ratio, or MPG_PREC_NEUMANN */
    MPG_PREC_GMRES_POLY = 7 /* new: the GMRES polynomial of D A: p(D A) D r with 1 - x p(x) = prod (1 - x / theta_i),
                               theta_i the jacobi_steps harmonic Ritz values of jacobi_steps Arnoldi steps on D A run
                               once at set-up (mpg_gmres_poly_roots and mpg_engine_prec_roots below;
                               mpg_*_poly_sweep_*, capi.h). No interval and no setting; nonsymmetric spectra give
                               complex pairs */
} mpg_prec_t;

typedef enum {
    MPG_ENGINE_SURFACE = 0,  /* generic driver over the kernels.hpp operator surface */
    MPG_ENGINE_FUSED = 1     /* fused Arnoldi kernels, device-side Givens, graph-captured cycles */
} mpg_engine_kind_t;

typedef enum { MPG_RESULT_CONVERGED = 1, MPG_RESULT_ABORTED = 3, MPG_RESULT_ERROR = -1 } mpg_result_status_t;

typedef struct {
    /* CSR matrix, 0-based int32 indices, fp64 values (host memory) */
    int32_t n;
    int64_t nnz;
    const int32_t* rowptr;
    const int32_t* col;
    const double* val;
    const double* b;       /* right-hand side (host, n) */
    const double* x_true;  /* for errNorm (host, n); may be NULL */
    int32_t mode, orth, prec, engine;
    int32_t rlen;          /* restart length m (--rlen) */
    double tol;            /* --tol */
    int64_t max_restarts;  /* --max-restarts */
    double rtol;           /* --rtol (0: base Convergence) */
    int32_t repeat_iter;   /* --repeat-iter */
    int32_t orthloss;      /* --orthloss */
    int32_t jacobi_steps;  /* --jacobi-steps: sweeps of MPG_PREC_ILU_JACOBI's solves; MPG_PREC_NEUMANN's,
                              MPG_PREC_CHEBYSHEV's and MPG_PREC_GMRES_POLY's sweep count s, 1 <= s <= 64 (anything else MPG_ERR_ARG) */
    int32_t verbose;       /* print the reference's stdout lines */
    int32_t device;        /* HIP device (mpg_solve only) */
    int32_t threads;       /* host threads (oracle only; 0 = default) */
    int32_t spmv_format;   /* fused engine Arnoldi SpMV: 0 auto, 1 CSR row blocks, 2 SELL-64,
                              3 node blocks (3-dof nodes, 3 x 3 blocks) */
    int32_t half_unscaled; /* mode mixed-half: 0 = fp16 values scaled per row by powers of two where
                              a row's magnitude needs it (mpg_csr_half_values, capi.h); 1 = plain
                              cast: a value outside fp16's range fails the set-up (MPG_ERR_RANGE) */
    int32_t stop_on_breakdown; /* 1: stop at the first non-finite |s(k+1)| or restart residual and
                                  return MPG_ERR_BREAKDOWN (--stop-on-breakdown); 0: the reference's
                                  behaviour (Orthogonalization.hpp:56-59 divides unguarded and the
                                  restart loop runs on), the count is only reported */
    int32_t accum;         /* fp32 Arnoldi's accumulation class (MPG_ACCUM_F64 0 / MPG_ACCUM_F32 1,
                              arnoldi.h): 1 keeps every dot, norm, gemv and SpMV partial sum in fp32 --
                              the class of the reference's cblas_s* / mkl_sparse_s_mv (--accum f32);
                              fused engine only (the operator surface refuses it: MPG_ERR_UNSUPPORTED);
                              ignored by an fp64 Arnoldi and by the oracle */
    int32_t prec_block;    /* MPG_PREC_BLOCK_JACOBI: unknowns per node, 2, 3 or 4 (0: 3; anything else
                              MPG_ERR_ARG); n must be a multiple of it. Appended last: a caller compiled
                              against the struct without it (the oracle) reads the same layout */
} mpg_solve_args;

typedef struct {
    int32_t status;           /* mpg_result_status_t */
    int64_t restarts;         /* value of i when the solver returned */
    int64_t inner_k;          /* k when converged inside a cycle, else 0 */
    int64_t total_iters;
    double res_norm, err_norm;
    double gmres_seconds, setup_seconds;
    double minvb_norm;
    /* caller-provided outputs (may be NULL / zero capacity) */
    double* x_out;            /* n */
    int64_t cycle_cap;        /* capacity of the per-cycle arrays */
    int64_t n_cycles;         /* number of check_initial calls recorded */
    double* cyc_r_norm;       /* true residual norm at each restart */
    double* cyc_normalization;/* ||b|| + ||A||_F ||x|| */
    double* cyc_beta;         /* preconditioned residual norm */
    int64_t step_cap;
    int64_t n_steps;          /* number of check calls recorded */
    double* step_res;         /* |s(k+1)| per Arnoldi step */
    int32_t* step_cycle;      /* cycle index of each step */
    char message[256];        /* error text when status == MPG_RESULT_ERROR */
    /* breakdown report (not a reference decision: the solve runs as the
       reference's does unless args->stop_on_breakdown) */
    int64_t nonfinite_steps;  /* Arnoldi steps whose |s(k+1)| was NaN/Inf (h_{k+1,k} = 0 or
                                 non-finite makes the normalisation 1/h non-finite) */
    int64_t nonfinite_cycles; /* restarts whose true residual norm or beta was NaN/Inf */
    int64_t first_nonfinite_step; /* index of the first such step in the step history, -1: none */
} mpg_solve_result;

/* HIP path (libmpgmres_host.so). Returns 0 on success (result->status tells
 * converged/aborted), < 0 on error (result->message). */
int mpg_solve(const mpg_solve_args* args, mpg_solve_result* result);
/* mpg_solve from the initial guess x0 (host, n; an addition to the reference's set, whose drivers start from
 * zeros): the iterate starts as x0 rounded once to the solve's outer type, and the first restart's true residual is
 * b - A x0. x0 == NULL is mpg_solve. Fused engine only: with the operator-surface engine and a non-NULL x0 the
 * call returns MPG_ERR_UNSUPPORTED and the message names the fused engine. The same bits as mpg_engine_rearm with
 * that x0 on an engine created from `args`. */
int mpg_solve_from(const mpg_solve_args* args, const double* x0, mpg_solve_result* result);

/* ---- stepped access to the fused engine (benchmarks, multi-GPU ranks) ----
 * mpg_engine_create uploads the problem, builds the preconditioner, zeroes
 * x and runs the first residual prologue. mpg_engine_run advances the
 * restarted solve by up to `max_cycles` outer iterations exactly as
 * mpg_solve does (check_initial on the host once per cycle, graph-replayed
 * cycle on the device) and returns the number of cycles run; *done is set
 * when the solve converged or aborted. All timing is left to the caller. */
typedef struct mpg_engine* mpg_engine_t;
int mpg_engine_create(const mpg_solve_args* args, mpg_engine_t* out, char* err, int errlen);
int mpg_engine_run(mpg_engine_t e, int max_cycles, int* done);
/* the error text of the last engine call that failed ("" otherwise) */
const char* mpg_engine_last_error(mpg_engine_t e);
/* ---- a sequence of systems on one engine (an addition to the reference's set) ----
 * mpg_engine_rearm starts another solve with the engine's matrix: a new right-hand side b (NULL: keep the current
 * one), an initial guess x0 (NULL: zeros) and a new x_true for errNorm (host, n; NULL: none -- it is copied, the
 * caller's array may go after the call). b and x0 are fp64 arrays of n in host memory, or in the memory of the
 * engine's device where `flags` says so (MPG_ARM_B_DEVICE, MPG_ARM_X0_DEVICE; the caller's own work on them must
 * have completed). It runs the part of mpg_engine_create that depends on b and x -- the casts to the solve's types,
 * ||b||, ||M^-1 b||, the first residual prologue -- and resets the solve's host state (history, counts, status, the
 * convergence strategy, the breakdown report), so the solve that follows has the bits of a new engine created with
 * these vectors. Nothing else is redone: the storage copies of A, the preconditioner, ||A||_F, the cycle policy and
 * the captured cycle graph are kept, and no buffer moves. Allowed after a converged, aborted, broken-down or
 * unfinished solve (nothing is in flight when mpg_engine_run returns). After it, mpg_engine_report reports the new
 * solve only, and its setup_seconds is the duration of the re-arm.
 * MPG_ERR_ARG: e is NULL (nothing is touched). MPG_ERR_UNSUPPORTED, the reason in mpg_engine_last_error: a
 * row-partitioned engine (the norms and the halo of x0 would have to cross the ranks), or an engine that ran
 * measurement launches (mpg_engine_time_*; mpg_engine_run's rule and text). */
#define MPG_ARM_B_DEVICE 1
#define MPG_ARM_X0_DEVICE 2
/* the initial guess is projected from the engine's guess store (below): x starts as project(b, x0) */
#define MPG_ARM_X0_PROJECT 4
int mpg_engine_rearm(mpg_engine_t e, const double* b, const double* x0, const double* x_true, int flags);
/* ---- the initial guess projected from earlier solutions (an addition to the reference's set) ----
 * An engine with guess depth L, 1 <= L <= MPG_GUESS_MAX_DEPTH (16, capi.h), owns two fp64 column-major panels Z and Q
 * of n x L on the device and a count held <= L, with Q(:, j) = A Z(:, j) and Q^T Q = I; A is the matrix of the
 * residual prologue (the fp64 A; in mode baseline double(float(A))).
 *   project(b, xbar): r = b - A xbar (one mpg_csr_spmv_f64, skipped for xbar = 0), c = Q^T r, x0 = xbar + Z c:
 *     ||b - A x0|| = ||(I - Q Q^T) r|| is the least over xbar + span Z and never above ||r||. rho0 = ||r||, and the
 *     predicted rho1 = sqrt(max(0, ||r||^2 - ||c||^2)). Two launches (mpg_guess_dots_f64, mpg_guess_update_f64).
 *   keep(x): w = A x, d = x, omega = ||w||; classical Gram-Schmidt twice (h = Q^T w, w -= Q h, d -= Z h); nu = ||w||;
 *     unless nu or omega is not finite or nu <= max(tol, n 2^-53) omega (a direction below what the solves resolve),
 *     Q(:, held) = w / nu, Z(:, held) = d / nu, held += 1. With held == L on entry, held = 0 first (Fischer's restart:
 *     the newest solution alone reseeds the store). The SpMV and four launches. Allowed whatever the solve's status.
 *   after mpg_engine_refresh_values the images are stale: the next project, keep or store read first keeps the held
 *     Z columns again, in order, from an empty store (held SpMVs and their orthogonalisation; counted in the guess
 *     store's seconds, not in mpg_engine_refresh_seconds).
 * mpg_engine_guess_depth allocates the store (L = 0 frees it; another L empties it; the same L is a no-op). With
 * MPG_ARM_X0_PROJECT in mpg_engine_rearm's flags the re-arm writes project(b, x0) where it writes x0 (x0 NULL: zeros).
 * mpg_engine_guess_keep runs keep() on the x the engine holds. mpg_engine_guess_info reads the count, the depth, rho0
 * and rho1 of the last projection and the wall-clock seconds of every project, keep and re-imaging so far (any
 * pointer may be NULL). mpg_engine_guess_store copies the held columns to host (n x held each, column-major, leading
 * dimension n; either may be NULL) and returns held. Without a depth nothing is allocated and no launch is made.
 * MPG_ERR_UNSUPPORTED with the reason in mpg_engine_last_error, the engine left usable: a row-partitioned engine; an
 * engine that ran measurement launches; modes single and single-prec (an fp32 outer type or preconditioner bounds
 * the solves near 1e-7: no guess worth a cycle); MPG_ARM_X0_PROJECT or mpg_engine_guess_keep without a depth.
 * MPG_ERR_ARG: e is NULL, or L outside [0, 16]. */
int mpg_engine_guess_depth(mpg_engine_t e, int depth);
int mpg_engine_guess_keep(mpg_engine_t e);
int mpg_engine_guess_info(mpg_engine_t e, int* held, int* depth, double* rho0, double* rho1, double* seconds);
int mpg_engine_guess_store(mpg_engine_t e, double* Z, double* Q);
/* ---- new matrix values on the unchanged sparsity pattern (Newton steps, time steps, parameter sweeps) ----
 * mpg_engine_refresh_values gives a live engine a new A with the pattern it was created with: val holds nnz fp64
 * values in CSR order, in host memory or, with MPG_REFRESH_VAL_DEVICE in `flags`, in the memory of the engine's
 * device (the caller's own work on them must have completed; they are only read). It runs the part of
 * mpg_engine_create that reads the values -- the fp64 copy, the residual and the Arnoldi matrix in their types,
 * Jacobi's diagonal, the Chebyshev interval, the GMRES-polynomial roots, the block-Jacobi inverses, the ILU factors
 * (the factor object is made again), ||A||_F -- and refills the storage copies in place (mpg_arnoldi_refresh_values).
 * Kept: the CSR analysis, the SELL-64 / node-block layouts, the Arnoldi workspace, the cycle policy, every address,
 * and the captured cycle graph where none of its launch arguments changed (identity, jacobi, bjacobi, neumann); with
 * chebyshev, gmres_poly, ilu and ilu_jacobi the graph is released and captured again by the next solve
 * (mpg_engine_graph_captures counts it). The engine is then UNARMED: ||M^-1 b|| and the first residual depend on the
 * new A, so mpg_engine_rearm must follow (b == NULL keeps b), and mpg_engine_run before it fails with MPG_ERR_ARG and
 * a message that says so. The solve that follows has the bits of a new engine created on these values;
 * mpg_engine_report's res_norm uses them. setup_seconds stays the re-arm's; mpg_engine_refresh_seconds is the
 * duration of the last refresh (0 before the first, -1 for NULL).
 * Nothing is touched and the engine stays usable on its old matrix when the call returns MPG_ERR_ARG (e is NULL, or
 * nnz is not the engine's), MPG_ERR_UNSUPPORTED with the reason in mpg_engine_last_error (a row-partitioned engine;
 * an engine that ran measurement launches; mode mixed-half where the engine was created on values that needed no row
 * scaling -- it runs the unscaled kernels -- and the new ones need it) or MPG_ERR_RANGE (mixed-half values that do not
 * fit fp16). The operator surface has no live engine, so no refresh. Any other failure -- an ILU zero pivot, an
 * allocation -- comes after the overwriting began: the engine is dead, and every later call that works on the solve
 * (run, rearm, refresh, x, report) returns that status and text; only mpg_engine_destroy is left. */
#define MPG_REFRESH_VAL_DEVICE 1
int mpg_engine_refresh_values(mpg_engine_t e, const double* val, int64_t nnz, int flags);
double mpg_engine_refresh_seconds(mpg_engine_t e);
/* rows [0, n) of the engine's iterate x widened to fp64 into dst (n entries; host memory, or the engine's device
 * where dst_on_device != 0); synchronises the engine's stream before it returns. MPG_ERR_ARG: e or dst is NULL. */
int mpg_engine_x(mpg_engine_t e, double* dst, int dst_on_device);
/* solves armed on the engine so far, mpg_engine_create's included (>= 1); MPG_ERR_ARG: e is NULL */
int mpg_engine_solves(mpg_engine_t e);
/* cycle graphs the engine has captured so far: 1 once a solve has replayed the cycle, however many solves
 * followed; 0 for an engine that runs eagerly or step by step (MPG_NO_GRAPH, the stepwise strategies);
 * MPG_ERR_ARG: e is NULL */
int mpg_engine_graph_captures(mpg_engine_t e);
int mpg_engine_sync(mpg_engine_t e);
int64_t mpg_engine_total_iters(mpg_engine_t e);
/* The solve so far as mpg_solve reports it: status, counts, the per-cycle
 * and per-step history, this rank's rows of x (result->x_out) and resNorm /
 * errNorm with the fp64 matrix (gmres_perf_test.cpp:104-117). Collective on a
 * row-partitioned engine (the norms are all-reduced). */
int mpg_engine_report(mpg_engine_t e, mpg_solve_result* result);
/* device-event timing of one phase kernel replayed `reps` times on the
 * engine's stream, back to back, averaged over the steps k = 0..m-1 of a
 * cycle (which: 0 = Arnoldi SpMV k_step_spmv, 1 = residual prologue,
 * 2 = CGS update, 3 = Gram-Schmidt panel dots) */
int mpg_engine_time_phase(mpg_engine_t e, int which, int reps, double* avg_ms);
/* the Arnoldi SpMV as it runs inside the cycle (Givens folded for k >= 1),
 * timed by each launch's own kernel events over `cycles` eager cycles:
 * returns the launch count (m per cycle), the mean in *avg_ms and up to
 * `cap` per-launch times in cycle order (measurement only: the cycles run
 * without the host's restart checks) */
int mpg_engine_time_spmv_incycle(mpg_engine_t e, int cycles, double* avg_ms, double* per_launch_ms, int cap);
/* a phase kernel's share of the stream inside graph replays of the cycle
 * (which: 0 the Arnoldi SpMV in the form each step runs, 2 the CGS update, 3
 * the panel dots): the cycle captured as the solve runs it and with every
 * launch of that phase issued twice in a row, replayed alternately `reps`
 * times between HIP events; *avg_ms = the median difference of the replay
 * times over the added launches (*launches, may be NULL) -- kernel plus
 * dispatch and release, as rocprofv3's kernel durations. MPG_ERR_UNSUPPORTED
 * when the engine runs eagerly. Measurement only. */
int mpg_engine_time_phase_dup(mpg_engine_t e, int which, int reps, double* avg_ms, int64_t* launches);
/* a phase kernel's own duration inside graph replays of the cycle (which: 2
 * the one-panel CGS update k_cgs_update_nc, 3 the one-panel dots k_dots_nc;
 * the SpMV stores no stamps): every launch of that phase in a captured cycle
 * stores its waves' wall-clock stamps (mpg_arnoldi_stamp_next), duration =
 * last wave end - first wave start; per-launch ms in cycle order, the launch
 * count returned (MPG_ERR_UNSUPPORTED when the engine runs eagerly or no
 * launch of the phase was a stamped form). Measurement only. */
int mpg_engine_time_phase_stamps(mpg_engine_t e, int which, int reps, double* avg_ms, double* per_launch_ms,
                                 int cap);
/* a phase kernel timed inside graph replays of the cycle (which: 0 the
 * Arnoldi SpMV, 2 the CGS update, 3 the panel dots): the cycle captured with
 * an event-record node on each side of every launch of that phase,
 * replayed `reps` times; per-launch times in cycle order (step k), the
 * launch count returned (m per replay for 0; MPG_ERR_UNSUPPORTED when the
 * engine runs eagerly). Measurement only, like the in-cycle timing above. */
int mpg_engine_time_phase_graph(mpg_engine_t e, int which, int reps, double* avg_ms, double* per_launch_ms,
                                int cap);
/* algorithmic bytes of one launch of phase `which` */
double mpg_engine_phase_bytes(mpg_engine_t e, int which);
/* storage of the engine's Arnoldi SpMV (mpg_arnoldi_spmv_layout) */
int mpg_engine_spmv_layout(mpg_engine_t e, int32_t* format, int32_t* vec_width, int32_t* col_bytes,
                           int64_t* stored, int32_t* window);
/* column form of the engine's SELL copy (mpg_arnoldi_sell_columns) */
int mpg_engine_sell_columns(mpg_engine_t e, int32_t* form, int64_t* csr_slices, int64_t* implicit_slices);
/* slices of the engine's SELL copy reading a shared column block (mpg_arnoldi_sell_shared_slices) */
int64_t mpg_engine_sell_shared_slices(mpg_engine_t e);
/* the engine's SELL-C-sigma window (mpg_arnoldi_sell_sigma; 0 unsorted) */
int mpg_engine_sell_sigma(mpg_engine_t e);
/* 1: the Givens step of step k-1 rides SpMV(k) (mpg_arnoldi_fold_pays); 0: its own launch */
int mpg_engine_givens_folded(mpg_engine_t e);
/* steps of a restart cycle that run the SpMV inside the panel dots' launch
 * (mpg_arnoldi_step_dots; MPG_STEP_DOTS), and the status that launch's
 * support check gives at step k (MPG_OK / MPG_ERR_UNSUPPORTED) */
int mpg_engine_step_dots_steps(mpg_engine_t e);
int mpg_engine_step_dots_status(mpg_engine_t e, int k);
/* 1: those launches carry the Givens step of step k-1 on a workgroup of its own, the
 * last of the grid (k_step_dots' rider); 0: no such launch, or the step is not folded */
int mpg_engine_givens_rider(mpg_engine_t e);
/* 1: the cycle ends with the givens+update launch (mpg_arnoldi_update_tail; MPG_TAIL_FOLD), 0: it does not */
int mpg_engine_tail_fold(mpg_engine_t e);
/* CGS update launches of a restart cycle that take the streaming form
 * (mpg_arnoldi_cgs_stream_at over the cycle's cgs_partials ops; MPG_CGS_PREFETCH) */
int mpg_engine_cgs_stream_steps(mpg_engine_t e);
/* block Jacobi: 1 when the apply runs inside the SpMV / residual launches, 0 when it is a
 * launch of its own between them and the dots; -1 for every other preconditioner */
int mpg_engine_prec_fused(mpg_engine_t e);
/* MPG_PREC_NEUMANN, MPG_PREC_CHEBYSHEV, MPG_PREC_GMRES_POLY: the sweep count the engine applies per preconditioner
 * application (jacobi_steps: one gdmv launch and that many minus one sweep launches; for MPG_PREC_GMRES_POLY the
 * number of roots, smaller than jacobi_steps where the set-up's Arnoldi found an invariant subspace); -1 for every
 * other preconditioner */
int mpg_engine_prec_sweeps(mpg_engine_t e);
/* MPG_PREC_CHEBYSHEV (an addition to the reference's set): the interval [*a, *b] the engine built its
 * coefficients for; returns 0, or -1 for every other preconditioner (a and b untouched) */
int mpg_engine_prec_interval(mpg_engine_t e, double* a, double* b);
/* The Chebyshev preconditioner's coefficients (an addition to the reference's set) for `steps` sweeps on the
 * interval [theta - delta, theta + delta], 0 < delta < theta: with sigma = theta / delta and rho_0 = 1 / sigma,
 *   alpha[0] = 1 / theta (z_1 = alpha[0] D r), beta[0] = 0, and for j = 1 .. steps - 1
 *   rho_j = 1 / (2 sigma - rho_{j-1});  alpha[j] = rho_j rho_{j-1};  beta[j] = 2 rho_j / delta
 * in fp64, in that operation order, without contraction; sweep j is
 *   z_{j+1} = z_j + alpha[j] (z_j - z_{j-1}) + beta[j] D (r - A z_j),  z_0 = 0.
 * alpha, beta: `steps` entries each. Both engines call it and round each value once to the vectors' type.
 * MPG_ERR_ARG: steps outside [1, 64], a NULL array, or not 0 < delta < theta (finite). Host arithmetic only. */
int mpg_cheb_coeffs(int steps, double theta, double delta, double* alpha, double* beta);
/* MPG_PREC_GMRES_POLY (an addition to the reference's set): the roots the engine applies, in the order it applies
 * them. Returns their count (mpg_engine_prec_sweeps' value) and stores the first min(count, cap) into re / im
 * (either may be NULL with cap == 0); -1 for every other preconditioner. */
int mpg_engine_prec_roots(mpg_engine_t e, double* re, double* im, int32_t cap);
/* The GMRES polynomial's roots (an addition to the reference's set) from the (s + 1) x s Hessenberg matrix of s
 * Arnoldi steps, H[i * ldh + j] = h_{i+1,j+1}, 1 <= s <= 64, ldh >= s: the harmonic Ritz values, that is the
 * eigenvalues of H_s + h^2 f e_s^T, h = h_{s+1,s}, H_s^T f = e_s solved by elimination with partial pivoting (h == 0:
 * the eigenvalues of H_s, the Ritz values of an invariant subspace). Eigenvalues by a shifted Hessenberg QR iteration
 * with Francis double steps, in fp64 without contraction; a 2 x 2 block with discriminant >= 0 gives two real
 * roots, else a pair with the same bits of re and opposite im. Returned in Leja order: first the root of largest
 * modulus, then each time the one that maximises sum_j log |theta - theta_j| over the members already placed (both
 * members of a placed pair); a pair takes two consecutive places, its im > 0 member first; ties go to the root the
 * iteration stored at the lower index. *count = s. MPG_ERR_ARG: s or ldh out of range, a NULL argument, h not
 * finite. MPG_ERR_BREAKDOWN: H_s singular to the elimination (with h != 0), the iteration not converged (*count =
 * the row it stopped at), or a root that is not finite or is zero (*count = its index before ordering). Host
 * arithmetic only. */
int mpg_gmres_poly_roots(int s, const double* H, int ldh, double* re, double* im, int* count);
/* the accumulation class the engine's Arnoldi runs: MPG_ACCUM_F64 0 / MPG_ACCUM_F32 1 (arnoldi.h) */
int mpg_engine_accum(mpg_engine_t e);
/* The storage of the engine's Krylov basis: MPG_BASIS_F32 0 / MPG_BASIS_F16 1 / MPG_BASIS_F16EMU 2
 * (mpg_arnoldi_set_basis, arnoldi.h). Chosen by the setting MPG_BASIS = f32 (default) / f16 / f16emu, read once when
 * the engine is created (any other value: MPG_ERR_ARG naming it). f16 stores each basis entry in 2 bytes (fp16 of
 * 2^14 v) and keeps all arithmetic in the Arnoldi precision; it costs at most about 2^-11 of orthonormality per
 * cycle (a cycle cannot reduce the residual by more than ~2.5e-4). It runs on the fused engine on one GPU, mode mixed,
 * orth cgs / cgsr, rlen <= 32, CSR or SELL storage (auto picks among the two), with every preconditioner and the
 * base and rtol strategies, in the plain launch forms (as under MPG_STEP_DOTS=0 MPG_CGS_PREFETCH=0 MPG_TAIL_FOLD=0;
 * asking for a fused form is MPG_ERR_UNSUPPORTED). Anything else -- another mode, mgs, rlen > 32, --orthloss, forced
 * node blocks, a row-partitioned engine, the operator-surface engine, f16emu on SELL -- is MPG_ERR_UNSUPPORTED with
 * the reason in the message. f16emu: the same values held as fp32, for tests. */
int mpg_engine_basis(mpg_engine_t e);
/* The matrix values the sweeps of MPG_PREC_NEUMANN (jacobi_steps >= 2), MPG_PREC_CHEBYSHEV and MPG_PREC_GMRES_POLY read:
 * MPG_PREC_VALUES_F32 0 / MPG_PREC_VALUES_F16 1 / MPG_PREC_VALUES_F16EMU 2 (mpg_arnoldi_set_prec_copy, arnoldi.h). Chosen
 * by the setting MPG_PREC_VALUES = f32 (default: the Arnoldi matrix itself, nothing allocated, no launch changed) / f16 /
 * f16emu, read once when the engine is created (any other value: MPG_ERR_ARG naming it). f16: the sweeps read A^ =
 * mpg_csr_half_values(A, scale = 1), 2 bytes per value and one int8 exponent per row, as an MPG_F16 SELL copy where the
 * Arnoldi SpMV runs on a SELL copy and in CSR order otherwise; the Arnoldi SpMV, the residual, Jacobi's diagonal, the
 * Chebyshev interval and the GMRES-polynomial roots stay on the fp32 and fp64 values. Values that do not fit (fp16 after
 * the row scaling, the int8 exponent, fp32 once unscaled) are MPG_ERR_RANGE at create and at mpg_engine_refresh_values,
 * where the engine keeps its matrix. It runs on the fused engine on one GPU in mode mixed; a preconditioner without
 * sweeps, another mode, a row-partitioned engine, the operator-surface engine and f16emu on SELL or node-block storage
 * are MPG_ERR_UNSUPPORTED with the reason in the message. f16emu: A^ held as fp32 values on CSR row blocks, for tests. */
int mpg_engine_prec_values(mpg_engine_t e);
/* the residual prologue's storage (mpg_arnoldi_prologue_format: 1 CSR, 2 SELL, 3 node blocks) */
int mpg_engine_prologue_format(mpg_engine_t e);
/* ranks of the engine's communicator as its transport reports them: 1 for a
 * single-GPU engine, ncclCommCount for an RCCL rank, the world size for the
 * host transport; < 0 on error */
int mpg_engine_comm_ranks(mpg_engine_t e);
/* slices per wave of the engine's SELL Arnoldi SpMV (mpg_arnoldi_slices_per_wave) */
int mpg_engine_slices_per_wave(mpg_engine_t e);
/* mode mixed-half: stats[4] of the fp16 cast (mpg_csr_half_values); zeros otherwise */
int mpg_engine_half_stats(mpg_engine_t e, int64_t* stats);
int mpg_engine_destroy(mpg_engine_t e);

/* ---- the fused engine's restart cycle as data ----
 * What decides the launches of a cycle, resolved once when the engine is
 * created (environment, ranks, preconditioner, what the workspace supports).
 * Flags are 0 / 1 unless said. The per-step arrays hold the first
 * MPG_CYCLE_POLICY_STEPS steps; a later step counts as unsupported (both
 * launches stop at 32 columns). */
#define MPG_CYCLE_POLICY_STEPS 128
typedef struct {
    int32_t ranks;        /* 0: one GPU, no communicator; else the ranks of the row-partitioned solve (1 included) */
    int32_t orth;         /* mpg_orth_t */
    int32_t m;            /* restart length */
    int32_t graph;        /* the cycle is captured and replayed (MPG_NO_GRAPH, capturable collectives) */
    int32_t pipeline;     /* cycles start with a snapshot of x (MPG_PIPELINE) */
    int32_t fold;         /* Givens(k-1) rides SpMV(k) (MPG_FOLD_GIVENS; agreed across ranks) */
    int32_t combine;      /* last-arriver combines (MPG_COMBINE) */
    int32_t cgs_partials; /* the CGS update sums the dots' partials itself (MPG_CGS_PARTIALS) */
    int32_t fuse_dots, fuse_dots_required, fuse_dots_k0; /* MPG_FUSE_DOTS (= 2: required), MPG_FUSE_DOTS_K0 */
    int32_t step_dots;    /* MPG_STEP_DOTS: 0 never, 1 wherever supported, 2 required, -1 the steps lo <= k + 1 <= hi */
    int32_t step_dots_lo, step_dots_hi;
    int32_t sep_prec;          /* a preconditioner that is not applied inside the phase kernels (ILU, block Jacobi,
                                  the Jacobi-sweep, Chebyshev and GMRES polynomials) */
    int32_t sep_prec_step;     /* ... a launch of its own after every SpMV */
    int32_t sep_prec_prologue; /* ... and after the residual prologue */
    int32_t partials_max_cols; /* mpg_arnoldi_partials_max_cols() */
    int32_t fold_max_m;        /* mpg_arnoldi_fold_max_m() */
    uint8_t step_dots_ok[MPG_CYCLE_POLICY_STEPS]; /* mpg_arnoldi_step_dots_supported(k) == MPG_OK */
    uint8_t spmv_dots_ok[MPG_CYCLE_POLICY_STEPS]; /* mpg_arnoldi_spmv_dots_supported(k) == MPG_OK */
    int32_t tail_fold;         /* one GPU, m <= 32: the last Givens step, update(m) and the x snapshot in one launch
                                  (MPG_TAIL_FOLD, mpg_arnoldi_update_tail_supported); 0: their own launches */
} mpg_cycle_policy;
/* The launches and collectives of one restart cycle under `p`, in order, as
 * text: one token per op, separated by single spaces, NUL-terminated and cut
 * at len - 1 characters. Returns the length the whole text needs (without
 * the NUL), or a status < 0: MPG_ERR_UNSUPPORTED (-5) where a required
 * launch (step_dots / fuse_dots = 2) cannot be taken, MPG_ERR_ARG (-2).
 * A token is name, name(a) or name(a,b) -- the step k, then the pass, the
 * column j, the fold form or the column count: x_snapshot halo(k) halo(x)
 * allreduce_partials+halo(k) spmv(k) givens+spmv(k) spmv_dots(k,f)
 * step_dots(k,f) apply_prec(wK) dots(k) dots_sums(k) allreduce_partials(nc)
 * reduce(nc) allreduce_sums(nc) cgs_partials(k) cgs(k,pass)
 * cgs_givens(k,pass) cgsr_wide_pass(k,pass) mgs_partials(k,j) givens(k)
 * givens_partials(k) update(k) prologue prologue_wnorm prologue_finish
 * prologue_finish_partials -- followed, where the op is a site of the phase
 * timers, by @P (P as `which` of mpg_engine_time_phase: 0 SpMV, 1 prologue,
 * 2 CGS update, 3 dots), then +dup where mpg_engine_time_phase_dup issues it
 * twice, then <D where the op D tokens back is issued again ahead of the
 * duplicate: "cgs_partials(3)@2+dup<1". */
int mpg_cycle_plan_describe(const mpg_cycle_policy* p, char* buf, int len);
/* the resolved policy of a live engine */
int mpg_engine_cycle_policy(mpg_engine_t e, mpg_cycle_policy* out);

/* process-wide counts of the operator-surface driver's cycle programs
 * (CycleProgram<Hip>, types_hip.hpp): cycles recorded into a graph, cycles
 * replayed from one, and recordings voided by a step that must read the
 * device (those cycles then run eagerly). Any pointer may be NULL. */
int mpg_cycle_program_counts(int64_t* recorded, int64_t* replayed, int64_t* voided);
/* the calling thread's counts of the operator surface's normalisation ride
 * (kernels_hip.cpp, MPG_SURFACE_FUSE bit 16): CGS updates that kept w's new
 * value apart, normalisations that rode the next SpMV, and those issued
 * separately instead (a call other than the SpMV came next). Any pointer
 * may be NULL. */
int mpg_surface_ride_counts(int64_t* redirects, int64_t* rides, int64_t* flushed);
/* The operator surface's spmv calls on this thread so far, by the storage
 * they ran on: node blocks (mpg_node_spmv_*), SELL-64, CSR. Pointers may be
 * NULL. */
int mpg_surface_spmv_counts(int64_t* node, int64_t* sell, int64_t* csr);
/* Host-value nrm2 calls of the operator surface on this thread answered from
 * the memo of the same vector's previous read (MPG_SURFACE_FUSE bit 32: no
 * device work issued through the surface in between, nothing deferred). */
int mpg_surface_host_norm_hits(int64_t* hits);
/* Host-value nrm2 calls of the operator surface on this thread that also
 * read the norm of the vector the preceding residual SpMV (alpha -1, beta 1)
 * took as input, in one launch (mpg_nrm2_pair_host; MPG_SURFACE_FUSE bit
 * 64): that vector's next host nrm2 is then a memo hit. */
int mpg_surface_host_norm_pairs(int64_t* pairs);

#ifdef __cplusplus
}
#endif
#endif /* MPGMRES_SOLVE_H */
