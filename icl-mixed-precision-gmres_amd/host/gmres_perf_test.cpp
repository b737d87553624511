// Derived from iamsonderr/icl-mixed-precision-gmres, Copyright (c) 2019-2021,
// University of Tennessee (BSD-3-Clause; the license text is in NOTICE).
// Command-line driver with the reference's flags and stdout lines
// (gmres_perf_test.cpp:309-455), running on MI355X through mpg_solve.
//
// Reference flags: --Apath --bpath --rlen --rtol --repeat-iter --orthloss
// --tol --max-restarts --rand --mode {mixed,baseline,single-prec,single}
// --orth {cgs,mgs,cgsr} --prec {ilu,identity,jacobi,ilu_jacobi}
// --jacobi-steps --gpu (accepted; this build always runs on the GPU).
// Additions: --matrix band:N[:LO:HI[:SEED]] | laplace:NX[:NY:NZ] |
// stencil27:NX[:DOF[:SEED]] (synthetic input instead of --Apath,
// mpg_gen_spec), --mode mixed-half, --half-unscaled (mixed-half: plain fp16
// cast, a value outside fp16's range is an error), --engine {fused,surface},
// --prec bjacobi [--prec-block {2,3,4}] (the inverse of each node's diagonal
// block; 3 unknowns per node unless told), --prec neumann [--jacobi-steps S]
// (S Jacobi sweeps on A z = r from z = 0, the truncated Neumann series;
// 1 <= S <= 64, S = 1 is --prec jacobi), --prec chebyshev [--jacobi-steps S]
// [--cheb-ratio R] [--cheb-lmax L] (the Chebyshev polynomial of S sweeps for a
// spectrum of D A near [b / R, b]: R > 1, default 30; b = L > 0, default the
// Gershgorin bound; the two flags set MPG_CHEB_RATIO / MPG_CHEB_LMAX for this
// process), --prec gmres_poly [--jacobi-steps S] (the GMRES polynomial of D A
// from S Arnoldi steps run once at set-up: S roots, no interval and no
// setting), --basis {f32,f16,f16emu} (the fused engine's Krylov basis in 2
// bytes per entry, fp16 of 2^14 v, all arithmetic in the Arnoldi precision:
// mode mixed, cgs / cgsr, rlen <= 32, one GPU; f16emu the same values as fp32;
// sets MPG_BASIS for this process, mpg_engine_basis in solve.h),
// --prec-values {f32,f16,f16emu} (the sweeps of --prec neumann / chebyshev /
// gmres_poly read an fp16 copy of A, 2 bytes per value and an int8 exponent per
// row; the Arnoldi SpMV and the residual keep theirs; mode mixed, one GPU;
// f16emu the same values as fp32 on CSR storage; sets MPG_PREC_VALUES for this
// process, mpg_engine_prec_values in solve.h),
// --device D, --stop-on-breakdown (end the solve with an error at the first
// non-finite Arnoldi residual; without it the count goes to stderr),
// --ngpus N (row-partition the fused solve over N GPUs of this process, one
// host thread per GPU, RCCL clique by ncclCommInitAll: mpg_solve_multi_gpu;
// devices --device .. --device+N-1; fails when fewer GPUs are visible),
// --solves N (N systems with the one matrix on one fused engine, set up once:
// mpg_engine_create, then mpg_engine_rearm per further system; the stdout
// block is printed once per solve; solve j takes x_true from --rand + j, or
// the --bpath vector every time; without the flag, or with N = 1, the one
// solve through mpg_solve as before), --vary-values EPS (with --solves N > 1:
// system j >= 1 has the matrix mpg_perturb_values(A, EPS, seed = j) on A's
// pattern and b_j = A_j x_true, given to the engine by
// mpg_engine_refresh_values before the re-arm; the stdout block is unchanged),
// --guess project [--guess-depth L] (with --solves N > 1: the engine keeps a
// store of its last solutions, at most L directions, default 8, and system
// j >= 1 starts from the least-squares guess in their span:
// mpg_engine_guess_depth, MPG_ARM_X0_PROJECT, mpg_engine_guess_keep; the stdout
// block is unchanged and the guess's residual norms go to stderr), --rhs-path K
// (x_true of system j is sum_{k < K} cos(0.37 (k + 1) j + k) rand_vect(--rand + k):
// the solutions of a sequence move in a K-dimensional space; not with --bpath).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "mpgmres/dist.h"
#include "mpgmres/problems.h"
#include "mpgmres/solve.h"

namespace {

double host_nrm2(const double* v, int64_t n) {
    double s = 0;
    for (int64_t i = 0; i < n; ++i) s += v[i] * v[i];
    return std::sqrt(s);
}

}  // namespace

int main(int argc, char* argv[]) {
    const char* a_path = nullptr;
    const char* b_path = nullptr;
    std::string synthetic;
    mpg_solve_args a{};
    a.rlen = 0;
    a.tol = 1e-6;
    a.max_restarts = 1000000;
    a.orth = MPG_ORTH_MGS;
    a.mode = MPG_MODE_MIXED;
    a.prec = MPG_PREC_ILU;
    a.jacobi_steps = 1;
    a.engine = MPG_ENGINE_FUSED;
    a.verbose = 1;
    unsigned rand_seed = 42;
    int ngpus = 0;  // 0: mpg_solve on one device
    int solves = 1;
    bool vary = false;  // --vary-values
    double vary_eps = 0.0;
    bool guess = false;    // --guess project
    int guess_depth = 8;   // --guess-depth
    int rhs_path = 0;      // --rhs-path (0: x_true = rand_vect(--rand + j))

    for (int i = 1; i < argc; ++i) {
        const std::string f = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) {
                std::cout << "Missing value for " << f << std::endl;
                std::exit(1);
            }
            return argv[++i];
        };
        if (f == "--Apath") a_path = next();
        else if (f == "--bpath") b_path = next();
        else if (f == "--matrix") synthetic = next();
        else if (f == "--rlen") a.rlen = std::stoi(next());
        else if (f == "--rtol") a.rtol = std::stod(next());
        else if (f == "--repeat-iter") a.repeat_iter = 1;
        else if (f == "--orthloss") a.orthloss = 1;
        else if (f == "--tol") a.tol = std::stod(next());
        else if (f == "--max-restarts") a.max_restarts = std::stol(next());
        else if (f == "--rand") rand_seed = (unsigned)std::stoi(next());
        else if (f == "--jacobi-steps") a.jacobi_steps = std::stoi(next());
        else if (f == "--prec-block") a.prec_block = std::stoi(next());
        else if (f == "--cheb-ratio") setenv("MPG_CHEB_RATIO", next(), 1);
        else if (f == "--cheb-lmax") setenv("MPG_CHEB_LMAX", next(), 1);
        else if (f == "--basis") setenv("MPG_BASIS", next(), 1);
        else if (f == "--prec-values") setenv("MPG_PREC_VALUES", next(), 1);
        else if (f == "--gpu") { /* always on the GPU */ }
        else if (f == "--device") a.device = std::stoi(next());
        else if (f == "--ngpus") ngpus = std::stoi(next());
        else if (f == "--solves") solves = std::stoi(next());
        else if (f == "--vary-values") {
            vary = true;
            vary_eps = std::stod(next());
        }
        else if (f == "--guess") {
            const std::string v = next();
            if (v != "project") { std::cout << "Unknown guess (project)" << std::endl; return 1; }
            guess = true;
        }
        else if (f == "--guess-depth") guess_depth = std::stoi(next());
        else if (f == "--rhs-path") rhs_path = std::stoi(next());
        else if (f == "--half-unscaled") a.half_unscaled = 1;
        else if (f == "--stop-on-breakdown") a.stop_on_breakdown = 1;
        else if (f == "--accum") {  // fp32 Arnoldi's accumulation class (solve.h)
            const std::string v = next();
            if (v == "f64") a.accum = 0;
            else if (v == "f32") a.accum = 1;
            else { std::cout << "Unknown accumulation (f64 | f32)" << std::endl; return 1; }
        }
        else if (f == "--mode") {
            const std::string v = next();
            if (v == "mixed") a.mode = MPG_MODE_MIXED;
            else if (v == "baseline") a.mode = MPG_MODE_BASELINE;
            else if (v == "single-prec") a.mode = MPG_MODE_SINGLE_PREC;
            else if (v == "single") a.mode = MPG_MODE_SINGLE;
            else if (v == "mixed-half") a.mode = MPG_MODE_MIXED_HALF;
            else { std::cout << "Unknown test mode" << std::endl; return 1; }
        } else if (f == "--orth") {
            const std::string v = next();
            if (v == "cgs") a.orth = MPG_ORTH_CGS;
            else if (v == "mgs") a.orth = MPG_ORTH_MGS;
            else if (v == "cgsr") a.orth = MPG_ORTH_CGSR;
            else { std::cout << "Unknown Orthogonalization" << std::endl; return 1; }
        } else if (f == "--prec") {
            const std::string v = next();
            if (v == "ilu") a.prec = MPG_PREC_ILU;
            else if (v == "identity") a.prec = MPG_PREC_IDENTITY;
            else if (v == "jacobi") a.prec = MPG_PREC_JACOBI;
            else if (v == "ilu_jacobi") a.prec = MPG_PREC_ILU_JACOBI;
            else if (v == "bjacobi") a.prec = MPG_PREC_BLOCK_JACOBI;
            else if (v == "neumann") a.prec = MPG_PREC_NEUMANN;
            else if (v == "chebyshev") a.prec = MPG_PREC_CHEBYSHEV;
            else if (v == "gmres_poly") a.prec = MPG_PREC_GMRES_POLY;
            else { std::cout << "Unknown Preconditioner" << std::endl; return 1; }
        } else if (f == "--engine") {
            const std::string v = next();
            if (v == "fused") a.engine = MPG_ENGINE_FUSED;
            else if (v == "surface") a.engine = MPG_ENGINE_SURFACE;
            else { std::cout << "Unknown engine" << std::endl; return 1; }
        } else {
            std::cout << "Unknown flag" << argv[i] << std::endl;
            return 1;
        }
    }
    if (a.repeat_iter && a.orthloss) {
        std::cout << "Repeated Iteration Restart cannot be used with OrthLoss restart" << std::endl;
        return 1;
    }
    if (a.rlen <= 0) {
        // the reference indexes an empty H when --rlen is missing
        std::cout << "A positive --rlen is required" << std::endl;
        return 1;
    }
    if (ngpus < 0 || (ngpus > 1 && a.engine != MPG_ENGINE_FUSED)) {
        std::cout << "--ngpus runs the fused engine on a positive number of GPUs" << std::endl;
        return 1;
    }
    if (!a_path && synthetic.empty()) {
        std::cout << "No value suplied for A" << std::endl;
        return 1;
    }
    if (solves < 1) {
        std::cout << "--solves takes a positive number of systems" << std::endl;
        return 1;
    }
    if (vary && solves < 2) {
        std::cout << "--vary-values changes the matrix between the systems of --solves N, N > 1" << std::endl;
        return 1;
    }
    if (vary && b_path) {
        std::cout << "--vary-values forms b_j = A_j x_true itself and cannot take --bpath" << std::endl;
        return 1;
    }
    if (guess && solves < 2) {
        std::cout << "--guess project starts the systems of --solves N, N > 1, from the earlier solutions" << std::endl;
        return 1;
    }
    if (rhs_path < 0 || (rhs_path > 0 && b_path)) {
        std::cout << "--rhs-path takes a positive number of directions and forms x_true itself (no --bpath)" << std::endl;
        return 1;
    }
    if (solves > 1 && (a.engine != MPG_ENGINE_FUSED || ngpus >= 1)) {
        // (the library's rule: mpg_engine_rearm exists on the fused engine, on one GPU)
        std::cerr << "mpg_solve failed: mpgmres: a sequence of solves on one engine (--solves) runs on the fused "
                     "engine on one GPU only: "
                  << (a.engine != MPG_ENGINE_FUSED ? "the operator surface's drivers set up one solve per call"
                                                   : "re-arming a row-partitioned engine is not available")
                  << std::endl;
        return 1;
    }

    mpg_host_csr A{};
    char err[256] = {0};
    if (a_path) {
        if (mpg_load_mtx(a_path, &A, err, sizeof err) != 0) {
            std::cerr << "LoadMatrix: " << err << std::endl;
            return 1;
        }
    } else {
        char e[256];
        if (mpg_gen_spec(synthetic.c_str(), &A, e, sizeof e) != 0) {
            std::cerr << e << std::endl;
            return 1;
        }
    }
    const int64_t n = A.nrows;
    std::vector<double> x_true((size_t)n), b((size_t)n);
    // x_true of system j: rand_vect(--rand + j), or the point j of --rhs-path's curve
    std::vector<std::vector<double>> path_dirs((size_t)rhs_path, std::vector<double>((size_t)n));
    for (int k = 0; k < rhs_path; ++k) mpg_rand_vect(n, rand_seed + (unsigned)k, path_dirs[(size_t)k].data());
    auto make_x_true = [&](int j) {
        if (rhs_path == 0) {
            mpg_rand_vect(n, rand_seed + (unsigned)j, x_true.data());
            return;
        }
        std::fill(x_true.begin(), x_true.end(), 0.0);
        for (int k = 0; k < rhs_path; ++k) {
            const double c = std::cos(0.37 * (k + 1) * j + k);
            for (int64_t i = 0; i < n; ++i) x_true[(size_t)i] += c * path_dirs[(size_t)k][(size_t)i];
        }
    };
    if (!b_path) {
        make_x_true(0);
        mpg_host_spmv(&A, x_true.data(), b.data());
    } else {
        std::fill(x_true.begin(), x_true.end(), 0.0);
        if (mpg_load_mtx_vector(b_path, 0, b.data(), n, err, sizeof err) != 0) {
            std::cerr << "LoadVector: " << err << std::endl;
            return 1;
        }
    }

    auto print_norms = [&] {
        std::cout << "||x|| = " << host_nrm2(x_true.data(), n) << std::endl;
        std::cout << "||b|| = " << host_nrm2(b.data(), n) << std::endl;
        std::cout << "||A|| = " << host_nrm2(A.val, A.nnz) << std::endl;
    };
    print_norms();

    a.n = (int32_t)n;
    a.nnz = A.nnz;
    a.rowptr = A.rowptr;
    a.col = A.col;
    a.val = A.val;
    a.b = b.data();
    a.x_true = x_true.data();
    mpg_solve_result r{};
    int st = 0;
    if (solves > 1) {
        // one engine, set up once; every further system re-arms it (solve.h)
        const char* banner = a.mode == MPG_MODE_MIXED || a.mode == MPG_MODE_MIXED_HALF ? "Doing Mixed Precision test"
                                                                                         : "Doing Baseline test";
        mpg_engine_t eng = nullptr;
        const std::vector<double> val0(A.val, A.val + (vary ? A.nnz : 0));
        for (int j = 0; j < solves && st == 0; ++j) {
            if (j > 0) {
                // --vary-values: system j's matrix, the first one's values perturbed with seed j
                if (vary) mpg_perturb_values(val0.data(), A.nnz, vary_eps, (uint64_t)j, A.val);
                if (!b_path) {
                    make_x_true(j);
                    mpg_host_spmv(&A, x_true.data(), b.data());
                }
                print_norms();
            }
            std::cout << banner << std::endl;
            if (j == 0) {
                st = mpg_engine_create(&a, &eng, r.message, (int)sizeof r.message);
                if (st == 0 && guess && (st = mpg_engine_guess_depth(eng, guess_depth)) != 0)
                    std::snprintf(r.message, sizeof r.message, "%s", mpg_engine_last_error(eng));
            } else {
                if (vary) st = mpg_engine_refresh_values(eng, A.val, A.nnz, 0);
                if (st == 0) st = mpg_engine_rearm(eng, b.data(), nullptr, x_true.data(), guess ? MPG_ARM_X0_PROJECT : 0);
                if (st != 0) std::snprintf(r.message, sizeof r.message, "%s", mpg_engine_last_error(eng));
            }
            if (st != 0) break;
            const auto t1 = std::chrono::steady_clock::now();
            int done = 0;
            while (!done && st == 0) {
                const int ran = mpg_engine_run(eng, 1 << 20, &done);
                if (ran < 0) {
                    st = ran;
                    std::snprintf(r.message, sizeof r.message, "%s", mpg_engine_last_error(eng));
                }
            }
            if (st != 0) break;
            mpg_engine_sync(eng);
            const double gmres_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
            r = mpg_solve_result{};
            st = mpg_engine_report(eng, &r);
            if (st != 0) break;
            std::cout << "  ilu took " << (float)r.setup_seconds << "s; gmres took " << (float)gmres_s << "s" << std::endl;
            std::cout << "  resNorm = " << r.res_norm << "; errNorm = " << r.err_norm << std::endl;
            if (guess) {
                // (stderr: the stdout block stays the reference's)
                int held = 0, depth = 0;
                double rho0 = 0, rho1 = 0, secs = 0;
                mpg_engine_guess_info(eng, &held, &depth, &rho0, &rho1, &secs);
                if (j > 0)
                    std::cerr << "guess: system " << j << ": ||b - A x0|| " << rho0 << " -> " << rho1 << " from " << held
                              << " of " << depth << " directions" << std::endl;
                st = mpg_engine_guess_keep(eng);
                if (st != 0) std::snprintf(r.message, sizeof r.message, "%s", mpg_engine_last_error(eng));
            }
        }
        mpg_engine_destroy(eng);
    } else if (ngpus >= 1 && !(ngpus == 1 && a.engine != MPG_ENGINE_FUSED)) {
        std::vector<int32_t> devices((size_t)ngpus);
        for (int q = 0; q < ngpus; ++q) devices[(size_t)q] = a.device + q;
        std::cout << (a.mode == MPG_MODE_MIXED || a.mode == MPG_MODE_MIXED_HALF ? "Doing Mixed Precision test"
                                                                                : "Doing Baseline test")
                  << std::endl;
        st = mpg_solve_multi_gpu(&a, ngpus, devices.data(), &r, nullptr);
        if (st == 0) {
            std::cout << "  ilu took " << (float)r.setup_seconds << "s; gmres took " << (float)r.gmres_seconds << "s"
                      << std::endl;
            std::cout << "  resNorm = " << r.res_norm << "; errNorm = " << r.err_norm << std::endl;
        }
    } else {
        st = mpg_solve(&a, &r);
    }
    mpg_host_csr_free(&A);
    // (stderr: the stdout lines stay the reference's, automated.py:33-38)
    if (r.nonfinite_steps > 0 || r.nonfinite_cycles > 0)
        std::cerr << "warning: breakdown: " << r.nonfinite_steps << " Arnoldi step(s) with a non-finite |s(k+1)| "
                  << "(first at step " << r.first_nonfinite_step << " of the history) and " << r.nonfinite_cycles
                  << " restart(s) with a non-finite residual norm; --stop-on-breakdown ends the solve there"
                  << std::endl;
    if (st != 0) {
        std::cerr << "mpg_solve failed: " << r.message << std::endl;
        return 1;
    }
    return 0;
}
