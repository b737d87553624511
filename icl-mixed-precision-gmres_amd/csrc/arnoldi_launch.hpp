// Launch code of the fused Arnoldi phases, templated on the accumulation
// class A of the fp32-Arnoldi kernels (arnoldi_spmv.hpp, arnoldi_dots.hpp,
// arnoldi_orth.hpp, arnoldi_update.hpp): arnoldi.hip instantiates A = double
// for every type combination, arnoldi_acc32.hip A = float for the
// fp32-Arnoldi combinations only (mpg_arnoldi_set_accum), each in its own
// translation unit so the two builds compile in parallel. Each hands its
// launches out as one table (mpg_arnoldi_phases, phases_of<A>).
#pragma once

#include "arnoldi_dots.hpp"
#include "arnoldi_orth.hpp"
#include "arnoldi_update.hpp"

#include <algorithm>
#include <cstdlib>
#include <tuple>
#include <type_traits>

namespace {

// the type combinations an accumulation class exists for: A = double for all
// of them, A = float for the fp32 Arnoldi (single, mixed, mixed-half) only
template <class A, class F>
int dispatch_acc(int combo, F&& f) {
    if constexpr (std::is_same_v<A, double>) {
        return dispatch(combo, f);
    } else {
        switch (combo) {
            case 2: return f(float(), float(), float(), float());
            case 3: return f(float(), double(), float(), float());
            case 4: return f(float(), double(), float(), half_v());
            default: return MPG_ERR_UNSUPPORTED;
        }
    }
}

template <class A>
int reduce_run(mpg_arnoldi_t a, int ncols) {
    if (!a || ncols < 1 || ncols > a->d.m + 4) return MPG_ERR_ARG;
    // one column per workgroup: 256 threads when the producer left <= 512
    // partials per column (one or two loads per thread), else 1024
    // (the once-per-cycle prologue keeps fp64 sums in the fp32 class too, arnoldi.h: the bits of
    // mpg_arnoldi_prologue_finish_partials' own column sums)
    if (a->last_prologue) {
        if (a->last_G <= 2 * kBlock) k_reduce_partials<kBlock, double><<<ncols, kBlock, 0, a->ctx->stream>>>(a->last_G, a->last_part, a->sums);
        else k_reduce_partials<1024, double><<<ncols, 1024, 0, a->ctx->stream>>>(a->last_G, a->last_part, a->sums);
    } else if (a->last_G <= 2 * kBlock) k_reduce_partials<kBlock, A><<<ncols, kBlock, 0, a->ctx->stream>>>(a->last_G, a->last_part, a->sums);
    else k_reduce_partials<1024, A><<<ncols, 1024, 0, a->ctx->stream>>>(a->last_G, a->last_part, a->sums);
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

// fold: 0 plain; 1 Givens(k-1) folded, ||w||^2 from sums[0]; 2 from the partials.
// dots: the panel dots fused (SellDots; MPG_ERR_UNSUPPORTED where the SELL
// copy, an fp32 basis with fp32 values, int16 columns and the window are
// not all present -- the caller then launches the dots itself).
// workgroup of the SELL step kernel without fused dots (4 slices per 256)
#ifndef MPG_STEP_SELL_BLOCK
#define MPG_STEP_SELL_BLOCK 256
#endif
constexpr int kStepSellBlock = MPG_STEP_SELL_BLOCK;
using kBlockC = std::integral_constant<int, kBlock>;

// The argument list of a SELL kernel (the step's and the prologue's): the
// slices of S with values of type V, the kernel's own operands `mid` behind
// them, the slices' patterns and CSR-summed rows, and the kernel's `tail`.
template <class CI, class V, class... M, class... E>
auto sell_args(const mpg_arnoldi* a, const SellCopy& S, std::tuple<M...> mid, std::tuple<E...> tail) {
    return std::tuple_cat(std::make_tuple(a->d.n, -a->front, a->d.n_ext, S.nslices, S.off, static_cast<const CI*>(S.col),
                                          static_cast<const V*>(S.val)),
                          mid,
                          std::make_tuple(S.sbase, S.spat, S.coff, static_cast<const CI*>(S.pat), S.xrp, S.xcol,
                                          static_cast<const V*>(S.xval)),
                          tail);
}

// launch_timed of an argument tuple
template <class K, class... X>
int launch_tuple(mpg_ctx* c, K kern, dim3 grid, dim3 block, const std::tuple<X...>& args) {
    std::apply([&](auto... x) { launch_timed(c, kern, grid, block, x...); }, args);
    return MPG_OK;
}

// the status spmv_run(a, k, fold, dots = true) returns ahead of its launch
template <class A>
int spmv_dots_check(const mpg_arnoldi* a, int k) {
    if (!a || k < 0 || k >= a->d.m) return MPG_ERR_ARG;
    if (!std::is_same_v<A, double> || a->basis != MPG_BASIS_F32 || a->d.n <= 0 || a->sell.nslices == 0 || !a->sell.c16 || !a->sell.win ||
        (a->combo != 2 && a->combo != 3) || k + 1 > kNC || a->d.orth == kOrthMGS)
        return MPG_ERR_UNSUPPORTED;
    return MPG_OK;
}

// The kernels with a compressed or emulated basis (mpg_arnoldi_set_basis) are
// built for an fp32 Arnoldi on fp32 values; set_basis admits no other workspace.
template <class T, class VI>
constexpr bool kBasisBuilt = std::is_same_v<T, float> && std::is_same_v<VI, float>;
inline bool plain_basis(const mpg_arnoldi* a) { return a->basis == MPG_BASIS_F32; }
inline bool half_basis(const mpg_arnoldi* a) { return a->basis == MPG_BASIS_F16; }

template <class A>
int spmv_run(mpg_arnoldi_t a, int k, int fold, bool dots) {
    if (!a || k < 0 || k >= a->d.m) return MPG_ERR_ARG;
    if (dots && !plain_basis(a)) return MPG_ERR_UNSUPPORTED;  // (the fused dots read an fp32 basis)
    if (dots)
        if (int st = spmv_dots_check<A>(a, k)) return st;
    if (fold && (k < 1 || a->d.m > kFoldMaxM)) return MPG_ERR_ARG;
    // (no node blocks under set_basis; of the CSR kernel's measurement modes only the default is built)
    if (!plain_basis(a) && (a->node.nblk > 0 || (a->sell.nslices == 0 && csr_mode() != 0))) return MPG_ERR_UNSUPPORTED;
    const mpg_csr* Acsr = a->d.A;
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto, auto p, auto vi) {
        using T = decltype(t);
        using P = decltype(p);
        using VI = decltype(vi);
        const P* diag = a->d.jacobi ? static_cast<const P*>(a->d.diag) : nullptr;
        GivensFold<T> gf{nullptr, 0, {}};
        if (fold)
            gf = GivensFold<T>{fold == 2 ? a->last_part : a->sums, fold == 2 ? a->last_G : 0, givens_args<T>(a, k - 1)};
        if (a->sell.nslices > 0) {
            const auto& S = a->sell;
            if (fold == 2 && a->last_G > kBlock) return (int)MPG_ERR_ARG;  // k_step_sell folds <= kBlock partials
            return sell_dispatch(S, [&](auto ci, auto wc) {
                using CI = decltype(ci);
                constexpr int Wc = decltype(wc)::value;
                // the step kernels' arguments (k_step_sell takes a sorted copy's rows behind them)
                // (a compressed V travels as T*: the kernels view it through basis_ptr)
                auto args = [&](SellDots dd) {
                    return sell_args<CI, typename SellStore<VI>::type>(
                        a, S,
                        std::make_tuple(static_cast<const T*>(a->w[k & 1]), static_cast<const T*>(a->inv()),
                                        static_cast<T*>(a->V), a->ld, k, diag, static_cast<T*>(a->w[(k + 1) & 1]), gf, dd),
                        std::make_tuple(a->d.inner_row_exp, S.ustride, sell_xcd_order(S) ? 1 : 0));
                };
                auto launch = [&](auto kern, SellDots dd, auto bs) {
                    constexpr int BS = decltype(bs)::value;
                    const int grid = (S.nslices + BS / kWave - 1) / (BS / kWave);
                    return launch_tuple(a->ctx, kern, dim3(grid), dim3(BS), std::tuple_cat(args(dd), std::make_tuple(S.rows)));
                };
                if constexpr (std::is_same_v<T, float> && std::is_same_v<VI, float> &&
                              std::is_same_v<CI, int16_t> && std::is_same_v<A, double>) {
                    if (dots) {
                        const SellDots dd{k + 1, a->fd_gs, a->fd_ng, a->fd_part, a->fd_cnt, a->dpart};
                        auto pick = [&](auto dn) {
                            constexpr int DN = decltype(dn)::value;
                            return with_flag(fold, [&](auto fo) {
                                return launch(k_step_sell<T, P, VI, CI, Wc, true, decltype(fo)::value, DN, kBlock, false, false, A>,
                                              dd, kBlockC());
                            });
                        };
                        if (k + 1 <= 8) return pick(std::integral_constant<int, 8>());
                        if (k + 1 <= 16) return pick(std::integral_constant<int, 16>());
                        return pick(std::integral_constant<int, 32>());
                    }
                }
                return sell_dispatch_win(S.win, [&](auto wn) {
                    constexpr bool WN = decltype(wn)::value;
                    using BSC = std::integral_constant<int, kStepSellBlock>;
                    const int be = sell_uniform(S) ? sell_pair(S) : 0;
                    if constexpr (std::is_same_v<CI, int16_t> && (Wc == 2 || Wc == 4)) if (be) {
                        // two slices per wave, at BE entries per row: 8 and 12, and 10 (Wc == 2, pregathered)
                        auto pair = [&](auto bec, auto pgc) {
                            return with_flag(fold, [&](auto fo) {
                                const int grid = (S.nslices + 2 * (kStepSellBlock / kWave) - 1) / (2 * (kStepSellBlock / kWave));
                                if constexpr (kBasisBuilt<T, VI>) {
                                    if (half_basis(a))
                                        return launch_tuple(a->ctx,
                                                            k_step_sell2<T, P, VI, Wc, WN, decltype(fo)::value, decltype(bec)::value,
                                                                         kStepSellBlock, decltype(pgc)::value,
                                                                         WithBasis<A, basis_f16>>,
                                                            dim3(grid), dim3(kStepSellBlock), args(SellDots{}));
                                }
                                return launch_tuple(a->ctx,
                                                    k_step_sell2<T, P, VI, Wc, WN, decltype(fo)::value, decltype(bec)::value,
                                                                 kStepSellBlock, decltype(pgc)::value, A>,
                                                    dim3(grid), dim3(kStepSellBlock), args(SellDots{}));
                            });
                        };
                        const char* pge = std::getenv("MPG_SELL_PREGATHER");
                        const bool pg = !(!WN && pge && *pge == '0');
                        if constexpr (Wc == 2) if (pg && be == 10) return pair(std::integral_constant<int, 10>(), std::true_type());
                        if (pg && be != 8 && be != 12) return (int)MPG_ERR_UNSUPPORTED;
                        return with_flag(pg, [&](auto pgc) {
                            return be == 8 ? pair(std::integral_constant<int, 8>(), pgc) : pair(std::integral_constant<int, 12>(), pgc);
                        });
                    }
                    auto step = [&](auto pipe) {
                        return with_flag(fold, [&](auto fo) {
                            return with_flag(sell_uniform(S), [&](auto uni) {
                                if constexpr (kBasisBuilt<T, VI>) {
                                    if (half_basis(a))
                                        return launch(k_step_sell<T, P, VI, CI, Wc, WN, decltype(fo)::value, 0, kStepSellBlock,
                                                                  decltype(uni)::value, decltype(pipe)::value,
                                                                  WithBasis<A, basis_f16>>,
                                                      SellDots{}, BSC());
                                }
                                return launch(k_step_sell<T, P, VI, CI, Wc, WN, decltype(fo)::value, 0, kStepSellBlock,
                                                          decltype(uni)::value, decltype(pipe)::value, A>,
                                              SellDots{}, BSC());
                            });
                        });
                    };
                    if constexpr (!WN && !std::is_same_v<CI, int16_t>) if (sell_pipe(S)) return step(std::true_type());
                    return step(std::false_type());
                });
            });
        }
        if (a->node.nblk > 0) {
            const NodeCopy& S = a->node;
            const int tpw = node_tpw(S);
            auto go = [&](auto kern, const P* dg) {
                launch_timed(a->ctx, kern, dim3((S.ntiles + tpw - 1) / tpw), dim3(kBlock),
                             static_cast<const int32_t*>(S.tiles), static_cast<const int32_t*>(S.bptr),
                             static_cast<const char*>(S.recs), static_cast<const T*>(a->w[k & 1]),
                             static_cast<const T*>(a->inv()), static_cast<T*>(a->V), a->ld, k, dg,
                             static_cast<T*>(a->w[(k + 1) & 1]), gf, a->d.inner_row_exp, S.ntiles, S.nblk, tpw,
                             node_xcd(S));
                return (int)MPG_OK;
            };
            return with_flag(fold, [&](auto fo) {
                constexpr bool FOLD = decltype(fo)::value;
                if (bj_fused(a))  // block Jacobi inside the launch (k_step_node_bj takes the inverses as `diag`)
                    return go(k_step_node_bj<T, P, VI, FOLD, A>, static_cast<const P*>(a->d.block_dinv));
                return with_flag(tpw > 1, [&](auto walk) {
                    return go(k_step_node<T, P, VI, FOLD, decltype(walk)::value, A>, diag);
                });
            });
        }
        if constexpr (kBasisBuilt<T, VI>) {
            if (!plain_basis(a))
                return with_flag(fold, [&](auto fo) {
                    return with_flag(half_basis(a), [&](auto hb) {
                        using BT = std::conditional_t<decltype(hb)::value, basis_f16, basis_f16emu>;
                        launch_timed(a->ctx, k_step_spmv<T, P, VI, decltype(fo)::value, 0, WithBasis<A, BT>>, dim3(rb_grid(a)),
                            dim3(kBlock), Acsr->blocks, Acsr->nblocks, Acsr->rowptr, Acsr->col,
                            static_cast<const VI*>(a->d.val_inner), Acsr->nnz, static_cast<const T*>(a->w[k & 1]),
                            static_cast<const T*>(a->inv()), static_cast<T*>(a->V), a->ld, k,
                            diag, static_cast<T*>(a->w[(k + 1) & 1]), gf, a->d.inner_row_exp);
                        return (int)MPG_OK;
                    });
                });
        }
        return with_int<4>(csr_mode(), [&](auto mode) {
            return with_flag(fold, [&](auto fo) {
                launch_timed(a->ctx, k_step_spmv<T, P, VI, decltype(fo)::value, decltype(mode)::value, A>, dim3(rb_grid(a)),
                    dim3(kBlock), Acsr->blocks, Acsr->nblocks, Acsr->rowptr, Acsr->col,
                    static_cast<const VI*>(a->d.val_inner), Acsr->nnz, static_cast<const T*>(a->w[k & 1]),
                    static_cast<const T*>(a->inv()), static_cast<T*>(a->V), a->ld, k, diag,
                    static_cast<T*>(a->w[(k + 1) & 1]), gf, a->d.inner_row_exp);
                return (int)MPG_OK;
            });
        });
    });
    if (st) return st;
    if (dots) {
        a->last_G = a->fd_ng;
        a->last_part = a->dpart;
        a->last_prologue = false;
    }
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

// The SpMV of step k inside the panel dots' launch (k_step_dots): MPG_OK when
// this workspace, accumulation class and step can run it, MPG_ERR_UNSUPPORTED
// otherwise (the caller then launches the SpMV and the dots apart). Built for
// the fp32 accumulation class on BAND's storage: uniform int16 slices of at
// most 10 entries per row in 2-wide steps, the v_k window, fp32 basis and values.
// (The fp64 class is not built: the held batch beside four slices' first
// batches and 32 fp64 accumulators does not fit 128 VGPRs.)
template <class A>
int step_dots_check(const mpg_arnoldi* a, int k) {
    if (!a || k < 0 || k >= a->d.m) return MPG_ERR_ARG;
    const SellCopy& S = a->sell;
    const bool ok = std::is_same_v<A, float> && (a->combo == 2 || a->combo == 3) && plain_basis(a) &&  // fp32 basis, fp32 values
                    a->d.orth != kOrthMGS && a->d.orth != kOrthCGSR && k + 1 <= kNC &&
                    a->d.n > 0 && a->d.n % 4 == 0 &&  // (dots_panel's tail rows belong to workgroup 0's sums)
                    (int64_t)a->Gd * kStepDotsRows >= a->d.n &&  // one pass
                    a->front == 0 && a->d.n_ext == a->d.n &&     // one GPU: no halo rows
                    // (k_step_sell2's storage; a copy of one slice, which the pair kernel leaves
                    // to k_step_sell, runs here too: the row sums are the same in every form)
                    S.nslices > 0 && S.c16 && S.win && !S.rows && sell_uniform(S) && S.W == 2 &&
                    S.ustride / kWave <= 10;
    return ok ? MPG_OK : MPG_ERR_UNSUPPORTED;
}

template <class A>
int step_dots_run(mpg_arnoldi_t a, int k, int fold) {
    if (!a || k < 0 || k >= a->d.m || fold < 0 || fold > 2) return MPG_ERR_ARG;
    if (int st = step_dots_check<A>(a, k)) return st;
    if (fold && (k < 1 || a->d.m > kFoldMaxM)) return MPG_ERR_ARG;
    if constexpr (std::is_same_v<A, float>) {
        using T = float;
        using P = float;
        // a repeat of step k's launch right behind it folds what the first folded
        const bool again = fold == 2 && a->sd_k == k && a->last_part == a->dpart;
        if (fold == 2 && !again) {
            a->sd_k = k;
            a->sd_part = a->last_part;
            a->sd_G = a->last_G;
        }
        if (fold == 2 && (a->sd_G > kBlock || a->sd_part == a->dpart)) return MPG_ERR_ARG;  // <= kBlock partials, not its own output
        GivensFold<T> gf{nullptr, 0, {}};
        if (fold) gf = GivensFold<T>{fold == 2 ? a->sd_part : a->sums, fold == 2 ? a->sd_G : 0, givens_args<T>(a, k - 1)};
        const SellCopy& S = a->sell;
        const P* diag = a->d.jacobi ? static_cast<const P*>(a->d.diag) : nullptr;
        int st = with_nc<kNC>(k + 1, [&](auto nc) {
            constexpr int NC = decltype(nc)::value;
            // (PF, the held first batch of basis columns: 27.54k against 27.05k it/s
            // without it on BAND-10M, 3 interleaved runs each; only that form is built)
            return with_flag(fold, [&](auto fo) {
                // (with the fold one workgroup more, last in the grid: the rider that runs the Givens step)
                launch_timed(a->ctx, k_step_dots<T, P, 2, decltype(fo)::value, 10, NC, true, A>,
                             dim3(a->Gd + (fold ? 1 : 0)), dim3(kCombineBlock), a->d.n, S.nslices,
                             static_cast<const int16_t*>(S.col), static_cast<const T*>(S.val),
                             static_cast<const T*>(a->w[k & 1]), static_cast<const T*>(a->inv()),
                             static_cast<T*>(a->V), a->ld, k, diag, static_cast<T*>(a->w[(k + 1) & 1]), gf, S.spat,
                             S.coff, static_cast<const int16_t*>(S.pat), S.ustride, a->dpart);
                return (int)MPG_OK;
            });
        });
        if (st) return st;
        a->last_G = a->Gd;
        a->last_part = a->dpart;
        a->last_prologue = false;
        MPG_LAUNCH_CHECK(a->ctx);
        return MPG_OK;
    } else {
        return MPG_ERR_UNSUPPORTED;
    }
}

// row groups per panel of k_dots_panels: about one workgroup per CU in all
// (the same on every rank: uniform groups set Gd = kCombineGroups), so each
// column has <= kCombineGroups / 2 partials for k_cgs_update_wide
inline int wide_groups(const mpg_arnoldi* a, int ncols) {
    const int np = (ncols + kNC - 1) / kNC;
    return std::max(1, std::min(a->Gd, kCombineGroups / np));
}

// measurement: the armed stamp slots (mpg_arnoldi_stamp_next) for this launch when they hold all of its waves;
// disarmed either way
inline unsigned long long* take_stamp(mpg_arnoldi* a, int64_t waves) {
    unsigned long long* p = a->ctx->stamp_next;
    a->ctx->stamp_next = nullptr;
    return p && waves <= a->ctx->stamp_cap ? p : nullptr;
}

template <class A>
int dots_run(mpg_arnoldi_t a, int k, bool combine) {
    if (!a || k < 0 || k >= a->d.m) return MPG_ERR_ARG;
    const int ndots_all = a->d.orth == kOrthMGS ? 1 : k + 1;
    if (combine && ndots_all > kNC) return MPG_ERR_ARG;
    // a compressed or emulated basis: the one-panel CGS / CGSR dots only
    if (!plain_basis(a) && (combine || ndots_all > kNC || a->d.orth == kOrthMGS)) return MPG_ERR_UNSUPPORTED;
    // an armed stamp belongs to this launch whatever its form (disarmed
    // here); only the one-panel k_dots_nc stores stamps
    unsigned long long* sp = take_stamp(a, (int64_t)a->Gd * (kCombineBlock / kWave));
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto, auto, auto vi) {
        using T = decltype(t);
        if constexpr (kBasisBuilt<T, decltype(vi)>) {
            if (half_basis(a))
                return with_nc<kNC>(ndots_all, [&](auto nc) {
                    return with_flag(sp != nullptr, [&](auto stamped) {
                        k_dots_nc<T, kCombineBlock, decltype(nc)::value, decltype(stamped)::value, WithBasis<A, basis_f16>>
                            <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, static_cast<const T*>(a->V),
                                                                           a->ld, static_cast<const T*>(a->w[(k + 1) & 1]),
                                                                           a->dpart, sp);
                        return (int)MPG_OK;
                    });
                });
        }
        if (combine) {
            k_panel_dots<T, kCombineBlock, true, A><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, 0, ndots_all, static_cast<const T*>(a->w[(k + 1) & 1]),
                a->partial, a->counters, a->sums);
            return (int)MPG_OK;
        }
        if (ndots_all <= kNC) {  // one panel: 1024-thread workgroups, one per CU -> Gd partials per column
            return with_nc<kNC>(ndots_all, [&](auto nc) {
                return with_flag(sp != nullptr, [&](auto stamped) {
                    k_dots_nc<T, kCombineBlock, decltype(nc)::value, decltype(stamped)::value, A>
                        <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, static_cast<const T*>(a->V), a->ld,
                                                                       static_cast<const T*>(a->w[(k + 1) & 1]), a->dpart, sp);
                    return (int)MPG_OK;
                });
            });
        }
        if (ndots_all <= kWideMax) {  // every panel in one launch -> wide_groups(a, k) partials per column
            const int np = (ndots_all + kNC - 1) / kNC;
            return with_nc<kNC>(ndots_all - (np - 1) * kNC, [&](auto ncl) {
                k_dots_panels<T, kCombineBlock, decltype(ncl)::value, A>
                    <<<dim3(wide_groups(a, ndots_all), np), kCombineBlock, 0, a->ctx->stream>>>(
                        a->d.n, static_cast<const T*>(a->V), a->ld, static_cast<const T*>(a->w[(k + 1) & 1]),
                        a->dpart);
                return (int)MPG_OK;
            });
        }
        for (int c0 = 0; c0 < ndots_all; c0 += kNC) {
            const int nc = ndots_all - c0 < kNC ? ndots_all - c0 : kNC;
            k_panel_dots<T, kBlock, false, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, c0, nc, static_cast<const T*>(a->w[(k + 1) & 1]),
                a->partial, nullptr, nullptr);
        }
        return (int)MPG_OK;
    });
    const bool wide = !combine && ndots_all > kNC && ndots_all <= kWideMax;
    a->last_G = combine || ndots_all <= kNC ? a->Gd : wide ? wide_groups(a, ndots_all) : row_grid(a);
    a->last_part = !combine && ndots_all <= kWideMax ? a->dpart : a->partial;
    a->last_prologue = false;
    if (st) return st;
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

// The in-launch-sum CGS update issuing its first row group under the
// coefficient sums (k_cgs_update_nc<..., PF>, steps with k + 1 <= one batch
// of columns): on by default in the fp32 accumulation class, where the held
// batch fits its registers (BAND-10M, 8 interleaved bench runs each:
// 26.92k against 26.75k it/s, the update 11.98 against 12.27 us;
// profiles/r06_pf/), off in the fp64 class (round 4: no gain).
// MPG_CGS_PREFETCH=0 / 1 forces it.
// (read when the workspace is created: mpg_arnoldi::cgs_pref)
template <class A>
inline bool cgs_prefetch(const mpg_arnoldi* a) {
    if (a->cgs_pref >= 0) return a->cgs_pref == 1;
    return std::is_same_v<A, float>;
}

// The form of the in-launch-sum CGS update at nc columns: kCgsPlain (the
// product form: the bit tests' reference, and the one the wave stamps time),
// kCgsPrefetch (PF, nc <= one batch) or kCgsStream (k_cgs_update_nc<...,
// STREAM>: the columns through a ring of LDS slots, requested under the
// coefficient sums and refilled as they are consumed; built for an fp32 basis
// in the fp32 accumulation class, every nc <= kNC). MPG_CGS_PREFETCH=0: plain
// everywhere; =1: the streaming form wherever it is built, else PF where that
// is; unset: kCgsStreamFrom and above stream, PF below it (fp32 class), and
// the fp64 class runs what it ran before the streaming form existed (plain).
// The multi-rank engine takes the same form: its partials are all-reduced in
// place ahead of this launch, which then sums them itself exactly as on one
// GPU (FROM_PARTS), so the same requests hide under the same sums
// (tests/test_cgs_stream_gpu.py::test_two_ranks_same_bits).
// A launch with an armed wave stamp (a timer's, never the solve's) runs the
// stamped plain form whatever this says.
enum { kCgsPlain = 0, kCgsPrefetch = 1, kCgsStream = 2 };
constexpr int kCgsStreamFrom = 9;  // (NC <= 8: PF measured 0 - 0.4 us per launch below the ring; profiles/r11_cgs_stream/)
template <class T, class A>
inline int cgs_update_form(const mpg_arnoldi* a, int nc) {
    if (!cgs_prefetch<A>(a)) return kCgsPlain;
    constexpr bool built = std::is_same_v<T, float> && std::is_same_v<A, float>;
    const bool forced = a->cgs_pref == 1;
    if (built && nc <= kNC && (forced || nc >= kCgsStreamFrom)) return kCgsStream;
    return nc <= kColBatch<T> ? kCgsPrefetch : kCgsPlain;
}

// The streaming form's launch (fp32 basis, fp32 class): the one place that
// names the instance, whatever type combination's dispatch reaches it.
template <int NC>
void cgs_stream_launch(mpg_arnoldi_t a, const float* V, const double* src, int part_G, float* coef_out, float* w) {
    k_cgs_update_nc<float, kCombineBlock, NC, true, false, false, false, float, true>
        <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, V, a->ld, src, part_G, coef_out, w, a->partial, nullptr);
}

// 1 when mpg_arnoldi_cgs_partials(a, k) takes the streaming form, else 0
// (asked without launching: mpg_arnoldi_cgs_stream_at)
template <class A>
int cgs_stream_check(const mpg_arnoldi* a, int k) {
    if (!a || k < 0 || k >= a->d.m) return MPG_ERR_ARG;
    if (!plain_basis(a)) return MPG_ERR_UNSUPPORTED;  // (the ring streams an fp32 basis)
    if (k + 1 > kNC || a->d.orth == kOrthCGSR) return 0;
    int form = kCgsPlain;
    dispatch_acc<A>(a->combo, [&](auto t, auto, auto, auto) {
        form = cgs_update_form<decltype(t), A>(a, k + 1);
        return (int)MPG_OK;
    });
    return form == kCgsStream;
}

// no_next (CGSR at 32 < k + 1 <= kWideMax, one GPU): a pass that takes its
// coefficients from the preceding one-launch panel dots and emits no next
// dots (the caller launches k_dots_panels on the updated w instead)
template <class A>
int cgs_run(mpg_arnoldi_t a, int k, int pass, bool givens, bool from_partials, bool no_next) {
    if (!a || k < 0 || k >= a->d.m || pass < 0 || pass > 1 || k + 1 > 256) return MPG_ERR_ARG;
    const bool cgsr = a->d.orth == kOrthCGSR;
    const bool next_dots = cgsr && pass == 0 && !no_next;
    // a compressed or emulated basis: the one-panel plain forms only (CGSR's
    // first pass from the sums, the last pass from the sums or the partials)
    if (!plain_basis(a) && (givens || no_next || k + 1 > kNC || (next_dots && from_partials) || a->d.orth == kOrthMGS))
        return MPG_ERR_UNSUPPORTED;
    if (givens && (next_dots || a->d.m > kFoldMaxM || from_partials)) return MPG_ERR_ARG;
    if (no_next && (!cgsr || !from_partials || k + 1 <= kNC)) return MPG_ERR_ARG;
    // from_partials: the coefficients are summed from the preceding one-panel
    // dots' partials inside this launch (no reduce launch)
    if (from_partials && ((pass != 0 && !no_next) || k + 1 > kWideMax || a->last_part != a->dpart)) return MPG_ERR_ARG;
    if (from_partials && k + 1 > kNC && (next_dots || a->last_G > kWideMax)) return MPG_ERR_ARG;
    const double* src = from_partials ? a->dpart : a->sums;
    const int part_G = from_partials ? a->last_G : 0;  // Gd (k_dots_nc) or fd_ng (k_step_sell's dots)
    if (part_G > kCombineGroups) return MPG_ERR_ARG;
    // an armed stamp belongs to this launch whatever its form (disarmed here);
    // only the one-panel product form below stores stamps
    unsigned long long* sp = take_stamp(a, (int64_t)a->Gd * (kCombineBlock / kWave));
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto, auto, auto vi) {
        using T = decltype(t);
        T* coef_out = pass == 0 ? static_cast<T*>(a->H) + (int64_t)k * (a->d.m + 1) : static_cast<T*>(a->corr());
        T* w = static_cast<T*>(a->w[(k + 1) & 1]);
        const GivensArgs<T> g = givens_args<T>(a, k);
        if constexpr (kBasisBuilt<T, decltype(vi)>) {
            if (half_basis(a)) {
                using AB = WithBasis<A, basis_f16>;
                const T* Vh = static_cast<const T*>(a->V);  // (viewed as fp16 through basis_ptr)
                if (!from_partials) sp = nullptr;
                return with_nc<kNC>(k + 1, [&](auto nc) {
                    constexpr int NC = decltype(nc)::value;
                    if (next_dots)  // (256-thread workgroups, as the fp32 basis' form)
                        k_cgs_update_nc<T, kBlock, NC, false, true, false, false, AB>
                            <<<row_grid(a), kBlock, 0, a->ctx->stream>>>(a->d.n, Vh, a->ld, src, 0, coef_out, w, a->partial,
                                                                          nullptr);
                    else if (from_partials)
                        return with_flag(sp != nullptr, [&](auto stamped) {
                            k_cgs_update_nc<T, kCombineBlock, NC, true, false, false, decltype(stamped)::value, AB>
                                <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, Vh, a->ld, src, part_G, coef_out, w,
                                                                               a->partial, sp);
                            return (int)MPG_OK;
                        });
                    else
                        k_cgs_update_nc<T, kCombineBlock, NC, false, false, false, false, AB>
                            <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, Vh, a->ld, src, 0, coef_out, w, a->partial,
                                                                           nullptr);
                    return (int)MPG_OK;
                });
            }
        }
        if (next_dots && k + 1 <= kNC && !from_partials) {
            // 256-thread workgroups (the NC fp64 dot accumulators need more
            // than the 128 VGPRs of a 1024-thread one) -> row_grid partials
            return with_nc<kNC>(k + 1, [&](auto nc) {
                k_cgs_update_nc<T, kBlock, decltype(nc)::value, false, true, false, false, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                    a->d.n, static_cast<const T*>(a->V), a->ld, src, 0, coef_out, w, a->partial, nullptr);
                return (int)MPG_OK;
            });
        } else if (next_dots) {
            with_flag(from_partials, [&](auto fp) {  // (part_G: 0 unless from_partials)
                k_cgs_update<T, true, false, kBlock, decltype(fp)::value, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                    a->d.n, static_cast<const T*>(a->V), a->ld, k, src, coef_out, w, a->partial, nullptr, g, part_G);
                return (int)MPG_OK;
            });
            for (int c0 = kNC; c0 < k + 1; c0 += kNC) {
                const int nc = k + 1 - c0 < kNC ? k + 1 - c0 : kNC;
                k_panel_dots<T, kBlock, false, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                    a->d.n, static_cast<const T*>(a->V), a->ld, c0, nc, w, a->partial, nullptr, nullptr);
            }
        } else if (givens) {
            k_cgs_update<T, false, true, kBlock, false, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, k, src, coef_out, w, a->partial, a->counters + 32, g, 0);
        } else if (from_partials && k + 1 > kNC) {  // GMRES(100): sums from k_dots_panels' partials
            k_cgs_update_wide<T, kCombineBlock, A><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, k + 1, src, part_G, coef_out, w, a->partial);
        } else if (k + 1 <= kNC) {  // last pass: 1024-thread workgroups, one per CU -> Gd ||w||^2 partials
            // the wave stamps of the product form only (in-launch sums, no
            // prefetch): the one bench.py's phases time
            // (an armed stamp times the stamped product form, so a measured
            // launch never takes the prefetch variant)
            if (!from_partials) sp = nullptr;
            const int form = from_partials && !sp ? cgs_update_form<T, A>(a, k + 1) : (int)kCgsPlain;
            const bool pf = form == kCgsPrefetch;
            return with_nc<kNC>(k + 1, [&](auto nc) {
                constexpr int NC = decltype(nc)::value;
                const T* Vp = static_cast<const T*>(a->V);
                // (NC in the condition: it must depend on this lambda's parameter
                // for the branch to be discarded where the form is not built)
                if constexpr (NC >= 1 && std::is_same_v<T, float> && std::is_same_v<A, float>) {
                    if (form == kCgsStream) {
                        cgs_stream_launch<NC>(a, Vp, src, part_G, coef_out, w);
                        return (int)MPG_OK;
                    }
                }
                // (the prefetch variant for one batch of columns only: wider
                // panels spilled with the prefetched batch held across the sums
                // in the fp64 class, and in the fp32 class the wider forms
                // (NC 9..28, no spills) aborted the process on the box
                // (round 6, profiles/r06_pf/); they are not built)
                if constexpr (NC <= kColBatch<T>) {
                    if (pf) {
                        k_cgs_update_nc<T, kCombineBlock, NC, true, false, true, false, A>
                            <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, Vp, a->ld, src, part_G, coef_out,
                                                                           w, a->partial, nullptr);
                        return (int)MPG_OK;
                    }
                }
                if (from_partials)  // (sp: only with from_partials, above)
                    return with_flag(sp != nullptr, [&](auto stamped) {
                        k_cgs_update_nc<T, kCombineBlock, NC, true, false, false, decltype(stamped)::value, A>
                            <<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(a->d.n, Vp, a->ld, src, part_G, coef_out, w,
                                                                           a->partial, sp);
                        return (int)MPG_OK;
                    });
                k_cgs_update_nc<T, kCombineBlock, NC, false, false, false, false, A><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                    a->d.n, Vp, a->ld, src, 0, coef_out, w, a->partial, nullptr);
                return (int)MPG_OK;
            });
        } else {
            k_cgs_update<T, false, false, kCombineBlock, false, A><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, k, src, coef_out, w, a->partial, nullptr, g, 0);
        }
        return (int)MPG_OK;
    });
    a->last_G = next_dots || givens ? row_grid(a) : a->Gd;
    a->last_part = a->partial;
    a->last_prologue = false;
    if (st) return st;
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

template <class A>
int mgs_run(mpg_arnoldi_t a, int k, int j, bool from_partials) {
    if (!a || k < 0 || k >= a->d.m || j < 0 || j > k) return MPG_ERR_ARG;
    if (!plain_basis(a)) return MPG_ERR_UNSUPPORTED;
    // from_partials: h_jk from the previous launch's partials; the update
    // writes into the other partial buffer (the previous one is still read)
    const double* src = from_partials ? a->last_part : a->sums;
    const int src_G = from_partials ? a->last_G : 0;
    double* dst = from_partials && a->last_part == a->partial ? a->dpart : a->partial;
    if (from_partials && src_G > kCombineGroups * 4) return MPG_ERR_ARG;
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto, auto, auto) {
        using T = decltype(t);
        T* hjk = static_cast<T*>(a->H) + (int64_t)k * (a->d.m + 1) + j;
        k_mgs_update<T, kCombineBlock, A><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
            a->d.n, static_cast<const T*>(a->V), a->ld, j, k, src, src_G, hjk, static_cast<T*>(a->w[(k + 1) & 1]),
            dst);
        return (int)MPG_OK;
    });
    a->last_G = a->Gd;
    a->last_part = dst;
    a->last_prologue = false;
    if (st) return st;
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

template <class A>
int givens_run(mpg_arnoldi_t a, int k, bool from_partials) {
    if (!a || k < 0 || k >= a->d.m) return MPG_ERR_ARG;
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto, auto, auto) {
        using T = decltype(t);
        k_givens<T, A><<<1, kBlock, 0, a->ctx->stream>>>(givens_args<T>(a, k), from_partials ? a->last_part : a->sums,
                                                      from_partials ? a->last_G : 0);
        return MPG_OK;
    });
    if (st) return st;
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

template <class A>
int update_run(mpg_arnoldi_t a, int k) {
    if (!a || k < 0 || k > a->d.m || k > 1024) return MPG_ERR_ARG;
    if (k == 0) return MPG_OK;
    if (!plain_basis(a) && k > kNC) return MPG_ERR_UNSUPPORTED;  // one panel
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto x, auto, auto vi) {
        using T = decltype(t);
        using X = decltype(x);
        if constexpr (kBasisBuilt<T, decltype(vi)> && std::is_same_v<X, double>) {
            if (half_basis(a))
                return with_nc<kNC>(k, [&](auto nc) {
                    k_update_x_nc<T, X, decltype(nc)::value, WithBasis<A, basis_f16>><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                        a->d.n, static_cast<const T*>(a->V), a->ld, static_cast<const T*>(a->s()),
                        static_cast<const T*>(a->H), a->d.m + 1, static_cast<X*>(a->d.x));
                    return (int)MPG_OK;
                });
        }
        if (k <= kNC) {  // x is an aligned allocation: row groups of 4 are 16/32-B aligned
            return with_nc<kNC>(k, [&](auto nc) {
                k_update_x_nc<T, X, decltype(nc)::value, A><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                    a->d.n, static_cast<const T*>(a->V), a->ld, static_cast<const T*>(a->s()),
                    static_cast<const T*>(a->H), a->d.m + 1, static_cast<X*>(a->d.x));
                return (int)MPG_OK;
            });
        } else if (k <= kWave) {
            k_update_x<T, X, true, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, k, static_cast<const T*>(a->s()),
                static_cast<const T*>(a->H), a->d.m + 1, static_cast<X*>(a->d.x));
        } else {
            const size_t packed = (size_t)k * (k + 1) / 2 * sizeof(T);
            if (k <= 2 * kWave && packed <= 65536)
                k_trsv_upper_lds<T, 2><<<1, kBlock, packed, a->ctx->stream>>>(
                    k, a->d.m + 1, static_cast<const T*>(a->H), static_cast<T*>(a->s()));
            else
                k_trsv_upper<T><<<1, kBlock, 0, a->ctx->stream>>>(k, a->d.m + 1, static_cast<const T*>(a->H),
                                                                  static_cast<T*>(a->s()));
            k_update_x<T, X, false, A><<<row_grid(a), kBlock, 0, a->ctx->stream>>>(
                a->d.n, static_cast<const T*>(a->V), a->ld, k, static_cast<const T*>(a->s()), nullptr, 0,
                static_cast<X*>(a->d.x));
        }
        return (int)MPG_OK;
    });
    if (st) return st;
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

// givens_partials(m - 1) + update(m) (+ the x snapshot, flags bit 0) in one
// launch (k_update_tail_nc): the whole restart length in one panel, and the
// ||w||^2 partials of a 1024-thread producer (at most kBlock of them, which
// fold_parts_sum adds in k_givens' order). Asked without launching:
// update_tail_ok.
inline bool update_tail_ok(const mpg_arnoldi* a) {
    return a && a->d.m >= 1 && a->d.m <= kNC && a->Gd <= kBlock && plain_basis(a);
}

template <class A>
int update_tail_run(mpg_arnoldi_t a, int m, int flags) {
    if (!update_tail_ok(a)) return a ? MPG_ERR_UNSUPPORTED : MPG_ERR_ARG;
    if (m != a->d.m || (flags & ~1) || a->last_G < 1 || a->last_G > kBlock) return MPG_ERR_ARG;
    if ((flags & 1) && !a->x_snap) return MPG_ERR_ARG;
    int st = dispatch_acc<A>(a->combo, [&](auto t, auto x, auto, auto) {
        using T = decltype(t);
        using X = decltype(x);
        const UpdateTail<T> tl{GivensFold<T>{a->last_part, a->last_G, givens_args<T>(a, m - 1)},
                               static_cast<T*>(a->tail_stage())};
        return with_nc<kNC>(m, [&](auto nc) {
            return with_flag(flags & 1, [&](auto snap) {
                constexpr bool stream = std::is_same_v<T, float> && std::is_same_v<A, float>;
                constexpr bool SNAP = decltype(snap)::value;
                k_update_tail_nc<T, X, decltype(nc)::value, A, stream, SNAP><<<a->Gd, kCombineBlock, 0, a->ctx->stream>>>(
                    a->d.n, static_cast<const T*>(a->V), a->ld, static_cast<X*>(a->d.x),
                    SNAP ? static_cast<X*>(a->x_snap) : nullptr, tl);
                return (int)MPG_OK;
            });
        });
    });
    if (st) return st;
    a->tail_staged = true;  // the next finish launch copies the staged column into H
    MPG_LAUNCH_CHECK(a->ctx);
    return MPG_OK;
}

}  // namespace

// The phase launches and queries of one accumulation class. arnoldi.hip
// holds the A = double table, arnoldi_acc32.hip the A = float one (fp32
// Arnoldi only: an fp64 combination returns MPG_ERR_UNSUPPORTED there).
struct mpg_arnoldi_phases {
    int (*reduce)(mpg_arnoldi* a, int ncols);
    int (*spmv)(mpg_arnoldi* a, int k, int fold, bool dots);
    int (*step_dots)(mpg_arnoldi* a, int k, int fold);
    int (*step_dots_ok)(const mpg_arnoldi* a, int k);
    int (*spmv_dots_ok)(const mpg_arnoldi* a, int k);
    int (*cgs_stream_at)(const mpg_arnoldi* a, int k);
    int (*dots)(mpg_arnoldi* a, int k, bool combine);
    int (*cgs)(mpg_arnoldi* a, int k, int pass, bool givens, bool from_partials, bool no_next);
    int (*mgs)(mpg_arnoldi* a, int k, int j, bool from_partials);
    int (*givens)(mpg_arnoldi* a, int k, bool from_partials);
    int (*update)(mpg_arnoldi* a, int k);
    int (*update_tail)(mpg_arnoldi* a, int m, int flags);
};
// (a function, not an object: host code only, so the device compilation never sees the table)
__attribute__((visibility("hidden"))) const mpg_arnoldi_phases& mpg_arnoldi_phases_acc32();

namespace {
template <class A>
mpg_arnoldi_phases phases_of() {
    return {reduce_run<A>, spmv_run<A>,     step_dots_run<A>, step_dots_check<A>, spmv_dots_check<A>, cgs_stream_check<A>,
            dots_run<A>,   cgs_run<A>,      mgs_run<A>,       givens_run<A>,      update_run<A>,      update_tail_run<A>};
}
}  // namespace
