// The fused engine's phase timers (mpg_engine_time_*): each walks the op list
// of a restart cycle (cycle_plan.hpp) and does its work around the ops tagged
// with the phase it times. Measurement only: the replayed and duplicated
// launches and the cycles run without the host's restart checks change V, H,
// w and x, so every timer sets `measured` and run() refuses afterwards.
#include <algorithm>

#include "fused_gmres.hpp"
#include "types_hip.hpp"

namespace mpg {

CapturedGraph::CapturedGraph(hipStream_t s, const std::function<void()>& build) {
    hipck(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal), "begin capture");
    std::exception_ptr failed;
    try {
        build();
    } catch (...) {
        failed = std::current_exception();
    }
    hipError_t st = hipStreamEndCapture(s, &graph);  // (also after a failed build: nothing is left capturing)
    if (!failed && st == hipSuccess) st = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (!failed && st == hipSuccess) return;
    reset();
    (void)hipGetLastError();
    if (failed) std::rethrow_exception(failed);
    hipck(st, "end capture / instantiate");
}
void CapturedGraph::reset() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
}

namespace {

// events created in order, destroyed on every path
struct Events {
    std::vector<hipEvent_t> v;
    hipEvent_t make() {
        hipEvent_t e;
        hipck(hipEventCreate(&e), "event");
        v.push_back(e);
        return e;
    }
    ~Events() {
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
    }
};

// An event-record node spliced into the capture in progress on `st`: the
// node depends on the capture's current tail and becomes the new tail. Same
// place in the graph as hipEventRecordWithFlags(hipEventRecordExternal),
// which the HIP runtime bundled with PyTorch (ROCm 7.0) rejects inside a
// capture ("invalid argument").
void capture_event_record(hipStream_t st, hipEvent_t ev) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t graph = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t ndeps = 0;
    hipck(hipStreamGetCaptureInfo_v2(st, &status, &id, &graph, &deps, &ndeps), "capture info");
    if (status != hipStreamCaptureStatusActive || !graph) throw StatusError(MPG_ERR_HIP, "timing mark outside a capture");
    hipGraphNode_t node = nullptr;
    hipck(hipGraphAddEventRecordNode(&node, graph, deps, ndeps, ev), "event record node");
    hipck(hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies), "capture tail");
}

}  // namespace

// Device-event time of one phase kernel in its place in the cycle: `reps`
// restart cycles run eagerly in cycle order, and at every op of phase `which`
// a kernel is first replayed kTimedReplays times back to back between one
// event pair (amortising the dispatch latency an event pair around a single
// launch would include), then the cycle's own op follows. The replays are of
// the op itself, except at the SpMV's sites, where they are of the plain SpMV
// whatever form the site runs. In-place mode (SpMV only) instead arms the
// kernel events that the site's own launch records
// (mpg_arnoldi_time_next_spmv). Replays of the non-idempotent CGS update
// leave the engine's state meaningless.
constexpr int kTimedReplays = 10;

double FusedEngine::time_phase(int which, int reps, bool inplace, std::vector<double>* per_launch) {
    measured = true;
    if (inplace && which != 0) throw std::invalid_argument("in-place timing covers the Arnoldi SpMV only");
    Events marks;
    for (int r = 0; r < reps; ++r)
        for (const Op& o : cycle_ops()) {
            if (o.phase == which) {
                const hipEvent_t e0 = marks.make(), e1 = marks.make();
                if (inplace) {
                    check(mpg_arnoldi_time_next_spmv(arnoldi(), e0, e1), "time spmv", ctx());
                } else {
                    const Op replay = which == 0 ? Op{OpKind::Spmv, -1, false, 0, o.a, 0} : o;
                    hipck(hipEventRecord(e0, stream()), "record");
                    for (int q = 0; q < kTimedReplays; ++q) issue(replay);
                    hipck(hipEventRecord(e1, stream()), "record");
                }
            }
            issue(o);
        }
    hipck(hipStreamSynchronize(stream()), "sync");
    float total_ms = 0;
    const size_t pairs = marks.v.size() / 2;
    for (size_t q = 0; q < pairs; ++q) {
        float ms = 0;
        hipck(hipEventElapsedTime(&ms, marks.v[2 * q], marks.v[2 * q + 1]), "elapsed");
        total_ms += ms;
        if (per_launch) per_launch->push_back(inplace ? ms : ms / kTimedReplays);
    }
    return pairs ? total_ms / (pairs * (inplace ? 1 : kTimedReplays)) : 0.0;
}

// the timers inside graph replays: a captured cycle and one of its kernels' phases
void FusedEngine::require_captured_phase(int which) {
    measured = true;
    if (!policy().graph) throw StatusError(MPG_ERR_UNSUPPORTED, "the cycle is not captured (MPG_NO_GRAPH / eager ranks)");
    if (which != 0 && which != 2 && which != 3) throw std::invalid_argument("phase: 0 spmv, 2 cgs update, 3 dots");
}

// A phase kernel timed inside graph replays of the cycle (which: 0 the
// Arnoldi SpMV, 2 the CGS update, 3 the panel dots): the cycle is captured
// once more with an external event node on each side of every op of that
// phase, and that graph is replayed `reps` times (each replay re-records
// the events; they are read after it).
double FusedEngine::time_phase_graph(int which, int reps, std::vector<double>* per_launch) {
    require_captured_phase(which);
    Events marks;
    const CapturedGraph g(stream(), [&] {
        for (const Op& o : cycle_ops()) {
            if (o.phase == which) capture_event_record(stream(), marks.make());
            issue(o);
            if (o.phase == which) capture_event_record(stream(), marks.make());
        }
    });
    double total = 0;
    size_t count = 0;
    for (int r = 0; r < reps; ++r) {
        hipck(hipGraphLaunch(g.exec, stream()), "graph launch");
        hipck(hipStreamSynchronize(stream()), "sync");
        for (size_t q = 0; q + 1 < marks.v.size(); q += 2) {
            float ms = 0;
            hipck(hipEventElapsedTime(&ms, marks.v[q], marks.v[q + 1]), "elapsed");
            total += ms;
            ++count;
            if (per_launch) per_launch->push_back(ms);
        }
    }
    return count ? total / count : 0.0;
}

// A phase kernel's own duration inside graph replays of the cycle (which: 0
// the Arnoldi SpMV, 2 the one-panel CGS update, 3 the one-panel dots): the
// cycle is captured once more (after a memset node clearing the slots) with
// every op of that phase armed to store its waves' wall-clock stamps
// (mpg_arnoldi_stamp_next, disarmed again behind the op, so a site that
// launches another form stores nothing); a launch lasts max(end) -
// min(start) over its waves -- the kernel alone, with no event packet in the
// queue around it. Launches of another form at the phase's site (the panel
// kernels past 32 columns) are skipped.
double FusedEngine::time_phase_stamps(int which, int reps, std::vector<double>* per_launch) {
    require_captured_phase(which);
    const int64_t cap = mpg_arnoldi_stamp_waves(arnoldi());  // waves per launch
    if (cap < 1) throw StatusError(MPG_ERR_HIP, "no SpMV waves");
    const int64_t slots = (int64_t)policy().m + 2;  // launch slots
    const size_t bytes = (size_t)(2 * cap * slots) * sizeof(unsigned long long);
    DevMem buf(ctx(), bytes);
    int dev = 0, khz = 0;
    hipck(hipGetDevice(&dev), "device");
    hipck(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev), "wall clock rate");
    if (khz <= 0) throw StatusError(MPG_ERR_HIP, "no wall clock rate");
    std::vector<unsigned long long> host(bytes / sizeof(unsigned long long));
    int64_t launches = 0;  // launches armed
    const CapturedGraph g(stream(), [&] {
        hipck(hipMemsetAsync(buf.p, 0, bytes, stream()), "clear stamps");
        for (const Op& o : cycle_ops()) {
            if (o.phase == which && launches < slots)
                check(mpg_arnoldi_stamp_next(arnoldi(), buf.as<unsigned long long>() + 2 * cap * launches++, cap), "stamp",
                      ctx());
            issue(o);
            if (o.phase == which) check(mpg_arnoldi_stamp_next(arnoldi(), nullptr, 0), "stamp", ctx());
        }
    });
    double total = 0;
    size_t count = 0;
    for (int r = 0; r < reps; ++r) {
        hipck(hipGraphLaunch(g.exec, stream()), "graph launch");
        hipck(hipStreamSynchronize(stream()), "sync");
        hipck(hipMemcpy(host.data(), buf.p, bytes, hipMemcpyDeviceToHost), "read stamps");
        for (int64_t q = 0; q < launches; ++q) {
            const unsigned long long* st = host.data() + 2 * cap * q;
            unsigned long long t0 = ~0ull, t1 = 0;
            for (int64_t wv = 0; wv < cap; ++wv) {
                if (st[2 * wv] && st[2 * wv] < t0) t0 = st[2 * wv];
                if (st[2 * wv + 1] > t1) t1 = st[2 * wv + 1];
            }
            if (t0 == ~0ull || t1 <= t0) continue;  // another form ran at the site
            const double ms = (double)(t1 - t0) / (double)khz;
            total += ms;
            ++count;
            if (per_launch) per_launch->push_back(ms);
        }
    }
    if (!count) throw StatusError(MPG_ERR_UNSUPPORTED, "no launch of the phase stored stamps");
    return total / count;
}

// A phase kernel's share of the stream inside graph replays of the cycle
// (which: 0 the Arnoldi SpMV in the form each step runs, 2 the CGS update, 3
// the panel dots), from HIP events around whole replays: the cycle is
// captured twice, as the solve runs it and with every op of that phase
// tagged `dup` issued twice in a row, and the graphs are replayed
// alternately; the difference of the replay times over the number of added
// launches is what one launch adds to the cycle -- the kernel plus its
// dispatch and release, with no marker packet near it (what rocprofv3's
// kernel duration measures). The duplicates run on the state the first
// launch left: the SpMV and the dots rewrite the same outputs; a second CGS
// update subtracts V h once more (the basis stays normalised; an update that
// sums the dots' partials itself gets the op `redo` back -- the dots, or the
// SpMV + dots launch -- re-run ahead of it, whose own share is measured and
// taken out). step_dots_only: among the phase's ops, double the SpMV + dots
// launches alone.
double FusedEngine::time_phase_dup(int which, int reps, int64_t* launches, bool step_dots_only) {
    require_captured_phase(which);
    const std::vector<Op>& ops = cycle_ops();
    auto doubled = [&](const Op& o) {
        return o.phase == which && o.dup && (!step_dots_only || o.kind == OpKind::StepDots);
    };
    int64_t added = 0, with_dots = 0, with_step = 0;
    for (size_t i = 0; i < ops.size(); ++i)
        if (doubled(ops[i])) {
            ++added;
            if (ops[i].redo) ++(ops[i - ops[i].redo].kind == OpKind::StepDots ? with_step : with_dots);
        }
    if (added < 1) throw StatusError(MPG_ERR_UNSUPPORTED, "the cycle has no launch of that phase");
    const CapturedGraph plain(stream(), [&] { issue(ops); });
    const CapturedGraph twice(stream(), [&] {
        for (size_t i = 0; i < ops.size(); ++i) {
            issue(ops[i]);
            if (!doubled(ops[i])) continue;
            if (ops[i].redo) issue(ops[i - ops[i].redo]);
            issue(ops[i]);
        }
    });
    const hipGraphExec_t g[2] = {plain.exec, twice.exec};
    Events ev;
    const hipEvent_t e0 = ev.make(), e1 = ev.make();
    for (hipGraphExec_t q : g) hipck(hipGraphLaunch(q, stream()), "graph launch");  // warm
    hipck(hipStreamSynchronize(stream()), "sync");
    std::vector<double> diff;
    for (int r = 0; r < reps; ++r) {
        float ms[2] = {0, 0};
        for (int q = 0; q < 2; ++q) {
            hipck(hipEventRecord(e0, stream()), "record");
            hipck(hipGraphLaunch(g[q], stream()), "graph launch");
            hipck(hipEventRecord(e1, stream()), "record");
            hipck(hipEventSynchronize(e1), "sync");
            hipck(hipEventElapsedTime(&ms[q], e0, e1), "elapsed");
        }
        diff.push_back((double)(ms[1] - ms[0]) / (double)added);
    }
    if (launches) *launches = added;
    std::sort(diff.begin(), diff.end());
    double ms = diff[diff.size() / 2];
    if (with_dots) ms -= time_phase_dup(3, reps) * (double)with_dots / (double)added;
    // updates behind the SpMV + dots launch: that launch's share, measured on those steps alone
    if (with_step) ms -= time_phase_dup(0, reps, nullptr, true) * (double)with_step / (double)added;
    return ms;
}

}  // namespace mpg

// ---------------------------------------------------------------- C-ABI
namespace {

// a timer that also gives per-launch times (t): the mean into *avg_ms, up to
// `cap` of the times out, the launch count returned
template <class F>
int per_launch_call(mpg_engine_t e, int which, int reps, double* avg_ms, double* per_launch_ms, int cap, F&& timer) {
    if (!e || !e->eng || !avg_ms || reps < 1 || cap < 0 || (cap && !per_launch_ms) ||
        (which != 0 && which != 2 && which != 3))
        return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] {
        std::vector<double> t;
        *avg_ms = timer(&t);
        for (size_t i = 0; i < t.size() && (int)i < cap; ++i) per_launch_ms[i] = t[i];
        return (int)t.size();
    });
}

}  // namespace

extern "C" {

int mpg_engine_time_phase(mpg_engine_t e, int which, int reps, double* avg_ms) {
    if (!e || !e->eng || !avg_ms || reps < 1 || which < 0 || which > 3) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] { return *avg_ms = e->eng->time_phase(which, reps), 0; }) ? MPG_ERR_HIP : MPG_OK;
}

int mpg_engine_time_spmv_incycle(mpg_engine_t e, int cycles, double* avg_ms, double* per_launch_ms, int cap) {
    const int st = per_launch_call(e, 0, cycles, avg_ms, per_launch_ms, cap,
                                   [&](auto* t) { return e->eng->time_phase(0, cycles, true, t); });
    return st < 0 && st != MPG_ERR_ARG ? MPG_ERR_HIP : st;
}

int mpg_engine_time_phase_dup(mpg_engine_t e, int which, int reps, double* avg_ms, int64_t* launches) {
    if (!e || !e->eng || !avg_ms || reps < 1 || (which != 0 && which != 2 && which != 3)) return MPG_ERR_ARG;
    return mpg::engine_call(e, [&] { return *avg_ms = e->eng->time_phase_dup(which, reps, launches), 0; });
}

int mpg_engine_time_phase_stamps(mpg_engine_t e, int which, int reps, double* avg_ms, double* per_launch_ms,
                                 int cap) {
    return per_launch_call(e, which, reps, avg_ms, per_launch_ms, cap,
                           [&](auto* t) { return e->eng->time_phase_stamps(which, reps, t); });
}

int mpg_engine_time_phase_graph(mpg_engine_t e, int which, int reps, double* avg_ms, double* per_launch_ms,
                                int cap) {
    return per_launch_call(e, which, reps, avg_ms, per_launch_ms, cap,
                           [&](auto* t) { return e->eng->time_phase_graph(which, reps, t); });
}

}  // extern "C"
