// ttm_optim.cpp - the optimiser loops of optimize() as host C++ behind the C ABI (include/ttm.h "optimisers").
//
// The reference hands every map component to scipy.optimize.minimize (TM:3108-3114 L-BFGS-B for separable maps,
// TM:3252-3257 BFGS for integrated-rectifier maps), one Python call per objective evaluation.  Here the same
// algorithm (csrc/ttm_lbfgsb.h) runs as a host loop that launches the device reduction, waits for the stream and
// reads the 1 + m sums from pinned memory: ~10 us per evaluation instead of ~80 us; csrc/ttm_bfgs.h is the same for
// SciPy's BFGS over the integrated-rectifier objective (ttm_optimize_integrated).  With a communicator the sums of
// all ranks are combined by ONE all-reduce of the fused [objective | gradient] buffer per evaluation (RCCL,
// ttm_allreduce_f64) before they are read - the sample-sharded optimisation of SURVEY.md section 8e.

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifndef TTM_HOST_ONLY          // (tests/hostemu compiles this file for the host: no streams, nothing to wait for)
#include <hip/hip_runtime.h>
#include <immintrin.h>
#endif

#include "../../include/ttm.h"
#include "ttm_bfgs.h"
#include "ttm_lbfgsb.h"

#ifndef TTM_HOST_ONLY  // the layout key of the armed rows of partial sums, 0: none for m, N (csrc/ttm_kernels.hip; not exported)
extern "C" int sentinel_layout(int32_t m, int64_t N);
#else                  // (the host double has no self-validating sums: its loops take the marked call)
static int sentinel_layout(int32_t, int64_t) { return 0; }
#endif

namespace {

#ifndef TTM_HOST_ONLY
// Poll *flag (pinned host memory, written by the device behind the results it announces) until it holds `mark`.
// Every status of the stream other than "not ready" ends the wait: an idle stream without the mark means the launch
// behind it failed, an error status (sticky launch failure, lost or reset device) that it never will arrive - results that
// were not written are never read.  The loads of the results that follow are ordered behind the load that saw the mark.
int poll_mark(const double* flag_, double mark, void* stream) {
    const std::atomic<double>* flag = reinterpret_cast<const std::atomic<double>*>(flag_);
    static_assert(sizeof(std::atomic<double>) == sizeof(double), "lock-free fp64 atomics expected");
    for (long spins = 0; flag->load(std::memory_order_acquire) != mark; ++spins) {
        if ((spins & 0xfffff) != 0xfffff) continue;
        const hipError_t st = hipStreamQuery((hipStream_t)stream);
        if (st == hipErrorNotReady) continue;
        if (st == hipSuccess) (void)hipStreamSynchronize((hipStream_t)stream);   // (idle: anything queued has been executed)
        if (flag->load(std::memory_order_acquire) != mark) return TTM_E_HIP;
        break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return TTM_OK;
}
#endif

// The self-validating results of ttm_objective_sep_cached_sent: the host fills the n slots with a bit pattern no arithmetic
// produces (arm_values), the finishing workgroup overwrites each slot with one 8-byte store, and the slots are polled until
// none holds the pattern - no completion mark, no drain on the device in front of it.  TTM_E_HIP: the stream went idle or
// failed without results, or the device gave up waiting for its own workgroups (the FAIL pattern); *retry (nullable): true for
// the idle stream and the FAIL pattern - nobody is going to answer, but the stream itself has not failed.
const uint64_t kSentBits = 0x7FF4DEADBEEF0001ull, kSentFail = 0x7FF4DEADBEEF0002ull;
void arm_values(double* v_, int n) {
    std::atomic<uint64_t>* v = reinterpret_cast<std::atomic<uint64_t>*>(v_);
    for (int i = 0; i < n; ++i) v[i].store(kSentBits, std::memory_order_relaxed);
    std::atomic_thread_fence(std::memory_order_release);
}
int poll_values(const double* v_, int n, void* stream, bool* retry = nullptr) {
    if (retry) *retry = false;
    const std::atomic<uint64_t>* v = reinterpret_cast<const std::atomic<uint64_t>*>(v_);
    static_assert(sizeof(std::atomic<uint64_t>) == sizeof(double), "lock-free 64-bit atomics expected");
    auto pending = [&]() {
        for (int i = 0; i < n; ++i)
            if (v[i].load(std::memory_order_acquire) == kSentBits) return true;
        return false;
    };
    for (long spins = 0; pending(); ++spins) {
#ifndef TTM_HOST_ONLY
        if ((spins & 0xfffff) != 0xfffff) continue;
        const hipError_t st = hipStreamQuery((hipStream_t)stream);
        if (st == hipErrorNotReady) continue;
        if (st == hipSuccess) (void)hipStreamSynchronize((hipStream_t)stream);
        if (pending()) {
            if (retry) *retry = st == hipSuccess;
            return TTM_E_HIP;
        }
#else
        (void)stream;
        return TTM_E_HIP;
#endif
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < n; ++i)
        if (v[i].load(std::memory_order_relaxed) == kSentFail) {
            if (retry) *retry = true;
            return TTM_E_HIP;
        }
    return TTM_OK;
}

// Completion of the work queued on `stream` so far: a mark written behind it into pinned host memory (*flag), polled
// here - a hipStreamSynchronize per evaluation costs ~12 us of host / driver latency on top of the ~13 us of device work.
int wait_for_mark(double* flag_, long& seq, void* stream) {
#ifndef TTM_HOST_ONLY
    const double mark = (double)(++seq);
    const int rc = ttm_signal(flag_, mark, stream);
    if (rc) return rc;
    return poll_mark(flag_, mark, stream);
#else
    (void)flag_; (void)seq; (void)stream;
    return TTM_OK;
#endif
}

// the stream calls of the separable loops (the host double has no streams: its work is done when a call returns)
#ifndef TTM_HOST_ONLY
void store_fence() { _mm_sfence(); }
int stream_idle(void* stream) { return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? TTM_OK : TTM_E_HIP; }
int copy_to_host(double* dst, const double* src, int n, void* stream) {
    return hipMemcpyAsync(dst, src, (size_t)n * 8, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? TTM_OK : TTM_E_HIP;
}
#else
void store_fence() { std::atomic_thread_fence(std::memory_order_seq_cst); }
int stream_idle(void*) { return TTM_OK; }
int copy_to_host(double* dst, const double* src, int n, void*) { memcpy(dst, src, (size_t)n * 8); return TTM_OK; }
#endif

// Independent component problems side by side (the reference's process pool over components, TM:2789-2845): worker
// threads draw tasks from a shared counter; each worker owns one HIP stream, so the reductions of different components
// overlap on the device and their completion polls overlap on the host.  run(t, stream) -> rc of task t.
template <class Run>
int run_batch(int ntasks, int nthreads, void* stream, Run run) {
    if (nthreads < 1) nthreads = 1;
    if (nthreads > ntasks) nthreads = ntasks;
    if (nthreads > 64) nthreads = 64;
    std::vector<int> rcs(ntasks, TTM_OK);
    // the error text of a failing task lives in the worker thread's own buffer (thread-local): the first failure's text is
    // copied here under a lock and republished on the calling thread before run_batch returns
    std::mutex err_lock;
    std::string err_text;
    auto note_failure = [&](int rc) {
        if (!rc) return;
        std::lock_guard<std::mutex> g(err_lock);
        if (err_text.empty()) err_text = ttm_last_error_string();
    };
    if (nthreads == 1) {
        for (int t = 0; t < ntasks; ++t) rcs[t] = run(t, stream);
    } else {
#ifndef TTM_HOST_ONLY
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return TTM_E_HIP;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return TTM_E_HIP;    // the producers of the inputs are done
        static std::vector<hipStream_t> pool[64];                                         // per device; kept for the process
        static std::atomic_flag pool_lock = ATOMIC_FLAG_INIT;
        while (pool_lock.test_and_set(std::memory_order_acquire)) {}
        std::vector<hipStream_t>& streams = pool[dev & 63];
        bool ok = true;
        while ((int)streams.size() < nthreads && ok) {
            hipStream_t s2;
            ok = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess;
            if (ok) streams.push_back(s2);
        }
        std::vector<hipStream_t> mine(streams.begin(), streams.begin() + (ok ? nthreads : 0));
        pool_lock.clear(std::memory_order_release);
        if (!ok) return TTM_E_HIP;
#endif
        std::atomic<int> next(0);
        auto worker = [&](int w) {
#ifndef TTM_HOST_ONLY
            const bool on_device = hipSetDevice(dev) == hipSuccess;
            void* st = (void*)mine[w];
#else
            const bool on_device = true;
            void* st = stream;
            (void)w;
#endif
            for (int t; (t = next.fetch_add(1)) < ntasks;) {
                rcs[t] = on_device ? run(t, st) : (int)TTM_E_HIP;
                note_failure(rcs[t]);
            }
        };
        std::vector<std::thread> threads;
        for (int w = 1; w < nthreads; ++w) {
            try {
                threads.emplace_back(worker, w);
            } catch (...) {                                              // no more threads to be had: the ones running share the tasks
                break;
            }
        }
        worker(0);
        for (auto& th : threads) th.join();
    }
    for (int t = 0; t < ntasks; ++t)
        if (rcs[t]) {
            if (!err_text.empty()) ttm_set_error_string(err_text.c_str());
            return rcs[t];
        }
    return TTM_OK;
}

// launch(flag, mark) enqueues a reduction that writes *flag = mark behind its results; wait until it has
template <class Launch>
int objective_and_wait(double* flag_, long& seq, void* stream, Launch launch) {
    const double mark = (double)(++seq);
    const int rc = launch(flag_, mark);
    if (rc) return rc;
#ifndef TTM_HOST_ONLY
    return poll_mark(flag_, mark, stream);
#else
    (void)stream;
    return TTM_OK;
#endif
}

}  // namespace

extern "C" {

int ttm_lbfgsb_minimize(int32_t n, double* x, const double* lb, const double* ub, ttm_objective_cb fun, void* user,
                        int32_t maxiter, double* result) {
    if (n < 1 || !x || !fun) return TTM_E_ARG;
    std::vector<double> l(n), u(n);
    std::vector<int> nbd(n);
    for (int i = 0; i < n; ++i) {
        const bool hl = lb && lb[i] > -INFINITY, hu = ub && ub[i] < INFINITY;
        l[i] = hl ? lb[i] : 0.0;
        u[i] = hu ? ub[i] : 0.0;
        nbd[i] = hl ? (hu ? 2 : 1) : (hu ? 3 : 0);
    }
    ttm_opt::LbfgsbOptions opt;
    if (maxiter > 0) opt.maxiter = maxiter;
    const ttm_opt::LbfgsbResult r = ttm_opt::lbfgsb_minimize(
        n, x, l.data(), u.data(), nbd.data(), [&](const double* xx, double* f, double* g) { return fun(n, xx, f, g, user); }, opt);
    if (result) {
        result[0] = r.f; result[1] = r.pgnorm; result[2] = r.nit; result[3] = r.nfev; result[4] = r.status;
    }
    return r.status < 0 ? TTM_E_HIP : TTM_OK;
}

}  // extern "C"

namespace {

// The checks every entry point of the separable loops makes before anything is launched or indexed.  A task evaluates from the
// cached derivative basis (dPsi) or recomputes it from the x_k column (xk, kinds, pars).
int check_task(const ttm_sep_task& q, int64_t N, double Ntotal, const double* sums_dev, const ttm_comm* comm) {
    if ((q.dPsi ? q.ldp < N : (!q.xk || !q.kinds || !q.pars)) || !q.A || !q.b || !q.x || !q.work || !q.counter || !q.sums_host ||
        q.m < 1 || N < 1 || !(Ntotal > 0.0) || (comm && !sums_dev))
        return TTM_E_ARG;
    return q.m > 16 ? TTM_E_LIMIT : TTM_OK;                 // (TTM_SEPC_MAXM of csrc/ttm_kernels.hip: the launches' limit)
}

std::atomic<uint32_t> g_server_gen{0};

// The evaluation of one loop - sums_host[0] = sum_n log dS_n, sums_host[1 + i] = sum_n dPsi_{n,i} / dS_n (TM:2990-3006) at the
// trial point cc, or an error code - in one of four ways, chosen before the loop starts (choose):
//   SERVER  ONE launch answers every evaluation of the loop (k_objective_sep_server, cached basis, m > 1): requests through a
//           mailbox the evaluator holds until it is destroyed;
//   SENT    a launch per evaluation with self-validating partial sums and results (no ticket, no mark);
//   MARKED  a launch per evaluation that writes its results and a completion mark;
//   COMM    a launch into sums_dev, the all-reduce over the ranks, the copy to sums_host and a completion mark behind them.
// A server that leaves unasked (its 0.2 s without a request ran out) or gives up (the FAIL pattern) is replaced - at most three
// servers per loop - and then the loop goes on with SENT: the same bits every way.
struct Evaluator {
    enum Kind { MARKED, SENT, SERVER, COMM };
    const ttm_sep_task& q;
    int64_t N;
    double delta;
    double* sums_dev;
    ttm_comm* comm;
    void* stream;
    Kind kind = MARKED;
    long seq = 0;                                            // MARKED / COMM: the last completion mark
    unsigned char* box = nullptr;                            // SERVER: the mailbox (fine-grained device memory, host-written)
    uint32_t gen = 0, round = 0;                             //   the running server's generation and its last request
    int starts = 0;                                          //   servers started in this loop

    Evaluator(const ttm_sep_task& q_, int64_t N_, double delta_, double* sums_dev_, ttm_comm* comm_, void* stream_)
        : q(q_), N(N_), delta(delta_), sums_dev(sums_dev_), comm(comm_), stream(stream_) {}
    Evaluator(const Evaluator&) = delete;                    // (it owns the mailbox)
    ~Evaluator() { drop_server(); }                          // (the server leaves; it would by itself after 0.2 s)

    // armed_ahead: an evaluation with self-validating sums is in flight already (the rows of `work` are armed).  Returns the layout
    // key of the rows this loop leaves armed (ttm_sep_task.armed), 0 for MARKED / COMM.
    int choose(bool armed_ahead) {
        const int key = comm ? 0 : sentinel_layout(q.m, N);
        if (!key || !(armed_ahead || q.armed == key || ttm_sentinel_fill(q.work, q.m, N, stream) == TTM_OK)) {
            kind = comm ? COMM : MARKED;
            q.sums_host[1 + q.m] = 0.0;                      // the completion mark (sums_host: >= 2 + m doubles)
            return 0;
        }
        kind = SENT;
        if (q.dPsi && q.m > 1 && (box = (unsigned char*)ttm_mailbox_acquire()) != nullptr) {
            if (start_server()) kind = SERVER;
            else drop_server();
        }
        return key;
    }

    int eval(const double* cc) {
        switch (kind) {
        case SERVER: return serve(cc);
        case SENT: {
            arm_values(q.sums_host, 1 + q.m);
            const int rc = q.dPsi ? ttm_objective_sep_cached_sent(q.dPsi, q.ldp, N, q.m, cc, delta, q.work, q.sums_host, stream)
                                  : ttm_objective_sep_direct_sent(q.xk, N, q.m, q.kinds, q.pars, cc, delta, q.work, q.sums_host, stream);
            return rc ? rc : poll_values(q.sums_host, 1 + q.m, stream);
        }
        case MARKED:
            return objective_and_wait(q.sums_host + 1 + q.m, seq, stream,
                                      [&](double* flag, double mark) { return launch_marked(cc, q.sums_host, flag, mark); });
        case COMM: {
            int rc = launch_marked(cc, sums_dev, nullptr, 0.0);
            if (!rc) rc = ttm_allreduce_f64(comm, sums_dev, 1 + q.m, TTM_OP_SUM, stream);
            if (!rc) rc = copy_to_host(q.sums_host, sums_dev, 1 + q.m, stream);
            return rc ? rc : wait_for_mark(q.sums_host + 1 + q.m, seq, stream);
        }
        }
        return TTM_E_ARG;
    }

  private:
    int launch_marked(const double* cc, double* out, double* flag, double mark) {
        return q.dPsi ? ttm_objective_sep_cached_marked(q.dPsi, q.ldp, N, q.m, cc, delta, q.work, q.counter, out, flag, mark, stream)
                      : ttm_objective_sep_direct_marked(q.xk, N, q.m, q.kinds, q.pars, cc, delta, q.work, q.counter, out, flag, mark, stream);
    }

    bool start_server() {
        gen = ++g_server_gen;
        round = 0;
        ++starts;
        return ttm_objective_sep_server_start(q.dPsi, q.ldp, N, q.m, delta, q.work, q.sums_host, box, gen, stream) == TTM_OK;
    }

    void post(uint32_t word) {                               // (the mailbox is a write-combining mapping: fenced stores)
        *(volatile uint64_t*)box = ((uint64_t)gen << 32) | word;
        store_fence();
    }

    void drop_server() {
        if (!box) return;
        post(0xffffffffu);
        ttm_mailbox_release(box);
        box = nullptr;
    }

    // request: the coefficients, then - behind a store fence - the word that announces them; the results arrive where a launch
    // per evaluation puts them (tests: TTM_SRV_TEST_STALL = k makes the host miss the server's 0.2 s in front of request k)
    int serve(const double* cc) {
        static const int stall_at = [] { const char* e = getenv("TTM_SRV_TEST_STALL"); return e ? atoi(e) : 0; }();
        if (stall_at > 0 && (int)round + 1 == stall_at) std::this_thread::sleep_for(std::chrono::milliseconds(300));
        for (;;) {
            arm_values(q.sums_host, 1 + q.m);
            volatile double* bc = (volatile double*)(box + 8);
            for (int i = 0; i < q.m; ++i) bc[i] = cc[i];
            store_fence();
            post(++round);
            bool retry = false;
            int rc = poll_values(q.sums_host, 1 + q.m, stream, &retry);
            if (!rc || !retry) return rc;
            // no answer with the stream idle, or the FAIL pattern: the server has left or gives up.  Make sure every workgroup has
            // left, then re-arm both regions of the rows (a workgroup that stored late may have dirtied one) before anything else
            // evaluates on them.
            post(0xffffffffu);
            if ((rc = stream_idle(stream)) != TTM_OK || (rc = ttm_sentinel_fill(q.work, q.m, N, stream)) != TTM_OK) return rc;
            if (starts < 3 && start_server()) continue;
            drop_server();
            kind = SENT;
            return eval(cc);
        }
    }
};

// The L-BFGS-B loop of one component (TM:2978-3018, TM:3108-3114) behind the checks of every entry point.  pre_x != NULL: the
// rows of q.work are armed and an evaluation at pre_x with self-validating results is in flight on `stream` (results: sums_host);
// the loop's first evaluation uses it when it is at that point, and it is waited for whatever happens.  q.armed, in: the layout
// key (sentinel_layout) the rows of q.work were left armed with; out: the key this loop leaves them armed with, or 0.
//
// ONE monotone term (m = 1: the filtering and smoothing maps of Examples C, most components of Markov-type maps): the sample
// sums are known in closed form once they have been taken at one point.  dS_n = dPsi_n c + delta dPsi_n = dPsi_n (c + delta)
// (TM:2990-2993), so sum_n log dS_n = N log(c + delta) + sum_n log dPsi_n and sum_n dPsi_n / dS_n = N / (c + delta): the
// first evaluation of the loop goes to the device, every later one is two host operations - the same function to
// rounding (1e-16 relative, like the order of a reduction), no launch, no round trip.
int run_task(ttm_sep_task& q, int64_t N, double Ntotal, double delta, double* sums_dev, ttm_comm* comm, void* stream, int32_t maxiter,
             double* result, const double* pre_x) {
    if (const int arg_rc = check_task(q, N, Ntotal, sums_dev, comm)) return q.rc = arg_rc;
    struct Loop {
        Evaluator ev;
        const ttm_sep_task& q;
        double invN, delta;
        const double* pre_x;                                 // the evaluation launched ahead, until it has been waited for
        bool closed, have0;
        double Nw, KN;                                       // closed form of m = 1: weights N, sum_n log dPsi_n
        int rc;
    } L{{q, N, delta, sums_dev, comm, stream}, q, 1.0 / Ntotal, delta, pre_x,
        q.dPsi && q.m == 1 && delta >= 0.0 && q.lb && q.lb[0] >= 0.0, false, 0.0, 0.0, 0};
    const int key = L.ev.choose(pre_x != nullptr);
    auto fun = [](int32_t n, const double* cc, double* f, double* g, void* user) -> int32_t {
        Loop& L = *(Loop*)user;
        double* sums = L.q.sums_host;
        if (L.pre_x) {                                       // the evaluation that was launched ahead: wait for it whatever it is good for
            const bool have = memcmp(cc, L.pre_x, (size_t)n * 8) == 0;
            L.pre_x = nullptr;
            if ((L.rc = poll_values(sums, 1 + n, L.ev.stream)) || (!have && (L.rc = L.ev.eval(cc)))) return L.rc;
        } else if (L.closed && L.have0 && cc[0] + L.delta > 0.0) {
            sums[0] = L.Nw * log(cc[0] + L.delta) + L.KN;
            sums[1] = L.Nw / (cc[0] + L.delta);
        } else if ((L.rc = L.ev.eval(cc))) return L.rc;
        if (L.closed && !L.have0 && cc[0] + L.delta > 0.0) {  // the point the closed form is anchored at
            const double nw = sums[1] * (cc[0] + L.delta), kn = sums[0] - nw * log(cc[0] + L.delta);
            if (nw > 0.0 && nw < 1.0e300 && kn == kn && kn > -1.0e300 && kn < 1.0e300) { L.Nw = nw; L.KN = kn; L.have0 = true; }
            else L.closed = false;                           // (a vanishing or negative derivative somewhere: the sums stay on the device)
        }
        // J = c'Ac/2 - sum log dS / N + c.b,  grad = Ac - sums/N + b   (TM:3008-3018)
        double quad = 0.0, lin = 0.0;
        for (int i = 0; i < n; ++i) {
            double ax = 0.0;
            for (int j = 0; j < n; ++j) ax += L.q.A[i * n + j] * cc[j];
            quad += cc[i] * ax;
            lin += cc[i] * L.q.b[i];
            g[i] = ax - sums[1 + i] * L.invN + L.q.b[i];
        }
        *f = quad / 2.0 - sums[0] * L.invN + lin;
        return 0;
    };
    const int rc = ttm_lbfgsb_minimize(q.m, q.x, q.lb, q.ub, fun, &L, maxiter, result);
    // (a loop that ended before its first evaluation: `work` and sums_host go back to the caller once nothing writes them)
    const int ahead_rc = L.pre_x ? poll_values(q.sums_host, 1 + q.m, stream) : TTM_OK;
    q.rc = L.rc ? L.rc : ahead_rc ? ahead_rc : rc;
    q.armed = q.rc == TTM_OK ? key : 0;
    return q.rc;
}

}  // namespace

extern "C" {

int ttm_optimize_separable(const double* dPsi, int64_t ldp, int64_t N, int32_t m, const double* A, const double* b, double Ntotal,
                           double delta, const double* lb, const double* ub, double* x, double* work, uint32_t* counter,
                           double* sums_dev, double* sums_host, ttm_comm* comm, void* stream, int32_t maxiter, double* result) {
    if (!dPsi) return TTM_E_ARG;                             // (the cached basis only: a task without it reads the x_k column)
    ttm_sep_task q{};
    q.dPsi = dPsi; q.ldp = ldp; q.m = m; q.A = A; q.b = b; q.lb = lb; q.ub = ub; q.x = x;
    q.work = work; q.counter = counter; q.sums_host = sums_host;
    return run_task(q, N, Ntotal, delta, sums_dev, comm, stream, maxiter, result, nullptr);
}

int ttm_optimize_separable_batch(ttm_sep_task* tasks, int32_t ntasks, int64_t N, double Ntotal, double delta, int32_t nthreads,
                                 void* stream, int32_t maxiter) {
    if (!tasks || ntasks < 1 || N < 1) return TTM_E_ARG;
    // Components with ONE monotone term need one device evaluation (the closed form of run_task takes over behind it).  When at
    // most one other component is in the batch - the filter's maps: two such components and one with special terms - no threads:
    // the first evaluations of the one-term components are launched ahead on `stream`, the other component's loop runs behind
    // them, and the one-term loops find their sums in place (a thread per component cost ~40 us each to start and fought the long
    // loop for the runtime's launch lock).  The same evaluations at the same points: the same bits as the threaded batch.
    std::vector<int> ahead, rest;
    for (int t = 0; t < ntasks; ++t) {
        const ttm_sep_task& q = tasks[t];
        const bool one = q.dPsi && q.m == 1 && delta >= 0.0 && check_task(q, N, Ntotal, nullptr, nullptr) == TTM_OK &&
                         q.lb && q.lb[0] >= 0.0;
        (one ? ahead : rest).push_back(t);
    }
    if (ahead.empty() || rest.size() > 1)
        return run_batch(ntasks, nthreads, stream, [&](int t, void* st) {
            return run_task(tasks[t], N, Ntotal, delta, nullptr, nullptr, st, maxiter, tasks[t].result, nullptr);
        });
    std::vector<double> x0(ntasks, 0.0);
    std::vector<char> flying(ntasks, 0);
    const int key = sentinel_layout(1, N);
    for (int t : ahead) {
        ttm_sep_task& q = tasks[t];
        double v = q.x[0];                                   // the start as lbfgsb_minimize projects it
        if (v <= q.lb[0]) v = q.lb[0];
        else if (q.ub && q.ub[0] < INFINITY && v >= q.ub[0]) v = q.ub[0];
        x0[t] = v;
        if (!key || (q.armed != key && ttm_sentinel_fill(q.work, 1, N, stream) != TTM_OK)) continue;
        arm_values(q.sums_host, 2);
        flying[t] = ttm_objective_sep_cached_sent(q.dPsi, q.ldp, N, 1, &x0[t], delta, q.work, q.sums_host, stream) == TTM_OK;
    }
    for (int t : rest) run_task(tasks[t], N, Ntotal, delta, nullptr, nullptr, stream, maxiter, tasks[t].result, nullptr);
    for (int t : ahead) run_task(tasks[t], N, Ntotal, delta, nullptr, nullptr, stream, maxiter, tasks[t].result, flying[t] ? &x0[t] : nullptr);
    for (int t = 0; t < ntasks; ++t)
        if (tasks[t].rc) return tasks[t].rc;
    return TTM_OK;
}

// (Gnn + ridge I)^-1 Gnm by Cholesky on the diagonally equilibrated matrix with one step of iterative refinement - the host
// class's _normal_solve, ridge > 0.  G: the (n + m) x (n + m) Gram matrix, row-major; y: n x m.  false: not positive
// definite / not finite (the caller decides what then).
static bool sep_normal_solve(const double* G, int n, int m, double ridge, std::vector<double>& y) {
    const int ld = n + m;
    std::vector<double> d(n), Ms((size_t)n * n), U((size_t)n * n, 0.0), rhs((size_t)n * m), r((size_t)n * m);
    for (int i = 0; i < n; ++i) {
        d[i] = sqrt(G[i * ld + i] + ridge);
        if (!(d[i] > 0.0) || !(d[i] < INFINITY)) return false;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            Ms[i * n + j] = ((G[i * ld + j] + (i == j ? ridge : 0.0)) / d[i]) / d[j];
            if (!(fabs(Ms[i * n + j]) < INFINITY)) return false;
        }
    for (int j = 0; j < n; ++j) {                       // Ms = U'U, U upper triangular
        double s = Ms[j * n + j];
        for (int k = 0; k < j; ++k) s -= U[k * n + j] * U[k * n + j];
        if (!(s > 0.0)) return false;
        const double ujj = sqrt(s);
        U[j * n + j] = ujj;
        for (int i = j + 1; i < n; ++i) {
            double t = Ms[j * n + i];
            for (int k = 0; k < j; ++k) t -= U[k * n + j] * U[k * n + i];
            U[j * n + i] = t / ujj;
        }
    }
    auto solve = [&](std::vector<double>& b) {          // U'U x = b, column by column, in place
        for (int c = 0; c < m; ++c) {
            for (int i = 0; i < n; ++i) {
                double t = b[i * m + c];
                for (int k = 0; k < i; ++k) t -= U[k * n + i] * b[k * m + c];
                b[i * m + c] = t / U[i * n + i];
            }
            for (int i = n - 1; i >= 0; --i) {
                double t = b[i * m + c];
                for (int k = i + 1; k < n; ++k) t -= U[i * n + k] * b[k * m + c];
                b[i * m + c] = t / U[i * n + i];
            }
        }
    };
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < m; ++c) {
            rhs[i * m + c] = G[i * ld + n + c] / d[i];
            if (!(fabs(rhs[i * m + c]) < INFINITY)) return false;
        }
    y = rhs;
    solve(y);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < m; ++c) {
            double t = rhs[i * m + c];
            for (int k = 0; k < n; ++k) t -= Ms[i * n + k] * y[k * m + c];
            r[i * m + c] = t;
        }
    solve(r);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < m; ++c) y[i * m + c] = (y[i * m + c] + r[i * m + c]) / d[i];
    return true;
}

// The reduced separable problem with L2 regularisation (TM:3021-3050, 3148-3169) from the Gram matrix of
// [Psi_nonmon | Psi_mon]: A (m x m) of the monotone coefficients' objective and the map c_mon -> c_nonmon = -sol c_mon
// (sol: n x m).  What transport_map.separable_setup computes with NumPy, for the optimiser batches of the filter and smoother
// updates (six small solves per update: 0.2 ms of Python).  TTM_E_UNSUPPORTED: a matrix is not positive definite - the
// caller's own dense solve takes over.
int ttm_separable_reduce_l2(const double* G, int32_t n, int32_t m, double lam, double* A, double* sol) {
    if (!G || !A || !sol || n < 1 || m < 1 || n > 256 || m > 64 || !(lam > 0.0)) return TTM_E_ARG;
    const int ld = n + m;
    std::vector<double> Gm, S2;
    if (!sep_normal_solve(G, n, m, lam, Gm) || !sep_normal_solve(G, n, m, 2.0 * lam, S2)) return TTM_E_UNSUPPORTED;
    // dd = Gmm - Gnm'Gm - Gm'Gnm + (Gm'Gnn) Gm;  A = dd / 2 + lam (Gm'Gm + I), symmetrised
    std::vector<double> W((size_t)m * n), dd((size_t)m * m);
    for (int a = 0; a < m; ++a)
        for (int j = 0; j < n; ++j) {
            double t = 0.0;
            for (int i = 0; i < n; ++i) t += Gm[i * m + a] * G[i * ld + j];
            W[a * n + j] = t;                           // (Gm'Gnn)[a][j]
        }
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) {
            double t1 = 0.0, t2 = 0.0, t3 = 0.0, gg = 0.0;
            for (int i = 0; i < n; ++i) {
                t1 += G[i * ld + n + a] * Gm[i * m + b];
                t2 += Gm[i * m + a] * G[i * ld + n + b];
                t3 += W[a * n + i] * Gm[i * m + b];
                gg += Gm[i * m + a] * Gm[i * m + b];
            }
            dd[a * m + b] = (((G[(n + a) * ld + n + b] - t1) - t2) + t3) / 2.0 + lam * (gg + (a == b ? 1.0 : 0.0));
        }
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) A[a * m + b] = (dd[a * m + b] + dd[b * m + a]) / 2.0;
    memcpy(sol, S2.data(), (size_t)n * m * 8);
    return TTM_OK;
}

int ttm_optimize_integrated_batch(const ttm_program* p, ttm_int_task* tasks, int32_t ntasks, const double* Xsoa, int64_t ldx, int64_t N,
                                  double Ntotal, int32_t nthreads, void* stream, int32_t maxiter) {
    if (!p || !tasks || ntasks < 1 || N < 1) return TTM_E_ARG;
    return run_batch(ntasks, nthreads, stream, [&](int t, void* st) {
        ttm_int_task& q = tasks[t];
        return q.rc = ttm_optimize_integrated(p, q.k, q.m, Xsoa, ldx, N, Ntotal, q.regularization, q.lambda, q.x, q.work, q.counter,
                                              nullptr, q.sums_host, nullptr, st, maxiter, q.result);
    });
}

int ttm_bfgs_minimize(int32_t n, double* x, ttm_objective_cb fun, void* user, int32_t maxiter, double* result) {
    if (n < 1 || !x || !fun) return TTM_E_ARG;
    ttm_opt::BfgsOptions opt;
    if (maxiter > 0) opt.maxiter = maxiter;
    const ttm_opt::BfgsResult r =
        ttm_opt::bfgs_minimize(n, x, [&](const double* xx, double* f, double* g) { return fun(n, xx, f, g, user); }, opt);
    if (result) {
        result[0] = r.f; result[1] = r.gnorm; result[2] = r.nit; result[3] = r.nfev; result[4] = r.status;
    }
    return r.status < 0 ? TTM_E_HIP : TTM_OK;
}

int ttm_optimize_integrated(const ttm_program* p, int32_t k, int32_t m, const double* Xsoa, int64_t ldx, int64_t N, double Ntotal,
                            int32_t regularization, const double* lambda, double* x, double* work, uint32_t* counter,
                            double* sums_dev, double* sums_host, ttm_comm* comm, void* stream, int32_t maxiter, double* result) {
    if (!p || !Xsoa || !x || !work || !counter || !sums_host || m < 1 || m > 128 || N < 1 || !(Ntotal > 0.0) || regularization < 0 ||
        regularization > 2 || (regularization && !lambda))
        return TTM_E_ARG;
    if (comm && !sums_dev) return TTM_E_ARG;
    struct Ctx {
        const ttm_program* p;
        int k;
        const double* Xsoa;
        int64_t ldx, N;
        double invN;
        int reg;
        const double* lam;
        double *work, *sums_dev, *sums_host;
        uint32_t* counter;
        ttm_comm* comm;
        void* stream;
        int rc;
        long seq;
    } c{p, (int)k, Xsoa, ldx, N, 1.0 / Ntotal, (int)regularization, lambda, work, sums_dev, sums_host, counter, comm, stream, 0, 0};
    sums_host[1 + m] = 0.0;                                  // the completion mark (sums_host: >= 2 + m doubles)
    auto fun = [](int32_t n, const double* cc, double* f, double* g, void* user) -> int32_t {
        Ctx& c = *(Ctx*)user;
        // sums[0] = sum_n of the objective's sample terms, sums[1 + i] = sum_n of their derivatives (TM:3300-3380, 3435-3573)
        double* out = c.comm ? c.sums_dev : c.sums_host;
        if (!c.comm) {
            c.rc = objective_and_wait(c.sums_host + 1 + n, c.seq, c.stream, [&](double* flag, double mark) {
                return ttm_objective_host_marked(c.p, c.k, cc, c.Xsoa, c.ldx, c.N, c.work, c.counter, out, flag, mark, c.stream);
            });
            if (c.rc) return c.rc;
        } else {
            c.rc = ttm_objective_host(c.p, c.k, cc, c.Xsoa, c.ldx, c.N, c.work, c.counter, out, c.stream);
            if (c.rc) return c.rc;
        }
        if (c.comm) {
            c.rc = ttm_allreduce_f64(c.comm, c.sums_dev, 1 + n, TTM_OP_SUM, c.stream);
            if (c.rc) return c.rc;
#ifdef TTM_HOST_ONLY
            memcpy(c.sums_host, c.sums_dev, (size_t)(1 + n) * 8);
#else
            if (hipMemcpyAsync(c.sums_host, c.sums_dev, (size_t)(1 + n) * 8, hipMemcpyDeviceToHost, (hipStream_t)c.stream) != hipSuccess)
                return c.rc = TTM_E_HIP;
#endif
            c.rc = wait_for_mark(c.sums_host + 1 + n, c.seq, c.stream);
            if (c.rc) return c.rc;
        }
        // mean over the ensemble + the penalty on the coefficients (TM:3382-3431, 3575-3633)
        double pen = 0.0;
        for (int i = 0; i < n; ++i) {
            double gi = c.sums_host[1 + i] * c.invN;
            if (c.reg == 1) {
                pen += c.lam[i] * fabs(cc[i]);
                gi += c.lam[i] * (cc[i] > 0.0 ? 1.0 : cc[i] < 0.0 ? -1.0 : 0.0);
            } else if (c.reg == 2) {
                pen += c.lam[i] * cc[i] * cc[i];
                gi += c.lam[i] * 2 * cc[i];
            }
            g[i] = gi;
        }
        *f = c.sums_host[0] * c.invN + pen;
        return 0;
    };
    const int rc = ttm_bfgs_minimize(m, x, fun, &c, maxiter, result);
    return c.rc ? c.rc : rc;
}

}  // extern "C"
