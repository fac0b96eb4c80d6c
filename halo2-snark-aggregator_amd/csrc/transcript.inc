// C ABI of the transcript side (included into h2agg.hip: shares the context internals).  SURVEY.md 8(f) row 2.
//   PoseidonChip (hash/poseidon.rs:144-231), PoseidonEncode (mock/transcript_encode.rs:28-74),
//   PoseidonTranscriptRead (systems/halo2/transcript.rs:10-179) — batched over the proofs of one circuit.

namespace {

// Wall-clock split of h2agg_verify_aggregation.  H2AGG_TRACE_PHASES=1: on stderr (tools/pipeline_time.py reads it);
// h2agg_debug_configure(ctx, "phases", 1): kept in the context for h2agg_last_phases() — how bench.py names the phase behind
// the slowest repetition of a leg (VERDICT r5 item 3).  Beside the phases: the CPU the calling thread started and ended on and
// how often the kernel took it off its core in between (involuntary context switches), and for every host sponge chain when it
// started after the call began, how long it ran and on which CPU — a chain that starts late is a worker woken late, one that
// runs long is a worker sharing its core.
struct PhaseTrace {
    struct Job { float start_us = -1, dur_us = 0; int cpu = -1; };
    bool on;
    std::string* keep = nullptr;
    std::chrono::steady_clock::time_point t0, t_call;
    std::string line;
    std::vector<Job> jobs;
    float posted_us = 0;   // when the chains were handed to the pool
    int cpu0 = -1;
    long nivcsw0 = 0, minflt0 = 0;
    static long nivcsw() {
        struct rusage ru;
        return getrusage(RUSAGE_THREAD, &ru) == 0 ? ru.ru_nivcsw : 0;
    }
    static long minflt() {   // page faults of the whole process
        struct rusage ru;
        return getrusage(RUSAGE_SELF, &ru) == 0 ? ru.ru_minflt + ru.ru_majflt : 0;
    }
    explicit PhaseTrace(std::string* keep_in = nullptr)
        : on(keep_in != nullptr || getenv("H2AGG_TRACE_PHASES") != nullptr), keep(keep_in), t0(std::chrono::steady_clock::now()), t_call(t0) {
        if (on) {
            cpu0 = sched_getcpu();
            nivcsw0 = nivcsw();
            minflt0 = minflt();
        }
    }
    void mark(const char* name) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        char buf[64];
        snprintf(buf, sizeof buf, " %s=%.3f", name, std::chrono::duration<double, std::milli>(t1 - t0).count());
        line += buf;
        t0 = t1;
    }
    float since_call_us() const { return std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t_call).count(); }
    ~PhaseTrace() {
        if (!on) return;
        char buf[128];
        snprintf(buf, sizeof buf, " [caller cpu %d->%d, preempted %ld x, process page faults %ld]", cpu0, sched_getcpu(), nivcsw() - nivcsw0,
                 minflt() - minflt0);
        line += buf;
        if (!jobs.empty()) {
            snprintf(buf, sizeof buf, " [sponge chains posted at %.0f us, start_us+run_us@cpu:", posted_us);
            line += buf;
            for (const Job& j : jobs) {
                snprintf(buf, sizeof buf, " %.0f+%.0f@%d", j.start_us, j.dur_us, j.cpu);
                line += buf;
            }
            line += "]";
        }
        if (keep) *keep = line;
        if (getenv("H2AGG_TRACE_PHASES")) fprintf(stderr, "[h2agg phases, ms]%s\n", line.c_str());
    }
};
thread_local PhaseTrace* g_trace = nullptr;   // the call in progress on this thread (h2agg_verify_aggregation), if it traces
inline void trace_mark(const char* name) {
    if (g_trace) g_trace->mark(name);
}

// ---- host worker threads ------------------------------------------------------------------------------------------
// Per-proof host work (a proof's sponge chain, its schema construction) is independent until the lambda fold, so it runs on
// a small pool: persistent threads, the caller takes part, jobs are claimed from a shared counter.  Sized by what the
// process may actually use (affinity mask and cgroup CPU quota), capped at 32; H2AGG_HOST_THREADS overrides.
struct HostPool {
    // Several runs can be open at once (contexts on different caller threads: one call's sponges run while another call is on
    // the device); the workers take jobs from whichever open run still has some, oldest run first.
    struct Run {
        std::function<void(size_t)> f;
        size_t n = 0, next = 0, active = 0;
        size_t workers = 0, limit = 0;   // pool threads on this run right now / at most (the caller of end() is extra)
    };
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    std::vector<std::thread> threads;
    std::vector<Run*> runs;   // open runs, in begin() order
    int want = 1;
    // A call that will post chains in a few hundred microseconds (the device is still decompressing its points) wakes that
    // many workers NOW: they spin on `posted` instead of sleeping, so a chain starts within a microsecond of being posted
    // instead of a futex wake-up + scheduler latency later (20-50 us, p95 — and on a core that has had time to clock up).
    // Only an idle pool is pre-woken: with several calls in flight the workers are busy anyway and spinning would steal
    // their cores.
    int spin_tickets = 0;                          // (m held) workers still to take up spinning
    int spinning = 0;                              // (m held) workers spinning right now
    std::atomic<uint64_t> posted{0};               // begin() count
    std::chrono::steady_clock::time_point spin_deadline;

    static int usable_cpus() {
        int n = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "<quota> <period>" or "max <period>"
            char q[64];
            long period = 0;
            if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
                const long quota = (atol(q) + period - 1) / period;
                if (quota >= 1 && quota < n) n = (int)quota;
            }
            fclose(f);
        }
        if (const char* e = getenv("H2AGG_HOST_THREADS")) n = atoi(e);
        return n < 1 ? 1 : n > 32 ? 32 : n;
    }
    static HostPool& get() {
        static HostPool* p = new HostPool();   // never destroyed: its threads may outlive static destruction
        return *p;
    }
    HostPool() : want(usable_cpus()) {}
    // (Placement of the workers is the scheduler's.  Round 6 measured three alternatives on 256-CPU hosts, 1 000-1 500 calls
    // each, alternating with the plain pool on the same box: one hardware thread per worker — the caller or a runtime thread
    // that lands on it stalls for milliseconds; the physical cores dealt out to the workers as affinity masks, so that no two
    // chains share a core — chains slower than 1.15 x the median 505 and 179 of 4 000 against 281 and 335 without, and more
    // multi-millisecond stalls; all workers confined to the first hardware thread of every core — 133 / 4 / 44 slow chains of
    // 6 000 against 24 / 21 / 51.  None kept.  profiles/r06_sweeps.txt section 2.)
    int size() const { return want; }
    void prewake(size_t n) {
        std::unique_lock<std::mutex> lk(m);
        if (!runs.empty() || spin_tickets > 0 || n == 0) return;
        while ((int)threads.size() < want) start_worker();
        spin_tickets = (int)std::min<size_t>(n, threads.size());
        spin_deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(1500);
        const int wake = spin_tickets;
        lk.unlock();   // (wake-ups go out with the mutex free: a woken worker's first act is to take it)
        for (int i = 0; i < wake; ++i) cv_work.notify_one();
    }
    void start_worker() {   // (m held)
        threads.emplace_back([this] { worker(); });
        threads.back().detach();
    }
    Run* pick() {   // (m held) the oldest open run with a job left
        for (Run* r : runs)
            if (r->next < r->n && r->workers < r->limit) return r;
        return nullptr;
    }
    void worker() {
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            Run* r = nullptr;
            cv_work.wait(lk, [&] { return (r = pick()) != nullptr || spin_tickets > 0; });
            if (!r) {   // pre-woken: wait for the run on the core, not in the kernel
                --spin_tickets;
                ++spinning;
                const uint64_t seen = posted.load(std::memory_order_relaxed);
                const auto until = spin_deadline;
                lk.unlock();
                // (polite: every ~10 us the spinner offers its CPU — a caller that comes back from a wait onto this
                // worker's run queue would otherwise sit behind it until the deadline, with the chains it is about to
                // post: 1.5-ms stalls, several in a row with several spinners)
                for (unsigned it = 0; posted.load(std::memory_order_acquire) == seen; ++it) {
                    __builtin_ia32_pause();
                    if ((it & 255) == 255) {
                        sched_yield();
                        if (std::chrono::steady_clock::now() > until) break;
                    }
                }
                lk.lock();
                --spinning;
                continue;
            }
            const size_t i = r->next++;
            ++r->active;
            ++r->workers;
            lk.unlock();
            r->f(i);
            lk.lock();
            --r->workers;
            if (--r->active == 0 && r->next >= r->n) {
                lk.unlock();
                cv_done.notify_all();   // (`r` may be gone from here on: end() deletes it once it sees active == 0)
                lk.lock();
            }
        }
    }
    // run f(0) .. f(n-1) on up to `max_threads` threads (the caller included); returns when all are done.  f must not throw.
    void run(size_t count, int max_threads, const std::function<void(size_t)>& f) {
        if (count == 0) return;
        if ((int)std::min<size_t>(count, (size_t)std::min(max_threads, want)) <= 1) {
            for (size_t i = 0; i < count; ++i) f(i);
            return;
        }
        end(begin(count, max_threads - 1, f));
    }
    // The same in two halves: begin() hands f(0) .. f(n-1) to the worker threads (at most `helpers` of them are started for
    // it) and returns at once — the caller does something else (records the schema the challenges will feed, or waits for the
    // device) — end() has the caller take whatever jobs of ITS run are left and waits for the rest.
    Run* begin(size_t count, int helpers, const std::function<void(size_t)>& f) {
        Run* r = new Run();
        r->f = f;
        r->n = count;
        r->limit = (size_t)std::max(0, helpers);
        std::unique_lock<std::mutex> lk(m);
        if (helpers > 0)   // (the workers are started on first use and sleep between runs)
            while ((int)threads.size() < want) start_worker();
        runs.push_back(r);
        posted.fetch_add(1, std::memory_order_release);   // spinning workers come for it
        // wake as many sleepers as the run can use and no more (waking all 16-32 for four chains had every one of them
        // take the mutex, find nothing and go back to sleep — on cores next to the ones that work)
        const size_t wake = std::min<size_t>(std::min<size_t>(count, r->limit), threads.size());
        const size_t awake = (size_t)(spinning + spin_tickets);   // spinning, or notified by prewake() and on their way
        spin_tickets = 0;   // (a pre-woken worker that arrives from here on finds the run itself; nobody spins for it any more)
        lk.unlock();
        for (size_t i = awake; i < wake; ++i) cv_work.notify_one();
        return r;
    }
    void end(Run* r) {
        std::unique_lock<std::mutex> lk(m);
        while (r->next < r->n) {
            const size_t i = r->next++;
            ++r->active;
            lk.unlock();
            r->f(i);
            lk.lock();
            --r->active;
        }
        // (the caller SLEEPS here.  Spinning for the last chain instead — a futex wake-up is 20-40 us behind it — was measured:
        // the caller's core is where the scheduler likes to put a woken worker's sibling thread, and a spinning caller slows
        // that chain from 760 to 1 100 us: sponge_wait p50 0.79 -> 1.11 ms.  profiles/r06_sweeps.txt section 2.)
        cv_done.wait(lk, [&] { return r->active == 0; });
        runs.erase(std::find(runs.begin(), runs.end(), r));
        lk.unlock();
        delete r;
    }
};

bool host_pool_pair_if_awake(const std::function<void()>& on_worker, const std::function<void()>& here) {
    HostPool& pool = HostPool::get();
    {
        std::unique_lock<std::mutex> lk(pool.m);
        if (pool.spinning + pool.spin_tickets == 0 || !pool.runs.empty()) return false;
    }
    HostPool::Run* r = pool.begin(1, 1, [&on_worker](size_t) { on_worker(); });
    here();
    pool.end(r);   // (should the spinner have given up in between, the job runs here: same result, later)
    return true;
}

const poseidon_host::Spec& poseidon_host_spec() {
    static const poseidon_host::Spec spec(PSD_T, PSD_RF, PSD_RP);   // ~40 ms, once per process
    return spec;
}
const poseidon_host::FastSpec& poseidon_fast_spec() {
    static const poseidon_host::FastSpec fs(poseidon_host_spec());
    return fs;
}

// Which backend runs the sponges of `nproofs` transcripts: 1 = device, 2 = host threads.
// cfg: 0 = auto, 1 / 2 forced (h2agg_transcript_configure; H2AGG_TRANSCRIPT=device|host overrides auto).
// auto: a chain costs ~T_dev on the device whatever the batch (one 16-lane group per proof) and T_host on a host core; the
// host finishes ceil(nproofs / threads) chains in a row.  Measured (profiles/r03_sweeps.txt): T_dev / T_host ~ PSD_HOST_GAIN.
constexpr int PSD_HOST_GAIN = 8;
int transcript_backend(const h2agg_ctx* c, size_t nproofs) {
    int cfg = c->cfg_transcript;
    if (cfg == 0) {
        static const int env = [] {
            const char* e = getenv("H2AGG_TRANSCRIPT");
            return !e ? 0 : !strcmp(e, "device") ? 1 : !strcmp(e, "host") ? 2 : 0;
        }();
        cfg = env;
    }
    if (cfg == 1 || cfg == 2) return cfg;
    const size_t threads = (size_t)HostPool::get().size();
    const size_t rounds = (nproofs + threads - 1) / threads;
    return rounds <= (size_t)PSD_HOST_GAIN ? 2 : 1;
}

// which arithmetic the host sponge runs on: 1 = AVX-512 IFMA (8 elements per vector, csrc/poseidon_ifma_host.hpp) when the CPU
// has it, 0 = portable 4 x 64-bit (csrc/poseidon_sponge_host.hpp).  H2AGG_HOST_SPONGE=scalar|ifma forces one (ifma only if
// the CPU can run it); h2agg_host_sponge_kind() reports the choice.
int host_sponge_kind() {
#ifdef H2AGG_HAVE_IFMA_BUILD
    static const int kind = [] {
        const bool can = poseidon_host::ifma::cpu_has_ifma();
        const char* e = getenv("H2AGG_HOST_SPONGE");
        if (e && !strcmp(e, "scalar")) return 0;
        return can ? 1 : 0;
    }();
    return kind;
#else
    return 0;
#endif
}
#ifdef H2AGG_HAVE_IFMA_BUILD
const poseidon_host::ifma::Consts& poseidon_ifma_consts() {
    static const poseidon_host::ifma::Consts c(poseidon_host_spec());
    return c;
}
#endif

// the sponges of `nproofs` element streams on host threads; returns FLAG_NONCANONICAL if an element was >= r
// kind: -1 = the process-wide choice (host_sponge_kind), 0 / 1 forced (differential tests)
uint32_t poseidon_run_host(const uint8_t* elems, size_t elem_stride, const uint32_t* upto, uint32_t nsq, size_t nproofs,
                           uint8_t* out, int max_threads = 1 << 30, int kind = -1) {
    const poseidon_host::FastSpec& fs = poseidon_fast_spec();
    std::atomic<uint32_t> bad{0};
    if (kind < 0) kind = host_sponge_kind();
#ifdef H2AGG_HAVE_IFMA_BUILD
    if (kind == 1 && poseidon_host::ifma::cpu_has_ifma() && poseidon_ifma_consts().ok) {
        const poseidon_host::ifma::Consts& C = poseidon_ifma_consts();
        HostPool::get().run(nproofs, max_threads, [&](size_t p) {
            if (!poseidon_host::ifma::sponge_run(C, elems + p * elem_stride, upto, nsq, out + 32 * (size_t)nsq * p))
                bad.fetch_or(FLAG_NONCANONICAL, std::memory_order_relaxed);
        });
        return bad.load();
    }
#endif
    HostPool::get().run(nproofs, max_threads, [&](size_t p) {
        if (!poseidon_host::sponge_run(fs, elems + p * elem_stride, upto, nsq, out + 32 * (size_t)nsq * p))
            bad.fetch_or(FLAG_NONCANONICAL, std::memory_order_relaxed);
    });
    return bad.load();
}

// the T = 9 / R_F = 8 / R_P = 63 constants, generated on the host (csrc/poseidon_host.hpp) and kept as device registers
int poseidon_spec(h2agg_ctx* c, const uint32_t** out) {
    if (!c->psd_ready) {
        const poseidon_host::Spec& spec = poseidon_host_spec();
        if (!spec.ok) return fail(c, H2AGG_ERR_INVALID, "Poseidon parameter generation failed");
        std::vector<uint8_t> canon((size_t)PSD_NCONST * 32);
        auto put = [&](uint32_t idx, const poseidon_host::HFr& v) {
            uint64_t w[4];
            poseidon_host::to_canonical(v, w);
            memcpy(canon.data() + 32 * (size_t)idx, w, 32);
        };
        for (int k = 0; k <= PSD_H; ++k)
            for (int i = 0; i < PSD_T; ++i) put(PSD_START + k * PSD_T + i, spec.start[k][i]);
        for (int k = 0; k < PSD_RP; ++k) put(PSD_PARTIAL + k, spec.partial[k]);
        for (int k = 0; k < PSD_H - 1; ++k)
            for (int i = 0; i < PSD_T; ++i) put(PSD_END + k * PSD_T + i, spec.end[k][i]);
        for (int i = 0; i < PSD_T; ++i)
            for (int j = 0; j < PSD_T; ++j) {
                put(PSD_MDS + i * PSD_T + j, spec.mds[i][j]);
                put(PSD_PRE + i * PSD_T + j, spec.pre_sparse[i][j]);
            }
        // partial rounds in their scaled form (Spec::scale_partial_rounds): SROW[k] = D_k | R_{k,1..8}, SCOL[k] = A_{k,1..8}
        for (int k = 0; k < PSD_RP; ++k) {
            put(PSD_SROW + k * PSD_T, spec.ps_d[k]);
            for (int j = 1; j < PSD_T; ++j) put(PSD_SROW + k * PSD_T + j, spec.ps_r[k][j - 1]);
            for (int j = 0; j < PSD_T - 1; ++j) put(PSD_SCOL + k * (PSD_T - 1) + j, spec.ps_a[k][j]);
        }
        for (int j = 0; j < PSD_T; ++j) put(PSD_FIN + j, spec.ps_fin[j]);
        TRY(ensure(c, c->psd_spec, (size_t)PSD_NCONST * REG_WORDS * 4 + canon.size()));
        uint8_t* d_canon = (uint8_t*)c->psd_spec.p + (size_t)PSD_NCONST * REG_WORDS * 4;
        HIP_TRY(c, hipMemcpyAsync(d_canon, canon.data(), canon.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_tape_load_consts, dim3((PSD_NCONST + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)d_canon, (uint32_t)PSD_NCONST, (uint32_t*)c->psd_spec.p, c->d_flags);
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // `canon` is pageable host memory
        c->psd_ready = true;
    }
    *out = (const uint32_t*)c->psd_spec.p;
    return H2AGG_OK;
}

// sponges over device-resident element streams; d_upto: device copy of the squeeze positions
int poseidon_run(h2agg_ctx* c, const uint8_t* d_elems, size_t elem_stride, const uint32_t* d_upto, uint32_t nsq,
                 uint32_t nproofs, uint8_t* d_out) {
    const uint32_t* spec = nullptr;
    TRY(poseidon_spec(c, &spec));
    hipLaunchKernelGGL(k_poseidon_transcript, dim3((nproofs + PSD_PER_BLOCK - 1) / PSD_PER_BLOCK), dim3(PSD_BLOCK), 0, c->stream,
                       spec, d_elems, elem_stride, d_upto, nsq, nproofs, d_out, c->d_flags);
    return H2AGG_OK;
}

// A transcript script: what a PoseidonTranscriptRead is asked to do, in order.
//   'P' read_point   'S' read_scalar   'Q' squeeze_challenge_scalar   'C' common_scalar(next constant)
//   'X' common_point(next external point of this proof)
struct TrLayout {
    std::vector<TrItem> items;
    std::vector<uint32_t> upto;
    uint32_t npoints = 0, nscalars = 0, nconsts = 0, next = 0, nelem = 0;
    size_t proof_len = 0;
};
bool parse_script(const char* script, size_t n, TrLayout& L) {
    for (size_t i = 0; i < n; ++i) {
        TrItem it{0, 0, L.nelem, 0};
        switch (script[i]) {
        case 'P':
            it.kind = TR_POINT;
            it.src = (uint32_t)L.proof_len;
            it.pidx = L.npoints++;
            L.proof_len += 32;
            L.nelem += 2;
            break;
        case 'S':
            it.kind = TR_SCALAR;
            it.src = (uint32_t)L.proof_len;
            L.nscalars++;
            L.proof_len += 32;
            L.nelem += 1;
            break;
        case 'C':
            it.kind = TR_CONST;
            it.src = L.nconsts++;
            L.nelem += 1;
            break;
        case 'X':
            it.kind = TR_POINT_EXT;
            it.src = L.next++;
            L.nelem += 2;
            break;
        case 'Q':
            L.upto.push_back(L.nelem);
            continue;
        default:
            return false;
        }
        L.items.push_back(it);
    }
    return true;
}

// device half: proofs (host) -> decompressed points + element streams + challenges, all left on the device
//   d_points  = c->tr_points  [nproofs][npoints][64]
//   d_chal    = c->tr_chal    [nproofs][nsq][32]
// host_elems != nullptr: only the element streams are produced and queued for download into *host_elems ([nproofs][stride]);
//   no sponge runs here.
// host_chal != nullptr: the sponges run on HOST threads instead (transcript_backend() == 2): the element streams come down,
//   the challenges [nproofs][nsq][32] are written to host_chal (nothing goes to c->tr_chal), *host_flags receives
//   FLAG_NONCANONICAL if a scalar of a proof was >= r; the caller's stream is synchronised on return.
// where the pieces of a transcript batch sit inside the staging block / c->tr_in
struct TrBlock {
    size_t hdr, hdr2, hdr3, total, elem_stride, nsq;
};
TrBlock transcript_block(const TrLayout& L, size_t nproofs) {
    TrBlock b;
    b.nsq = L.upto.size();
    b.elem_stride = 32 * (size_t)(L.nelem ? L.nelem : 1);
    b.hdr = ((L.items.size() * sizeof(TrItem) + 255) & ~(size_t)255);
    b.hdr2 = b.hdr + ((b.nsq * 4 + 255) & ~(size_t)255);
    b.hdr3 = b.hdr2 + ((L.nconsts * 32 + 255) & ~(size_t)255);
    b.total = b.hdr3 + nproofs * L.proof_len;
    return b;
}
// the element-stream kernel, all of it or one of its two halves (see k_transcript_elements: `which`)
void transcript_elements_launch(h2agg_ctx* c, const TrLayout& L, const TrBlock& b, size_t nproofs, const uint8_t* d_ext_points,
                                hipStream_t st, int which) {
    uint8_t* d = (uint8_t*)c->tr_in.p;
    const size_t work = nproofs * L.items.size();
    hipLaunchKernelGGL(k_transcript_elements, dim3(grid_for(c, work ? work : 1)), dim3(BLOCK), 0, st,
                       (const uint8_t*)(d + b.hdr3), L.proof_len, d_ext_points, L.next, (const uint8_t*)(d + b.hdr2),
                       (const TrItem*)d, (uint32_t)L.items.size(), (uint32_t)nproofs, L.npoints, (uint8_t*)c->tr_points.p,
                       (uint8_t*)c->tr_elems.p, b.elem_stride, c->d_flags, which);
}
// Early half of a transcript batch, on `st` (an auxiliary stream): stage + upload the layout and the proof bytes, decompress
// every proof point and lay out everything that does not need the external points.  The staging block is written at
// c->h_stage + stage_off (the caller has sized it with ensure_pinned and keeps other data elsewhere in it).
int transcript_begin(h2agg_ctx* c, const TrLayout& L, const TrBlock& b, const uint8_t* const* proofs, size_t nproofs,
                     const uint8_t* consts, hipStream_t st, size_t stage_off) {
    TRY(ensure(c, c->tr_in, b.total));
    TRY(ensure(c, c->tr_points, nproofs * (size_t)(L.npoints ? L.npoints : 1) * 64));
    TRY(ensure(c, c->tr_elems, nproofs * b.elem_stride));
    TRY(ensure(c, c->tr_chal, nproofs * (b.nsq ? b.nsq : 1) * 32));
    uint8_t* h = c->h_stage + stage_off;
    memcpy(h, L.items.data(), L.items.size() * sizeof(TrItem));
    if (b.nsq) memcpy(h + b.hdr, L.upto.data(), b.nsq * 4);
    if (L.nconsts) memcpy(h + b.hdr2, consts, (size_t)L.nconsts * 32);
    for (size_t i = 0; i < nproofs; ++i) memcpy(h + b.hdr3 + i * L.proof_len, proofs[i], L.proof_len);
    HIP_TRY(c, hipMemcpyAsync(c->tr_in.p, h, b.total, hipMemcpyHostToDevice, st));
    transcript_elements_launch(c, L, b, nproofs, nullptr, st, 1);
    return H2AGG_OK;
}

int transcript_run(h2agg_ctx* c, const TrLayout& L, const uint8_t* proofs, size_t nproofs, const uint8_t* consts,
                   const uint8_t* d_ext_points /* device, [nproofs][next][64] canonical affine */,
                   uint8_t* host_chal = nullptr, uint32_t* host_flags = nullptr, std::vector<uint8_t>* host_elems = nullptr) {
    const TrBlock b = transcript_block(L, nproofs);
    const size_t nsq = b.nsq, elem_stride = b.elem_stride, hdr = b.hdr, hdr2 = b.hdr2, hdr3 = b.hdr3, total = b.total;
    TRY(ensure_pinned(c, c->h_stage, total, "staging block"));
    TRY(ensure(c, c->tr_in, total));
    TRY(ensure(c, c->tr_points, nproofs * (size_t)(L.npoints ? L.npoints : 1) * 64));
    TRY(ensure(c, c->tr_elems, nproofs * elem_stride));
    TRY(ensure(c, c->tr_chal, nproofs * (nsq ? nsq : 1) * 32));
    uint8_t* h = c->h_stage;
    memcpy(h, L.items.data(), L.items.size() * sizeof(TrItem));
    if (nsq) memcpy(h + hdr, L.upto.data(), nsq * 4);
    if (L.nconsts) memcpy(h + hdr2, consts, (size_t)L.nconsts * 32);
    memcpy(h + hdr3, proofs, nproofs * L.proof_len);
    uint8_t* d = (uint8_t*)c->tr_in.p;
    HIP_TRY(c, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, c->stream));
    transcript_elements_launch(c, L, b, nproofs, d_ext_points, c->stream, 0);
    if (nsq && host_elems) {   // the caller runs the sponges itself, later (h2agg_verify_aggregation: under its schema construction)
        host_elems->resize(nproofs * elem_stride);
        HIP_TRY(c, hipMemcpyAsync(host_elems->data(), c->tr_elems.p, host_elems->size(), hipMemcpyDeviceToHost, c->stream));
    } else if (nsq && host_chal) {
        std::vector<uint8_t>& he = c->h_elems;
        he.resize(nproofs * elem_stride);
        HIP_TRY(c, hipMemcpyAsync(he.data(), c->tr_elems.p, he.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        trace_mark("tr_elements");
        const uint32_t f = poseidon_run_host(he.data(), elem_stride, L.upto.data(), (uint32_t)nsq, nproofs, host_chal);
        trace_mark("tr_host_sponge");
        if (host_flags) *host_flags |= f;
    } else if (nsq) {
        TRY(poseidon_run(c, (const uint8_t*)c->tr_elems.p, elem_stride, (const uint32_t*)(d + hdr), (uint32_t)nsq,
                         (uint32_t)nproofs, (uint8_t*)c->tr_chal.p));
    }
    return H2AGG_OK;
}

// ---- the ShaRead family (transcript/sha.rs:23-127): SHA-256 / Keccak-256 over uncompressed points ---------------------------
// The same scripts, the same TrLayout — with points of 64 bytes (x | y, sha.rs:53-54), items[].dst and upto[] counting 32-bit
// WORDS of the proof's message stream (a point's block is 24 words, a scalar's 16: sha.rs:94-126) — and the same two device
// buffers downstream: c->tr_points, c->tr_chal.  c->tr_elems holds the message streams, word-interleaved over groups of 64
// proofs (csrc/hash_transcript_kernels.hpp).
bool hash_kind_ok(int kind) { return kind == H2AGG_TRANSCRIPT_KIND_SHA256 || kind == H2AGG_TRANSCRIPT_KIND_KECCAK256; }
bool parse_script_hash(const char* script, size_t n, TrLayout& L) {
    for (size_t i = 0; i < n; ++i) {
        TrItem it{0, 0, L.nelem, 0};
        switch (script[i]) {
        case 'P':
            it.kind = TR_POINT;
            it.src = (uint32_t)L.proof_len;
            it.pidx = L.npoints++;
            L.proof_len += 64;
            L.nelem += 24;
            break;
        case 'S':
            it.kind = TR_SCALAR;
            it.src = (uint32_t)L.proof_len;
            L.nscalars++;
            L.proof_len += 32;
            L.nelem += 16;
            break;
        case 'C':
            it.kind = TR_CONST;
            it.src = L.nconsts++;
            L.nelem += 16;
            break;
        case 'X':
            it.kind = TR_POINT_EXT;
            it.src = L.next++;
            L.nelem += 24;
            break;
        case 'Q':
            L.upto.push_back(L.nelem);
            continue;
        default:
            return false;
        }
        L.items.push_back(it);
    }
    return true;
}
size_t hash_stream_bytes(const TrLayout& L, size_t nproofs) {   // whole groups of 64 proofs: the chain's idle lanes read too
    const size_t groups = (nproofs + HT_LANES - 1) / HT_LANES;
    return groups * HT_LANES * (size_t)(L.nelem ? L.nelem : 1) * 4;
}
// Which backend runs the chains of `nproofs` hash transcripts: 1 = device, 2 = host threads.  Forced as for Poseidon
// (h2agg_transcript_configure, H2AGG_TRANSCRIPT).  auto: one lane walks one transcript serially, so the device only pays with
// thousands of proofs in flight; measured (profiles/hash_transcript.txt) the host pool is ahead up to HASH_DEVICE_FROM proofs.
constexpr size_t HASH_DEVICE_FROM = (size_t)1 << 62;   // not reached: auto = host (DESIGN.md 5.4)
int hash_backend(const h2agg_ctx* c, size_t nproofs) {
    int cfg = c->cfg_transcript;
    if (cfg == 0) {
        const char* e = getenv("H2AGG_TRANSCRIPT");
        cfg = !e ? 0 : !strcmp(e, "device") ? 1 : !strcmp(e, "host") ? 2 : 0;
    }
    if (cfg == 1 || cfg == 2) return cfg;
    return nproofs >= HASH_DEVICE_FROM ? 1 : 2;
}
void hash_stream_launch(h2agg_ctx* c, const TrLayout& L, const TrBlock& b, size_t nproofs, const uint8_t* d_ext_points,
                        hipStream_t st, int which) {
    uint8_t* d = (uint8_t*)c->tr_in.p;
    const size_t work = nproofs * L.items.size();
    if (!work) return;
    hipLaunchKernelGGL(k_hash_transcript_stream, dim3(grid_for(c, work)), dim3(BLOCK), 0, st, (const uint8_t*)(d + b.hdr3),
                       L.proof_len, d_ext_points, L.next, (const uint8_t*)(d + b.hdr2), (const TrItem*)d, (uint32_t)L.items.size(),
                       (uint32_t)nproofs, L.npoints, (uint8_t*)c->tr_points.p, (uint32_t*)c->tr_elems.p, L.nelem, c->d_flags, which);
}
// stage + upload layout and proof bytes, then everything that needs the proof bytes only (the early half, on `st`)
int hash_transcript_begin(h2agg_ctx* c, const TrLayout& L, const TrBlock& b, const uint8_t* const* proofs, const uint8_t* flat,
                          size_t nproofs, const uint8_t* consts, hipStream_t st) {
    TRY(ensure(c, c->tr_in, b.total));
    TRY(ensure(c, c->tr_points, nproofs * (size_t)(L.npoints ? L.npoints : 1) * 64));
    TRY(ensure(c, c->tr_elems, hash_stream_bytes(L, nproofs)));
    TRY(ensure(c, c->tr_chal, nproofs * (b.nsq ? b.nsq : 1) * 32));
    uint8_t* h = c->h_stage;
    memcpy(h, L.items.data(), L.items.size() * sizeof(TrItem));
    if (b.nsq) memcpy(h + b.hdr, L.upto.data(), b.nsq * 4);
    if (L.nconsts) memcpy(h + b.hdr2, consts, (size_t)L.nconsts * 32);
    if (flat) memcpy(h + b.hdr3, flat, nproofs * L.proof_len);
    else
        for (size_t i = 0; i < nproofs; ++i) memcpy(h + b.hdr3 + i * L.proof_len, proofs[i], L.proof_len);
    HIP_TRY(c, hipMemcpyAsync(c->tr_in.p, h, b.total, hipMemcpyHostToDevice, st));
    hash_stream_launch(c, L, b, nproofs, nullptr, st, 1);
    return H2AGG_OK;
}
// the chains over the finished message streams, on the context's stream.  Device: challenges to c->tr_chal.  Host
// (host_chal != nullptr): the streams come down, one proof per job on the pool, challenges [nproofs][nsq][32] to host_chal;
// the stream is synchronised on return.
int hash_chain_run(h2agg_ctx* c, int kind, const TrLayout& L, const TrBlock& b, size_t nproofs, uint8_t* host_chal) {
    if (!b.nsq) return H2AGG_OK;
    if (!host_chal) {
        const uint32_t* d_upto = (const uint32_t*)((const uint8_t*)c->tr_in.p + b.hdr);
        const dim3 grid((unsigned)((nproofs + HT_LANES - 1) / HT_LANES));
        if (kind == H2AGG_TRANSCRIPT_KIND_SHA256)
            hipLaunchKernelGGL(k_hash_transcript_chain<HT_SHA256>, grid, dim3(HT_LANES), 0, c->stream, (const uint32_t*)c->tr_elems.p,
                               L.nelem, d_upto, (uint32_t)b.nsq, (uint32_t)nproofs, (uint8_t*)c->tr_chal.p);
        else
            hipLaunchKernelGGL(k_hash_transcript_chain<HT_KECCAK256>, grid, dim3(HT_LANES), 0, c->stream, (const uint32_t*)c->tr_elems.p,
                               L.nelem, d_upto, (uint32_t)b.nsq, (uint32_t)nproofs, (uint8_t*)c->tr_chal.p);
        return H2AGG_OK;
    }
    std::vector<uint8_t>& he = c->h_elems;
    he.resize(hash_stream_bytes(L, nproofs));
    HIP_TRY(c, hipMemcpyAsync(he.data(), c->tr_elems.p, he.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    trace_mark("tr_elements");
    std::vector<uint32_t> seg_bytes(L.upto);
    for (uint32_t& v : seg_bytes) v *= 4;
    const uint32_t* msg = (const uint32_t*)he.data();
    const uint32_t nwords = L.nelem, nsq = (uint32_t)b.nsq;
    const int hk = kind == H2AGG_TRANSCRIPT_KIND_SHA256 ? hash_host::KIND_SHA256 : hash_host::KIND_KECCAK256;
    HostPool::get().run(nproofs, 1 << 30, [&](size_t p) {
        hash_host::chain_run(hk, msg + ((p / HT_LANES) * nwords) * HT_LANES + p % HT_LANES, HT_LANES, seg_bytes.data(), nsq,
                             host_chal + 32 * (size_t)nsq * p);
    });
    trace_mark("tr_host_chain");
    return H2AGG_OK;
}

// the whole of a ShaRead batch on host threads (no device): checks, blocks, chains.  -> FLAG_* bits
uint32_t hash_transcript_host(int kind, const TrLayout& L, const uint8_t* proofs, size_t nproofs, const uint8_t* consts,
                              const uint8_t* ext, uint8_t* points_out, uint8_t* chal_out, int max_threads) {
    std::atomic<uint32_t> flags{0};
    std::vector<uint32_t> seg_bytes(L.upto);
    for (uint32_t& v : seg_bytes) v *= 4;
    const int hk = kind == H2AGG_TRANSCRIPT_KIND_SHA256 ? hash_host::KIND_SHA256 : hash_host::KIND_KECCAK256;
    HostPool::get().run(nproofs, max_threads, [&](size_t p) {
        std::vector<uint32_t> msg((size_t)L.nelem + 1);
        uint8_t* m = (uint8_t*)msg.data();
        const uint8_t* proof = proofs + p * L.proof_len;
        uint32_t f = 0;
        for (const TrItem& it : L.items) {
            uint8_t* dst = m + 4 * (size_t)it.dst;
            if (it.kind == TR_CONST || it.kind == TR_SCALAR) {
                const uint8_t* s = it.kind == TR_CONST ? consts + 32 * (size_t)it.src : proof + it.src;
                if (!hash_host::scalar_ok(s)) f |= FLAG_NONCANONICAL;
                hash_host::block_scalar(dst, s);
            } else {
                const uint8_t* xy = it.kind == TR_POINT_EXT ? ext + 64 * (p * L.next + it.src) : proof + it.src;
                const bool good = hash_host::point_ok(xy);
                if (!good) f |= FLAG_BAD_POINT;
                if (it.kind == TR_POINT) {
                    uint8_t* po = points_out + 64 * (p * L.npoints + it.pidx);
                    if (good) memcpy(po, xy, 64);
                    else memset(po, 0, 64);
                }
                hash_host::block_point(dst, xy);
            }
        }
        if (!L.upto.empty())
            hash_host::chain_run(hk, msg.data(), 1, seg_bytes.data(), (uint32_t)L.upto.size(), chal_out + 32 * L.upto.size() * p);
        if (f) flags.fetch_or(f, std::memory_order_relaxed);
    });
    return flags.load();
}

}  // namespace

extern "C" {

int h2agg_hash_transcript_read_batch(h2agg_ctx* c, int kind, const uint8_t* proofs, size_t proof_len, size_t nproofs,
                                     const char* script, size_t script_len, const uint8_t* consts, size_t nconsts,
                                     const uint8_t* ext_points_aff, size_t next, uint8_t* points_out, uint8_t* challenges_out) try {
    TRY(bind(c));
    if (!hash_kind_ok(kind)) return fail(c, H2AGG_ERR_INVALID, "transcript kind must be H2AGG_TRANSCRIPT_KIND_SHA256 or _KECCAK256");
    if (!script) return fail(c, H2AGG_ERR_INVALID, "null script");
    TrLayout L;
    if (!parse_script_hash(script, script_len, L)) return fail(c, H2AGG_ERR_INVALID, "script: unknown operation (P S Q C X)");
    if (L.proof_len != proof_len)
        return fail(c, H2AGG_ERR_INVALID, "proof length does not match the script: 64 bytes per point, 32 per scalar (read_exact would fail: sha.rs:46,65)");
    if (L.nconsts != nconsts || L.next != next) return fail(c, H2AGG_ERR_INVALID, "script uses a different number of constants / external points");
    if (nproofs == 0) return H2AGG_OK;
    if ((proof_len && !proofs) || (nconsts && !consts) || (next && !ext_points_aff) || (L.npoints && !points_out) ||
        (!L.upto.empty() && !challenges_out))
        return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const uint8_t* d_ext = nullptr;
    if (next) {
        TRY(ensure(c, c->in_c, nproofs * next * 64));
        HIP_TRY(c, hipMemcpyAsync(c->in_c.p, ext_points_aff, nproofs * next * 64, hipMemcpyHostToDevice, c->stream));
        d_ext = (const uint8_t*)c->in_c.p;
    }
    TRY(clear_flags(c));
    const TrBlock b = transcript_block(L, nproofs);
    TRY(ensure_pinned(c, c->h_stage, b.total, "staging block"));
    TRY(hash_transcript_begin(c, L, b, nullptr, proofs, nproofs, consts, c->stream));
    if (next) hash_stream_launch(c, L, b, nproofs, d_ext, c->stream, 2);
    const bool host = hash_backend(c, nproofs) == 2;
    TRY(hash_chain_run(c, kind, L, b, nproofs, host ? challenges_out : nullptr));
    if (L.npoints)
        HIP_TRY(c, hipMemcpyAsync(points_out, c->tr_points.p, nproofs * (size_t)L.npoints * 64, hipMemcpyDeviceToHost, c->stream));
    if (!L.upto.empty() && !host)
        HIP_TRY(c, hipMemcpyAsync(challenges_out, c->tr_chal.p, nproofs * L.upto.size() * 32, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} API_CATCH

// the host backend on its own: no context, no device (CPU-testable), like h2agg_poseidon_squeeze_batch_host
int h2agg_hash_transcript_read_batch_host(int kind, const uint8_t* proofs, size_t proof_len, size_t nproofs, const char* script,
                                          size_t script_len, const uint8_t* consts, size_t nconsts, const uint8_t* ext_points_aff,
                                          size_t next, uint8_t* points_out, uint8_t* challenges_out, int max_threads) try {
    if (!hash_kind_ok(kind) || !script) return H2AGG_ERR_INVALID;
    TrLayout L;
    if (!parse_script_hash(script, script_len, L)) return H2AGG_ERR_INVALID;
    if (L.proof_len != proof_len || L.nconsts != nconsts || L.next != next) return H2AGG_ERR_INVALID;
    if (nproofs == 0) return H2AGG_OK;
    if ((proof_len && !proofs) || (nconsts && !consts) || (next && !ext_points_aff) || (L.npoints && !points_out) ||
        (!L.upto.empty() && !challenges_out))
        return H2AGG_ERR_INVALID;
    const uint32_t f = hash_transcript_host(kind, L, proofs, nproofs, consts, ext_points_aff, points_out, challenges_out,
                                            max_threads > 0 ? max_threads : 1 << 30);
    // (the order of flags_to_status)
    return (f & FLAG_NONCANONICAL) ? H2AGG_ERR_NONCANONICAL : (f & FLAG_BAD_POINT) ? H2AGG_ERR_BAD_POINT : H2AGG_OK;
} API_CATCH

int h2agg_hash_digest_host(int kind, const uint8_t* msg, size_t len, uint8_t out[32]) {
    if (!hash_kind_ok(kind) || (len && !msg) || !out) return H2AGG_ERR_INVALID;
    return hash_host::digest(kind == H2AGG_TRANSCRIPT_KIND_SHA256 ? hash_host::KIND_SHA256 : hash_host::KIND_KECCAK256, msg, len, out)
               ? H2AGG_OK : H2AGG_ERR_INVALID;
}

int h2agg_poseidon_squeeze_batch(h2agg_ctx* c, const uint8_t* elems, size_t nproofs, size_t nelem, const uint32_t* upto,
                                 size_t nsq, uint8_t* out) try {
    TRY(bind(c));
    if (nproofs == 0 || nsq == 0) return H2AGG_OK;
    if ((nelem && !elems) || !upto || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    uint32_t prev = 0;
    for (size_t q = 0; q < nsq; ++q) {
        if (upto[q] < prev || upto[q] > nelem) return fail(c, H2AGG_ERR_INVALID, "squeeze positions must be non-decreasing and <= nelem");
        prev = upto[q];
    }
    const size_t stride = 32 * (nelem ? nelem : 1);
    if (transcript_backend(c, nproofs) == 2) {   // host threads: the element streams are host memory already
        std::vector<uint8_t> pad;
        const uint8_t* e = elems;
        if (!nelem) {
            pad.assign(nproofs * stride, 0);
            e = pad.data();
        }
        if (poseidon_run_host(e, stride, upto, (uint32_t)nsq, nproofs, out))
            return flags_to_status(c, FLAG_NONCANONICAL, false);
        return H2AGG_OK;
    }
    TRY(ensure(c, c->tr_elems, nproofs * stride));
    TRY(ensure(c, c->tr_chal, nproofs * nsq * 32));
    TRY(ensure(c, c->tr_in, nsq * 4));
    if (nelem) HIP_TRY(c, hipMemcpyAsync(c->tr_elems.p, elems, nproofs * nelem * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->tr_in.p, upto, nsq * 4, hipMemcpyHostToDevice, c->stream));
    TRY(clear_flags(c));
    TRY(poseidon_run(c, (const uint8_t*)c->tr_elems.p, stride, (const uint32_t*)c->tr_in.p, (uint32_t)nsq, (uint32_t)nproofs,
                     (uint8_t*)c->tr_chal.p));
    HIP_TRY(c, hipMemcpyAsync(out, c->tr_chal.p, nproofs * nsq * 32, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
} API_CATCH

// the host twin of h2agg_poseidon_squeeze_batch: no context, no device (what the host backend runs; CPU-testable)
int h2agg_poseidon_squeeze_batch_host(const uint8_t* elems, size_t nproofs, size_t nelem, const uint32_t* upto, size_t nsq,
                                      uint8_t* out, int max_threads) try {
    if (nproofs == 0 || nsq == 0) return H2AGG_OK;
    if ((nelem && !elems) || !upto || !out) return H2AGG_ERR_INVALID;
    uint32_t prev = 0;
    for (size_t q = 0; q < nsq; ++q) {
        if (upto[q] < prev || upto[q] > nelem) return H2AGG_ERR_INVALID;
        prev = upto[q];
    }
    if (!poseidon_host_spec().ok) return H2AGG_ERR_INVALID;
    const size_t stride = 32 * (nelem ? nelem : 1);
    std::vector<uint8_t> pad;
    if (!nelem) {
        pad.assign(nproofs * stride, 0);
        elems = pad.data();
    }
    // max_threads: bits 0..15 = thread cap (0 = all usable); bit 16 set = force the portable 4 x 64-bit arithmetic, bit 17 =
    // force AVX-512 IFMA (falls back to portable if the CPU lacks it) — differential testing of the two host kernels
    const int cap = max_threads & 0xffff, kind = (max_threads & 0x10000) ? 0 : (max_threads & 0x20000) ? 1 : -1;
    return poseidon_run_host(elems, stride, upto, (uint32_t)nsq, nproofs, out, cap > 0 ? cap : 1 << 30, kind)
               ? H2AGG_ERR_NONCANONICAL : H2AGG_OK;
} API_CATCH

int h2agg_transcript_configure(h2agg_ctx* c, int backend) {
    if (!c || backend < 0 || backend > 2) return H2AGG_ERR_INVALID;
    c->cfg_transcript = backend;
    return H2AGG_OK;
}
int h2agg_host_threads(void) { return HostPool::get().size(); }
int h2agg_host_sponge_kind(void) { return host_sponge_kind(); }

int h2agg_transcript_read_batch(h2agg_ctx* c, const uint8_t* proofs, size_t proof_len, size_t nproofs, const char* script,
                                size_t script_len, const uint8_t* consts, size_t nconsts, const uint8_t* ext_points_aff,
                                size_t next, uint8_t* points_out, uint8_t* challenges_out) try {
    TRY(bind(c));
    if (!script) return fail(c, H2AGG_ERR_INVALID, "null script");
    TrLayout L;
    if (!parse_script(script, script_len, L)) return fail(c, H2AGG_ERR_INVALID, "script: unknown operation (P S Q C X)");
    if (L.proof_len != proof_len)
        return fail(c, H2AGG_ERR_INVALID, "proof length does not match the script (read_exact would fail: transcript.rs:63,101)");
    if (L.nconsts != nconsts || L.next != next) return fail(c, H2AGG_ERR_INVALID, "script uses a different number of constants / external points");
    if (nproofs == 0) return H2AGG_OK;
    if ((proof_len && !proofs) || (nconsts && !consts) || (next && !ext_points_aff) || (L.npoints && !points_out) ||
        (!L.upto.empty() && !challenges_out))
        return fail(c, H2AGG_ERR_INVALID, "null buffer");
    const uint8_t* d_ext = nullptr;
    if (next) {
        TRY(ensure(c, c->in_c, nproofs * next * 64));
        HIP_TRY(c, hipMemcpyAsync(c->in_c.p, ext_points_aff, nproofs * next * 64, hipMemcpyHostToDevice, c->stream));
        d_ext = (const uint8_t*)c->in_c.p;
    }
    TRY(clear_flags(c));
    const bool host = !L.upto.empty() && transcript_backend(c, nproofs) == 2;
    uint32_t host_flags = 0;
    TRY(transcript_run(c, L, proofs, nproofs, consts, d_ext, host ? challenges_out : nullptr, &host_flags));
    if (L.npoints)
        HIP_TRY(c, hipMemcpyAsync(points_out, c->tr_points.p, nproofs * (size_t)L.npoints * 64, hipMemcpyDeviceToHost, c->stream));
    if (!L.upto.empty() && !host)
        HIP_TRY(c, hipMemcpyAsync(challenges_out, c->tr_chal.p, nproofs * L.upto.size() * 32, hipMemcpyDeviceToHost, c->stream));
    return finish(c, host_flags);
} API_CATCH

}  // extern "C"
