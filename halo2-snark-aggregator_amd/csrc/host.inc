// The host layer every C-ABI entry point stands on (included into h2agg.hip ahead of msm_run.inc and of every family: shares the
// context internals): the growing-buffer rules and the exact-size allocation over the owners of csrc/hip_owners.hpp, the launch
// grid of the element-wise kernels, the binding of a call to its context, the look-up of a base table, the staging of a host
// twin, the phase clock of the debug key phases, and the catch blocks behind every extern "C" function.
// A new family of entry points starts from here (the Fr families: from fr_host.inc on top of it).

namespace {

int flush_deferred_tail(h2agg_ctx* c, bool behind_sort);   // csrc/msm_run.inc
int join_tails(h2agg_ctx* c);                               // csrc/msm_run.inc

// A failed allocation also leaves HIP's last-error slot set, which the hipGetLastError() behind the next launches would report
// as that call's failure: taken out there, so that the context stays usable after H2AGG_ERR_NOMEM.
int ensure(h2agg_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return H2AGG_OK;
    if (b.p) {
        // a grow-only buffer is replaced: nothing queued on ANY stream of the device may still refer to the old one
        // (nor anything not yet queued: a deferred tail goes out first)
        TRY(flush_deferred_tail(c, false));
        HIP_TRY(c, hipDeviceSynchronize());
        HIP_TRY(c, hipFree(b.p));
    }
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, H2AGG_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    b.cap = want;
    return H2AGG_OK;
}

// the same for a page-locked host block: the caller has joined whatever copied through the old one
int ensure_pinned(h2agg_ctx* c, PinnedBuf& b, size_t bytes, const char* what) {
    if (bytes <= b.cap) return H2AGG_OK;
    if (b.p) HIP_TRY(c, hipHostFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    const hipError_t e = hipHostMalloc((void**)&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, H2AGG_ERR_NOMEM, std::string("hipHostMalloc(") + what + "): " + hipGetErrorString(e));
    }
    b.cap = want;
    return H2AGG_OK;
}

// an allocation of exactly `bytes` (a base table's column, the work memory of one call)
int dev_alloc(h2agg_ctx* c, DevMem& m, size_t bytes, const char* what) {
    if (m.alloc(bytes) != hipSuccess) return fail(c, H2AGG_ERR_NOMEM, std::string("hipMalloc(") + what + ")");
    return H2AGG_OK;
}

// The most workgroups of a grid-stride launch whose cap goes by the device: per_cu for each compute unit (debug key launch_cus:
// that many units instead, so that a test's few thousand elements walk the stride loop several times).  The key sizes grids
// and nothing else: routes, plans and stream placement never see it (tests/test_launch_geometry_host.py: cu_count is read
// here and by h2agg_describe only).
size_t launch_cap(const h2agg_ctx* c, unsigned per_cu) {
    return (size_t)(c->dbg_launch_cus ? c->dbg_launch_cus : c->cu_count) * per_cu;
}

int grid_for(const h2agg_ctx* c, size_t n) {
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    size_t cap = launch_cap(c, 8);
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// Called from each entry point's own body: the return address is the crash breadcrumb of the call.
int bind(h2agg_ctx* c) {
    crumb((uintptr_t)__builtin_return_address(0), 0);
    if (!c) return H2AGG_ERR_INVALID;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, H2AGG_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return H2AGG_OK;
}

int find_table(h2agg_ctx* c, uint64_t handle, Table** out) {
    auto it = c->tables.find(handle);
    if (it == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown base-table handle");
    *out = &it->second;
    return H2AGG_OK;
}

// A host twin of a _device entry point: ensure its staging buffers, stage_in the arguments, clear_flags, queue what the
// _device call queues, stage_out.
//   in: `bytes` of `src` to offset `at` of `b`
int stage_in(h2agg_ctx* c, DevBuf& b, const uint8_t* src, size_t bytes, size_t at = 0) {
    if (bytes) HIP_TRY(c, hipMemcpyAsync((uint8_t*)b.p + at, src, bytes, hipMemcpyHostToDevice, c->stream));
    return H2AGG_OK;
}
//   in, to device memory that is no grow-only buffer (a column store's slab)
int stage_in(h2agg_ctx* c, uint8_t* d_dst, const uint8_t* src, size_t bytes) {
    if (bytes) HIP_TRY(c, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return H2AGG_OK;
}
//   out, the tail of the call: `bytes` at d_src back to the host, then finish() synchronises and reports the flags
int stage_out(h2agg_ctx* c, uint8_t* dst, const void* d_src, size_t bytes) {
    HIP_TRY(c, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    return finish(c);
}

int set_identity_jac(uint8_t out[96]) {
    memset(out, 0, 96);
    out[32] = 1;
    return 0;
}

// the tail of a call whose result is one Jacobian point at d_res_jac
int fetch_result_jac(h2agg_ctx* c, uint8_t out[96]) {
    TRY(join_tails(c));
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned, c->d_res_jac, 96, hipMemcpyDeviceToHost, c->stream));
    TRY(finish(c));
    memcpy(out, c->h_pinned, 96);
    return H2AGG_OK;
}

// Debug key phases: the split of one call by events on the context's stream, for h2agg_last_phases.  mark(i): phase i starts
// here, the phase before it ends; mark(END) behind the last one.  A phase may be entered several times: its laps add up.  A
// failed create or record switches the clock off for the rest of the call.  Without the key nothing is recorded and the line
// of the last keyed call stays.
struct PhaseClock {
    enum { END = -1 };
    h2agg_ctx* c;
    const bool want;
    bool on;
    std::vector<std::pair<int, Event>> marks;
    explicit PhaseClock(h2agg_ctx* c_) : c(c_), want(c_->dbg_phases != 0), on(want) {}
    void mark(int phase) {
        if (!on) return;
        Event e;
        if (e.create(hipEventDefault) != hipSuccess || hipEventRecord(e, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            on = false;
            return;
        }
        marks.emplace_back(phase, std::move(e));
    }
    // waits for the last event; c->last_phases = " name=%.4f" for each of the `count` phases, or with only_entered for those
    // among them that were entered and left
    void report(const char* const* names, int count, bool only_entered = false) {
        if (!want) return;
        c->last_phases.clear();
        if (!on || marks.empty() || hipEventSynchronize(marks.back().second) != hipSuccess) return;
        std::vector<double> ms((size_t)count, 0.0);
        std::vector<bool> entered((size_t)count, false);
        for (size_t i = 0; i + 1 < marks.size(); ++i) {
            float t = 0;
            if (hipEventElapsedTime(&t, marks[i].second, marks[i + 1].second) != hipSuccess) return;
            ms[(size_t)marks[i].first] += t;
            entered[(size_t)marks[i].first] = true;
        }
        for (int i = 0; i < count; ++i) {
            if (only_entered && !entered[(size_t)i]) continue;
            char buf[48];
            snprintf(buf, sizeof buf, " %s=%.4f", names[i], ms[(size_t)i]);
            c->last_phases += buf;
        }
    }
};

}  // namespace

// behind the body of every extern "C" function: `int h2agg_...(...) try { ... } API_CATCH`
#define API_CATCH                                                                                      \
    catch (const std::bad_alloc&) { return H2AGG_ERR_NOMEM; /* no C++ exception crosses the C ABI */ } \
    catch (...) { return H2AGG_ERR_INVALID; }
