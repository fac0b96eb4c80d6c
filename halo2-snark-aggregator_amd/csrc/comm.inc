// Multi-GPU exchange of the path (SURVEY.md 8(b) lines 363-365, 8(e)): the ONE collective of a sharded aggregation —
// an all-gather of every rank's partial accumulators over RCCL / xGMI, then a local fold with the group law (RCCL has no
// reduction over group elements: ncclRedOp_t is sum / prod / min / max on numeric dtypes, so BASELINE.json's "all-reduce
// of (W_x, W_e)" is an all-gather + EC adds; 96 B per point per rank, latency-bound).
//
// Stands behind the fold the reference does in one process,
//   acc = acc * lambda + proof          halo2-snark-aggregator-api/src/systems/halo2/verify.rs:926-938
// made distributive across ranks (W = sum_r W_r with the lambda powers already inside W_r), for the production caller
//   calc_verify_circuit_final_pair      halo2-snark-aggregator-circuit/src/verify_circuit.rs:114-201.
//
// RCCL is resolved at the first comm call with dlopen (the torch wheel ships its own librccl.so.1; whichever copy is
// already in the process is the one used), so the library has no load-time dependency on it.
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
};

RcclApi& rccl_state() {
    static RcclApi api;
    return api;
}
// why rccl() returned nullptr (for the caller's error string)
std::string rccl_why() {
    const std::string& e = rccl_state().err;
    return e.empty() ? std::string("RCCL is not available") : "RCCL is not available: " + e;
}

RcclApi* rccl() {
    RcclApi& api = rccl_state();
    static bool tried = false;
    if (tried) return api.lib ? &api : nullptr;
    tried = true;
    // H2AGG_RCCL_LIB = path of the RCCL build to use instead (an operator's own build; the one-GPU rehearsals of the
    // multi-rank paths point it at tests/cpp/rccl_stub.cpp, whatever librccl the process already carries)
    const char* forced = getenv("H2AGG_RCCL_LIB");
    if (forced && *forced) {
        api.lib = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
        if (!api.lib) {
            const char* e = dlerror();
            api.err = std::string("dlopen(H2AGG_RCCL_LIB): ") + (e ? e : "not found");
            return nullptr;   // (never silently another library than the one asked for)
        }
    }
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (size_t i = 0; !api.lib && i < sizeof names / sizeof *names; ++i) api.lib = dlopen(names[i], RTLD_NOW | RTLD_NOLOAD);
    for (size_t i = 0; !api.lib && i < sizeof names / sizeof *names; ++i) api.lib = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
    if (!api.lib) {
        const char* e = dlerror();   // (returns the message ONCE and clears it)
        api.err = std::string("dlopen(librccl): ") + (e ? e : "not found");
        return nullptr;
    }
    bool ok = true;
    auto sym = [&](const char* n) {
        void* p = dlsym(api.lib, n);
        if (!p) {
            ok = false;
            api.err = std::string("librccl lacks ") + n;
        }
        return p;
    };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.CommCount = (decltype(api.CommCount))sym("ncclCommCount");
    api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    if (!ok) {
        api.lib = nullptr;
        return nullptr;
    }
    return &api;
}

void comm_release(h2agg_ctx* c) {
    if (c->comm) {
        RcclApi* a = rccl();
        if (a) a->CommDestroy((ncclComm_t)c->comm);
        c->comm = nullptr;
        c->comm_size = 0;
    }
}

#define NCCL_TRY(ctx, api, expr)                                                                          \
    do {                                                                                                  \
        ncclResult_t r_ = (expr);                                                                         \
        if (r_ != ncclSuccess)                                                                            \
            return fail(ctx, H2AGG_ERR_HIP, std::string(#expr) + ": " + (api)->GetErrorString(r_));       \
    } while (0)

}  // namespace

extern "C" {

int h2agg_comm_unique_id(uint8_t out[128]) try {
    if (!out) return H2AGG_ERR_INVALID;
    RcclApi* a = rccl();
    if (!a) return H2AGG_ERR_HIP;   // (h2agg_comm_last_error() says why)
    ncclUniqueId id;
    if (a->GetUniqueId(&id) != ncclSuccess) return H2AGG_ERR_HIP;
    static_assert(sizeof id.internal == 128, "RCCL unique id is 128 bytes");
    memcpy(out, id.internal, 128);
    return H2AGG_OK;
} catch (...) {
    return H2AGG_ERR_INVALID;
}

// one process per GPU: every rank calls this with the id rank 0 obtained from h2agg_comm_unique_id and passed around by
// the host's own means (a file, MPI, torch.distributed's store, ...)
int h2agg_comm_init_rank(h2agg_ctx* c, const uint8_t id_bytes[128], int rank, int nranks) try {
    TRY(bind(c));
    if (!id_bytes || rank < 0 || nranks < 1 || rank >= nranks) return fail(c, H2AGG_ERR_INVALID, "bad rank / nranks / id");
    RcclApi* a = rccl();
    if (!a) return fail(c, H2AGG_ERR_HIP, rccl_why());
    if (c->comm) return fail(c, H2AGG_ERR_INVALID, "this context already has a communicator");
    ncclUniqueId id;
    memcpy(id.internal, id_bytes, 128);
    ncclComm_t comm = nullptr;
    NCCL_TRY(c, a, a->CommInitRank(&comm, nranks, id, rank));
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_size = nranks;
    return H2AGG_OK;
} API_CATCH

// one process driving several GPUs: a context per device plus ncclCommInitAll (SURVEY.md 8(b))
int h2agg_comm_create(const int* devices, int ndev, h2agg_ctx** ctxs_out) try {
    if (!devices || !ctxs_out || ndev < 1) return H2AGG_ERR_INVALID;
    RcclApi* a = rccl();
    if (!a) return H2AGG_ERR_HIP;
    for (int i = 0; i < ndev; ++i) ctxs_out[i] = nullptr;
    for (int i = 0; i < ndev; ++i) {
        const int rc = h2agg_create(devices[i], &ctxs_out[i]);
        if (rc != H2AGG_OK) {
            for (int j = 0; j < i; ++j) {
                h2agg_destroy(ctxs_out[j]);
                ctxs_out[j] = nullptr;
            }
            return rc;
        }
    }
    std::vector<ncclComm_t> comms(ndev);
    const ncclResult_t r = a->CommInitAll(comms.data(), ndev, devices);
    if (r != ncclSuccess) {
        ctxs_out[0]->err = std::string("ncclCommInitAll: ") + a->GetErrorString(r);
        // the contexts stay valid (and carry the message); the caller destroys them
        return H2AGG_ERR_HIP;
    }
    for (int i = 0; i < ndev; ++i) {
        ctxs_out[i]->comm = comms[i];
        ctxs_out[i]->comm_rank = i;
        ctxs_out[i]->comm_size = ndev;
    }
    return H2AGG_OK;
} API_CATCH

// why the last context-less comm call (h2agg_comm_unique_id / h2agg_comm_create before any context exists) failed
const char* h2agg_comm_last_error(void) {
    static thread_local std::string msg;
    msg = rccl_state().err;
    return msg.c_str();
}

int h2agg_comm_size(h2agg_ctx* c) { return (c && c->comm) ? c->comm_size : 0; }
int h2agg_comm_rank(h2agg_ctx* c) { return (c && c->comm) ? c->comm_rank : -1; }

// out_aff[64 * k] = to_affine( sum over all ranks of that rank's k-th partial point ), identical on every rank.
// nctx == 1: this process is ONE rank of the communicator set up by h2agg_comm_init_rank; partial_jac = its npts points.
// nctx == comm size: single-process mode (h2agg_comm_create); partial_jac = [rank][npts] points, the result of rank 0 is
// returned (all ranks compute the same).
int h2agg_allgather_add_points(h2agg_ctx** ctxs, int nctx, const uint8_t* partial_jac, size_t npts, uint8_t* out_aff) try {
    if (!ctxs || nctx < 1 || !ctxs[0]) return H2AGG_ERR_INVALID;
    h2agg_ctx* c0 = ctxs[0];
    if (!partial_jac || !out_aff || npts == 0) return fail(c0, H2AGG_ERR_INVALID, "null buffer or no points");
    RcclApi* a = rccl();
    if (!a) return fail(c0, H2AGG_ERR_HIP, rccl_why());
    for (int i = 0; i < nctx; ++i)
        if (!ctxs[i] || !ctxs[i]->comm) return fail(c0, H2AGG_ERR_INVALID, "context without a communicator");
    const int world = c0->comm_size;
    if (nctx != 1 && nctx != world) return fail(c0, H2AGG_ERR_INVALID, "pass one context (this rank) or all of the communicator's");
    const size_t bytes = 96 * npts;
    for (int i = 0; i < nctx; ++i) {
        h2agg_ctx* c = ctxs[i];
        TRY(bind(c));
        TRY(join_tails(c));
        TRY(ensure(c, c->in_a, bytes));
        TRY(ensure(c, c->in_b, bytes * world));
        TRY(ensure(c, c->out, 64 * npts));
        HIP_TRY(c, hipMemcpyAsync(c->in_a.p, partial_jac + (nctx == 1 ? 0 : bytes * i), bytes, hipMemcpyHostToDevice, c->stream));
        TRY(clear_flags(c));
    }
    // Nothing returns between GroupStart and GroupEnd, and every context is drained (finish) whatever happened: an early
    // return would leave RCCL inside an open group and the other contexts' streams unsynchronised (ADVICE r2).
    int rc_all = H2AGG_OK;
    auto note = [&](h2agg_ctx* c, int rc) {
        if (rc != H2AGG_OK && rc_all == H2AGG_OK) {
            rc_all = rc;
            if (c != c0) c0->err = c->err;
        }
    };
    auto nccl_note = [&](h2agg_ctx* c, ncclResult_t r, const char* what) {
        if (r != ncclSuccess) note(c, fail(c, H2AGG_ERR_HIP, std::string(what) + ": " + a->GetErrorString(r)));
    };
    bool grouped = false;
    if (nctx > 1) {
        const ncclResult_t r = a->GroupStart();
        nccl_note(c0, r, "ncclGroupStart");
        grouped = r == ncclSuccess;
    }
    if (rc_all == H2AGG_OK) {
        for (int i = 0; i < nctx; ++i) {
            h2agg_ctx* c = ctxs[i];
            if (nctx > 1) {
                const int rc = bind(c);
                if (rc != H2AGG_OK) {
                    note(c, rc);
                    break;
                }
            }
            const ncclResult_t r = a->AllGather(c->in_a.p, c->in_b.p, bytes, ncclUint8, (ncclComm_t)c->comm, c->stream);
            nccl_note(c, r, "ncclAllGather");
            if (r != ncclSuccess) break;
        }
    }
    if (grouped) nccl_note(c0, a->GroupEnd(), "ncclGroupEnd");
    for (int i = 0; i < nctx; ++i) {
        h2agg_ctx* c = ctxs[i];
        const int rb = bind(c);
        if (rb != H2AGG_OK) {
            note(c, rb);
            continue;
        }
        if (rc_all == H2AGG_OK) {
            // gathered layout [rank][npts]: point k of every rank is at stride npts
            hipLaunchKernelGGL(k_g1_sum_strided_affine, dim3((unsigned)npts), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_b.p,
                               (size_t)world, npts, (uint8_t*)c->out.p, c->d_flags);
            if (i == 0 && hipMemcpyAsync(out_aff, c->out.p, 64 * npts, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                note(c, fail(c, H2AGG_ERR_HIP, "hipMemcpyAsync of the folded points failed"));
        }
        const std::string keep = c->err;   // finish() of a healthy stream must not wipe the first error's message
        const int rc = finish(c);
        if (rc != H2AGG_OK) note(c, rc);
        else if (rc_all != H2AGG_OK) c->err = keep;
    }
    if (rc_all != H2AGG_OK && ctxs[0]->err.empty()) ctxs[0]->err = "a rank reported an error";
    return rc_all;
} API_CATCH

}  // extern "C"
