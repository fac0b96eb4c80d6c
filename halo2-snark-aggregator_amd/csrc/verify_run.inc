// One aggregation call on the GPU backend (included into h2agg.hip after verifier.inc, which has the verifying key, the
// recording helpers, build_queries and the plan types).  DESIGN.md sections 5.4, 5.6 and 6.
//
//     AggCall         what the caller asked for: the four extern "C" entries at the end of this file fill one
//     ShardExchange   the two all-gathers of a sharded call and the rule that a failing rank still enters them
//     AggState        what one call owns on the host, in the order its lifetimes need
//     SpongeRun       the hand-over of the proofs' sponge chains to the host pool: post() ... join()
//     agg_*           the stages; verify_aggregation_impl is their sequence
//
// Who takes which way is decided by four facts, fixed before the first launch: call.each (per-proof mode: no fold), call.shard,
// st.host_sponge (host threads or the device run the sponges) and, per circuit, CircuitHost::hashed (a ShaRead circuit).

namespace {

// advice_out (optional): the advice commitments of every proof, in aggregation order, num_advice_columns x 64 B each
// (canonical affine) — the fourth return value of verify_aggregation_proofs_in_chip (`commits`, verify.rs:852-856,927-939),
// which the production caller feeds to `coherent` (halo2-snark-aggregator-circuit/src/verify_circuit.rs:487-492).
// advice_cap: bytes available; too small -> H2AGG_ERR_INVALID before any work.
// each (h2agg_verify_proofs): no aggregation challenge and no fold — every proof's own (left, right) to each_pairs (128 B per
// proof of this call, in its order), a proof whose W count does not fit its rotation groups gets H2AGG_ERR_INVALID in
// each_status and is left out; left_aff / right_aff are only zeroed, lambda_out, s_g2 are not used.  The recording is never cached.
struct AggCall {
    const h2agg_circuit_proofs* circuits = nullptr;
    size_t ncircuits = 0;
    const h2agg_shard* shard = nullptr;   // null: the whole aggregation is this call's
    const uint8_t* s_g2 = nullptr;        // with g2 and pairing_ok, or none of the three
    const uint8_t* g2 = nullptr;
    uint8_t* left_aff = nullptr;
    uint8_t* right_aff = nullptr;
    uint8_t* lambda_out = nullptr;        // optional
    int* pairing_ok = nullptr;
    uint8_t* advice_out = nullptr;        // optional
    size_t advice_cap = 0;
    bool each = false;                    // per-proof mode
    uint8_t* each_pairs = nullptr;
    int32_t* each_status = nullptr;
};

// ---- the exchanges of a sharded aggregation ------------------------------------------------------------------------------
// Both exchanges carry a STATUS word per rank (0 = fine, else the H2AGG_ERR_* code of a failure local to that rank: a proof that
// does not decode, a non-canonical scalar, no memory ...).  A rank that fails between the validation of its shard description
// and an exchange still enters that exchange, with its code in the word; every rank then leaves the call at the same point —
// the failing one with its own error, the others with H2AGG_ERR_PEER — instead of waiting forever in an all-gather one rank
// never joins (ADVICE r4).
//
// Two invariants:
//   POINT OF COMMITMENT.  Constructing a ShardExchange commits a shard to both exchanges (include/h2agg.h).  Only the
//   argument checks and the checks of the shard description (agg_check_call, agg_check_shard) come before it: those every rank
//   fails alike.  Whatever fails after it — a circuit's argument checks, a TRY of any stage, a std::bad_alloc — must end in
//   leave(rc); a check moved ahead of the construction leaves the peers waiting in an all-gather.
//   SHARD_FAIL POSITIONS.  allgather() counts the call's gathers in dbg_shard_calls (zeroed at the point of commitment) and the
//   debug key shard_fail injects a failure of THIS rank at 1: before lambda(), 2: between lambda() and sum_pair() (both in
//   the stages), 3 / 4: inside exchange 1 / 2 BEFORE its all-gather (here).  Tests pin all four relative to the gathers.
//
// ex1 / ex2: that exchange's all-gather has RETURNED on this rank — from there on every rank has seen the same bytes, so a
// failure is one every rank has alike; before it (no memory for the buffers, a transport error: ADVICE r5) the failure is this
// rank's alone and the others still wait for it.  `global` marks a failure raised inside an exchange AFTER its all-gather (a
// peer's status, positions claimed twice, a non-canonical squeeze): every rank leaves at the same point and leave() adds nothing.
struct ShardExchange {
    h2agg_ctx* const c;
    const h2agg_shard* const sh;   // null: not a sharded call, leave() hands rc through
    const size_t N_all;
    bool ex1 = false, ex2 = false, global = false;

    ShardExchange(h2agg_ctx* c_, const h2agg_shard* sh_, size_t N_all_) : c(c_), sh(sh_), N_all(N_all_) { c->dbg_shard_calls = 0; }

    // Exchange 1: every rank's last squeezes -> the same lambda on every rank
    int lambda(const uint8_t* local_sq, size_t nlocal, uint8_t lam[32]) {
        uint32_t fl = 0;
        const int rc = gather_lambda(local_sq, nlocal, lam, fl, 0);
        global = ex1;   // (whatever follows the gather is the same on every rank)
        if (rc != H2AGG_OK) return rc;
        if (fl) return fail(c, H2AGG_ERR_NONCANONICAL, "a proof's squeeze is not a canonical scalar");
        global = false;
        return H2AGG_OK;
    }
    // Exchange 2: every rank's partial pair, summed on every rank
    int sum_pair(uint8_t left_aff[64], uint8_t right_aff[64]) {
        const int rc = gather_sum_pair(left_aff, right_aff, 0);
        global = ex2;
        if (rc != H2AGG_OK) return rc;
        global = false;
        return H2AGG_OK;
    }
    // The way out of a committed call: a rank that failed on its own enters the exchange it has not been through, with its
    // code in the status word; its own message is kept.
    int leave(int rc) {
        if (!sh || rc == H2AGG_OK || global || (ex1 && ex2)) return rc;
        const std::string why = c->err;   // (the exchange below must not replace this rank's own message)
        try {
            if (!ex1) {          // the others learn it in exchange 1 and leave there: no exchange 2 for anybody
                uint8_t lam0[32];
                uint32_t fl = 0;
                (void)gather_lambda(nullptr, 0, lam0, fl, (uint32_t)rc);
            } else {             // ... in exchange 2
                uint8_t l0[64] = {}, r0[64] = {};
                (void)gather_sum_pair(l0, r0, (uint32_t)rc);
            }
        } catch (...) {
        }
        c->err = why;
        return rc;
    }

private:
    // One all-gather: every rank contributes `bytes`, every rank receives [world][bytes].  Through the caller's transport
    // (shard->allgather: MPI, a torch.distributed store, sockets, ...) or, without one, through the context's RCCL
    // communicator over xGMI.
    int allgather(const uint8_t* send, size_t bytes, std::vector<uint8_t>& recv) {
        const int nth = ++c->dbg_shard_calls;   // (debug key shard_fail 3 / 4: a failure of THIS rank inside exchange 1 / 2, before the gather)
        if ((c->dbg_shard_fail == 3 && nth == 1) || (c->dbg_shard_fail == 4 && nth == 2))
            return fail(c, H2AGG_ERR_NOMEM, "injected failure inside an exchange before its all-gather (debug key shard_fail)");
        recv.assign(bytes * sh->world, 0);
        if (sh->allgather) {
            const int rc = sh->allgather(sh->user, send, bytes, recv.data());
            if (rc != 0) return fail(c, H2AGG_ERR_HIP, "the caller's all-gather reported error " + std::to_string(rc));
            return H2AGG_OK;
        }
        RcclApi* a = rccl();
        if (!a) return fail(c, H2AGG_ERR_HIP, rccl_why());
        TRY(ensure(c, c->in_a, bytes));
        TRY(ensure(c, c->in_b, bytes * sh->world));
        HIP_TRY(c, hipMemcpyAsync(c->in_a.p, send, bytes, hipMemcpyHostToDevice, c->stream));
        NCCL_TRY(c, a, a->AllGather(c->in_a.p, c->in_b.p, bytes, ncclUint8, (ncclComm_t)c->comm, c->stream));
        HIP_TRY(c, hipMemcpyAsync(recv.data(), c->in_b.p, bytes * sh->world, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return H2AGG_OK;
    }
    // the status words of a gathered block: 0 when every rank reported 0
    int peer_status(const uint8_t* recv, size_t stride, size_t off, uint32_t my_status, const char* where) {
        for (size_t r = 0; r < sh->world; ++r) {
            uint32_t st;
            memcpy(&st, recv + r * stride + off, 4);
            if (st == 0) continue;
            if (my_status) return (int)my_status;   // (the caller keeps its own message)
            return fail(c, H2AGG_ERR_PEER, "sharded aggregation: rank " + std::to_string(r) + " failed with code " + std::to_string(st) + " " + where);
        }
        return H2AGG_OK;
    }
    // Exchange 1 (verify.rs:909-913, :924): the aggregation transcript absorbs EVERY proof's last squeeze, in aggregation order,
    // before it yields lambda.  Each rank contributes its status word and {position, squeeze} records for its proofs (N_all
    // slots per rank, unused ones marked), every rank assembles the same N_all x 32 bytes and runs the same sponge: the same
    // lambda everywhere.
    int gather_lambda(const uint8_t* local_sq, size_t nlocal, uint8_t lam[32], uint32_t& flags, uint32_t my_status) {
        constexpr size_t REC = 36, HDR = 4;
        std::vector<uint8_t> send(HDR + N_all * REC, 0xff), recv;
        memcpy(send.data(), &my_status, 4);
        for (size_t i = 0; i < nlocal && !my_status; ++i) {
            const uint32_t g = sh->global_index[i];
            memcpy(send.data() + HDR + REC * i, &g, 4);
            memcpy(send.data() + HDR + REC * i + 4, local_sq + 32 * i, 32);
        }
        TRY(allgather(send.data(), send.size(), recv));
        ex1 = true;
        TRY(peer_status(recv.data(), send.size(), 0, my_status, "before the lambda exchange"));
        std::vector<uint8_t> all(N_all * 32);
        std::vector<uint8_t> seen(N_all, 0);
        for (size_t r = 0; r < sh->world; ++r)
            for (size_t i = 0; i < N_all; ++i) {
                const uint8_t* rec = recv.data() + r * send.size() + HDR + i * REC;
                uint32_t g;
                memcpy(&g, rec, 4);
                if (g == 0xffffffffu) continue;
                if (g >= N_all || seen[g]) return fail(c, H2AGG_ERR_INVALID, "sharded aggregation: two ranks claim one proof position (or a position is out of range)");
                seen[g] = 1;
                memcpy(all.data() + 32 * (size_t)g, rec + 4, 32);
            }
        for (size_t g = 0; g < N_all; ++g)
            if (!seen[g]) return fail(c, H2AGG_ERR_INVALID, "sharded aggregation: no rank holds proof " + std::to_string(g));
        const uint32_t upto = (uint32_t)N_all;
        flags |= poseidon_run_host(all.data(), 32 * N_all, &upto, 1, 1, lam, 1);
        return H2AGG_OK;
    }
    // Exchange 2 (the fold of verify.rs:926-938 made distributive): all-gather of every rank's partial (W_x, W_g) and status
    // word, summed with the group law on every rank.  The partials come from the transport: they are checked like any other
    // input of the C ABI — canonical coordinates AND on the curve (k_g1_sum_strided_affine refuses either with FLAG_BAD_POINT /
    // FLAG_NONCANONICAL) — before they enter the sum that goes to the pairing.
    int gather_sum_pair(uint8_t left_aff[64], uint8_t right_aff[64], uint32_t my_status) {
        constexpr size_t PAY = 132;
        uint8_t mine[PAY] = {};
        if (!my_status) {
            memcpy(mine, left_aff, 64);
            memcpy(mine + 64, right_aff, 64);
        }
        memcpy(mine + 128, &my_status, 4);
        std::vector<uint8_t> recv;
        TRY(allgather(mine, PAY, recv));
        ex2 = true;
        TRY(peer_status(recv.data(), PAY, 128, my_status, "between the two exchanges"));
        std::vector<uint8_t> jac(96 * 2 * (size_t)sh->world, 0);   // [rank][2] canonical Jacobian: (x, y, 1), identity (0, 1, 0)
        for (size_t k = 0; k < 2 * (size_t)sh->world; ++k) {
            const uint8_t* a = recv.data() + PAY * (k / 2) + 64 * (k & 1);
            bool zero = true;
            for (int b = 0; b < 64 && zero; ++b) zero = a[b] == 0;
            uint8_t* j = jac.data() + 96 * k;
            if (zero) j[32] = 1;
            else {
                memcpy(j, a, 64);
                j[64] = 1;
            }
        }
        TRY(ensure(c, c->in_b, jac.size()));
        TRY(ensure(c, c->out, 128));
        TRY(clear_flags(c));
        HIP_TRY(c, hipMemcpyAsync(c->in_b.p, jac.data(), jac.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_g1_sum_strided_affine, dim3(2), dim3(BLOCK), 0, c->stream, (const uint8_t*)c->in_b.p, (size_t)sh->world, (size_t)2,
                           (uint8_t*)c->out.p, c->d_flags);
        HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 1024, c->out.p, 128, hipMemcpyDeviceToHost, c->stream));
        TRY(finish(c));   // (a partial that is not a canonical point of the curve surfaces here)
        memcpy(left_aff, c->h_pinned + 1024, 64);
        memcpy(right_aff, c->h_pinned + 1024 + 64, 64);
        return H2AGG_OK;
    }
};

// ---- what one call owns on the host ----------------------------------------------------------------------------------------
struct CircuitHost {
    std::vector<uint8_t> points, chal, inst_aff;   // downloaded
    std::vector<uint8_t> elems;                    // host sponge: the proofs' element streams
    const uint8_t* elems_p = nullptr;              // ... where they are (the vector, or the context's page-locked block)
    TrLayout L;                                    // the script's layout (L.upto: the squeeze positions)
    TrBlock tb{};                                  // where the pieces of the transcript batch sit in the staging block
    size_t npoints = 0, nsq = 0, n_w = 0, elem_stride = 0, first_proof = 0;
    size_t total_vals = 0;                         // instance values of all proofs and columns
    bool hashed = false;                           // a ShaRead circuit: its challenges are in `chal` when its turn ends
    std::string script;
};
// byte offset of proof i's last squeeze in a circuit's challenges ([nproofs][nsq][32], on the host or in c->tr_chal)
size_t last_squeeze(const CircuitHost& h, size_t i) { return 32 * (h.nsq * i + h.nsq - 1); }

struct TraceScope {   // the call whose phases trace_mark() stamps from the layers below
    explicit TraceScope(PhaseTrace* t) { g_trace = t; }
    ~TraceScope() { g_trace = nullptr; }
};
struct SchemaGuard {   // a schema recorded by this call and not (yet) handed to the context's plan cache
    h2agg_schema* s = nullptr;
    ~SchemaGuard() { if (s) h2agg_schema_destroy(s); }
};

// The hand-over of the Poseidon chains to the host pool.  post(): one job per proof of every Poseidon circuit goes to the
// workers, which run while the posting thread records the schema their challenges will feed; join(): the posting thread takes
// whatever chains are left and waits for the rest.  The workers hold raw pointers to the circuits' host data, to this object
// and to the trace: all three must outlive the run, so the destructor joins — an early return between post() and join() ends
// the run before anything it reads goes away.
struct SpongeRun {
    std::vector<std::pair<size_t, size_t>> jobs;   // job -> (circuit, proof)
    std::atomic<uint32_t> bad{0};                  // FLAG_NONCANONICAL once a chain met a scalar >= r
    HostPool::Run* run = nullptr;                  // open between post() and join()

    static bool chain(CircuitHost& h, size_t i, const poseidon_host::FastSpec* fs, const void* ic_any) {
        const uint8_t* el = h.elems_p + i * h.elem_stride;
        uint8_t* out = h.chal.data() + 32 * h.nsq * i;
#ifdef H2AGG_HAVE_IFMA_BUILD
        if (ic_any) return poseidon_host::ifma::sponge_run(*(const poseidon_host::ifma::Consts*)ic_any, el, h.L.upto.data(), (uint32_t)h.nsq, out);
#endif
        (void)ic_any;
        return poseidon_host::sponge_run(*fs, el, h.L.upto.data(), (uint32_t)h.nsq, out);
    }
    void post(const AggCall& call, std::vector<CircuitHost>& H, PhaseTrace& trace) {
        for (size_t ci = 0; ci < call.ncircuits; ++ci)
            for (size_t i = 0; i < call.circuits[ci].nproofs && !H[ci].hashed; ++i) jobs.push_back({ci, i});
        const poseidon_host::FastSpec* fs = &poseidon_fast_spec();
        const void* ic_any = nullptr;   // (captured by VALUE: the workers run after post() is left)
#ifdef H2AGG_HAVE_IFMA_BUILD
        if (host_sponge_kind() == 1 && poseidon_host::ifma::cpu_has_ifma() && poseidon_ifma_consts().ok) ic_any = &poseidon_ifma_consts();
#endif
        if (trace.on) {
            trace.jobs.resize(jobs.size());
            trace.posted_us = trace.since_call_us();
        }
        PhaseTrace* tr = trace.on ? &trace : nullptr;
        CircuitHost* Hp = H.data();
        HostPool& pool = HostPool::get();
        run = pool.begin(jobs.size(), pool.size(), [this, Hp, fs, ic_any, tr](size_t j) {
            struct Stamp {
                PhaseTrace* t;
                size_t j;
                float t_in;
                Stamp(PhaseTrace* t_, size_t j_) : t(t_), j(j_), t_in(t_ ? t_->since_call_us() : 0) {}
                ~Stamp() {
                    if (t) t->jobs[j] = {t_in, t->since_call_us() - t_in, sched_getcpu()};
                }
            } stamp(tr, j);
            if (!chain(Hp[jobs[j].first], jobs[j].second, fs, ic_any)) bad.fetch_or(FLAG_NONCANONICAL, std::memory_order_relaxed);
        });
    }
    void join() {
        if (!run) return;
        HostPool::Run* r = run;
        run = nullptr;
        HostPool::get().end(r);   // this thread takes whatever chains are left, then waits for the rest
    }
    SpongeRun() = default;
    ~SpongeRun() { join(); }
    SpongeRun(const SpongeRun&) = delete;
    SpongeRun& operator=(const SpongeRun&) = delete;
};

// Everything a call keeps between its stages.  LIFETIMES are the declaration order (members go in reverse): `trace` is the
// caller's and outlives the state; `sponges` is declared LAST, so its destructor ends an open run before H, or anything else
// its workers read, is destroyed; `guard` destroys a schema `fresh` refers to, never one the cache has taken (agg_plan_keep).
struct AggState {
    PhaseTrace& trace;                // the call's phase clock; the sponge workers stamp their jobs in it
    size_t total_proofs = 0;          // the proofs THIS call holds (a shard: this rank's)
    size_t N_all = 0;                 // the length of the whole aggregation (no shard: total_proofs)
    bool host_sponge = false;         // host threads run the Poseidon chains (csrc/transcript.inc transcript_backend)
    bool cache_on = false;            // this call may use and feed the plan cache
    size_t last_ci = 0;               // the last circuit that has proofs (ncircuits: none)
    size_t proof_base = 0;            // proofs of the circuits before the one whose turn it is
    size_t advice_off = 0;            // bytes of advice_out written
    std::vector<CircuitHost> H;       // per circuit: layout, downloads, challenges
    std::vector<uint8_t> agg_host;    // every proof's last squeeze, on the host (host sponges, or a shard's exchange 1)
    uint32_t host_flags = 0;          // FLAG_* raised by host sponges, handed to finish()
    struct {
        bool on = false;
        size_t ci = 0, off_points = 0, off_inst = 0;
    } late;                           // split download: circuit `ci`'s points / instance commitments are still on their way
                                      // into c->h_down at these offsets (valid until the next call grows the block)
    uint8_t lambda[32] = {0};         // the aggregation challenge
    std::string sig;                  // the call's shape (agg_signature)
    AggPlan fresh;                    // the recording of this call, when no kept one fits
    AggPlan* plan = nullptr;          // the recording the call runs: a kept one, or &fresh
    h2agg_schema* sc = nullptr;       // ... its schema
    std::vector<std::pair<uint32_t, uint32_t>> roots;   // recorded afresh: (w_x, w_g) of every proof that has them, in order ...
    std::vector<size_t> each_idx;     // ... and (per-proof mode) its place in the call
    SchemaGuard guard;                // owns fresh's schema until the cache takes it
    SpongeRun sponges;                // the chains on the host pool; LAST: its workers read H, trace and itself
    explicit AggState(PhaseTrace& t) : trace(t) {}
};

// ---- the checks ---------------------------------------------------------------------------------------------------------------
int agg_check_call(h2agg_ctx* c, const AggCall& call) {
    if (!call.circuits || call.ncircuits == 0 || !call.left_aff || !call.right_aff) return fail(c, H2AGG_ERR_INVALID, "null argument");
    if ((call.s_g2 == nullptr) != (call.g2 == nullptr) || (call.s_g2 && !call.pairing_ok))
        return fail(c, H2AGG_ERR_INVALID, "pass s_g2, g2 and pairing_ok together (or none)");
    if (call.pairing_ok) *call.pairing_ok = 0;
    memset(call.left_aff, 0, 64);
    memset(call.right_aff, 0, 64);
    if (call.shard)   // before the point of commitment: no exchange is entered (include/h2agg.h: out of scope for now)
        for (size_t ci = 0; ci < call.ncircuits; ++ci)
            if (call.circuits[ci].vk && call.circuits[ci].vk->multiopen_kind != H2AGG_MULTIOPEN_GWC)
                return fail(c, H2AGG_ERR_INVALID, "the sharded aggregation does not take Shplonk keys yet: aggregate them with h2agg_verify_aggregation(_ex)");
    if (!call.each)   // the reference never folds ShaRead proofs under an aggregation transcript (include/h2agg.h)
        for (size_t ci = 0; ci < call.ncircuits; ++ci)
            if (call.circuits[ci].vk && call.circuits[ci].vk->transcript_kind != H2AGG_TRANSCRIPT_KIND_POSEIDON)
                return fail(c, H2AGG_ERR_INVALID, "aggregation of proofs written with the SHA-256 / Keccak-256 transcript is not supported: verify them with h2agg_verify_proofs");
    return H2AGG_OK;
}
// Sharded aggregation (SURVEY.md 8(e)): the proofs are spread over `world` ranks, this call holds those whose positions in the
// aggregation order are shard->global_index[]; N_all = the length of the whole aggregation.  The last checks before the point
// of commitment (ShardExchange).
int agg_check_shard(h2agg_ctx* c, const AggCall& call, AggState& st) {
    const h2agg_shard* shard = call.shard;
    for (size_t ci = 0; ci < call.ncircuits; ++ci) st.total_proofs += call.circuits[ci].nproofs;
    st.N_all = shard ? shard->total_proofs : st.total_proofs;
    if (st.N_all == 0) return fail(c, H2AGG_ERR_INVALID, "no proofs (the reference unwraps an empty fold: verify.rs:940)");
    if (!shard) return H2AGG_OK;
    if (shard->world < 1 || shard->rank >= shard->world || st.total_proofs > st.N_all || (st.total_proofs && !shard->global_index))
        return fail(c, H2AGG_ERR_INVALID, "bad shard description");
    if (!shard->allgather && (!c->comm || c->comm_size != (int)shard->world || c->comm_rank != (int)shard->rank))
        return fail(c, H2AGG_ERR_INVALID, "sharded aggregation without an exchange: pass shard->allgather or give the context an RCCL communicator of that rank / world (h2agg_comm_init_rank)");
    for (size_t i = 0; i < st.total_proofs; ++i) {
        if (shard->global_index[i] >= st.N_all) return fail(c, H2AGG_ERR_INVALID, "global_index out of range");
        for (size_t j = 0; j < i; ++j)
            if (shard->global_index[j] == shard->global_index[i]) return fail(c, H2AGG_ERR_INVALID, "global_index repeats");
    }
    return H2AGG_OK;
}

// What a proof's shape alone decides (verify.rs:487-490, :601-603): null, or why the reference refuses it.
// lens: the proof's instance column lengths; len_fits: proof_len_fits() of its transcript.
const char* proof_shape_fault(const h2agg_vk& vk, size_t table_n, bool len_fits, const uint32_t* lens) {
    if (!len_fits) return "proof too short for this verifying key (read_exact fails: transcript.rs:63,101; sha.rs:46,65)";
    const uint64_t max_len = ((uint64_t)1 << vk.k) - (vk.blinding_factors + 1);
    for (size_t col = 0; col < vk.num_instance; ++col) {
        if (lens[col] > max_len) return "assert!(instance.len() <= params.n() - (blinding_factors + 1)) failed (verify.rs:601-603)";
        if (lens[col] > table_n) return "instance column longer than the g_lagrange table";
    }
    return nullptr;
}
// One circuit's argument checks: no HIP call, no allocation on the device.  Null pointers and unknown handles refuse the call.
// What a proof's shape decides refuses the call as well when it is an aggregation (each_status null) — all of a circuit's
// proofs must then have one length, and its layout goes to *h; per-proof mode (h2agg_verify_proofs) takes a status per proof
// instead, appended to *each_status (H2AGG_OK or H2AGG_ERR_INVALID), and leaves the layout to the groups of one length.
int agg_check_circuit(h2agg_ctx* c, const h2agg_circuit_proofs& cp, std::vector<int32_t>* each_status, CircuitHost* h) {
    if (!cp.vk || cp.vk->ctx != c || !cp.name) return fail(c, H2AGG_ERR_INVALID, "circuit without a verifying key / name");
    const h2agg_vk& vk = *cp.vk;
    if (cp.nproofs == 0) return H2AGG_OK;
    if (!cp.transcripts || !cp.transcript_lens || (vk.num_instance && (!cp.instances || !cp.instance_lens)))
        return fail(c, H2AGG_ERR_INVALID, "null proof data");
    const auto tit = c->tables.find(cp.g_lagrange);
    if (vk.num_instance && tit == c->tables.end()) return fail(c, H2AGG_ERR_INVALID, "unknown g_lagrange handle");
    const size_t ncol = vk.num_instance, table_n = ncol ? tit->second.n : 0;
    // ---- proof layout: all proofs of a circuit have the same length; the W points are whatever is left (verify.rs:487-490)
    size_t n_w = 0;
    bool fits = false;
    if (!each_status) {
        for (size_t i = 0; i < cp.nproofs; ++i)
            if (cp.transcript_lens[i] != cp.transcript_lens[0] || !cp.transcripts[i])
                return fail(c, H2AGG_ERR_INVALID, "proofs of one circuit must have one length");
        fits = proof_len_fits(vk, cp.transcript_lens[0], &n_w);
    }
    for (size_t i = 0; i < cp.nproofs; ++i) {
        if (each_status) fits = proof_len_fits(vk, cp.transcript_lens[i], nullptr);
        const char* fault = proof_shape_fault(vk, table_n, fits, ncol ? cp.instance_lens + i * ncol : nullptr);
        if (fault && !each_status) return fail(c, H2AGG_ERR_INVALID, fault);
        if (each_status) each_status->push_back(fault ? H2AGG_ERR_INVALID : H2AGG_OK);
    }
    size_t total_vals = 0;
    for (size_t i = 0; i < cp.nproofs; ++i) {
        if (!cp.transcripts[i]) return fail(c, H2AGG_ERR_INVALID, "null proof data");
        size_t pl = 0;
        for (size_t col = 0; col < ncol; ++col) pl += cp.instance_lens[i * ncol + col];
        if (pl && !cp.instances[i]) return fail(c, H2AGG_ERR_INVALID, "null instance data");
        total_vals += pl;
    }
    if (!h) return H2AGG_OK;
    h->n_w = n_w;
    h->total_vals = total_vals;
    h->hashed = vk.transcript_kind != H2AGG_TRANSCRIPT_KIND_POSEIDON;
    h->script = proof_script(vk, h->n_w);
    if (h->hashed) parse_script_hash(h->script.data(), h->script.size(), h->L);
    else parse_script(h->script.data(), h->script.size(), h->L);
    h->tb = transcript_block(h->L, cp.nproofs);
    h->npoints = h->L.npoints;
    h->nsq = h->L.upto.size();
    h->elem_stride = h->tb.elem_stride;
    return H2AGG_OK;
}

// ---- the stages -------------------------------------------------------------------------------------------------------------
// before the first circuit: the advice_out bound, the sponge backend, the buffers every circuit shares
int agg_begin(const AggCall& call, h2agg_ctx* c, AggState& st) {
    if (call.advice_out) {
        size_t need = 0;
        for (size_t ci = 0; ci < call.ncircuits; ++ci)
            if (call.circuits[ci].vk) need += call.circuits[ci].nproofs * (size_t)call.circuits[ci].vk->num_advice * 64;
        if (need > call.advice_cap) return fail(c, H2AGG_ERR_INVALID, "advice_out is too small for the proofs' advice commitments");
    }
    // sponge backend for this call (csrc/transcript.inc): host threads for small batches, the device sponge for large ones
    st.host_sponge = transcript_backend(c, st.total_proofs) == 2;
    if (st.host_sponge && c->dbg_prewake) HostPool::get().prewake(st.total_proofs);   // the chains are posted ~0.3 ms from here
    if (st.host_sponge) st.agg_host.resize(st.total_proofs * 32);
    // per-proof squeezes of every circuit, absorbed by the aggregation transcript (verify.rs:909-913, :924)
    TRY(ensure(c, c->agg_elems, st.total_proofs * 32 + 64));
    st.H.resize(call.ncircuits);
    TRY(clear_flags(c));
    st.last_ci = call.ncircuits;
    for (size_t ci = 0; ci < call.ncircuits; ++ci)
        if (call.circuits[ci].nproofs) st.last_ci = ci;
    return H2AGG_OK;
}

// the instance columns' MSMs against g_lagrange: inst_vals (device, proof-major) -> inst_jac
int agg_instance_msms(h2agg_ctx* c, const h2agg_circuit_proofs& cp, size_t ncol) {
    bool uniform = cp.nproofs * ncol > 1 && cp.instance_lens[0] > 0;
    for (size_t i = 1; uniform && i < cp.nproofs * ncol; ++i) uniform = cp.instance_lens[i] == cp.instance_lens[0];
    if (uniform)   // [batch][n] scalars over one table: ONE set of launches (h2agg_g1_msm_device_batch_async)
        return h2agg_g1_msm_device_batch_async(c, cp.g_lagrange, c->inst_vals.p, cp.instance_lens[0], cp.nproofs * ncol, c->inst_jac.p);
    size_t off = 0;
    for (size_t i = 0; i < cp.nproofs * ncol; ++i) {
        uint8_t* dst = (uint8_t*)c->inst_jac.p + 96 * i;
        const size_t len = cp.instance_lens[i];
        if (len == 0) {                                               // None => assign_const(identity)  (:638)
            uint8_t idj[96];
            set_identity_jac(idj);
            HIP_TRY(c, hipMemcpyAsync(dst, idj, 96, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        } else {
            TRY(h2agg_g1_msm_device_async(c, cp.g_lagrange, (const uint8_t*)c->inst_vals.p + 32 * off, len, dst));
        }
        off += len;
    }
    return H2AGG_OK;
}

// assign_instance_commitment (verify.rs:574-649) for circuit ci: one MSM per (proof, instance column) against g_lagrange, with
// the early half of the circuit's transcripts started beside them on the auxiliary stream
int agg_instance_commitments(const AggCall& call, h2agg_ctx* c, AggState& st, size_t ci) {
    const h2agg_circuit_proofs& cp = call.circuits[ci];
    const h2agg_vk& vk = *cp.vk;
    const CircuitHost& h = st.H[ci];
    PhaseTrace& trace = st.trace;
    const size_t ncol = vk.num_instance;
    TRY(ensure(c, c->inst_jac, (cp.nproofs * ncol + 1) * 96));
    TRY(ensure(c, c->inst_aff, (cp.nproofs * ncol + 1) * 64));
    // ONE page-locked staging block for this circuit: [transcript layout + proof bytes | instance values].  The transcript
    // half goes up on the auxiliary stream, where point decompression (a 254-step square root per point, ~0.17 ms of pure
    // latency) and everything else that depends on the proof bytes only run BESIDE the instance-column MSMs; only the
    // instance commitments' own two elements per proof wait for those (k_transcript_elements `which` = 1 / 2).
    const size_t inst_off = (h.tb.total + 255) & ~(size_t)255;
    TRY(ensure_pinned(c, c->h_stage, inst_off + h.total_vals * 32 + 32, "staging block"));
    trace.mark("entry");
    HIP_TRY(c, hipEventRecord(c->ev_aux_go, c->stream));                 // (the previous users of tr_* are behind us)
    HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_aux_go, 0));
    chaos_wait(8, c->aux_stream);
    if (h.hashed) TRY(hash_transcript_begin(c, h.L, h.tb, cp.transcripts, nullptr, cp.nproofs, vk.vk_scalar, c->aux_stream));
    else TRY(transcript_begin(c, h.L, h.tb, cp.transcripts, cp.nproofs, vk.vk_scalar, c->aux_stream, 0));
    HIP_TRY(c, hipEventRecord(c->ev_aux, c->aux_stream));
    trace.mark("tr_begin");
    if (ncol) {
        TRY(ensure(c, c->inst_vals, h.total_vals * 32 + 32));
        size_t off = 0;
        uint8_t* hs = c->h_stage + inst_off;
        for (size_t i = 0; i < cp.nproofs; ++i) {
            size_t pl = 0;
            for (size_t col = 0; col < ncol; ++col) pl += cp.instance_lens[i * ncol + col];
            if (pl) memcpy(hs + 32 * off, cp.instances[i], 32 * pl);
            off += pl;
        }
        HIP_TRY(c, hipMemcpyAsync(c->inst_vals.p, hs, 32 * h.total_vals, hipMemcpyHostToDevice, c->stream));   // one copy
        if (trace.on) {
            trace.mark("inst_h2d_call");
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            trace.mark("inst_upload");
        }
        TRY(agg_instance_msms(c, cp, ncol));
        TRY(join_tails(c));
        if (trace.on) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            trace.mark("inst_msm_join");
        }
        hipLaunchKernelGGL(k_g1_batch_to_affine, dim3(grid_for(c, cp.nproofs * ncol)), dim3(BLOCK), 0, c->stream,
                           (const uint8_t*)c->inst_jac.p, cp.nproofs * ncol, (uint8_t*)c->inst_aff.p, c->d_flags);
    }
    if (trace.on) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        trace.mark("instance_msm");
    }
    return H2AGG_OK;
}

// ShaRead: no square roots and no sponge — the on-curve checks and the message streams are done; the chains run now (device
// or host threads, csrc/transcript.inc hash_backend) and this circuit's challenges are complete when its turn ends
int agg_hashed_transcripts(h2agg_ctx* c, AggState& st, const h2agg_circuit_proofs& cp, CircuitHost& h) {
    const size_t ncol = cp.vk->num_instance;
    if (h.L.next) hash_stream_launch(c, h.L, h.tb, cp.nproofs, (const uint8_t*)c->inst_aff.p, c->stream, 2);
    const bool chain_host = hash_backend(c, cp.nproofs) == 2;
    TRY(hash_chain_run(c, cp.vk->transcript_kind, h.L, h.tb, cp.nproofs, chain_host ? h.chal.data() : nullptr));
    if (!chain_host && !h.chal.empty())
        HIP_TRY(c, hipMemcpyAsync(h.chal.data(), c->tr_chal.p, h.chal.size(), hipMemcpyDeviceToHost, c->stream));
    if (!h.points.empty()) HIP_TRY(c, hipMemcpyAsync(h.points.data(), c->tr_points.p, h.points.size(), hipMemcpyDeviceToHost, c->stream));
    if (ncol) HIP_TRY(c, hipMemcpyAsync(h.inst_aff.data(), c->inst_aff.p, cp.nproofs * ncol * 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // tr_* and the staging block are reused by the next circuit
    st.trace.mark("hash_transcripts");
    return H2AGG_OK;
}

// Split download.  The LAST circuit's downloads are taken apart (host sponges, no advice_out): only the element streams stand
// between the device and the sponges, so they come down first, into page-locked memory, and the chains are posted; the
// decompressed points and the instance commitments — wanted by the recording, 0.3 ms later — follow without the host waiting
// for them (agg_sponges_post collects them).  (All three went to pageable vectors, which makes every hipMemcpyAsync a
// blocking round trip: 75 us in front of the sponges.)
int agg_split_download(h2agg_ctx* c, AggState& st, const h2agg_circuit_proofs& cp, size_t ci) {
    CircuitHost& h = st.H[ci];
    const size_t ncol = cp.vk->num_instance;
    const size_t nb_el = cp.nproofs * h.tb.elem_stride, nb_pt = h.points.size(), nb_in = ncol ? cp.nproofs * ncol * 64 : 0;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    TRY(ensure_pinned(c, c->h_down, al(nb_el) + al(nb_pt) + al(nb_in) + 256, "download block"));
    st.late.on = true;
    st.late.ci = ci;
    st.late.off_points = al(nb_el);
    st.late.off_inst = al(nb_el) + al(nb_pt);
    h.elems_p = c->h_down;
    HIP_TRY(c, hipMemcpyAsync(c->h_down, c->tr_elems.p, nb_el, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the element streams are here: the sponges can go
    if (nb_pt) HIP_TRY(c, hipMemcpyAsync(c->h_down + st.late.off_points, c->tr_points.p, nb_pt, hipMemcpyDeviceToHost, c->stream));
    if (nb_in) HIP_TRY(c, hipMemcpyAsync(c->h_down + st.late.off_inst, c->inst_aff.p, nb_in, hipMemcpyDeviceToHost, c->stream));
    st.trace.mark("tr_elements");
    return H2AGG_OK;
}

// The transcripts of circuit ci's proofs: the late half (the instance commitments' elements), then the hashed chains or the
// Poseidon sponges' input, and the downloads the recording reads — split, host or device shaped.
int agg_circuit_transcripts(const AggCall& call, h2agg_ctx* c, AggState& st, size_t ci) {
    const h2agg_circuit_proofs& cp = call.circuits[ci];
    CircuitHost& h = st.H[ci];
    const size_t ncol = cp.vk->num_instance;
    h.points.resize(cp.nproofs * h.npoints * 64);
    h.chal.resize(cp.nproofs * h.nsq * 32);
    h.inst_aff.resize(cp.nproofs * ncol * 64 + 1);
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_aux, 0));
    if (h.hashed) return agg_hashed_transcripts(c, st, cp, h);
    if (h.L.next) transcript_elements_launch(c, h.L, h.tb, cp.nproofs, (const uint8_t*)c->inst_aff.p, c->stream, 2);
    // host backend: only the element streams are made on the device (point decompression + PoseidonEncode); the sponges run
    // on worker threads further down, UNDER the recording of the schema their challenges feed
    if (st.host_sponge && !call.advice_out && ci == st.last_ci && c->dbg_prewake) return agg_split_download(c, st, cp, ci);
    if (st.host_sponge) {
        h.elems.resize(cp.nproofs * h.tb.elem_stride);
        h.elems_p = h.elems.data();
        HIP_TRY(c, hipMemcpyAsync(h.elems.data(), c->tr_elems.p, h.elems.size(), hipMemcpyDeviceToHost, c->stream));
    } else if (h.tb.nsq) {
        TRY(poseidon_run(c, (const uint8_t*)c->tr_elems.p, h.tb.elem_stride, (const uint32_t*)((const uint8_t*)c->tr_in.p + h.tb.hdr),
                         (uint32_t)h.tb.nsq, (uint32_t)cp.nproofs, (uint8_t*)c->tr_chal.p));
    }
    if (!h.points.empty()) HIP_TRY(c, hipMemcpyAsync(h.points.data(), c->tr_points.p, h.points.size(), hipMemcpyDeviceToHost, c->stream));
    if (ncol) HIP_TRY(c, hipMemcpyAsync(h.inst_aff.data(), c->inst_aff.p, cp.nproofs * ncol * 64, hipMemcpyDeviceToHost, c->stream));
    if (!st.host_sponge) {   // the last squeeze of every proof -> the aggregation transcript's elements (device)
        HIP_TRY(c, hipMemcpyAsync(h.chal.data(), c->tr_chal.p, h.chal.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpy2DAsync((uint8_t*)c->agg_elems.p + 32 * st.proof_base, 32, (const uint8_t*)c->tr_chal.p + last_squeeze(h, 0),
                                    32 * h.nsq, 32, cp.nproofs, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // tr_* and the staging block are reused by the next circuit
    st.trace.mark(st.host_sponge ? "tr_elements" : "transcripts");
    return H2AGG_OK;
}

// a proof's advice commitments = its first num_advice 'P' items, column order restored
void agg_advice_out(const AggCall& call, AggState& st, size_t ci) {
    if (!call.advice_out) return;
    const h2agg_circuit_proofs& cp = call.circuits[ci];
    const CircuitHost& h = st.H[ci];
    const std::vector<uint32_t> advice_pt = advice_point_order(*cp.vk);
    for (size_t i = 0; i < cp.nproofs; ++i)
        for (uint32_t col = 0; col < cp.vk->num_advice; ++col, st.advice_off += 64)
            memcpy(call.advice_out + st.advice_off, h.points.data() + 64 * (h.npoints * i + advice_pt[col]), 64);
}

// Host sponges: every proof's chain goes to a worker thread NOW and runs while this thread records the schema with placeholder
// registers for the challenges (Tape::add_const_placeholder) — the values are patched in before the tape runs.
int agg_sponges_post(const AggCall& call, h2agg_ctx* c, AggState& st) {
    st.sponges.post(call, st.H, st.trace);
    st.trace.mark("pool_begin");
    if (st.late.on) {   // the chains are running: now the points and instance commitments the recording reads
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        CircuitHost& h = st.H[st.late.ci];
        if (!h.points.empty()) memcpy(h.points.data(), c->h_down + st.late.off_points, h.points.size());
        if (h.inst_aff.size() > 1) memcpy(h.inst_aff.data(), c->h_down + st.late.off_inst, h.inst_aff.size() - 1);
        st.trace.mark("points_down");
    }
    return H2AGG_OK;
}
// ... their end: the chains' challenges are in H[].chal, the aggregation challenge follows on this thread
int agg_sponges_join(const AggCall& call, h2agg_ctx* c, AggState& st) {
    st.sponges.join();
    for (size_t j = 0; j < st.sponges.jobs.size(); ++j) {
        const CircuitHost& h = st.H[st.sponges.jobs[j].first];
        memcpy(st.agg_host.data() + 32 * j, h.chal.data() + last_squeeze(h, st.sponges.jobs[j].second), 32);
    }
    const uint32_t upto = (uint32_t)st.total_proofs;
    st.host_flags |= st.sponges.bad.load();
    if (!call.shard && !call.each) st.host_flags |= poseidon_run_host(st.agg_host.data(), 32 * st.total_proofs, &upto, 1, 1, st.lambda, 1);
    st.trace.mark("sponge_wait");
    return finish(c, st.host_flags);   // every transcript has run: bad point encodings / non-canonical scalars surface here
}
// Device sponges: they have run, circuit by circuit; the aggregation challenge follows on the device (a shard's follows its
// exchange, per-proof mode has none)
int agg_device_lambda(const AggCall& call, h2agg_ctx* c, AggState& st) {
    if (call.each || call.shard) return finish(c);   // every transcript has run: bad point encodings / non-canonical scalars surface here
    uint32_t upto = (uint32_t)st.total_proofs;
    TRY(ensure(c, c->tr_in, 256));
    HIP_TRY(c, hipMemcpyAsync(c->tr_in.p, &upto, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(poseidon_run(c, (const uint8_t*)c->agg_elems.p, 32 * st.total_proofs, (const uint32_t*)c->tr_in.p, 1, 1,
                     (uint8_t*)c->agg_elems.p + 32 * st.total_proofs));
    HIP_TRY(c, hipMemcpyAsync(c->h_pinned + 1024, (uint8_t*)c->agg_elems.p + 32 * st.total_proofs, 32, hipMemcpyDeviceToHost, c->stream));
    TRY(finish(c));   // every transcript has run: bad point encodings / non-canonical scalars surface here
    memcpy(st.lambda, c->h_pinned + 1024, 32);
    st.trace.mark("lambda");
    return H2AGG_OK;
}

// ---- the recording: kept, refilled or made afresh ------------------------------------------------------------------------------
// the SHAPE of a call: which keys, how many proofs of each, their length (AggPlan, csrc/verifier.inc)
std::string agg_signature(const AggCall& call, const AggState& st) {
    std::string sig;
    for (size_t ci = 0; ci < call.ncircuits; ++ci) {
        const h2agg_circuit_proofs& cp = call.circuits[ci];
        char buf[96];
        snprintf(buf, sizeof buf, "%llu:%d:%zu:%zu:", (unsigned long long)cp.vk->uid, cp.vk->multiopen_kind, cp.nproofs,
                 cp.nproofs ? cp.transcript_lens[0] : (size_t)0);   // (the kind: a key may be switched between two calls)
        sig += buf;
        sig += cp.name;
        sig += ';';
    }
    if (call.shard) {   // a shard's recording carries ITS powers of lambda
        sig += "shard:" + std::to_string(st.N_all) + ":";
        for (size_t i = 0; i < st.total_proofs; ++i) sig += std::to_string(call.shard->global_index[i]) + ",";
    }
    return sig;
}
AggPlan* agg_plan_find(h2agg_ctx* c, const std::string& sig) {
    AggPlan* plan = nullptr;
    if (c->agg_plans)
        for (AggPlan& pl : c->agg_plans->plans)
            if (pl.sig == sig) plan = &pl;
    return plan;
}
// a kept recording: this call's proof scalars and commitments into its registers and payloads (the challenges follow the sponges)
void agg_plan_refill(const AggCall& call, h2agg_ctx* c, AggState& st) {
    AggPlan* plan = st.plan;
    st.sc = plan->sc;
    plan->stamp = ++c->agg_plans->clock;
    ++c->agg_plans->hits;
    Tape& t = st.sc->s.tape;
    for (const AggPlan::ScalarPatch& sp : plan->scalars) t.set_const(sp.reg, call.circuits[sp.circuit].transcripts[sp.proof] + sp.off);
    for (const AggPlan::PointPatch& pp : plan->points)
        memcpy(st.sc->s.points.data() + 64 * (size_t)pp.slot, (pp.kind ? st.H[pp.circuit].inst_aff.data() : st.H[pp.circuit].points.data()) + pp.off, 64);
    st.sc->tape_done_ops = (size_t)-1;   // the register file on the device holds the previous call's values
    st.trace.mark("plan_refill");
}
// (the recording is good whatever this call's VALUES were) a fresh, cacheable one is kept for the next call of this shape;
// the least recently used goes first
void agg_plan_keep(h2agg_ctx* c, AggState& st, int rc_eval) {
    if (st.plan != &st.fresh || !st.cache_on || !st.fresh.cacheable) return;
    if (rc_eval != H2AGG_OK && rc_eval != H2AGG_ERR_NONCANONICAL && rc_eval != H2AGG_ERR_DIV_ZERO) return;
    if (!c->agg_plans) c->agg_plans = new AggPlanCache();
    AggPlanCache& pc = *c->agg_plans;
    ++pc.misses;
    if (pc.plans.size() >= AggPlanCache::MAX_PLANS) {
        size_t lru = 0;
        for (size_t k = 1; k < pc.plans.size(); ++k)
            if (pc.plans[k].stamp < pc.plans[lru].stamp) lru = k;
        h2agg_schema_destroy(pc.plans[lru].sc);
        pc.plans.erase(pc.plans.begin() + (long)lru);
    }
    st.fresh.stamp = ++pc.clock;
    pc.plans.push_back(std::move(st.fresh));
    st.guard.s = nullptr;   // the cache owns the schema now
}

// Challenges and scalars of proof i of circuit ci, in reading order, into P: every one a register of its own, whatever its
// value (see AggPlan), with the patch that refills it in `plan` — a scalar from the proof's bytes now and on every later
// call, a challenge from H[ci].chal once the sponges have run.
void read_proof_regs(Schema& S, const h2agg_vk& vk, const CircuitHost& h, size_t ci, size_t i, const uint8_t* proof, AggPlan& plan,
                     ProofRegs& P) {
    size_t soff = 0;   // byte offset of the first scalar = point bytes * (#P before the evals)
    for (char ch : h.script) {
        if (ch == 'S') break;
        if (ch == 'P') soff += proof_point_bytes(vk);
    }
    auto next_scalar = [&] {
        const uint32_t r = S.tape.add_const_placeholder();
        S.tape.set_const(r, proof + soff);
        plan.scalars.push_back({r, (uint32_t)ci, (uint32_t)i, (uint32_t)soff});
        soff += 32;
        return r;
    };
    size_t qn = 0;
    auto next_chal = [&] {
        const uint32_t reg = S.tape.add_const_placeholder();
        plan.chal.push_back({reg, (uint32_t)ci, 32 * (h.nsq * i + qn++)});
        return reg;
    };
    P.challenges.assign(vk.num_challenges, Rec(S).cu64(0));
    for (uint32_t phase = 0; phase <= vk.max_phase; ++phase)
        for (uint32_t k2 = 0; k2 < vk.num_challenges; ++k2)
            if (vk.challenge_phase[k2] == phase) P.challenges[k2] = next_chal();
    P.theta = next_chal();
    P.beta = next_chal();
    P.gamma = next_chal();
    P.y = next_chal();
    P.x = next_chal();
    if (vk.multiopen_kind == H2AGG_MULTIOPEN_SHPLONK) P.y_open = next_chal();
    P.v = next_chal();
    P.u = next_chal();
    for (size_t q = 0; q < vk.instance_q.size(); ++q) P.instance_evals.push_back(next_scalar());
    for (size_t q = 0; q < vk.advice_q.size(); ++q) P.advice_evals.push_back(next_scalar());
    for (size_t q = 0; q < vk.fixed_q.size(); ++q) P.fixed_evals.push_back(next_scalar());
    P.random_eval = next_scalar();
    for (size_t q = 0; q < vk.perm_commitments.size() / 64; ++q) P.permutation_evals.push_back(next_scalar());
    for (uint32_t si = 0; si < vk.n_sets; ++si) {                      // verify.rs:215-237
        ProofRegs::Set set;
        set.eval = next_scalar();
        set.next = next_scalar();
        set.last = si + 1 < vk.n_sets ? next_scalar() : ~0u;
        P.sets.push_back(set);
    }
    for (size_t j = 0; j < vk.lookups.size(); ++j) {                   // verify.rs:308-312
        ProofRegs::Lk lk;
        lk.product = next_scalar();
        lk.product_next = next_scalar();
        lk.input = next_scalar();
        lk.input_inv = next_scalar();
        lk.table = next_scalar();
        P.lookups.push_back(lk);
    }
}

// Recorded afresh — the reference's control flow over tape registers: every proof's queries and its multiopen, (w_x, w_g) per
// proof to st.roots in aggregation order.  The W commitments must be one per rotation group (multiopen.rs:48), checked by
// batch_multi_open_regs: the aggregation refuses the call, per-proof mode marks that proof and goes on.
int agg_record(const AggCall& call, h2agg_ctx* c, AggState& st) {
    TRY(h2agg_schema_create(c, &st.sc));
    st.guard.s = st.sc;
    st.fresh.sc = st.sc;
    st.plan = &st.fresh;
    Schema& S = st.sc->s;
    S.track_src = true;
    for (size_t ci = 0; ci < call.ncircuits; ++ci) {
        const h2agg_circuit_proofs& cp = call.circuits[ci];
        const h2agg_vk& vk = *cp.vk;
        const CircuitHost& h = st.H[ci];
        for (size_t i = 0; i < cp.nproofs; ++i) {
            const uint8_t* pts = h.points.data() + 64 * h.npoints * i;
            ProofRegs P;
            read_proof_regs(S, vk, h, ci, i, cp.transcripts[i], st.fresh, P);
            const std::string key = std::string(cp.name) + "_p" + std::to_string(i);   // verify_circuit.rs:140
            std::vector<Query> qs;
            TRY(build_queries(c, S, vk, key, P, h.inst_aff.data() + 64 * vk.num_instance * i, pts, qs));
            std::vector<int32_t> rot(qs.size());
            std::vector<uint32_t> preg(qs.size()), qnode(qs.size()), poly(qs.size());
            for (size_t q = 0; q < qs.size(); ++q) {
                rot[q] = qs[q].rotation;
                preg[q] = qs[q].point_reg;
                qnode[q] = qs[q].node;
                poly[q] = qs[q].poly;
            }
            const bool shplonk = vk.multiopen_kind == H2AGG_MULTIOPEN_SHPLONK;   // its H1, H2: the proof's last two points
            const uint8_t* w = pts + 64 * (h.npoints - (shplonk ? 2 : h.n_w));
            uint32_t w_x = 0, w_g = 0;
            const bool ok = shplonk ? shplonk_multi_open_regs(S, key.c_str(), qs.size(), poly.data(), rot.data(), preg.data(), qnode.data(), w,
                                                              w + 64, P.y_open, P.v, P.u, w_x, w_g)
                                    : S.batch_multi_open_regs(key.c_str(), qs.size(), rot.data(), preg.data(), qnode.data(), h.n_w, w, P.v,
                                                              P.u, w_x, w_g);
            if (!ok) {
                if (!call.each) return fail(c, H2AGG_ERR_INVALID, S.err);
                call.each_status[h.first_proof + i] = H2AGG_ERR_INVALID;   // (this proof only: the others go on)
                continue;
            }
            st.roots.push_back({w_x, w_g});
            if (call.each) st.each_idx.push_back(h.first_proof + i);
        }
    }
    return H2AGG_OK;
}

// Where the recording's points came from.  Every commitment it refers to must be accounted for: this call's decompressed
// proof points / instance commitments (refilled on a hit) or the verifying key's own (constant for the key).  A point copied
// in from anywhere else would be frozen into the recording as the first call's value — such a recording is used once and not
// kept (ADVICE r3).
void agg_point_sources(const AggCall& call, AggState& st) {
    Schema& S = st.sc->s;
    auto inside = [](const uint8_t* p, const std::vector<uint8_t>& v) { return !v.empty() && p >= v.data() && p + 64 <= v.data() + v.size(); };
    for (size_t slot = 0; slot < S.point_src.size(); ++slot) {
        const uint8_t* src = S.point_src[slot];
        bool known = false;
        for (size_t ci = 0; ci < call.ncircuits && !known; ++ci) {
            const CircuitHost& h = st.H[ci];
            if (inside(src, h.points)) {
                st.fresh.points.push_back({(uint32_t)slot, (uint32_t)ci, 0, (size_t)(src - h.points.data())});
                known = true;
            } else if (inside(src, h.inst_aff)) {
                st.fresh.points.push_back({(uint32_t)slot, (uint32_t)ci, 1, (size_t)(src - h.inst_aff.data())});
                known = true;
            } else if (inside(src, call.circuits[ci].vk->fixed_commitments) || inside(src, call.circuits[ci].vk->perm_commitments)) {
                known = true;
            }
        }
        if (!known) st.fresh.cacheable = false;
    }
    S.track_src = false;
    S.point_src.clear();
    S.point_src.shrink_to_fit();
}

// acc = acc * lambda + proof  (verify.rs:926-938)
// Recorded in its distributed form  sum_i lambda^(N-1-i) * proof_i  (what the nested fold expands to; field arithmetic is
// exact, the entries keep the fold's order): every proof's entries meet ONE factor, lambda^e built by halving, instead of
// being multiplied through once per later proof — the nested form costs O(N^2) tape operations (4 ms of host time and a
// 700 k-operation tape at 64 proofs).
int agg_record_fold(const AggCall& call, h2agg_ctx* c, AggState& st) {
    (void)c;
    Schema& S = st.sc->s;
    const std::vector<std::pair<uint32_t, uint32_t>>& proofs = st.roots;
    const h2agg_shard* shard = call.shard;
    const size_t N_all = st.N_all;
    const uint32_t lam_reg = S.tape.add_const_placeholder();
    auto weighted = [&](uint32_t node, size_t i) {   // (a shard: i-th LOCAL proof, exponent from its place in the whole aggregation)
        const uint32_t e = (uint32_t)(N_all - 1 - (shard ? (size_t)shard->global_index[i] : i));
        if (e == 0) return node;
        return S.add_binary(SchemaNode::MUL, node, S.add_leaf_reg(SchemaNode::SCALAR, S.tape.pow(lam_reg, e)));
    };
    uint32_t acc_x = weighted(proofs[0].first, 0), acc_g = weighted(proofs[0].second, 0);
    for (size_t i = 1; i < proofs.size(); ++i) {
        acc_x = S.add_binary(SchemaNode::ADD, acc_x, weighted(proofs[i].first, i));
        acc_g = S.add_binary(SchemaNode::ADD, acc_g, weighted(proofs[i].second, i));
    }
    // the host half of the evaluation (both eval_prepare walks, the tape's dependency levels): still under the sponges
    TRY(h2agg_evaluate_multiopen_prepare(st.sc, acc_x, acc_g));
    st.trace.mark("host_prepare");
    if (st.trace.on) {
        char buf[160];
        snprintf(buf, sizeof buf, " [tape: %zu ops, %u levels, %u consts, %u live at once: %s]", S.tape.ops.size(), st.sc->prep.tape.maxlevel,
                 S.tape.nconst, st.sc->prep.tape.lds_peak, st.sc->prep.tape.lds ? "register file in LDS" : "register file in L2");
        st.trace.line += buf;
    }
    agg_point_sources(call, st);
    st.fresh.sig = st.sig;
    st.fresh.lam_reg = lam_reg;
    st.fresh.acc_x = acc_x;
    st.fresh.acc_g = acc_g;
    return H2AGG_OK;
}

// a shard's exchange 1: every rank's squeezes -> the same lambda on every rank
int agg_lambda_exchange(const AggCall& call, h2agg_ctx* c, AggState& st, ShardExchange& xch) {
    if (!st.host_sponge) {
        st.agg_host.resize(st.total_proofs * 32);
        size_t j = 0;
        for (size_t ci = 0; ci < call.ncircuits; ++ci)
            for (size_t i = 0; i < call.circuits[ci].nproofs; ++i, ++j)
                memcpy(st.agg_host.data() + 32 * j, st.H[ci].chal.data() + last_squeeze(st.H[ci], i), 32);
    }
    TRY(xch.lambda(st.agg_host.data(), st.total_proofs, st.lambda));
    st.trace.mark("lambda_exchange");
    if (c->dbg_shard_fail == 2) return fail(c, H2AGG_ERR_INVALID, "injected failure between the exchanges (debug key shard_fail)");
    return H2AGG_OK;
}
// more ranks than proofs: this rank only takes part in the two exchanges (identity partials)
int agg_empty_rank(const AggCall& call, h2agg_ctx* c, ShardExchange& xch) {
    uint8_t lam0[32];
    TRY(xch.lambda(nullptr, 0, lam0));
    if (call.lambda_out) memcpy(call.lambda_out, lam0, 32);
    if (c->dbg_shard_fail == 2) return fail(c, H2AGG_ERR_INVALID, "injected failure between the exchanges (debug key shard_fail)");
    TRY(xch.sum_pair(call.left_aff, call.right_aff));
    if (call.s_g2) TRY(h2agg_final_pair_check(c, call.left_aff, call.right_aff, call.s_g2, call.g2, call.pairing_ok));
    return H2AGG_OK;
}

// verify_single_proof_in_chip: every proof's own evaluate_multiopen_proof, 2N sides in one set of launches
int agg_evaluate_each(const AggCall& call, h2agg_ctx* c, AggState& st) {
    (void)c;
    if (st.roots.empty()) return H2AGG_OK;
    std::vector<uint8_t> pairs(128 * st.roots.size());
    TRY(evaluate_multiopen_many(st.sc, st.roots, pairs.data()));
    for (size_t k = 0; k < st.each_idx.size(); ++k) memcpy(call.each_pairs + 128 * st.each_idx[k], pairs.data() + 128 * k, 128);
    st.trace.mark("evaluate");
    return H2AGG_OK;
}

// ---- the call ---------------------------------------------------------------------------------------------------------------
// A committed call, stage by stage.  Whatever makes it return early — any TRY, an exception — is followed by xch.leave() in
// verify_aggregation, which also owns the trace and the state.
int verify_aggregation_impl(const AggCall& call, h2agg_ctx* c, AggState& st, ShardExchange& xch) {
    PhaseTrace& trace = st.trace;
    const h2agg_shard* shard = call.shard;
    if (c->dbg_shard_fail == 1 && shard) return fail(c, H2AGG_ERR_INVALID, "injected failure before the lambda exchange (debug key shard_fail)");
    if (shard && st.total_proofs == 0) return agg_empty_rank(call, c, xch);
    TRY(agg_begin(call, c, st));
    for (size_t ci = 0; ci < call.ncircuits; ++ci) {   // circuit by circuit: tr_* and the staging block are shared
        TRY(agg_check_circuit(c, call.circuits[ci], nullptr, &st.H[ci]));
        if (call.circuits[ci].nproofs == 0) continue;
        st.H[ci].first_proof = st.proof_base;
        TRY(agg_instance_commitments(call, c, st, ci));
        TRY(agg_circuit_transcripts(call, c, st, ci));
        agg_advice_out(call, st, ci);
        st.proof_base += call.circuits[ci].nproofs;
    }
    // ---- the sponges.  Device backend: they have run (above).  Host backend: posted here, joined below, the recording between
    if (st.host_sponge) TRY(agg_sponges_post(call, c, st));
    else TRY(agg_device_lambda(call, c, st));
    // ---- a recording of this shape from an earlier call?  (h2agg_debug_configure "plan_cache" 0: record every call afresh)
    st.cache_on = c->dbg_plan_cache != 0 && !call.each;
    st.sig = agg_signature(call, st);
    st.plan = st.cache_on ? agg_plan_find(c, st.sig) : nullptr;
    if (st.plan) {
        agg_plan_refill(call, c, st);
    } else {
        TRY(agg_record(call, c, st));
        trace.mark("host_queries");
        if (!call.each) TRY(agg_record_fold(call, c, st));
    }
    if (st.host_sponge) TRY(agg_sponges_join(call, c, st));
    if (shard) TRY(agg_lambda_exchange(call, c, st, xch));
    Tape& tape = st.sc->s.tape;
    for (const AggPlan::ChalPatch& pt : st.plan->chal) tape.set_const(pt.reg, st.H[pt.circuit].chal.data() + pt.off);
    if (call.each) return agg_evaluate_each(call, c, st);
    if (call.lambda_out) memcpy(call.lambda_out, st.lambda, 32);
    tape.set_const(st.plan->lam_reg, st.lambda);
    // (the pairing behind the evaluation wants one worker awake: its second pair's Miller loop runs there)
    if (call.s_g2 && !shard && c->dbg_prewake) HostPool::get().prewake(1);
    const uint32_t acc_x = st.plan->acc_x, acc_g = st.plan->acc_g;   // (agg_plan_keep moves the plan)
    const int rc_eval = h2agg_evaluate_multiopen_proof(st.sc, acc_x, acc_g, call.left_aff, call.right_aff);
    agg_plan_keep(c, st, rc_eval);
    TRY(rc_eval);
    trace.mark("evaluate");
    if (shard) {
        if (call.s_g2 && c->dbg_prewake) HostPool::get().prewake(1);   // (the pairing's second Miller loop; the exchange is ~0.1 ms)
        TRY(xch.sum_pair(call.left_aff, call.right_aff));
        trace.mark("pair_exchange");
    }
    if (call.s_g2) TRY(h2agg_final_pair_check(c, call.left_aff, call.right_aff, call.s_g2, call.g2, call.pairing_ok));
    trace.mark("pairing");
    return H2AGG_OK;
}

int verify_aggregation(h2agg_ctx* c, const AggCall& call) try {
    TRY(bind(c));
    TRY(agg_check_call(c, call));
    PhaseTrace trace(c->dbg_phases ? &c->last_phases : nullptr);
    TraceScope trace_scope(&trace);
    AggState st(trace);
    TRY(agg_check_shard(c, call, st));
    ShardExchange xch(c, call.shard, st.N_all);   // the point of commitment
    int rc;
    try {
        rc = verify_aggregation_impl(call, c, st, xch);
    } catch (const std::bad_alloc&) {
        rc = fail(c, H2AGG_ERR_NOMEM, "out of host memory");
    } catch (...) {
        rc = fail(c, H2AGG_ERR_INVALID, "unexpected exception");
    }
    st.sponges.join();   // (an early return between post() and join(): the chains end before this rank's exchange, as ever)
    return xch.leave(rc);
} API_CATCH

// ---- h2agg_verify_proofs: each proof on its own ---------------------------------------------------------------------------
// e(left_i, s_g2) * e(right_i, -g2) == 1 for every proof whose status is OK, one proof per job on the host pool; the prepared
// lines of s_g2 and -g2 are made once for all of them
template <class P>
int pair_checks_t(h2agg_ctx* c, const uint8_t* pairs, const int32_t* status, size_t n, const uint8_t s_g2[128], const uint8_t g2[128],
                  int* ok) {
    std::vector<typename P::G1> ps(2 * n);
    std::vector<typename P::G2> qs(2);
    uint8_t g2s[256];
    memcpy(g2s, s_g2, 128);
    memcpy(g2s + 128, g2, 128);
    {   // (the G2 points' checks, beside the generator of G1)
        uint8_t gen2[128] = {0};
        gen2[0] = gen2[64] = 1;
        gen2[32] = gen2[96] = 2;
        std::vector<typename P::G1> p0;
        TRY(pairing_load<P>(c, gen2, g2s, 2, p0, qs));
    }
    P::negate(qs[1]);
    const std::shared_ptr<const typename P::Prepared> keep[2] = {P::prepared(s_g2, false, qs[0]), P::prepared(g2, true, qs[1])};
    const std::vector<const typename P::Prepared*> preps = {keep[0].get(), keep[1].get()};
    std::vector<size_t> todo;
    for (size_t i = 0; i < n; ++i) {
        ok[i] = 0;
        if (status[i] != H2AGG_OK) continue;
        for (int side = 0; side < 2; ++side) {
            const int r = P::load1(pairs + 128 * i + 64 * side, ps[2 * i + side]);
            if (r == 1) return fail(c, H2AGG_ERR_HIP, "pairing: an evaluated G1 coordinate is >= p");
            if (r) return fail(c, H2AGG_ERR_HIP, "pairing: an evaluated G1 point is not on the curve");
        }
        todo.push_back(i);
    }
    HostPool::get().run(todo.size(), HostPool::get().size(), [&](size_t j) {
        const size_t i = todo[j];
        ok[i] = P::check_prepared(std::vector<typename P::G1>{ps[2 * i], ps[2 * i + 1]}, preps) ? 1 : 0;
    });
    return H2AGG_OK;
}

struct EachItem {
    size_t ci, i, g;   // proof i of circuit ci, the g-th proof of the call
};
// What h2agg_verify_proofs hands to a group and gets back, at the proofs' places in the call
struct EachResults {
    int32_t* status;           // [N]
    uint8_t* pairs;            // [N][128]
    uint8_t* advice_out;       // optional
    const size_t* advice_at;   // [N] byte offset of every proof's advice commitments in advice_out
};

// One verify_aggregation call (per-proof mode) over a list of proofs: each circuit's proofs grouped by length (the device
// transcripts take one length per launch); results scattered back to the proofs' places
int verify_each_group(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, const std::vector<EachItem>& list, const EachResults& res) {
    std::vector<h2agg_circuit_proofs> sub;
    std::vector<std::string> names;
    std::vector<std::vector<const uint8_t*>> tr, in;
    std::vector<std::vector<size_t>> lens;
    std::vector<std::vector<uint32_t>> ilens;
    std::vector<size_t> order;   // the call's proof j -> the item's place g
    std::vector<bool> taken(list.size(), false);
    for (size_t a = 0; a < list.size(); ++a) {
        if (taken[a]) continue;
        const h2agg_circuit_proofs& cp = circuits[list[a].ci];
        const size_t plen = cp.transcript_lens[list[a].i], ncol = cp.vk->num_instance;
        tr.emplace_back();
        in.emplace_back();
        lens.emplace_back();
        ilens.emplace_back();
        for (size_t b = a; b < list.size(); ++b) {
            if (taken[b] || list[b].ci != list[a].ci || cp.transcript_lens[list[b].i] != plen) continue;
            taken[b] = true;
            tr.back().push_back(cp.transcripts[list[b].i]);
            lens.back().push_back(plen);
            if (ncol) {
                in.back().push_back(cp.instances[list[b].i]);
                for (size_t col = 0; col < ncol; ++col) ilens.back().push_back(cp.instance_lens[list[b].i * ncol + col]);
            }
            order.push_back(list[b].g);
        }
        // (a circuit split by length: every group's keys of its own, "{name}_p{i}" must not meet twice in one schema)
        names.push_back(std::string(cp.name) + "#" + std::to_string(names.size()));
        h2agg_circuit_proofs g = cp;
        g.nproofs = tr.back().size();
        sub.push_back(g);
    }
    for (size_t k = 0; k < sub.size(); ++k) {
        sub[k].name = names[k].c_str();
        sub[k].transcripts = tr[k].data();
        sub[k].transcript_lens = lens[k].data();
        sub[k].instances = in[k].empty() ? nullptr : in[k].data();
        sub[k].instance_lens = ilens[k].empty() ? nullptr : ilens[k].data();
    }
    const size_t n = order.size();
    std::vector<uint8_t> p(128 * n, 0), adv;
    std::vector<int32_t> st(n, H2AGG_OK);
    size_t adv_need = 0;
    for (const h2agg_circuit_proofs& g : sub) adv_need += g.nproofs * (size_t)g.vk->num_advice * 64;
    if (res.advice_out) adv.resize(adv_need + 1);
    uint8_t l0[64], r0[64];
    AggCall call;
    call.circuits = sub.data();
    call.ncircuits = sub.size();
    call.left_aff = l0;
    call.right_aff = r0;
    call.advice_out = res.advice_out ? adv.data() : nullptr;
    call.advice_cap = adv_need;
    call.each = true;
    call.each_pairs = p.data();
    call.each_status = st.data();
    TRY(verify_aggregation(c, call));
    size_t aoff = 0;
    for (size_t j = 0; j < n; ++j) {   // (advice in the call's order: circuit groups, proofs in order)
        const size_t g = order[j];
        res.status[g] = st[j];
        if (st[j] == H2AGG_OK) memcpy(res.pairs + 128 * g, p.data() + 128 * j, 128);
        if (!res.advice_out) continue;
        size_t ci = 0, base = 0;
        while (g >= base + circuits[ci].nproofs) base += circuits[ci++].nproofs;
        const size_t bytes = (size_t)circuits[ci].vk->num_advice * 64;
        if (st[j] == H2AGG_OK) memcpy(res.advice_out + res.advice_at[g], adv.data() + aoff, bytes);
        aoff += bytes;
    }
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_verify_proofs(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2, const uint8_t* g2,
                        uint8_t* left_aff, uint8_t* right_aff, int32_t* status, int* pairing_ok, uint8_t* advice_out,
                        size_t advice_cap) try {
    TRY(bind(c));
    if (!circuits || ncircuits == 0 || !left_aff || !right_aff || !status) return fail(c, H2AGG_ERR_INVALID, "null argument");
    if ((s_g2 == nullptr) != (g2 == nullptr) || (s_g2 && !pairing_ok))
        return fail(c, H2AGG_ERR_INVALID, "pass s_g2, g2 and pairing_ok together (or none)");
    // ---- what is decided by a proof's shape alone (verify.rs:487-490, :601-603): that proof's status, before any work
    size_t advice_need = 0;
    std::vector<size_t> advice_at;   // byte offset of every proof's advice commitments in advice_out
    std::vector<int32_t> shape;      // every proof's status as its shape decides it
    for (size_t ci = 0; ci < ncircuits; ++ci) {
        TRY(agg_check_circuit(c, circuits[ci], &shape, nullptr));
        for (size_t i = 0; i < circuits[ci].nproofs; ++i) {
            advice_at.push_back(advice_need);
            advice_need += (size_t)circuits[ci].vk->num_advice * 64;
        }
    }
    const size_t N = shape.size();
    if (N == 0) return fail(c, H2AGG_ERR_INVALID, "no proofs");
    if (advice_out && advice_need > advice_cap) return fail(c, H2AGG_ERR_INVALID, "advice_out is too small for the proofs' advice commitments");
    memset(left_aff, 0, 64 * N);
    memset(right_aff, 0, 64 * N);
    if (pairing_ok) memset(pairing_ok, 0, sizeof(int) * N);
    if (advice_out) memset(advice_out, 0, advice_need);
    std::vector<EachItem> items;
    size_t g = 0;
    for (size_t ci = 0; ci < ncircuits; ++ci)
        for (size_t i = 0; i < circuits[ci].nproofs; ++i, ++g) {
            status[g] = shape[g];
            if (shape[g] == H2AGG_OK) items.push_back({ci, i, g});
        }
    std::vector<uint8_t> pairs(128 * N);
    const EachResults res{status, pairs.data(), advice_out, advice_at.data()};
    if (!items.empty()) {
        const int rc = verify_each_group(c, circuits, items, res);
        if (rc == H2AGG_ERR_BAD_POINT || rc == H2AGG_ERR_NONCANONICAL) {
            // a proof's bytes do not decode (the device's flags are batch-wide): verify the proofs one by one to name it
            for (const EachItem& it : items) {
                const int r1 = verify_each_group(c, circuits, std::vector<EachItem>{it}, res);
                if (r1 == H2AGG_ERR_BAD_POINT || r1 == H2AGG_ERR_NONCANONICAL || r1 == H2AGG_ERR_INVALID || r1 == H2AGG_ERR_EMPTY)
                    status[it.g] = r1;
                else if (r1 != H2AGG_OK)
                    return r1;
            }
        } else if (rc != H2AGG_OK) {
            return rc;
        }
    }
    for (size_t k = 0; k < N; ++k) {
        memcpy(left_aff + 64 * k, pairs.data() + 128 * k, 64);
        memcpy(right_aff + 64 * k, pairs.data() + 128 * k + 64, 64);
    }
    // (h2agg_last_phases: the phases of the per-proof verification as the aggregation names them, then the pairings)
    if (s_g2) {
        const auto t0 = std::chrono::steady_clock::now();
        int rc;
#ifdef H2AGG_PAIRING_ADX_BUILD
        if (pairing_adx_ok()) rc = pair_checks_t<pairing_adx::Api>(c, pairs.data(), status, N, s_g2, g2, pairing_ok);
        else
#endif
        rc = pair_checks_t<pairing::Api>(c, pairs.data(), status, N, s_g2, g2, pairing_ok);
        TRY(rc);
        if (c->dbg_phases) {
            char buf[64];
            snprintf(buf, sizeof buf, " pairing=%.3f", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            c->last_phases += buf;
        }
    }
    return H2AGG_OK;
} API_CATCH

int h2agg_verify_plan_stats(h2agg_ctx* c, uint64_t* hits, uint64_t* misses, uint64_t* plans_kept) {
    if (!c) return H2AGG_ERR_INVALID;
    const AggPlanCache* pc = c->agg_plans;
    if (hits) *hits = pc ? pc->hits : 0;
    if (misses) *misses = pc ? pc->misses : 0;
    if (plans_kept) *plans_kept = pc ? pc->plans.size() : 0;
    return H2AGG_OK;
}

const char* h2agg_last_phases(h2agg_ctx* c) { return c ? c->last_phases.c_str() : ""; }

}  // extern "C"

namespace {
// the arguments of the three aggregation entries as a call
AggCall agg_call(const h2agg_circuit_proofs* circuits, size_t ncircuits, const h2agg_shard* shard, const uint8_t* s_g2, const uint8_t* g2,
                 uint8_t* left_aff, uint8_t* right_aff, uint8_t* lambda_out, int* pairing_ok, uint8_t* advice_out, size_t advice_cap) {
    AggCall call;
    call.circuits = circuits;
    call.ncircuits = ncircuits;
    call.shard = shard;
    call.s_g2 = s_g2;
    call.g2 = g2;
    call.left_aff = left_aff;
    call.right_aff = right_aff;
    call.lambda_out = lambda_out;
    call.pairing_ok = pairing_ok;
    call.advice_out = advice_out;
    call.advice_cap = advice_cap;
    return call;
}
}  // namespace

extern "C" {

int h2agg_verify_aggregation_ex(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                                const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64], uint8_t lambda_out[32],
                                int* pairing_ok, uint8_t* advice_out, size_t advice_cap) {
    return verify_aggregation(c, agg_call(circuits, ncircuits, nullptr, s_g2, g2, left_aff, right_aff, lambda_out, pairing_ok, advice_out, advice_cap));
}

int h2agg_verify_aggregation(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const uint8_t* s_g2,
                             const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64], uint8_t lambda_out[32],
                             int* pairing_ok) {
    return verify_aggregation(c, agg_call(circuits, ncircuits, nullptr, s_g2, g2, left_aff, right_aff, lambda_out, pairing_ok, nullptr, 0));
}

int h2agg_verify_aggregation_sharded(h2agg_ctx* c, const h2agg_circuit_proofs* circuits, size_t ncircuits, const h2agg_shard* shard,
                                     const uint8_t* s_g2, const uint8_t* g2, uint8_t left_aff[64], uint8_t right_aff[64],
                                     uint8_t lambda_out[32], int* pairing_ok, uint8_t* advice_out, size_t advice_cap) {
    if (!c) return H2AGG_ERR_INVALID;
    if (!shard) return fail(c, H2AGG_ERR_INVALID, "null shard description");
    return verify_aggregation(c, agg_call(circuits, ncircuits, shard, s_g2, g2, left_aff, right_aff, lambda_out, pairing_ok, advice_out, advice_cap));
}

}  // extern "C"
