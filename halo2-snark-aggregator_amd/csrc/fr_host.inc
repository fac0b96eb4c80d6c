// What the Fr prover entry points share on top of host.inc (included into h2agg.hip ahead of params.inc, fr_fft.inc,
// poly_open.inc and prod.inc: shares the context internals): field constants, the checks every entry point repeats and the
// level plan of the chunked sweeps (geometry: fr_chunk.hpp).  The growing-buffer rule, the staging of a host twin and the
// catch blocks behind every extern "C" function are host.inc's.

namespace {

// the value 2^261 (the device's Montgomery radix) as a host field element: x * fr_radix() is what the device holds for x
const ph::HFr& fr_radix() {
    static const ph::HFr r = [] {
        ph::HFr x = ph::one();
        for (int i = 0; i < 29 * NL; ++i) x = ph::add(x, x);
        return x;
    }();
    return r;
}

void hfr_words(const ph::HFr& a, uint32_t out[8]) {
    uint8_t b[32];
    hfr_bytes(a, b);
    memcpy(out, b, 32);
}

// EvaluationDomain::get_omega: ROOT_OF_UNITY^(2^(S - k))
ph::HFr fft_omega(unsigned k) {
    ph::HFr w = ph::from_words(FR_ROOT_OF_UNITY);
    for (unsigned i = k; i < (unsigned)FR_S; ++i) w = ph::mul(w, w);
    return w;
}

// 32 canonical little-endian bytes -> a host field element
int fr_parse(h2agg_ctx* c, const uint8_t* b, ph::HFr* out) {
    if (!fr_bytes_canonical(b)) return fail(c, H2AGG_ERR_NONCANONICAL, "input integer >= modulus");
    uint64_t w[4];
    memcpy(w, b, 32);
    *out = ph::from_words(w);
    return H2AGG_OK;
}

int fr_check_k(h2agg_ctx* c, unsigned k) {
    if (k > FFT_MAX_K) return fail(c, H2AGG_ERR_INVALID, "k must be <= 24");
    return H2AGG_OK;
}

// the levels of one chunked sweep: cnt[0] = n0 elements per query, cnt[l + 1] = ceil(cnt[l] / 2^t), down to 1.  Level l >= 1 is
// [query][cnt[l]] elements at off[l] of the family's level buffer; total: the elements of all levels, over the nq queries.
// t comes from the caller's debug key (fr_poly_chunk, fr_scan_chunk) or is FR_CHUNK_LOG.
struct FrLevelPlan {
    unsigned t = 0;
    size_t nq = 0;
    std::vector<uint32_t> cnt;
    std::vector<size_t> off;
    size_t total = 0;
    size_t launches() const { return cnt.size() - 1; }
};

FrLevelPlan fr_level_plan(unsigned t, size_t n0, size_t nq) {
    FrLevelPlan p;
    p.t = t;
    p.nq = nq;
    p.cnt.push_back((uint32_t)n0);
    p.off.push_back(0);
    do {
        p.cnt.push_back((p.cnt.back() + (1u << t) - 1u) >> t);
        p.off.push_back(p.total);
        p.total += nq * p.cnt.back();
    } while (p.cnt.back() > 1);
    return p;
}

}  // namespace
