// The pairing check on the host (included into h2agg.hip behind config_api.inc: shares the context internals; arithmetic in
// pairing.hpp, compiled twice: portable and for BMI2 + ADX): h2agg_pairing_product, h2agg_pairing_check,
// h2agg_g2_batch_decompress, h2agg_final_pair_check.  They need no device: ctx may be NULL (then no message is kept).

namespace {

// csrc/transcript.inc (HostPool): if a pool worker is spinning for work, `on_worker` runs there while `here` runs on the
// calling thread, both done on return (true); otherwise nothing has run (false)
bool host_pool_pair_if_awake(const std::function<void()>& on_worker, const std::function<void()>& here);
bool pairing_adx_ok() {
#ifdef H2AGG_PAIRING_ADX_BUILD
    static const bool ok = __builtin_cpu_supports("bmi2") && __builtin_cpu_supports("adx") && !getenv("H2AGG_PAIRING_PORTABLE");
    return ok;
#else
    return false;
#endif
}
template <class P>
int pairing_load(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, std::vector<typename P::G1>& ps,
                 std::vector<typename P::G2>& qs) {
    if (n && (!g1_aff || !g2_aff)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ps.resize(n);
    qs.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const int r1 = P::load1(g1_aff + 64 * i, ps[i]);
        if (r1 == 1) return fail(c, H2AGG_ERR_NONCANONICAL, "pairing: G1 coordinate >= p");
        if (r1) return fail(c, H2AGG_ERR_BAD_POINT, "pairing: G1 point not on the curve");
        const int r2 = P::load2(g2_aff + 128 * i, qs[i]);
        if (r2 == 1) return fail(c, H2AGG_ERR_NONCANONICAL, "pairing: G2 coordinate >= p");
        if (r2 == 2) return fail(c, H2AGG_ERR_BAD_POINT, "pairing: G2 point not on the twist");
        if (r2) return fail(c, H2AGG_ERR_BAD_POINT, "pairing: G2 point outside the order-r subgroup");
    }
    return H2AGG_OK;
}
template <class P>
int pairing_product_t(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, uint8_t out_gt[384]) {
    std::vector<typename P::G1> ps;
    std::vector<typename P::G2> qs;
    TRY(pairing_load<P>(c, g1_aff, g2_aff, n, ps, qs));
    // (prepared lines: a G2 point that comes back — [s]_2, [1]_2 of one ParamsKZG — pays its doubling / addition steps once)
    std::vector<std::shared_ptr<const typename P::Prepared>> keep(n);
    std::vector<const typename P::Prepared*> preps(n);
    for (size_t i = 0; i < n; ++i) {
        keep[i] = P::prepared(g2_aff + 128 * i, false, qs[i]);
        preps[i] = keep[i].get();
    }
    P::product_prepared(ps, preps, out_gt);
    return H2AGG_OK;
}
template <class P>
int pairing_check_t(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, int* ok) {
    std::vector<typename P::G1> ps;
    std::vector<typename P::G2> qs;
    TRY(pairing_load<P>(c, g1_aff, g2_aff, n, ps, qs));
    *ok = P::check(ps, qs) ? 1 : 0;
    return H2AGG_OK;
}
// e(left, [s]_2) * e(right, -[1]_2) == 1 ?   (verify.rs:733-739: `n_g2_prepared = -params.g2()`)
template <class P>
int final_pair_check_t(h2agg_ctx* c, const uint8_t left_aff[64], const uint8_t right_aff[64], const uint8_t s_g2[128], const uint8_t g2[128],
                       int* ok) {
    uint8_t g1s[128], g2s[256];
    memcpy(g1s, left_aff, 64);
    memcpy(g1s + 64, right_aff, 64);
    memcpy(g2s, s_g2, 128);
    memcpy(g2s + 128, g2, 128);
    std::vector<typename P::G1> ps;
    std::vector<typename P::G2> qs;
    TRY(pairing_load<P>(c, g1s, g2s, 2, ps, qs));
    P::negate(qs[1]);
    const std::shared_ptr<const typename P::Prepared> keep[2] = {P::prepared(s_g2, false, qs[0]), P::prepared(g2, true, qs[1])};
    const std::vector<const typename P::Prepared*> preps = {keep[0].get(), keep[1].get()};
    // With a pool worker already awake and waiting (h2agg_verify_aggregation wakes one while the evaluation is on the device),
    // the second pair's Miller loop runs there beside the first one's here: 64 squarings + 89 sparse products per thread
    // instead of 64 + 178 on one — the loop part of the check 0.25 -> 0.16 ms.  Without one (a busy pool: many calls in
    // flight; a direct call of this entry point) both pairs share one loop, which is less work in total.
    typename P::Gt f0, f1;
    const bool split = host_pool_pair_if_awake(
        [&] { f1 = P::miller_prepared(std::vector<typename P::G1>{ps[1]}, std::vector<const typename P::Prepared*>{preps[1]}); },
        [&] { f0 = P::miller_prepared(std::vector<typename P::G1>{ps[0]}, std::vector<const typename P::Prepared*>{preps[0]}); });
    *ok = (split ? P::check_product(f0, f1) : P::check_prepared(ps, preps)) ? 1 : 0;
    return H2AGG_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- pairing check (host)
int h2agg_pairing_product(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, uint8_t out_gt[384]) try {
    if (!out_gt) return fail(c, H2AGG_ERR_INVALID, "null buffer");
#ifdef H2AGG_PAIRING_ADX_BUILD
    if (pairing_adx_ok()) return pairing_product_t<pairing_adx::Api>(c, g1_aff, g2_aff, n, out_gt);
#endif
    return pairing_product_t<pairing::Api>(c, g1_aff, g2_aff, n, out_gt);
} API_CATCH

int h2agg_pairing_check(h2agg_ctx* c, const uint8_t* g1_aff, const uint8_t* g2_aff, size_t n, int* ok) try {
    if (!ok) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    *ok = 0;
#ifdef H2AGG_PAIRING_ADX_BUILD
    if (pairing_adx_ok()) return pairing_check_t<pairing_adx::Api>(c, g1_aff, g2_aff, n, ok);
#endif
    return pairing_check_t<pairing::Api>(c, g1_aff, g2_aff, n, ok);
} API_CATCH

// ParamsKZG's g2 / s_g2 as stored by ParamsKZG::write (fs.rs:40-55 reads them back through halo2_proofs): 64-byte
// compressed G2 points -> the 128-byte affine form the pairing entry points take
int h2agg_g2_batch_decompress(h2agg_ctx* c, const uint8_t* in, size_t n, uint8_t* out_aff) try {
    if (n && (!in || !out_aff)) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    for (size_t i = 0; i < n; ++i) {
        pairing::G2Affine q;
        const int r = pairing::g2_decompress(in + 64 * i, q);
        if (r == 1) return fail(c, H2AGG_ERR_NONCANONICAL, "G2 coordinate >= p");
        if (r) return fail(c, H2AGG_ERR_BAD_POINT, "invalid G2 point encoding (x^3 + b is not a square)");
        pairing::g2_to_bytes(q, out_aff + 128 * i);
    }
    return H2AGG_OK;
} API_CATCH

int h2agg_final_pair_check(h2agg_ctx* c, const uint8_t left_aff[64], const uint8_t right_aff[64], const uint8_t s_g2[128],
                           const uint8_t g2[128], int* ok) try {
    if (!ok || !left_aff || !right_aff || !s_g2 || !g2) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    *ok = 0;
#ifdef H2AGG_PAIRING_ADX_BUILD
    if (pairing_adx_ok()) return final_pair_check_t<pairing_adx::Api>(c, left_aff, right_aff, s_g2, g2, ok);
#endif
    return final_pair_check_t<pairing::Api>(c, left_aff, right_aff, s_g2, g2, ok);
} API_CATCH

}  // extern "C"
