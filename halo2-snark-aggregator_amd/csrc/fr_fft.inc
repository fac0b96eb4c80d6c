// Fourier transform over Fr, host side (included into h2agg.hip: shares the context internals; kernels and the pass plan in
// fr_fft_kernels.hpp, field constants and checks in fr_host.inc, staging in host.inc): h2agg_fr_fft, h2agg_fr_fft_device, h2agg_fr_fft_batch.  They stand for
// halo2_proofs' best_fft and EvaluationDomain::{lagrange_to_coeff, coeff_to_lagrange, coeff_to_extended, extended_to_coeff} —
// an unvendored git dependency of the reference, recalled from upstream (DESIGN.md section 2); the yardstick is the definition
// in include/h2agg.h.

namespace {

// d_out[i] = (base^i in the device's Montgomery form), i < n <= 2^12; queued on the context's stream, constants by value.
// plain: base^i as a canonical integer instead (k_fr_powers' A = 1: csrc/keygen_kernels.hpp multiplies by such a table).
void fr_powers_launch(h2agg_ctx* c, ph::HFr base, uint32_t n, uint8_t* d_out, bool plain = false) {
    FrPowersArgs args;
    for (int j = 0; j < FRW_TABLE; ++j) {
        hfr_words(base, args.pw[j]);
        base = ph::mul(base, base);
    }
    hfr_words(plain ? ph::one() : fr_radix(), args.a);
    const uint32_t threads = (n + FRP_CHUNK - 1) / FRP_CHUNK;
    hipLaunchKernelGGL(k_fr_powers, dim3((threads + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, args, n, d_out);
}

// the two-level table of base^e, e < 2^bits: lo[i] = base^i, i < 2^T, then hi[i] = base^(i * 2^T), i < 2^(bits - T), T = ceil(bits / 2)
unsigned fr_table_split(unsigned bits) { return (bits + 1) / 2; }
size_t fr_table_bytes(unsigned bits) { return 32 * (((size_t)1 << fr_table_split(bits)) + ((size_t)1 << (bits - fr_table_split(bits)))); }
void fr_table_launch(h2agg_ctx* c, const ph::HFr& base, unsigned bits, uint8_t* d_tab) {
    const unsigned T = fr_table_split(bits);
    fr_powers_launch(c, base, 1u << T, d_tab);
    ph::HFr hb = base;
    for (unsigned i = 0; i < T; ++i) hb = ph::mul(hb, hb);
    fr_powers_launch(c, hb, 1u << (bits - T), d_tab + ((size_t)32 << T));
}

// twiddle tables of w_K (inverse: w_K^-1) for the largest K asked for so far, resident in the context
int fr_fft_ensure_twiddles(h2agg_ctx* c, unsigned k, int inv) {
    if (c->frfft_tw_k[inv] >= (int)k) return H2AGG_OK;
    c->frfft_tw_k[inv] = -1;
    TRY(ensure(c, c->frfft_tw[inv], fr_table_bytes(k)));   // (a replaced buffer: ensure() drains the device first)
    const ph::HFr w = fft_omega(k);
    fr_table_launch(c, inv ? ph::inv(w) : w, k, (uint8_t*)c->frfft_tw[inv].p);
    c->frfft_tw_k[inv] = (int)k;
    return H2AGG_OK;
}

// A contiguous slab of `cols` columns, stride 2^k elements: one source of a batch
struct FrFftSeg {
    const uint8_t* base;
    size_t cols;
};

// the work array a batch of m columns of 2^k asks for: the whole batch up to 2^FR_FFT_BATCH_WORK_LOG elements, and one column
// whatever its size.  (The buffer only grows: what an earlier caller ensured stays the floor.)
size_t fr_fft_batch_work_bytes(size_t m, unsigned k) {
    const size_t column = (size_t)1 << k, budget = (size_t)1 << FR_FFT_BATCH_WORK_LOG;
    const size_t all = m > budget >> k ? budget : m * column;   // min(m 2^k, budget) without overflow
    return 32 * std::max(column, all);
}

// Queues the transforms of the m columns that `segs` lists, in order, into the slab d_out[m][2^k] on the context's stream (no
// synchronisation unless a workspace has to grow).  The batch runs in chunks of B columns, every pass of a chunk being one
// launch: B = the columns the work array holds (a transform of one pass needs no work array), or the debug key
// fr_fft_batch_chunk.  d_out may be the one segment's base: a chunk's first pass has read its columns into the work array
// before its last pass writes them, and a single-pass workgroup holds whole transforms.
// shift: null, or the checked non-zero shift; its table is built once, for all columns.
int fr_fft_queue_batch(h2agg_ctx* c, const FrFftSeg* segs, size_t nseg, size_t m, unsigned k, int inv, const ph::HFr* shift,
                       uint8_t* d_out) {
    const unsigned L = c->dbg_fr_fft_local ? (unsigned)c->dbg_fr_fft_local : FR_FFT_LOCAL;
    const unsigned P = k ? (k + L - 1) / L : 1;
    {
        size_t cols = 0;
        for (size_t g = 0; g < nseg; ++g) cols += segs[g].cols;
        if (nseg > (size_t)FR_FFT_SEGS || cols != m) return fail(c, H2AGG_ERR_INVALID, "fr_fft: the source slabs do not make up the batch");
    }
    if (P > 1) TRY(ensure(c, c->frfft_work, fr_fft_batch_work_bytes(m, k)));
    if (k) TRY(fr_fft_ensure_twiddles(c, k, inv));
    if (shift) {
        TRY(ensure(c, c->frfft_shift, fr_table_bytes(k)));
        fr_table_launch(c, inv ? ph::inv(*shift) : *shift, k, (uint8_t*)c->frfft_shift.p);
    }
    FrFftPass p = {};
    const unsigned K = k ? (unsigned)c->frfft_tw_k[inv] : 0;
    p.tw_T = fr_table_split(K);
    p.tw_lo = (const uint8_t*)c->frfft_tw[inv].p;
    p.tw_hi = p.tw_lo + ((size_t)32 << p.tw_T);
    p.tw_up = K - k;
    if (shift) {
        p.sh_T = fr_table_split(k);
        p.sh_lo = (const uint8_t*)c->frfft_shift.p;
        p.sh_hi = p.sh_lo + ((size_t)32 << p.sh_T);
    }
    p.flags = c->d_flags;
    p.k = k;
    p.local = L;
    p.digits = P - 1;
    {   // x -> x R [/ n]: the first pass multiplies by R^2 [/ n]
        ph::HFr cv = ph::mul(fr_radix(), fr_radix());
        if (inv) cv = ph::mul(cv, ph::inv(hfr_u64((uint64_t)1 << k)));
        uint32_t w[8];
        hfr_words(cv, w);
        for (int i = 0; i < NL; ++i) {
            const int bit = 29 * i;
            uint64_t v = w[bit / 32];
            if (bit / 32 + 1 < 8) v |= (uint64_t)w[bit / 32 + 1] << 32;
            p.cvt[i] = (uint32_t)(v >> (bit % 32)) & ((1u << 29) - 1u);
        }
    }
    const size_t col = (size_t)32 << k;
    size_t B = P > 1 ? std::max<size_t>(1, (c->frfft_work.cap / 32) >> k) : m;
    if (c->dbg_fr_fft_batch_chunk) B = std::min(B, (size_t)c->dbg_fr_fft_batch_chunk);   // (never more than the work array holds)
    B = std::min(B, (size_t)1 << (31 - k));   // a launch's tiles, at most B 2^k, index with 32 bits
    for (size_t c0 = 0; c0 < m; c0 += B) {
        const size_t b = std::min(B, m - c0);
        // the chunk's columns [c0, c0 + b) as a segment table of its own
        int used = 0;
        size_t start = 0;
        for (size_t g = 0; g < nseg; start += segs[g].cols, ++g) {
            const size_t lo = std::max(start, c0), hi = std::min(start + segs[g].cols, c0 + b);
            if (lo >= hi) continue;
            p.seg_base[used] = segs[g].base + (lo - start) * col;
            p.seg_first[used] = (uint32_t)(lo - c0);
            ++used;
        }
        for (int g = used; g < FR_FFT_SEGS; ++g) {
            p.seg_base[g] = nullptr;
            p.seg_first[g] = ~0u;
        }
        p.m = (uint32_t)b;
        for (unsigned q = 0; q < P; ++q) {
            p.first = q == 0;
            p.last = q + 1 == P;
            p.width = p.last ? k - (P - 1) * L : L;
            p.hb = q * L;
            p.lb = k - p.hb - p.width;
            if (!p.first) {   // the work array: one slab
                p.seg_base[0] = (const uint8_t*)c->frfft_work.p;
                for (int g = 1; g < FR_FFT_SEGS; ++g) p.seg_first[g] = ~0u;
            }
            p.dst = p.last ? d_out + c0 * col : (uint8_t*)c->frfft_work.p;
            p.sh_first = shift && !inv && p.first;
            p.sh_last = shift && inv && p.last;
            const size_t tiles = b << (k - p.width), per = FR_FFT_TILE >> p.width;
            assert(tiles <= 0xffffffffu);
            hipLaunchKernelGGL(k_fr_fft_pass, dim3((unsigned)((tiles + per - 1) / per)), dim3(FR_FFT_THREADS), 0, c->stream, p);
        }
    }
    HIP_TRY(c, hipGetLastError());
    return H2AGG_OK;
}

// the batch of one
int fr_fft_queue(h2agg_ctx* c, const uint8_t* d_in, unsigned k, int inv, const ph::HFr* shift, uint8_t* d_out) {
    const FrFftSeg seg = {d_in, 1};
    return fr_fft_queue_batch(c, &seg, 1, 1, k, inv, shift, d_out);
}

// k, shift -> refusals; *has: a shift other than null
int fr_fft_check(h2agg_ctx* c, unsigned k, const uint8_t* shift, ph::HFr* s) {
    TRY(fr_check_k(c, k));
    if (!shift) return H2AGG_OK;
    TRY(fr_parse(c, shift, s));
    if (ph::is_zero(*s)) return fail(c, H2AGG_ERR_INVALID, "fr_fft: shift == 0 (the inverse transform divides by shift^j)");
    return H2AGG_OK;
}

}  // namespace

extern "C" {

int h2agg_fr_fft_device(h2agg_ctx* c, const void* d_in, unsigned k, int inverse, const uint8_t shift[32], void* d_out) try {
    TRY(bind(c));
    if (!d_in || !d_out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr s;
    TRY(fr_fft_check(c, k, shift, &s));
    return fr_fft_queue(c, (const uint8_t*)d_in, k, inverse ? 1 : 0, shift ? &s : nullptr, (uint8_t*)d_out);
} API_CATCH

int h2agg_fr_fft(h2agg_ctx* c, const uint8_t* in, unsigned k, int inverse, const uint8_t shift[32], uint8_t* out) try {
    TRY(bind(c));
    if (!in || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    ph::HFr s;
    TRY(fr_fft_check(c, k, shift, &s));
    const size_t bytes = (size_t)32 << k;
    TRY(ensure(c, c->in_a, bytes));
    TRY(stage_in(c, c->in_a, in, bytes));
    TRY(clear_flags(c));
    TRY(fr_fft_queue(c, (const uint8_t*)c->in_a.p, k, inverse ? 1 : 0, shift ? &s : nullptr, (uint8_t*)c->in_a.p));
    return stage_out(c, out, c->in_a.p, bytes);
} API_CATCH

int h2agg_fr_fft_batch(h2agg_ctx* c, const uint8_t* in, size_t m, unsigned k, int inverse, const uint8_t shift[32],
                       uint8_t* out) try {
    TRY(bind(c));
    if (!in || !out) return fail(c, H2AGG_ERR_INVALID, "null buffer");
    if (m == 0) return fail(c, H2AGG_ERR_INVALID, "fr_fft_batch: m == 0");
    ph::HFr s;
    TRY(fr_fft_check(c, k, shift, &s));
    if (m > (SIZE_MAX >> 1) / ((size_t)32 << k)) return fail(c, H2AGG_ERR_NOMEM, "fr_fft_batch: the slab does not fit the address space");
    const size_t bytes = m * ((size_t)32 << k);
    TRY(ensure(c, c->in_a, bytes));
    TRY(stage_in(c, c->in_a, in, bytes));
    TRY(clear_flags(c));
    const FrFftSeg seg = {(const uint8_t*)c->in_a.p, m};
    TRY(fr_fft_queue_batch(c, &seg, 1, m, k, inverse ? 1 : 0, shift ? &s : nullptr, (uint8_t*)c->in_a.p));
    return stage_out(c, out, c->in_a.p, bytes);
} API_CATCH

}  // extern "C"
