// Host side of the ShaRead transcript family (halo2-snark-aggregator-api/src/transcript/sha.rs:23-127): portable SHA-256 and
// Keccak-256 (no external crypto library), the chain of a proof's squeezes over its message stream, and — for the entry point
// that runs without a device — the message stream itself: from_repr / from_xy checks and the 96- / 64-byte blocks of
// common_point / common_scalar.
//
// A proof's MESSAGE STREAM is every byte its transcript absorbs apart from the squeeze prefixes, in order; seg_end[q] is how
// many of them precede squeeze q.  Squeeze q hashes  [digest q-1, 32 bytes, if q > 0] | stream[seg_end[q-1] .. seg_end[q]) | 0x00
// (sha.rs:81-92: update(&[0]), finalize a clone, restart from the digest) and yields the digest read as a little-endian
// integer mod r (Challenge255::new = Fr::from_bytes_wide of digest | 32 zero bytes; halo2_proofs, unvendored: recalled).
// Everything in a stream is whole 32-bit words; the device keeps it word-interleaved over the 64 proofs of a wave, so the
// chain reads it through a word stride (1 for a plain stream).
#pragma once
#include <stdint.h>
#include <string.h>

namespace hash_host {

enum : int { KIND_SHA256 = 1, KIND_KECCAK256 = 2 };

struct Sha256 {
    uint32_t h[8];
    uint8_t buf[64];
    uint64_t len = 0;
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    static const uint32_t* K() {
        static const uint32_t k[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
            0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
            0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
            0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
            0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
            0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
            0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        return k;
    }
    Sha256() {
        static const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
        memcpy(h, iv, sizeof h);
    }
    void block(const uint8_t* p) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        const uint32_t* k = K();
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
        }
        h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
    }
    void update(const uint8_t* p, size_t n) {
        size_t fill = (size_t)(len & 63);
        len += n;
        while (n) {
            const size_t take = n < 64 - fill ? n : 64 - fill;
            memcpy(buf + fill, p, take);
            fill += take, p += take, n -= take;
            if (fill == 64) block(buf), fill = 0;
        }
    }
    void finalize(uint8_t out[32]) {
        const uint64_t bits = len * 8;
        const uint8_t one = 0x80, zero = 0;
        update(&one, 1);
        while ((len & 63) != 56) update(&zero, 1);
        uint8_t l[8];
        for (int i = 0; i < 8; ++i) l[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(l, 8);
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
    }
};

// Keccak[r = 1088, c = 512] with the ORIGINAL padding 0x01 .. 0x80 (sha3::Keccak256; SHA3-256 pads 0x06)
struct Keccak256 {
    uint64_t s[25];
    size_t fill = 0;   // bytes absorbed into the current 136-byte block
    Keccak256() { memset(s, 0, sizeof s); }
    static uint64_t rotl(uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; }
    static void permute(uint64_t a[25]) {
        static const int rho[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
        uint64_t rc = 1;   // the round constants from their LFSR (x^8 + x^6 + x^5 + x^4 + 1)
        uint8_t lfsr = 1;
        for (int round = 0; round < 24; ++round) {
            rc = 0;
            for (int j = 0; j < 7; ++j) {
                if (lfsr & 1) rc ^= (uint64_t)1 << ((1 << j) - 1);
                lfsr = (uint8_t)((lfsr << 1) ^ ((lfsr & 0x80) ? 0x71 : 0));
            }
            uint64_t c[5], b[25];
            for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
            for (int x = 0; x < 5; ++x) {
                const uint64_t d = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
                for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
            }
            for (int x = 0; x < 5; ++x)
                for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], rho[x + 5 * y]);
            for (int y = 0; y < 25; y += 5)
                for (int x = 0; x < 5; ++x) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
            a[0] ^= rc;
        }
    }
    void update(const uint8_t* p, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            s[fill >> 3] ^= (uint64_t)p[i] << (8 * (fill & 7));
            if (++fill == 136) permute(s), fill = 0;
        }
    }
    void finalize(uint8_t out[32]) {
        s[fill >> 3] ^= (uint64_t)0x01 << (8 * (fill & 7));
        s[16] ^= (uint64_t)0x80 << 56;
        permute(s);
        for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(s[i >> 3] >> (8 * (i & 7)));
    }
};

inline bool digest(int kind, const uint8_t* msg, size_t n, uint8_t out[32]) {
    if (kind == KIND_SHA256) {
        Sha256 d;
        d.update(msg, n);
        d.finalize(out);
    } else if (kind == KIND_KECCAK256) {
        Keccak256 d;
        d.update(msg, n);
        d.finalize(out);
    } else
        return false;
    return true;
}

// ---- 256-bit helpers (little-endian 4 x 64) -------------------------------------------------------------------------
static const uint64_t FR_MOD[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t FQ_MOD[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

inline bool geq(const uint64_t a[4], const uint64_t m[4]) {
    for (int i = 3; i >= 0; --i)
        if (a[i] != m[i]) return a[i] > m[i];
    return true;
}
inline void sub(uint64_t a[4], const uint64_t m[4]) {
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 d = (unsigned __int128)a[i] - m[i] - borrow;
        a[i] = (uint64_t)d;
        borrow = (d >> 64) & 1;
    }
}
// a digest (32 bytes, little-endian integer < 2^256 < 6 r) -> canonical bytes mod r
inline void digest_to_challenge(const uint8_t dg[32], uint8_t out[32]) {
    uint64_t w[4];
    memcpy(w, dg, 32);
    while (geq(w, FR_MOD)) sub(w, FR_MOD);
    memcpy(out, w, 32);
}
// Montgomery product mod p (CIOS), for the curve equation only
inline void fq_mont(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]) {
    static const uint64_t inv = [] {   // -p^-1 mod 2^64 by Newton
        uint64_t x = 1;
        for (int i = 0; i < 6; ++i) x *= 2 - FQ_MOD[0] * x;
        return (uint64_t)0 - x;
    }();
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) {
            c += (unsigned __int128)a[j] * b[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * inv;
        c = (unsigned __int128)m * FQ_MOD[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; ++j) {
            c += (unsigned __int128)m * FQ_MOD[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    memcpy(out, t, 32);
    if (t[4] || geq(out, FQ_MOD)) sub(out, FQ_MOD);
}
// from_repr on both coordinates and from_xy (sha.rs:44-57): canonical, on y^2 = x^3 + 3, not (0, 0)
inline bool point_ok(const uint8_t xy[64]) {
    uint64_t x[4], y[4];
    memcpy(x, xy, 32);
    memcpy(y, xy + 32, 32);
    if (geq(x, FQ_MOD) || geq(y, FQ_MOD)) return false;
    // with mont(a, b) = a b / R:  y^2 / R^2  ==  x^3 / R^2 + 3 / R^2
    const uint64_t one[4] = {1, 0, 0, 0}, three[4] = {3, 0, 0, 0};
    uint64_t l[4], r[4], c[4];
    fq_mont(y, y, l);
    fq_mont(l, one, l);
    fq_mont(x, x, r);
    fq_mont(r, x, r);
    fq_mont(three, one, c);
    fq_mont(c, one, c);
    unsigned __int128 carry = 0;
    for (int i = 0; i < 4; ++i) {
        carry += (unsigned __int128)r[i] + c[i];
        r[i] = (uint64_t)carry;
        carry >>= 64;
    }
    if (carry || geq(r, FQ_MOD)) sub(r, FQ_MOD);
    return memcmp(l, r, 32) == 0;   // ((0, 0): 0 != 3)
}
inline void put_be(uint8_t* dst, const uint8_t le[32]) {
    for (int i = 0; i < 32; ++i) dst[i] = le[31 - i];
}
// common_point (sha.rs:94-112): 31 zero bytes, 0x01, x and y big-endian
inline void block_point(uint8_t dst[96], const uint8_t xy[64]) {
    memset(dst, 0, 32);
    dst[31] = 1;
    put_be(dst + 32, xy);
    put_be(dst + 64, xy + 32);
}
// common_scalar (sha.rs:114-126): 31 zero bytes, 0x02, the scalar big-endian
inline void block_scalar(uint8_t dst[64], const uint8_t s[32]) {
    memset(dst, 0, 32);
    dst[31] = 2;
    put_be(dst + 32, s);
}
inline bool scalar_ok(const uint8_t s[32]) {
    uint64_t w[4];
    memcpy(w, s, 32);
    return !geq(w, FR_MOD);
}

// the squeezes of ONE proof: msg = its message stream as 32-bit words, word w at msg[w * word_stride]; seg_end in BYTES
template <class D>
inline void chain_run_t(const uint32_t* msg, size_t word_stride, const uint32_t* seg_end, uint32_t nsq, uint8_t* out /* [nsq][32] */) {
    uint8_t dg[32];
    uint32_t pos = 0;
    for (uint32_t q = 0; q < nsq; ++q) {
        D d;
        if (q) d.update(dg, 32);
        for (; pos < seg_end[q]; pos += 4) {
            const uint32_t w = msg[(size_t)(pos >> 2) * word_stride];
            d.update((const uint8_t*)&w, 4);
        }
        const uint8_t zero = 0;
        d.update(&zero, 1);
        d.finalize(dg);
        digest_to_challenge(dg, out + 32 * (size_t)q);
    }
}
inline void chain_run(int kind, const uint32_t* msg, size_t word_stride, const uint32_t* seg_end, uint32_t nsq, uint8_t* out) {
    if (kind == KIND_SHA256) chain_run_t<Sha256>(msg, word_stride, seg_end, nsq, out);
    else chain_run_t<Keccak256>(msg, word_stride, seg_end, nsq, out);
}

}  // namespace hash_host
