// Device side of the ShaRead transcript family (halo2-snark-aggregator-api/src/transcript/sha.rs:23-127):
// the proofs of one circuit, batched — SHA-256 (the outer proof as verify_circuit.rs:985,1032-1055 writes and checks it) or
// Keccak-256 (solidity/src/transcript/codegen.rs:34,196-214).  Two kernels, as on the Poseidon side:
//   k_hash_transcript_stream   one lane per (proof, item): from_repr / from_xy checks (sha.rs:44-57,63-71), the canonical
//                              points, and the item's 96- / 64-byte block of common_point / common_scalar (sha.rs:94-126)
//                              at its place in the proof's message stream;
//   k_hash_transcript_chain    one lane per proof: the chain of squeezes (sha.rs:81-92) over that stream, state in registers.
// A proof's message stream is every byte its transcript absorbs apart from the squeeze prefixes.  It is kept as 32-bit words
// (every block is a multiple of 32 bytes), WORD-INTERLEAVED over the 64 proofs of a wave: word w of proof p sits at
// ((p / 64) * nwords + w) * 64 + p % 64, so the chain's lanes read one 256-byte line per word and the stream kernel's lanes
// (consecutive lanes = consecutive proofs of one item) write one.
#pragma once
#include "poseidon_kernels.hpp"   // TrItem, TR_*

namespace h2agg {

constexpr int HT_LANES = 64;   // proofs per interleaving group = one wave of the chain kernel
enum : int { HT_SHA256 = 1, HT_KECCAK256 = 2 };

FP_INLINE size_t ht_word_at(uint32_t p, uint32_t w, uint32_t nwords) {
    return ((size_t)(p / HT_LANES) * nwords + w) * HT_LANES + (p % HT_LANES);
}
// bytes 0..31 of a block: 31 zero bytes and the prefix; then `v` (little-endian limbs) as 32 big-endian bytes
FP_INLINE void ht_put_prefix(uint32_t* __restrict__ msg, uint32_t p, uint32_t w0, uint32_t nwords, uint32_t prefix) {
#pragma unroll
    for (int i = 0; i < 7; ++i) msg[ht_word_at(p, w0 + i, nwords)] = 0;
    msg[ht_word_at(p, w0 + 7, nwords)] = prefix << 24;   // byte 31
}
FP_INLINE void ht_put_be(uint32_t* __restrict__ msg, uint32_t p, uint32_t w0, uint32_t nwords, const U256& v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) msg[ht_word_at(p, w0 + i, nwords)] = __builtin_bswap32(v.w[7 - i]);
}
FP_INLINE bool ht_on_curve(const Fq& x, const Fq& y) {   // canonical x, y: y^2 == x^3 + 3  ((0, 0) is not)
    const Fq xm = fp_to_mont<FqParams>(x), ym = fp_to_mont<FqParams>(y);
    Fq three;
#pragma unroll
    for (int k = 0; k < NL; ++k) three.l[k] = 0;
    three.l[0] = 3;
    const Fq rhs = FQ_ADD(FQ_MUL(FQ_SQR(xm), xm), fp_to_mont<FqParams>(three));
    return fp_is_zero_mod<8, FqParams>(FQ_SUB(4, FQ_SQR(ym), rhs));
}

// items[].src: byte offset inside the proof (points are 64 bytes here: x | y uncompressed, sha.rs:53-54) / constant index /
// external point index; items[].dst: first WORD of the item's block in the message stream.  `which` as k_transcript_elements.
__global__ void __launch_bounds__(BLOCK) k_hash_transcript_stream(const uint8_t* __restrict__ proofs, size_t proof_stride,
                                                                  const uint8_t* __restrict__ ext_points, uint32_t n_ext,
                                                                  const uint8_t* __restrict__ consts,
                                                                  const TrItem* __restrict__ items, uint32_t nitems,
                                                                  uint32_t nproofs, uint32_t npoints,
                                                                  uint8_t* __restrict__ points_out /* [proof][npoints][64] */,
                                                                  uint32_t* __restrict__ msg, uint32_t nwords, uint32_t* flags,
                                                                  int which) {
    const size_t total = (size_t)nproofs * nitems;
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (size_t)gridDim.x * BLOCK) {
        const uint32_t p = (uint32_t)(t % nproofs);   // consecutive lanes: consecutive proofs, one item
        const TrItem it = items[t / nproofs];
        if ((which == 1 && it.kind == TR_POINT_EXT) || (which == 2 && it.kind != TR_POINT_EXT)) continue;
        if (it.kind == TR_CONST || it.kind == TR_SCALAR) {
            const U256 s = u256_load(it.kind == TR_CONST ? consts + 32 * (size_t)it.src : proofs + (size_t)p * proof_stride + it.src);
            if (!u256_is_canonical_fr(s)) atomicOr(flags, FLAG_NONCANONICAL);   // "invalid field element encoding in proof"
            ht_put_prefix(msg, p, it.dst, nwords, 2u);
            ht_put_be(msg, p, it.dst + 8, nwords, s);
        } else {
            const uint8_t* src = it.kind == TR_POINT_EXT ? ext_points + 64 * ((size_t)p * n_ext + it.src)
                                                         : proofs + (size_t)p * proof_stride + it.src;
            const U256 xw = u256_load(src), yw = u256_load(src + 32);
            const Fq x = fp_unpack<FqParams>(xw.w), y = fp_unpack<FqParams>(yw.w);
            // "invalid base encoding" / "invalid point encoding" / "cannot write points at infinity to the transcript"
            const bool good = fp_is_canonical<FqParams>(x) && fp_is_canonical<FqParams>(y) && ht_on_curve(x, y);
            if (!good) atomicOr(flags, FLAG_BAD_POINT);
            if (it.kind == TR_POINT) {
                uint4* po = reinterpret_cast<uint4*>(points_out + 64 * ((size_t)p * npoints + it.pidx));
                const uint4 z = make_uint4(0, 0, 0, 0);
                po[0] = good ? make_uint4(xw.w[0], xw.w[1], xw.w[2], xw.w[3]) : z;
                po[1] = good ? make_uint4(xw.w[4], xw.w[5], xw.w[6], xw.w[7]) : z;
                po[2] = good ? make_uint4(yw.w[0], yw.w[1], yw.w[2], yw.w[3]) : z;
                po[3] = good ? make_uint4(yw.w[4], yw.w[5], yw.w[6], yw.w[7]) : z;
            }
            ht_put_prefix(msg, p, it.dst, nwords, 1u);
            ht_put_be(msg, p, it.dst + 8, nwords, xw);
            ht_put_be(msg, p, it.dst + 16, nwords, yw);
        }
    }
}

// ---- SHA-256 (FIPS 180-4), one block: rolling 16-word schedule, every round unrolled (all indices compile-time) --------
FP_INLINE uint32_t ht_rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
FP_INLINE void sha256_block(uint32_t (&h)[8], uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = h[i];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (ht_rotr(w15, 7) ^ ht_rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (ht_rotr(w2, 17) ^ ht_rotr(w2, 19) ^ (w2 >> 10));
        }
        // the working variables a .. h are s[(0 - i) & 7] .. s[(7 - i) & 7]: renamed per round instead of moved
        const uint32_t a = s[(0 - i) & 7], b = s[(1 - i) & 7], c = s[(2 - i) & 7], e = s[(4 - i) & 7], f = s[(5 - i) & 7], g = s[(6 - i) & 7];
        const uint32_t t1 = s[(7 - i) & 7] + (ht_rotr(e, 6) ^ ht_rotr(e, 11) ^ ht_rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const uint32_t t2 = (ht_rotr(a, 2) ^ ht_rotr(a, 13) ^ ht_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        s[(3 - i) & 7] += t1;        // d + t1 is the next round's e
        s[(7 - i) & 7] = t1 + t2;    // the next round's a
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] += s[i];
}

// ---- Keccak-f[1600]: 25 lanes in registers; a round's indices are compile-time, the 24 rounds are a loop (the round constant
// is a wave-uniform load; unrolling them as well makes ~15 k instructions per call site for no shorter dependency chain) ----
__device__ const uint64_t HT_KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
template <int N>
FP_INLINE uint64_t ht_rotl64(uint64_t x) {
    if constexpr (N == 0) return x;
    else return (x << N) | (x >> (64 - N));
}
FP_INLINE void keccak_f1600(uint64_t (&a)[25]) {
#pragma unroll 1
    for (int round = 0; round < 24; ++round) {
        uint64_t c[5];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const uint64_t d = c[(x + 4) % 5] ^ ht_rotl64<1>(c[(x + 1) % 5]);
#pragma unroll
            for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
        }
        uint64_t b[25];   // rho + pi: b[y + 5 ((2x + 3y) % 5)] = rotl(a[x + 5y], rho[x + 5y])
        b[0] = a[0];
        b[10] = ht_rotl64<1>(a[1]);
        b[20] = ht_rotl64<62>(a[2]);
        b[5] = ht_rotl64<28>(a[3]);
        b[15] = ht_rotl64<27>(a[4]);
        b[16] = ht_rotl64<36>(a[5]);
        b[1] = ht_rotl64<44>(a[6]);
        b[11] = ht_rotl64<6>(a[7]);
        b[21] = ht_rotl64<55>(a[8]);
        b[6] = ht_rotl64<20>(a[9]);
        b[7] = ht_rotl64<3>(a[10]);
        b[17] = ht_rotl64<10>(a[11]);
        b[2] = ht_rotl64<43>(a[12]);
        b[12] = ht_rotl64<25>(a[13]);
        b[22] = ht_rotl64<39>(a[14]);
        b[23] = ht_rotl64<41>(a[15]);
        b[8] = ht_rotl64<45>(a[16]);
        b[18] = ht_rotl64<15>(a[17]);
        b[3] = ht_rotl64<21>(a[18]);
        b[13] = ht_rotl64<8>(a[19]);
        b[14] = ht_rotl64<18>(a[20]);
        b[24] = ht_rotl64<2>(a[21]);
        b[9] = ht_rotl64<61>(a[22]);
        b[19] = ht_rotl64<56>(a[23]);
        b[4] = ht_rotl64<14>(a[24]);
#pragma unroll
        for (int y = 0; y < 25; y += 5)
#pragma unroll
            for (int x = 0; x < 5; ++x) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        a[0] ^= HT_KECCAK_RC[round];
    }
}

// the digest as a little-endian integer (< 2^256 < 6 r) -> canonical mod r: five conditional subtractions
FP_INLINE void ht_reduce_mod_r(uint32_t (&v)[8]) {
    constexpr uint32_t RW[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t d[8];
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t t = (uint64_t)v[i] - RW[i] - borrow;
            d[i] = (uint32_t)t;
            borrow = (uint32_t)(t >> 63);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = borrow ? v[i] : d[i];
    }
}
FP_INLINE void ht_store_challenge(uint8_t* out, const uint32_t (&v)[8]) {
    uint4* o = reinterpret_cast<uint4*>(out);
    o[0] = make_uint4(v[0], v[1], v[2], v[3]);
    o[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// One lane per proof, one wave per workgroup.  seg_end[q]: words of the message stream in front of squeeze q.  Squeeze q hashes
// [digest q-1 | stream words seg_end[q-1] .. seg_end[q] | 0x00], stores the digest mod r at chal[p][q] (the layout of the
// Poseidon path: everything downstream is shared) and restarts the state from the raw digest.  The script is the same for
// every proof, so all control flow here is wave-uniform.  msg is padded to whole groups of 64 proofs: the lanes past nproofs
// read words of their own (never stored).
template <int KIND>
__global__ void __launch_bounds__(HT_LANES) k_hash_transcript_chain(const uint32_t* __restrict__ msg, uint32_t nwords,
                                                                    const uint32_t* __restrict__ seg_end, uint32_t nsq,
                                                                    uint32_t nproofs, uint8_t* __restrict__ chal) {
    const uint32_t p = blockIdx.x * HT_LANES + threadIdx.x;
    const uint32_t* my = msg + (size_t)blockIdx.x * nwords * HT_LANES + threadIdx.x;   // word w: my[w * HT_LANES]
    uint32_t pos = 0;
    if constexpr (KIND == HT_SHA256) {
        uint32_t dg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t q = 0; q < nsq; ++q) {
            uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
            uint32_t w[16];
            // blocks are two 32-byte halves; `half`: w[0..7] holds the first one
            bool half = q != 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = dg[i];
            const uint32_t end = seg_end[q];
            const uint32_t nbytes = (q ? 32u : 0u) + 4u * (end - pos) + 1u;
#pragma unroll 1
            for (; pos < end; pos += 8) {
                uint32_t c[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) c[i] = __builtin_bswap32(my[(size_t)(pos + i) * HT_LANES]);
                if (!half) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = c[i];
                    half = true;
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[8 + i] = c[i];
                    sha256_block(h, w);
                    half = false;
                }
            }
            // the squeeze prefix 0x00, the padding bit, the length: they always fit the open block
            if (!half) {
#pragma unroll
                for (int i = 0; i < 8; ++i) w[i] = 0;
                w[0] = 0x00800000u;
            }
            w[8] = half ? 0x00800000u : 0u;
#pragma unroll
            for (int i = 9; i < 15; ++i) w[i] = 0;
            w[15] = nbytes * 8u;
            sha256_block(h, w);
#pragma unroll
            for (int i = 0; i < 8; ++i) dg[i] = h[i];   // (big-endian words of the digest: the next state's first half block)
            uint32_t v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = __builtin_bswap32(h[i]);
            ht_reduce_mod_r(v);
            if (p < nproofs) ht_store_challenge(chal + 32 * ((size_t)p * nsq + q), v);
        }
    } else {
        uint64_t dg[4] = {0, 0, 0, 0};
        for (uint32_t q = 0; q < nsq; ++q) {
            uint64_t a[25];
#pragma unroll
            for (int i = 0; i < 25; ++i) a[i] = 0;
            uint32_t lane = 0;   // 64-bit lanes of the 17-lane (136-byte) block absorbed so far
            if (q) {
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = dg[i];
                lane = 4;
            }
            const uint32_t end = seg_end[q];
#pragma unroll 1
            for (; pos < end; pos += 2) {
                const uint64_t v = (uint64_t)my[(size_t)pos * HT_LANES] | ((uint64_t)my[(size_t)(pos + 1) * HT_LANES] << 32);
#pragma unroll
                for (int i = 0; i < 17; ++i) a[i] ^= (i == (int)lane) ? v : 0ull;   // (a select per lane: no dynamic register index)
                if (++lane == 17) {
                    keccak_f1600(a);
                    lane = 0;
                }
            }
            // the squeeze prefix 0x00 then the padding 0x01 .. 0x80 (the original Keccak padding, not SHA-3's 0x06)
#pragma unroll
            for (int i = 0; i < 17; ++i) a[i] ^= (i == (int)lane) ? 0x0100ull : 0ull;
            a[16] ^= 0x8000000000000000ull;
            keccak_f1600(a);
            uint32_t v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dg[i] = a[i];
                v[2 * i] = (uint32_t)a[i];
                v[2 * i + 1] = (uint32_t)(a[i] >> 32);
            }
            ht_reduce_mod_r(v);
            if (p < nproofs) ht_store_challenge(chal + 32 * ((size_t)p * nsq + q), v);
        }
    }
}

}  // namespace h2agg
