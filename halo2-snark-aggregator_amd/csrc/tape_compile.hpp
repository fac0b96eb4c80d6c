// The Fr tape's host half: its encoding (shared with the kernels of schema.hpp) and the compilation of a recorded tape into
// what those kernels run — dependency levels, and the liveness allocation of the LDS register file.  Plain C++17, no HIP: the
// CPU test (tests/cpp/tape_lds_driver.cpp) includes this file as it stands.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace h2agg {

enum : uint32_t { TAPE_MUL = 0, TAPE_ADD = 1, TAPE_SUB = 2, TAPE_INV = 3,     // INV: dst = 1 / a (b unused); 1 / 0 raises FLAG_DIV_ZERO
                  TAPE_SQRN = 4 };   // dst = a^(2^b), b an IMMEDIATE count (not a register): `pow_constant(x, n)` for n = 2^k
                                     // (verify.rs:498) as ONE operation — k dependent squarings are k levels of the tape otherwise,
                                     // each a round trip through the register file; recorded by the verifier pipeline only
struct TapeOp {
    uint32_t dst, a, b, op;
};

// k_tape_run_lds's encoding (schema.hpp):
//   op.a / op.b:  bit 31 set: LDS slot (low bits); clear: never happens for a register operand (constants have slots too)
//   op.op:        opcode | (LDS slot of the result, or TAPE_NOSLOT when nothing in the tape reads it) << 8
constexpr uint32_t TAPE_LDS_SLOTS = 4096;          // x 36 B = 144 KiB of the CU's 160
constexpr uint32_t TAPE_NOSLOT = 0xffffffu;
constexpr uint32_t TAPE_SLOTBIT = 0x80000000u;

// Dependency levels of a tape (operands precede results): ops sorted by level, lstart[l] .. lstart[l + 1] = the ops of
// level l + 1.  Returns false if an operand is not defined before its use.
inline bool schedule_levels(const std::vector<TapeOp>& ops, uint32_t nreg, std::vector<TapeOp>& sorted,
                            std::vector<uint32_t>& lstart, uint32_t& maxlevel) {
    const uint32_t nops = (uint32_t)ops.size();
    std::vector<uint32_t> level(nreg, 0);
    maxlevel = 0;
    // An inversion level costs a whole safegcd (~13 k instructions of one wave's latency) however many inversions share it
    // (every lane of the level inverts its own operand, in lock step: no batching trick, and none needed): put EVERY inversion
    // on the level of the latest one.  First pass: as soon as possible; second pass: the same with the inversions held back
    // to that level.
    uint32_t inv_level = 0;
    for (int pass = 0; pass < 2; ++pass) {
        maxlevel = 0;
        uint32_t latest_inv = 0;
        for (uint32_t k = 0; k < nops; ++k) {
            const TapeOp& o = ops[k];
            const bool imm_b = o.op == TAPE_SQRN;   // b = number of squarings (<= 255), not an operand
            if (o.dst >= nreg || o.a >= o.dst || (imm_b ? o.b > 255u : o.b >= o.dst)) return false;
            const uint32_t lb = imm_b ? 0u : level[o.b];
            uint32_t lv = 1 + (level[o.a] > lb ? level[o.a] : lb);
            if (o.op == TAPE_INV) {
                if (lv > latest_inv) latest_inv = lv;
                if (pass == 1 && lv < inv_level) lv = inv_level;
            }
            level[o.dst] = lv;
            if (lv > maxlevel) maxlevel = lv;
        }
        if (pass == 0) {
            if (latest_inv == 0) break;   // no inversions: the first pass is final
            inv_level = latest_inv;
            std::fill(level.begin(), level.end(), 0u);
        }
    }
    std::vector<uint32_t> start(maxlevel + 2, 0);
    for (uint32_t k = 0; k < nops; ++k) start[level[ops[k].dst] + 1]++;
    for (uint32_t l = 1; l <= maxlevel + 1; ++l) start[l] += start[l - 1];
    std::vector<uint32_t> cur(start.begin(), start.end());
    sorted.resize(nops);
    for (uint32_t k = 0; k < nops; ++k) sorted[cur[level[ops[k].dst]]++] = ops[k];
    lstart.assign(start.begin() + 1, start.end());
    return true;
}

// Liveness allocation of the tape's values to the LDS register file of k_tape_run_lds (schema.hpp).  `sorted` / `lstart` come
// from schedule_levels; a value is live from the level that makes it (constants: from the start) to the last level that reads
// it, and its slot is handed out again one level later (inside a level one lane may still be reading what another would
// overwrite).  Values nothing in the tape reads get no slot.  On success `sorted` is rewritten in the kernel's encoding and
// cslot[i] is constant i's slot; false (nothing touched): more than TAPE_LDS_SLOTS values are live at some level.
inline bool tape_lds_assign(std::vector<TapeOp>& sorted, const std::vector<uint32_t>& lstart, uint32_t nconst, uint32_t nreg,
                            std::vector<uint32_t>& cslot, uint32_t* peak_out = nullptr) {
    const uint32_t nlevels = lstart.empty() ? 0 : (uint32_t)lstart.size() - 1;
    std::vector<uint32_t> last(nreg, 0), slot(nreg, TAPE_NOSLOT);   // last[r]: last level (1-based) that reads register r
    for (uint32_t l = 0; l < nlevels; ++l)
        for (uint32_t k = lstart[l]; k < lstart[l + 1]; ++k) {
            const TapeOp& o = sorted[k];
            last[o.a] = l + 1;
            if (o.op != TAPE_SQRN) last[o.b] = l + 1;
        }
    // values to release after each level, as lists threaded through `next_dead`
    std::vector<uint32_t> dead_head(nlevels + 2, 0xffffffffu), next_dead(nreg, 0xffffffffu);
    auto retire_at = [&](uint32_t r) {
        next_dead[r] = dead_head[last[r]];
        dead_head[last[r]] = r;
    };
    std::vector<uint32_t> free_slots;
    uint32_t fresh = 0, peak = 0, live = 0;
    auto take = [&]() -> uint32_t {
        ++live;
        if (live > peak) peak = live;
        if (!free_slots.empty()) {
            const uint32_t sl = free_slots.back();
            free_slots.pop_back();
            return sl;
        }
        return fresh++;
    };
    for (uint32_t r = 0; r < nconst; ++r)
        if (last[r]) {
            slot[r] = take();
            retire_at(r);
        }
    bool fits = fresh <= TAPE_LDS_SLOTS;
    for (uint32_t l = 0; l < nlevels && fits; ++l) {
        for (uint32_t k = lstart[l]; k < lstart[l + 1]; ++k) {
            const uint32_t d = sorted[k].dst;
            if (!last[d]) continue;
            slot[d] = take();
            retire_at(d);
        }
        fits = fresh <= TAPE_LDS_SLOTS;
        for (uint32_t r = dead_head[l + 1]; r != 0xffffffffu; r = next_dead[r]) {   // read for the last time in this level
            free_slots.push_back(slot[r]);
            --live;
        }
    }
    if (peak_out) *peak_out = peak;
    if (!fits) return false;
    for (TapeOp& o : sorted) {
        o.op = (o.op & 0xffu) | (slot[o.dst] << 8);
        o.a = slot[o.a] | TAPE_SLOTBIT;
        if ((o.op & 0xffu) != TAPE_SQRN) o.b = slot[o.b] | TAPE_SLOTBIT;
    }
    cslot.assign(slot.begin(), slot.begin() + nconst);
    return true;
}

// A tape as the device runs it.
struct CompiledTape {
    std::vector<TapeOp> sorted;      // by dependency level; in k_tape_run_lds's encoding when `lds`
    std::vector<uint32_t> lstart;    // lstart[l] .. lstart[l + 1] = level l + 1
    std::vector<uint32_t> cslot;     // the constants' LDS slots (lds only, empty otherwise)
    uint32_t maxlevel = 0;
    uint32_t lds_peak = 0;           // most values live at once (slots needed); 0 when the LDS file was not asked for
    bool lds = false;                // run by k_tape_run_lds; otherwise k_tape_load_consts + k_tape_run
};
// ops: resolved (dst / a / b are final register numbers; registers 0 .. nconst - 1 are the constants, op k writes nconst + k).
// EVERY operation is kept and run, read or not: a TAPE_INV has a side effect (FLAG_DIV_ZERO on a zero operand) that callers
// record on purpose without reading the inverse (schema_shplonk.hpp: rotations with equal points).  A pass that drops unread
// operations must keep the inversions.
// want_lds: take the LDS register file if the tape's live values fit (a tape without operations never does).
// false: an operand is not defined before its use.
inline bool compile_tape(const std::vector<TapeOp>& ops, uint32_t nconst, bool want_lds, CompiledTape& out) {
    const uint32_t nreg = nconst + (uint32_t)ops.size();
    out = CompiledTape();
    if (!schedule_levels(ops, nreg, out.sorted, out.lstart, out.maxlevel)) return false;
    out.lds = want_lds && !ops.empty() && tape_lds_assign(out.sorted, out.lstart, nconst, nreg, out.cslot, &out.lds_peak);
    return true;
}

}  // namespace h2agg
