// lz_replay_merge.h -- scalar arithmetic of merging duplicate positions across the replay window, record to record
// (lz_replay_merge.hip, lz_dedup_host.cpp; liuzhou_amd/replay_window.py is the interface, DESIGN.md section 30 the
// reasons).
//
// A 360-byte trajectory record (lz_train.hip) already holds what a key and a merge need: the four 36-bit boards and the
// phase are words 0..3, the legal set is seven u32 words, the policy 72 floats at the ranks of the legal actions.  So a
// record's key is computed from its 88 header bytes, and a group of records leaves as ONE record: the header of its
// first member, canonical as lz_pack_trajectory_rows writes it, with the members' policies averaged on the first
// member's legal set.  Both results equal, byte for byte, what lz_dedup.h gives for the rows that
// lz_unpack_trajectory_rows makes of the records, packed again -- for ANY 360 bytes, because unpacking is total.
//
// The sums keep the one association of lz_dedup.h (chunks of kChunk members, all double).
#pragma once
#include <stdint.h>

#include "lz_dedup.h"

namespace lzrmerge {

using lz::kActions;
using lz::kFull;
using lz::kSym;
using lz::kSyms;
using lzdedup::kChunk;
using lzdedup::kKeyWords;

constexpr int kRecBytes = 360;
constexpr int kMaskOff = 32, kPolicyOff = 60, kValueOff = 348;     // byte offsets inside a record
constexpr int kPolicySlots = 72;
constexpr uint32_t kLastMaskWord = 0x0FFFFFFFu;                    // actions 192..219 of mask word 6; bits 220..223 unowned

// ---- the header ----------------------------------------------------------------------------------------------------------
// w: the four board words as stored (w[0] with whatever stands above bit 35); b: the legal bits 0..219 as four 64-bit
// words, bit (a & 63) of word a >> 6
struct Header {
    uint64_t w[4];
    uint64_t b[4];
};
LZ_HD Header read_header(const uint8_t* rec) {                      // records are 8-byte aligned (the entry points check)
    const uint64_t* wq = reinterpret_cast<const uint64_t*>(rec);
    const uint32_t* mq = reinterpret_cast<const uint32_t*>(rec + kMaskOff);
    Header h;
    h.w[0] = wq[0]; h.w[1] = wq[1]; h.w[2] = wq[2]; h.w[3] = wq[3];
    h.b[0] = (uint64_t)mq[0] | ((uint64_t)mq[1] << 32); h.b[1] = (uint64_t)mq[2] | ((uint64_t)mq[3] << 32);
    h.b[2] = (uint64_t)mq[4] | ((uint64_t)mq[5] << 32); h.b[3] = (uint64_t)(mq[6] & kLastMaskWord);
    return h;
}
LZ_HD int header_phase(const Header& h) { return (int)((h.w[0] >> 36) & 7); }
LZ_HD int legal_count(const Header& h) {
    return __builtin_popcountll(h.b[0]) + __builtin_popcountll(h.b[1]) + __builtin_popcountll(h.b[2]) +
           __builtin_popcountll(h.b[3]);
}
LZ_HD uint64_t pick4(int i, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    return i == 0 ? a : i == 1 ? b : i == 2 ? c : d;               // selects: no private array indexed by a lane
}
LZ_HD bool legal_bit(const Header& h, int a) { return (pick4(a >> 6, h.b[0], h.b[1], h.b[2], h.b[3]) >> (a & 63)) & 1ull; }
// the rank of action a among the legal bits (the policy slot it owns when its bit is set)
LZ_HD int legal_rank(const Header& h, int a) {
    const int wi = a >> 6, bi = a & 63;
    const int c1 = __builtin_popcountll(h.b[0]), c2 = c1 + __builtin_popcountll(h.b[1]),
              c3 = c2 + __builtin_popcountll(h.b[2]);
    return (wi == 0 ? 0 : wi == 1 ? c1 : wi == 2 ? c2 : c3) +
           __builtin_popcountll(pick4(wi, h.b[0], h.b[1], h.b[2], h.b[3]) & ((1ull << bi) - 1ull));
}
// the position of the r-th set bit of x (r < popcount(x)): six popcounts
LZ_HD int select_bit(uint64_t x, int r) {
    int pos = 0;
    for (int s = 32; s >= 1; s >>= 1) {
        const int cnt = __builtin_popcountll((x >> pos) & ((1ull << s) - 1ull));
        if (r >= cnt) { r -= cnt; pos += s; }
    }
    return pos;
}
// the r-th legal action (r < legal_count)
LZ_HD int legal_action(const Header& h, int r) {
    const int c1 = __builtin_popcountll(h.b[0]), c2 = c1 + __builtin_popcountll(h.b[1]),
              c3 = c2 + __builtin_popcountll(h.b[2]);
    const int wi = r < c1 ? 0 : r < c2 ? 1 : r < c3 ? 2 : 3;
    const int base = wi == 0 ? 0 : wi == 1 ? c1 : wi == 2 ? c2 : c3;
    return wi * 64 + select_bit(pick4(wi, h.b[0], h.b[1], h.b[2], h.b[3]), r - base);
}
// the policy of action a as the unpacked row holds it, as bits: the slot at its rank, 0 when the bit is clear or the
// rank is past the 72 slots.  The load stays inside the record whatever its mask holds.
LZ_HD uint32_t policy_bits(const uint8_t* rec, const Header& h, int a) {
    const int rank = legal_rank(h, a);
    const uint32_t pw = reinterpret_cast<const uint32_t*>(rec + kPolicyOff)[rank < kPolicySlots ? rank : kPolicySlots - 1];
    return legal_bit(h, a) && rank < kPolicySlots ? pw : 0u;
}
LZ_HD float bits_float(uint32_t u) {
    union { uint32_t u; float f; } x;
    x.u = u;
    return x.f;
}
LZ_HD uint32_t float_bits(float f) {
    union { uint32_t u; float f; } x;
    x.f = f;
    return x.u;
}

// ---- the key of one record (the host build; the keys kernel takes the same steps with ballots) ---------------------------
LZ_HD void record_key(const uint8_t* rec, bool symmetric, int64_t* key, int8_t* sym) {
    const Header h = read_header(rec);
    uint64_t img[4];
    const int k = lzdedup::choose_sym(h.w, symmetric, img);
    lzdedup::key_boards(img, header_phase(h), key);
    uint64_t m[4] = {0, 0, 0, 0};
    for (int a = 0; a < kActions; ++a)
        if (legal_bit(h, a)) { const int b = kSym.action[k][a]; m[b >> 6] |= 1ull << (b & 63); }
    for (int w = 0; w < 4; ++w) key[4 + w] = (int64_t)m[w];
    *sym = (int8_t)k;
}

// ---- the canonical header of an output record, as lz_pack_trajectory_rows writes it ---------------------------------------
LZ_HD void write_header(const Header& h, uint8_t* out) {
    uint64_t* wq = reinterpret_cast<uint64_t*>(out);
    uint32_t* mq = reinterpret_cast<uint32_t*>(out + kMaskOff);
    wq[0] = (h.w[0] & kFull) | ((uint64_t)header_phase(h) << 36);
    wq[1] = h.w[1] & kFull; wq[2] = h.w[2] & kFull; wq[3] = h.w[3] & kFull;
    mq[0] = (uint32_t)h.b[0]; mq[1] = (uint32_t)(h.b[0] >> 32); mq[2] = (uint32_t)h.b[1]; mq[3] = (uint32_t)(h.b[1] >> 32);
    mq[4] = (uint32_t)h.b[2]; mq[5] = (uint32_t)(h.b[2] >> 32); mq[6] = (uint32_t)h.b[3];
}
// whether a member has a policy: a non-zero entry among its first min(legal count, 72) slots
LZ_HD bool has_policy(const uint8_t* rec, const Header& h) {
    const int cnt = legal_count(h) < kPolicySlots ? legal_count(h) : kPolicySlots;
    const uint32_t* pv = reinterpret_cast<const uint32_t*>(rec + kPolicyOff);
    bool any = false;
    for (int r = 0; r < cnt; ++r) any = any || bits_float(pv[r]) != 0.f;
    return any;
}

// ---- one group, sequentially -------------------------------------------------------------------------------------------
// members[0..c) positions in `slot` (the caller has checked them, their slots and their syms), members[0] the first
// member.  Writes the 360 bytes of `out`; returns whether the first member has more than 72 legal bits (the record then
// holds the first 72 legal actions' slots, as pack leaves it).
LZ_HD bool merge_record_group(const uint8_t* records, const int64_t* slot, const int8_t* sym, const int64_t* members,
                              int64_t c, uint8_t* out) {
    const uint8_t* rf = records + slot[members[0]] * kRecBytes;
    const Header hf = read_header(rf);
    write_header(hf, out);
    uint32_t* po = reinterpret_cast<uint32_t*>(out + kPolicyOff);
    uint32_t* vo = reinterpret_cast<uint32_t*>(out + kValueOff);
    const int legal = legal_count(hf), used = legal < kPolicySlots ? legal : kPolicySlots;
    for (int r = used; r < kPolicySlots; ++r) po[r] = 0u;
    vo[2] = 0u;
    if (c == 1) {                                             // a group of one: a bit copy
        const uint32_t* pf = reinterpret_cast<const uint32_t*>(rf + kPolicyOff);
        const uint32_t* vf = reinterpret_cast<const uint32_t*>(rf + kValueOff);
        for (int r = 0; r < used; ++r) po[r] = pf[r];
        vo[0] = vf[0]; vo[1] = vf[1];
        return legal > kPolicySlots;
    }
    const int sf = sym[members[0]];
    int64_t cp = 0;
    for (int64_t i = 0; i < c; ++i) {
        const uint8_t* rm = records + slot[members[i]] * kRecBytes;
        cp += has_policy(rm, read_header(rm));
    }
    for (int r = 0; r < used; ++r) {
        const int b = legal_action(hf, r);
        double total = 0.0;
        for (int64_t c0 = 0; c0 < c; c0 += kChunk) {
            double part = 0.0;
            const int64_t c1 = c0 + kChunk < c ? c0 + kChunk : c;
            for (int64_t i = c0; i < c1; ++i) {
                const uint8_t* rm = records + slot[members[i]] * kRecBytes;
                const int e = lzdedup::frame_map(sf, sym[members[i]]);
                part += (double)bits_float(policy_bits(rm, read_header(rm), kSym.action[kSym.inv[e]][b]));
            }
            total += part;
        }
        po[r] = cp > 0 ? float_bits((float)(total / (double)cp)) : 0u;
    }
    double tv = 0.0, ts = 0.0;
    for (int64_t c0 = 0; c0 < c; c0 += kChunk) {
        double pv = 0.0, ps = 0.0;
        const int64_t c1 = c0 + kChunk < c ? c0 + kChunk : c;
        for (int64_t i = c0; i < c1; ++i) {
            const uint32_t* vm = reinterpret_cast<const uint32_t*>(records + slot[members[i]] * kRecBytes + kValueOff);
            pv += (double)bits_float(vm[0]); ps += (double)bits_float(vm[1]);
        }
        tv += pv; ts += ps;
    }
    vo[0] = float_bits((float)(tv / (double)c)); vo[1] = float_bits((float)(ts / (double)c));
    return legal > kPolicySlots;
}

}  // namespace lzrmerge
