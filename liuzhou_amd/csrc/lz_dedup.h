// lz_dedup.h -- scalar arithmetic of merging duplicate positions among training rows, up to board symmetry
// (lz_dedup.hip, lz_dedup_host.cpp; liuzhou_amd/position_dedup.py is the interface, DESIGN.md section 24 the reasons).
//
// A training row's planes are exact 0/1 images of four 36-bit boards plus a phase (lz_ops.hip: model_input_kernel).
// Reading them back gives the position {own, opp, own-marked, opp-marked, phase}; its key is the position's image under
// the row's canonical symmetry k* (exact mode: k* = 0) together with the legal bits moved the same way.  Rows with equal
// keys form a group; the group leaves as ONE row in the frame of its first member, its policy / value / soft value the
// mean over the members, each member's policy carried into that frame by e_m = sym[f]^-1 o sym[m].
//
// Every sum has one association, so that the kernels, the host build and the numpy restatement
// (tests/position_dedup.py) agree bit for bit: members in order in chunks of kChunk, a chunk's partial sum accumulated
// sequentially from 0.0, the partial sums added in ascending chunk order to a total that starts at 0.0.  All double.
#pragma once
#include <stdint.h>

#include "lz_symmetry.h"

namespace lzdedup {

using lz::kActions;
using lz::kFull;
using lz::kSym;
using lz::kSyms;

constexpr int kChunk = 256;                 // members per partial sum
constexpr int kKeyWords = 8;                // int64 words of a key
constexpr int kPlaneFloats = 396;           // 11 planes of 36 cells
constexpr int64_t kNoKey = INT64_MIN;       // word 0 of a row that is not representable: kNoKey | row index

// ---- reading a row from bit words ---------------------------------------------------------------------------------------
// `set` has bit x iff the plane's value at cell x is not zero, `good` iff it is +-0.0 or 1.0 (36 bits each).
LZ_HD bool value_set(float x) { return x != 0.f; }
LZ_HD bool value_good(float x) { return x == 0.f || x == 1.f; }
// a board plane (0..3): every cell 0 or 1
LZ_HD bool board_plane_ok(uint64_t good) { return (good & kFull) == kFull; }
// phase plane ph (1..7 for planes 4..10), taken in ascending order with `phase` starting at 0: constant over the board
// at 0 or 1, at most one of the seven set.  Returns whether the row is still representable.
LZ_HD bool phase_plane_step(uint64_t set, uint64_t good, int ph, int& phase) {
    set &= kFull;
    bool ok = (good & kFull) == kFull && (set == 0 || set == kFull);
    if (set) { ok = ok && phase == 0; phase = ph; }
    return ok;
}

// ---- the row's symmetry --------------------------------------------------------------------------------------------------
// (a0..a3) < (b0..b3), lexicographically, as unsigned numbers
LZ_HD bool tuple_less(uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3, uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3) {
    if (a0 != b0) return a0 < b0;
    if (a1 != b1) return a1 < b1;
    if (a2 != b2) return a2 < b2;
    return a3 < b3;
}
// k*: the lowest k whose image of the four boards is the smallest; 0 in exact mode.  img receives that image.
LZ_HD int choose_sym(const uint64_t w[4], bool symmetric, uint64_t img[4]) {
    int best = 0;
    for (int p = 0; p < 4; ++p) img[p] = w[p] & kFull;
    if (!symmetric) return 0;
    for (int k = 1; k < kSyms; ++k) {
        const uint64_t c0 = lz::sym_board(k, w[0] & kFull), c1 = lz::sym_board(k, w[1] & kFull),
                       c2 = lz::sym_board(k, w[2] & kFull), c3 = lz::sym_board(k, w[3] & kFull);
        if (tuple_less(c0, c1, c2, c3, img[0], img[1], img[2], img[3])) {
            img[0] = c0; img[1] = c1; img[2] = c2; img[3] = c3; best = k;
        }
    }
    return best;
}

// ---- key words -------------------------------------------------------------------------------------------------------------
// words 0..3 of a representable row: the image of the boards, the phase above bit 35 of word 0 (the trajectory codec's
// layout); words 4..7 are the legal bits of the image, bit (b & 63) of word 4 + (b >> 6)
LZ_HD void key_boards(const uint64_t img[4], int phase, int64_t* key) {
    key[0] = (int64_t)(img[0] | ((uint64_t)phase << 36));
    key[1] = (int64_t)img[1]; key[2] = (int64_t)img[2]; key[3] = (int64_t)img[3];
}
LZ_HD void key_not_representable(int64_t row, int64_t* key) {
    key[0] = kNoKey | row;
    for (int w = 1; w < kKeyWords; ++w) key[w] = 0;
}
// the legal bits of the image under k, from a row's mask bytes
LZ_HD void key_mask(const uint8_t* mask, int k, int64_t* key) {
    uint64_t m[4] = {0, 0, 0, 0};
    for (int a = 0; a < kActions; ++a)
        if (mask[a] != 0) { const int b = kSym.action[k][a]; m[b >> 6] |= 1ull << (b & 63); }
    for (int w = 0; w < 4; ++w) key[4 + w] = (int64_t)m[w];
}

// one row, start to end (the host build; the keys kernel takes the same steps with ballots): returns whether the row is
// representable, *sym = k*
LZ_HD bool row_key(const float* planes, const uint8_t* mask, int64_t row, bool symmetric, int64_t* key, int8_t* sym) {
    uint64_t w[4];
    bool ok = true;
    int phase = 0;
    for (int p = 0; p < 11; ++p) {
        uint64_t set = 0, good = 0;
        for (int x = 0; x < 36; ++x) {
            const float v = planes[p * 36 + x];
            set |= (uint64_t)value_set(v) << x; good |= (uint64_t)value_good(v) << x;
        }
        if (p < 4) { w[p] = set; ok = board_plane_ok(good) && ok; }
        else ok = phase_plane_step(set, good, p - 3, phase) && ok;
    }
    if (!ok) { key_not_representable(row, key); *sym = 0; return false; }
    uint64_t img[4];
    const int k = choose_sym(w, symmetric, img);
    key_boards(img, phase, key);
    key_mask(mask, k, key);
    *sym = (int8_t)k;
    return true;
}

// ---- the frame map -----------------------------------------------------------------------------------------------------------
// e_m: from member m's frame to the first member f's frame
LZ_HD int frame_map(int sym_f, int sym_m) { return kSym.comp[kSym.inv[sym_f & 7]][sym_m & 7]; }

// ---- one group, sequentially ----------------------------------------------------------------------------------------------
// members[0..c) ascending row indices (all inside [0, n), the caller checks), members[0] the first member.  Writes the
// group's policy[220], value and soft value; planes and mask are bit copies of the first member and not handled here.
LZ_HD void merge_group(const float* policy, const float* value, const float* soft, const int8_t* sym,
                       const int64_t* members, int64_t c, float* out_policy, float* out_value, float* out_soft) {
    if (c == 1) {                                             // a group of one: a bit copy
        const uint32_t* p = reinterpret_cast<const uint32_t*>(policy + members[0] * kActions);
        uint32_t* o = reinterpret_cast<uint32_t*>(out_policy);
        for (int a = 0; a < kActions; ++a) o[a] = p[a];
        *reinterpret_cast<uint32_t*>(out_value) = *reinterpret_cast<const uint32_t*>(value + members[0]);
        *reinterpret_cast<uint32_t*>(out_soft) = *reinterpret_cast<const uint32_t*>(soft + members[0]);
        return;
    }
    const int sf = sym[members[0]];
    int64_t cp = 0;
    for (int64_t i = 0; i < c; ++i) {
        const float* p = policy + members[i] * kActions;
        bool any = false;
        for (int a = 0; a < kActions; ++a) any = any || p[a] != 0.f;
        cp += any;
    }
    for (int b = 0; b < kActions; ++b) {
        double total = 0.0;
        for (int64_t c0 = 0; c0 < c; c0 += kChunk) {
            double part = 0.0;
            const int64_t c1 = c0 + kChunk < c ? c0 + kChunk : c;
            for (int64_t i = c0; i < c1; ++i) {
                const int e = frame_map(sf, sym[members[i]]);
                part += (double)policy[members[i] * kActions + kSym.action[kSym.inv[e]][b]];
            }
            total += part;
        }
        out_policy[b] = cp > 0 ? (float)(total / (double)cp) : 0.f;
    }
    double tv = 0.0, ts = 0.0;
    for (int64_t c0 = 0; c0 < c; c0 += kChunk) {
        double pv = 0.0, ps = 0.0;
        const int64_t c1 = c0 + kChunk < c ? c0 + kChunk : c;
        for (int64_t i = c0; i < c1; ++i) { pv += (double)value[members[i]]; ps += (double)soft[members[i]]; }
        tv += pv; ts += ps;
    }
    *out_value = (float)(tv / (double)c);
    *out_soft = (float)(ts / (double)c);
}

}  // namespace lzdedup
