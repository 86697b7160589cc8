// lz_opening_book.h -- the scalar rules of the opening book (host + device): which lz::Packed records of a start bank
// may open an arena game, and the key under which two of them are one opening.
//
// book_valid: the record is a position a game can be started from --
//   canonical (pack(unpack(p)) == p bit for bit: words 1..3 carry nothing above bit 35; word 0 owns all its 64 bits),
//   phase in 1..7 (the all-zero rows of an unfilled bank have phase 0), no cell both black and white, the game still
//   running (game_status == 0), at least one legal action (the tree search's enumeration, fallback_forced = 0; a position
//   with a move there has one under the tensor semantics too), and min_move <= move_count <= max_move.
// book_key: the four boards replaced by the smallest of their eight images (lzdedup::choose_sym: the lowest k among
//   equals), the metadata of word 0 from the phase up (bits 50..63: phase, player, forced, pm_req, pm_rem, pc_req,
//   pc_rem) above bit 35 of word 0.  move_count and moves_since_capture are NOT part of the key: two positions that
//   differ only in how they were reached are one opening.  An invalid record gets {kNoKey | row, 0, 0, 0}, sym 0 -- the
//   convention of lz_dedup_position_keys -- so an exact grouping never merges two invalid records.
// The kernels (lz_opening_book.hip) and their sequential host twins (lz_opening_book_host.cpp) are built on these alone.
#pragma once
#include <stdint.h>

#include "lz_dedup.h"
#include "lz_rules.h"
#include "lz_symmetry.h"

namespace lzbook {

using lz::Packed;
using lz::State;

constexpr int kKeyWords = 4;
constexpr int kMetaShift = 50;                           // word 0 from the phase up

LZ_HD bool canonical(const Packed& p) {
    const Packed q = lz::pack(lz::unpack(p));
    return q.w0 == p.w0 && q.w1 == p.w1 && q.w2 == p.w2 && q.w3 == p.w3;
}

LZ_HD bool book_valid(const Packed& p, int64_t min_move, int64_t max_move) {
    if (!canonical(p)) return false;
    const State s = lz::unpack(p);
    if (s.phase < 1 || s.phase > 7) return false;
    if ((s.black & s.white) != 0) return false;
    if (lz::game_status(s) != 0) return false;
    if (lz::legal_count(lz::legal_actions(s, /*fallback_forced=*/0)) <= 0) return false;
    return (int64_t)s.move_count >= min_move && (int64_t)s.move_count <= max_move;
}

// the key of a VALID record; *sym = the image's index
LZ_HD void book_key(const Packed& p, int64_t key[kKeyWords], int8_t* sym) {
    const uint64_t w[4] = {p.w0 & lz::kFull, p.w1 & lz::kFull, p.w2 & lz::kFull, p.w3 & lz::kFull};
    uint64_t img[4];
    const int k = lzdedup::choose_sym(w, true, img);
    key[0] = (int64_t)(img[0] | ((p.w0 >> kMetaShift) << 36));
    key[1] = (int64_t)img[1]; key[2] = (int64_t)img[2]; key[3] = (int64_t)img[3];
    *sym = (int8_t)k;
}

LZ_HD void key_invalid(int64_t row, int64_t key[kKeyWords], int8_t* sym) {
    key[0] = lzdedup::kNoKey | row; key[1] = 0; key[2] = 0; key[3] = 0;
    *sym = 0;
}

// one record, start to end: returns its validity
LZ_HD bool record_key(const Packed& p, int64_t row, int64_t min_move, int64_t max_move, int64_t key[kKeyWords], int8_t* sym) {
    const bool ok = book_valid(p, min_move, max_move);
    if (ok) book_key(p, key, sym);
    else key_invalid(row, key, sym);
    return ok;
}

}  // namespace lzbook
