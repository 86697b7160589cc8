// lz_start_bank.h -- the scalar rules of the start bank (host + device): self-play games that start from positions of
// earlier games instead of the empty board (game forking).
//
// The bank is a ring of lz::Packed records, entries uint8[capacity, 32], and cursor int64[1] = the number of positions
// ever appended; filled = min(cursor, capacity) and the filled entries are the physical rows [0, filled).
//   capture (once per ply, on the searched roots): slot g is a candidate when it is live, its search is neither terminal
//     nor without a move, min_move <= move_count <= max_move and u01(draw(seed, game, ply, purpose 3, index 1020).x) <
//     capture_prob.  Candidates are appended in ascending slot order: rank r goes to row (total + r) % capacity, and of
//     more candidates than rows only the last `capacity` write, so no two candidates of a launch write one row.
//   seed (a slot that starts a game): r = draw(seed, game, 0, purpose 3, index 1021); with filled > 0 and u01(r.x) <
//     fork_prob the game starts from entry (r.y * filled) >> 32 -- integers only.
// The kernels (lz_ops.hip) and their sequential host twins (lz_start_bank_host.cpp) are built on these functions alone.
#pragma once
#include <stdint.h>

#include "lz_rng.h"
#include "lz_rules.h"

namespace lzbank {

constexpr int64_t kMaxCapacity = 1ll << 24;            // the candidate ranks of a launch are 32-bit
constexpr int kCounters = 3;                            // forked_games, fork_move_sum, captured
enum Counter : int { kForkedGames = 0, kForkMoveSum = 1, kCaptured = 2 };

LZ_RNG_HD int64_t filled(int64_t total, int64_t capacity) {
    return total < 0 ? 0 : (total < capacity ? total : capacity);
}

// the ring position of the candidate of rank `rank` of a launch that found the bank with `total` positions ever appended
LZ_RNG_HD int64_t ring_row(int64_t total, int64_t rank, int64_t capacity) { return (total + rank) % capacity; }

// of `count` candidates of one launch only the last `capacity` write
LZ_RNG_HD bool rank_writes(int64_t rank, int64_t count, int64_t capacity) { return rank >= count - capacity; }

LZ_RNG_HD bool capture_draw(uint64_t seed, int64_t game, int64_t ply, float capture_prob) {
    return lzrng::u01(lzrng::draw(seed, game, ply, lzrng::kPurposeGumbel, lzrng::kIndexStartCapture, 0u).x) < capture_prob;
}

// everything but the draw (cheap, asked first)
LZ_RNG_HD bool eligible(int done, int terminal, int chosen_valid, int64_t move_count, int64_t min_move, int64_t max_move) {
    return done == 0 && terminal == 0 && chosen_valid != 0 && move_count >= min_move && move_count <= max_move;
}

LZ_RNG_HD bool candidate(int done, int terminal, int chosen_valid, int64_t move_count, int64_t min_move, int64_t max_move,
                         uint64_t seed, int64_t game, int64_t ply, float capture_prob) {
    return eligible(done, terminal, chosen_valid, move_count, min_move, max_move) &&
           capture_draw(seed, game, ply, capture_prob);
}

// the entry a game forks from, -1: it starts from the empty board
LZ_RNG_HD int64_t fork_entry(uint64_t seed, int64_t game, float fork_prob, int64_t filled_rows) {
    if (filled_rows <= 0) return -1;
    const lzrng::U4 r = lzrng::draw(seed, game, 0, lzrng::kPurposeGumbel, lzrng::kIndexStartFork, 0u);
    if (!(lzrng::u01(r.x) < fork_prob)) return -1;
    return (int64_t)(((uint64_t)r.y * (uint64_t)filled_rows) >> 32);
}

}  // namespace lzbank
