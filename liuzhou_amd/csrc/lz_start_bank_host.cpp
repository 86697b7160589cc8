// lz_start_bank_host.cpp -- host (CPU-tensor) build of lz_start_bank_capture / lz_start_bank_seed
// (include/liuzhou_hip.h), part of libliuzhou_host.so: the scalar rules of csrc/lz_start_bank.h as plain loops over the
// slots in ascending order, with the semantics of the kernels in lz_ops.hip.  `stream` is ignored.
#include <cstdint>
#include <cstring>

#include "lz_soa.h"
#include "lz_start_bank.h"
#include "lz_state_rows_host.h"

using namespace lz;

using namespace lzhost;                                    // soa_ok, aligned, soa_aligned, load, store

extern "C" int lz_start_bank_capture(const LzStateSoA* s, int64_t G, const uint8_t* done, const uint8_t* terminal_mask,
                                     const uint8_t* chosen_valid_mask, const int64_t* plies, const int64_t* slot_game,
                                     int64_t game_base, uint64_t seed, float capture_prob, int64_t min_move,
                                     int64_t max_move, uint8_t* entries, int64_t capacity, int64_t* cursor,
                                     int64_t* counters, void*) {
    if (G < 0 || capacity < 1 || capacity > lzbank::kMaxCapacity || min_move < 0 || max_move < min_move ||
        !(capture_prob >= 0.f && capture_prob <= 1.f))
        return LZ_ERR_ARG;
    if (G == 0) return LZ_OK;
    if (!soa_ok(s) || !done || !terminal_mask || !chosen_valid_mask || !plies || !entries || !cursor || !counters)
        return LZ_ERR_ARG;
    if (!soa_aligned(s) || !aligned(entries, 16) || !aligned(cursor, 8) || !aligned(counters, 8)) return LZ_ERR_ALIGN;
    if (!(capture_prob > 0.f)) return LZ_OK;
    auto is_candidate = [&](int64_t j) {
        return lzbank::candidate(done[j], terminal_mask[j], chosen_valid_mask[j], s->move_count[j], min_move, max_move,
                                 seed, (slot_game ? slot_game[j] : j) + game_base, plies[j], capture_prob);
    };
    int64_t count = 0;
    for (int64_t j = 0; j < G; ++j) count += is_candidate(j) ? 1 : 0;
    if (count == 0) return LZ_OK;
    const int64_t total = *cursor < 0 ? 0 : *cursor;
    int64_t rank = 0;
    for (int64_t j = 0; j < G; ++j) {
        if (!is_candidate(j)) continue;
        if (lzbank::rank_writes(rank, count, capacity)) {
            const Packed p = pack(load(s, j));
            const uint64_t w[4] = {p.w0, p.w1, p.w2, p.w3};
            std::memcpy(entries + 32 * lzbank::ring_row(total, rank, capacity), w, 32);
        }
        ++rank;
    }
    *cursor = total + count;
    counters[lzbank::kCaptured] += count;
    return LZ_OK;
}

extern "C" int lz_start_bank_seed(const LzStateSoA* s, int64_t G, const uint8_t* fresh, const int64_t* slot_game,
                                  int64_t game_base, uint64_t seed, float fork_prob, const uint8_t* entries,
                                  int64_t capacity, const int64_t* cursor, int64_t* counters, void*) {
    if (G < 0 || capacity < 1 || capacity > lzbank::kMaxCapacity || !(fork_prob >= 0.f && fork_prob <= 1.f))
        return LZ_ERR_ARG;
    if (G == 0) return LZ_OK;
    if (!soa_ok(s) || !fresh || !entries || !cursor || !counters) return LZ_ERR_ARG;
    if (!soa_aligned(s) || !aligned(entries, 16) || !aligned(cursor, 8) || !aligned(counters, 8)) return LZ_ERR_ALIGN;
    const int64_t filled = lzbank::filled(*cursor, capacity);
    for (int64_t g = 0; g < G; ++g) {
        if (fresh[g] == 0) continue;
        const int64_t j = lzbank::fork_entry(seed, (slot_game ? slot_game[g] : g) + game_base, fork_prob, filled);
        if (j < 0) continue;
        uint64_t w[4];
        std::memcpy(w, entries + 32 * j, 32);
        const State st = unpack(Packed{w[0], w[1], w[2], w[3]});
        store(s, g, st);
        counters[lzbank::kForkedGames] += 1;
        counters[lzbank::kForkMoveSum] += st.move_count;
    }
    return LZ_OK;
}
