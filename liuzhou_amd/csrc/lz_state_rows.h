// lz_state_rows.h -- one lane <-> one row of the 12-tensor SoA state (device only): the row's three 36-byte planes move
// as 9 dwords each, the bitboards are built from / expanded into those dwords in registers.  Shared by the transition
// kernels of lz_ops.hip and the opening-book kernels of lz_opening_book.hip.
#pragma once
#include <stdint.h>

#include "lz_soa.h"

namespace lz {

__device__ __forceinline__ void load_row_words(const void* base, int64_t row, uint32_t (&w)[9]) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(base) + row * kCells);
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = p[i];
}
__device__ __forceinline__ void store_row_words(void* base, int64_t row, const uint32_t (&w)[9]) {
    uint32_t* p = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(base) + row * kCells);
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = w[i];
}
__device__ __forceinline__ uint64_t words_eq(const uint32_t (&w)[9], uint32_t byte_value) {
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= (uint64_t)(((w[i] >> (8 * k)) & 0xFFu) == byte_value) << (i * 4 + k);
    }
    return m;
}
__device__ __forceinline__ uint64_t words_nonzero(const uint32_t (&w)[9]) {
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= (uint64_t)(((w[i] >> (8 * k)) & 0xFFu) != 0u) << (i * 4 + k);
    }
    return m;
}
__device__ __forceinline__ void board_words(uint64_t black, uint64_t white, uint32_t (&w)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = i * 4 + k;
            const uint32_t byte = ((black >> c) & 1) ? 0x01u : (((white >> c) & 1) ? 0xFFu : 0u);
            v |= byte << (8 * k);
        }
        w[i] = v;
    }
}
__device__ __forceinline__ void mark_words(uint64_t m, uint32_t (&w)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const uint32_t nib = (uint32_t)(m >> (i * 4)) & 0xFu;
        w[i] = (nib * 0x00204081u) & 0x01010101u;
    }
}

__device__ __forceinline__ State load_state(const LzStateSoA& s, int64_t row) {
    uint32_t w[9];
    State st;
    load_row_words(s.board, row, w);
    st.black = words_eq(w, 0x01u);
    st.white = words_eq(w, 0xFFu);
    load_row_words(s.marks_black, row, w);
    st.mb = words_nonzero(w);
    load_row_words(s.marks_white, row, w);
    st.mw = words_nonzero(w);
    st.phase = (int)s.phase[row];
    st.player = (int)s.current_player[row];
    st.pm_req = (int)s.pending_marks_required[row];
    st.pm_rem = (int)s.pending_marks_remaining[row];
    st.pc_req = (int)s.pending_captures_required[row];
    st.pc_rem = (int)s.pending_captures_remaining[row];
    st.forced = (int)s.forced_removals_done[row];
    st.move_count = (int)s.move_count[row];
    st.msc = (int)s.moves_since_capture[row];
    return st;
}
__device__ __forceinline__ void store_state(const LzStateSoA& o, int64_t row, const State& st) {
    uint32_t w[9];
    board_words(st.black, st.white, w);
    store_row_words(o.board, row, w);
    mark_words(st.mb, w);
    store_row_words(o.marks_black, row, w);
    mark_words(st.mw, w);
    store_row_words(o.marks_white, row, w);
    o.phase[row] = st.phase;
    o.current_player[row] = st.player;
    o.pending_marks_required[row] = st.pm_req;
    o.pending_marks_remaining[row] = st.pm_rem;
    o.pending_captures_required[row] = st.pc_req;
    o.pending_captures_remaining[row] = st.pc_rem;
    o.forced_removals_done[row] = st.forced;
    o.move_count[row] = st.move_count;
    o.moves_since_capture[row] = st.msc;
}

}  // namespace lz
