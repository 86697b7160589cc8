// lz_state_rows_host.h -- one row of the 12-tensor SoA state <-> lz::State on the host, and the pointer checks of the
// entry points that take an LzStateSoA: shared by the host (CPU-tensor) builds lz_start_bank_host.cpp and
// lz_opening_book_host.cpp.  The device side of the same is lz_state_rows.h.
#pragma once
#include <cstdint>

#include "lz_soa.h"

namespace lzhost {

using namespace lz;

inline bool soa_ok(const LzStateSoA* s) {
    return s && s->board && s->marks_black && s->marks_white && s->phase && s->current_player &&
           s->pending_marks_required && s->pending_marks_remaining && s->pending_captures_required &&
           s->pending_captures_remaining && s->forced_removals_done && s->move_count && s->moves_since_capture;
}
inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
inline bool soa_aligned(const LzStateSoA* s) {
    return aligned(s->board, 4) && aligned(s->marks_black, 4) && aligned(s->marks_white, 4);
}

inline State load(const LzStateSoA* s, int64_t i) {
    State st;
    st.black = cells_equal(s->board + i * kCells, 1);
    st.white = cells_equal(s->board + i * kCells, -1);
    st.mb = cells_nonzero(s->marks_black + i * kCells);
    st.mw = cells_nonzero(s->marks_white + i * kCells);
    st.phase = (int)s->phase[i]; st.player = (int)s->current_player[i];
    st.pm_req = (int)s->pending_marks_required[i]; st.pm_rem = (int)s->pending_marks_remaining[i];
    st.pc_req = (int)s->pending_captures_required[i]; st.pc_rem = (int)s->pending_captures_remaining[i];
    st.forced = (int)s->forced_removals_done[i]; st.move_count = (int)s->move_count[i];
    st.msc = (int)s->moves_since_capture[i];
    return st;
}
inline void store(const LzStateSoA* o, int64_t i, const State& s) {
    for (int c = 0; c < kCells; ++c) {
        o->board[i * kCells + c] = (int8_t)(((s.black >> c) & 1) ? 1 : (((s.white >> c) & 1) ? -1 : 0));
        o->marks_black[i * kCells + c] = (uint8_t)((s.mb >> c) & 1);
        o->marks_white[i * kCells + c] = (uint8_t)((s.mw >> c) & 1);
    }
    o->phase[i] = s.phase; o->current_player[i] = s.player;
    o->pending_marks_required[i] = s.pm_req; o->pending_marks_remaining[i] = s.pm_rem;
    o->pending_captures_required[i] = s.pc_req; o->pending_captures_remaining[i] = s.pc_rem;
    o->forced_removals_done[i] = s.forced; o->move_count[i] = s.move_count; o->moves_since_capture[i] = s.msc;
}

}  // namespace lzhost
