// lz_opening_book.hip -- gfx950 kernels of the opening book (include/liuzhou_hip.h, csrc/lz_opening_book.h).
//
// opening_book_keys: one lane per record.  The record comes in with two 16-byte loads (as start_bank_seed_kernel reads a
// bank entry), validity and key are the scalar rules of lz_opening_book.h on registers -- the eight images are shifts
// and ors with compile-time cell maps -- and the lane leaves two 16-byte key stores and two byte stores.  Adjacent
// lanes read and write adjacent memory.  No LDS, no atomics.
//
// states_from_packed: one lane per row, the inverse of lz_pack_states: row g becomes unpack(records[index[g]]) through
// store_state (lz_state_rows.h); a row whose index is outside the bank is not touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz_opening_book.h"
#include "lz_soa.h"
#include "lz_state_rows.h"

using namespace lz;

namespace {

constexpr int kBlock = 256;

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int launch_status() { return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH; }
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline unsigned grid_threads(int64_t items) { return (unsigned)((items + kBlock - 1) / kBlock); }
inline bool soa_ok(const LzStateSoA* s) {
    return s && s->board && s->marks_black && s->marks_white && s->phase && s->current_player &&
           s->pending_marks_required && s->pending_marks_remaining && s->pending_captures_required &&
           s->pending_captures_remaining && s->forced_removals_done && s->move_count && s->moves_since_capture;
}
inline bool soa_aligned(const LzStateSoA* s) {
    return aligned(s->board, 4) && aligned(s->marks_black, 4) && aligned(s->marks_white, 4);
}

__global__ __launch_bounds__(kBlock) void opening_book_keys_kernel(const ulonglong2* __restrict__ records, int64_t m,
                                                                   int64_t min_move, int64_t max_move,
                                                                   uint8_t* __restrict__ valid, ulonglong2* __restrict__ keys,
                                                                   int8_t* __restrict__ sym) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const ulonglong2 a = records[2 * i], b = records[2 * i + 1];
    int64_t key[lzbook::kKeyWords];
    int8_t k;
    const bool ok = lzbook::record_key(Packed{a.x, a.y, b.x, b.y}, i, min_move, max_move, key, &k);
    keys[2 * i] = make_ulonglong2((unsigned long long)key[0], (unsigned long long)key[1]);
    keys[2 * i + 1] = make_ulonglong2((unsigned long long)key[2], (unsigned long long)key[3]);
    valid[i] = ok ? 1 : 0;
    sym[i] = k;
}

__global__ __launch_bounds__(kBlock) void states_from_packed_kernel(const ulonglong2* __restrict__ records, int64_t capacity,
                                                                    const int64_t* __restrict__ index, int64_t n,
                                                                    LzStateSoA s) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n) return;
    const int64_t j = index[g];
    if (j < 0 || j >= capacity) return;
    const ulonglong2 a = records[2 * j], b = records[2 * j + 1];
    store_state(s, g, unpack(Packed{a.x, a.y, b.x, b.y}));
}

}  // namespace

extern "C" {

int lz_opening_book_keys(const uint8_t* records, int64_t m, int64_t min_move, int64_t max_move, uint8_t* valid,
                         int64_t* keys, int8_t* sym, void* stream) {
    if (m < 0 || min_move < 0 || max_move < min_move) return LZ_ERR_ARG;
    if (m == 0) return LZ_OK;
    if (!records || !valid || !keys || !sym) return LZ_ERR_ARG;
    if (!aligned(records, 16) || !aligned(keys, 16)) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(opening_book_keys_kernel, dim3(grid_threads(m)), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<const ulonglong2*>(records), m, min_move, max_move, valid,
                       reinterpret_cast<ulonglong2*>(keys), sym);
    return launch_status();
}

int lz_states_from_packed(const uint8_t* records, int64_t capacity, const int64_t* index, int64_t n,
                          const LzStateSoA* s, void* stream) {
    if (n < 0 || capacity < 0) return LZ_ERR_ARG;
    if (n == 0) return LZ_OK;
    if (!soa_ok(s) || !index || (capacity > 0 && !records)) return LZ_ERR_ARG;
    if (!soa_aligned(s) || !aligned(records, 16) || !aligned(index, 8)) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(states_from_packed_kernel, dim3(grid_threads(n)), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<const ulonglong2*>(records), capacity, index, n, *s);
    return launch_status();
}

}  // extern "C"
