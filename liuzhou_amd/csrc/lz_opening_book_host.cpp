// lz_opening_book_host.cpp -- host (CPU-tensor) build of lz_opening_book_keys / lz_states_from_packed
// (include/liuzhou_hip.h), part of libliuzhou_host.so: the scalar rules of csrc/lz_opening_book.h as plain loops over the
// records and rows in ascending order, with the semantics of the kernels in lz_opening_book.hip.  `stream` is ignored.
#include <cstdint>
#include <cstring>

#include "lz_opening_book.h"
#include "lz_soa.h"
#include "lz_state_rows_host.h"

using namespace lz;

using namespace lzhost;                                    // soa_ok, aligned, soa_aligned, store

namespace {

Packed record(const uint8_t* records, int64_t i) {
    uint64_t w[4];
    std::memcpy(w, records + 32 * i, 32);
    return Packed{w[0], w[1], w[2], w[3]};
}

}  // namespace

extern "C" int lz_opening_book_keys(const uint8_t* records, int64_t m, int64_t min_move, int64_t max_move, uint8_t* valid,
                                    int64_t* keys, int8_t* sym, void*) {
    if (m < 0 || min_move < 0 || max_move < min_move) return LZ_ERR_ARG;
    if (m == 0) return LZ_OK;
    if (!records || !valid || !keys || !sym) return LZ_ERR_ARG;
    if (!aligned(records, 16) || !aligned(keys, 16)) return LZ_ERR_ALIGN;
    for (int64_t i = 0; i < m; ++i)
        valid[i] = lzbook::record_key(record(records, i), i, min_move, max_move, keys + i * lzbook::kKeyWords, sym + i) ? 1 : 0;
    return LZ_OK;
}

extern "C" int lz_states_from_packed(const uint8_t* records, int64_t capacity, const int64_t* index, int64_t n,
                                     const LzStateSoA* s, void*) {
    if (n < 0 || capacity < 0) return LZ_ERR_ARG;
    if (n == 0) return LZ_OK;
    if (!soa_ok(s) || !index || (capacity > 0 && !records)) return LZ_ERR_ARG;
    if (!soa_aligned(s) || !aligned(records, 16) || !aligned(index, 8)) return LZ_ERR_ALIGN;
    for (int64_t g = 0; g < n; ++g) {
        const int64_t j = index[g];
        if (j < 0 || j >= capacity) continue;
        store(s, g, unpack(record(records, j)));
    }
    return LZ_OK;
}
