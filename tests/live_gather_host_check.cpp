// Host build of csrc/lz_live_index.h (tests/test_live_gather_cpu.py): the index arithmetic of the gathering network
// launch, driven the way the kernel drives it -- masks from the live flags, the exclusive prefix of their popcounts,
// then every row of the launch looked up on its own.
#include <stdint.h>
#include <stddef.h>
#include <vector>

#include "../liuzhou_amd/csrc/lz_live_index.h"

extern "C" {

// live[B] (non-zero = live) -> games_out[row] for every row; returns the number of rows, or -1 if the prefix, a word
// look-up or a bit look-up disagrees with what the masks say
int lzlive_rows(const uint8_t* live, int B, int32_t* games_out) {
    const int words = lzlive::mask_words(B);
    std::vector<uint64_t> masks((size_t)words, 0);
    for (int g = 0; g < B; ++g)
        if (live[g]) masks[(size_t)(g >> 6)] |= 1ull << (g & 63);
    std::vector<int> prefix((size_t)words, -1);
    const int n = lzlive::prefix_popcounts(masks.data(), words, prefix.data());
    for (int row = 0; row < n; ++row) {
        const int w = lzlive::find_word(prefix.data(), words, row);
        if (w < 0 || w >= words || prefix[(size_t)w] > row || row - prefix[(size_t)w] >= lzlive::popc64(masks[(size_t)w])) return -1;
        const int bit = lzlive::select_bit(masks[(size_t)w], row - prefix[(size_t)w]);
        if (bit < 0 || bit > 63 || !((masks[(size_t)w] >> bit) & 1)) return -1;
        games_out[row] = lzlive::row_to_game(masks.data(), prefix.data(), words, row);
        if (games_out[row] != w * 64 + bit) return -1;
    }
    return n;
}

// k-th set bit of one word, every k; out[k] for k < popcount; returns the popcount
int lzlive_select_all(uint64_t m, int32_t* out) {
    const int n = lzlive::popc64(m);
    for (int k = 0; k < n; ++k) out[k] = lzlive::select_bit(m, k);
    return n;
}

}
