// lz_live_index.h -- index arithmetic of the gathering network launch (lz_net.hip: net_forward_gather_kernel).
// The live games of a launch are the set bits of a bit mask, one 64-bit word per 64 games; row r of the launch is the
// r-th live game in ascending order.  Pure integer functions, compiled for the device and for the host
// (tests/live_gather_host_check.cpp checks them against a plain loop).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZ_LIVE_HD __host__ __device__
#else
#define LZ_LIVE_HD
#endif

namespace lzlive {

LZ_LIVE_HD inline int popc64(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(m);
#else
    return __builtin_popcountll(m);
#endif
}

// number of mask words of `games` games
LZ_LIVE_HD inline int mask_words(int64_t games) { return (int)((games + 63) >> 6); }

// prefix[w] = live games in the words before w (exclusive prefix of the popcounts); returns the total
LZ_LIVE_HD inline int prefix_popcounts(const uint64_t* masks, int words, int* prefix) {
    int run = 0;
    for (int w = 0; w < words; ++w) { prefix[w] = run; run += popc64(masks[w]); }
    return run;
}

// the word that holds row `row` (0 <= row < total): the LAST word whose prefix is <= row.  Empty words share their
// prefix with the next live word and lie before it, so the last one is the word with the bit.
LZ_LIVE_HD inline int find_word(const int* prefix, int words, int row) {
    int lo = 0, hi = words - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// position of the k-th set bit of m (k = 0 is the lowest; 0 <= k < popc64(m)): six halving steps
LZ_LIVE_HD inline int select_bit(uint64_t m, int k) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const uint64_t low = m & ((1ull << width) - 1ull);
        const int c = popc64(low);
        if (k >= c) { k -= c; m >>= width; pos += width; }
    }
    return pos;
}

// game of row `row`
LZ_LIVE_HD inline int row_to_game(const uint64_t* masks, const int* prefix, int words, int row) {
    const int w = find_word(prefix, words, row);
    return w * 64 + select_bit(masks[w], row - prefix[w]);
}

}  // namespace lzlive
