// Host build of csrc/lz_dedup.h (tests/test_position_dedup_cpu.py): a row's key and symmetry, the choice of k* from bit
// words, the frame map and the sequential merge of one group, against the numpy restatement tests/position_dedup.py.
#include <stdint.h>
#include <stddef.h>

#include "../liuzhou_amd/csrc/lz_dedup.h"

extern "C" {

// keys[n,8], sym[n] of n rows; returns the rows that are not representable
int64_t lzdedup_row_keys(const float* planes, const uint8_t* masks, int64_t n, int symmetric, int64_t* keys, int8_t* sym) {
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
        bad += !lzdedup::row_key(planes + i * lzdedup::kPlaneFloats, masks + i * lzdedup::kActions, i, symmetric != 0,
                                 keys + i * lzdedup::kKeyWords, sym + i);
    return bad;
}

// k* of four boards given as bit words, img[4] its image
int lzdedup_choose_sym(const uint64_t* w, int symmetric, uint64_t* img) { return lzdedup::choose_sym(w, symmetric != 0, img); }

int lzdedup_frame_map(int sym_f, int sym_m) { return lzdedup::frame_map(sym_f, sym_m); }

void lzdedup_merge_group(const float* policy, const float* value, const float* soft, const int8_t* sym,
                         const int64_t* members, int64_t c, float* out_policy, float* out_value, float* out_soft) {
    lzdedup::merge_group(policy, value, soft, sym, members, c, out_policy, out_value, out_soft);
}

}
