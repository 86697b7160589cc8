// lz_dedup_host.cpp -- host (CPU-tensor) build of the position-dedup entry points of include/liuzhou_hip.h, part of
// libliuzhou_host.so: the arithmetic of csrc/lz_dedup.h as plain loops over rows and groups, with the semantics of
// lz_dedup.hip; and of the record-to-record pair over the replay window (csrc/lz_replay_merge.h, lz_replay_merge.hip).
// `stream` is ignored.
#include <cstdint>
#include <cstring>

#include "lz_dedup.h"
#include "lz_replay_merge.h"
#include "lz_soa.h"

using namespace lzdedup;

extern "C" {

int lz_dedup_position_keys(const float* planes, const uint8_t* masks, int64_t n, int32_t symmetric, int64_t* keys,
                           int8_t* sym, int32_t* not_representable, void*) {
    if (n < 0 || (symmetric != 0 && symmetric != 1)) return LZ_ERR_ARG;
    if (n == 0) return LZ_OK;
    if (!planes || !masks || !keys || !sym || !not_representable) return LZ_ERR_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (!row_key(planes + i * kPlaneFloats, masks + i * kActions, i, symmetric != 0, keys + i * kKeyWords, sym + i))
            *not_representable += 1;
    return LZ_OK;
}

int lz_dedup_merge_groups(const float* planes, const uint8_t* masks, const float* policy, const float* value,
                          const float* soft, int64_t n, const int8_t* sym, const int64_t* order,
                          const int64_t* group_begin, int64_t groups, float* out_planes, uint8_t* out_masks,
                          float* out_policy, float* out_value, float* out_soft, int32_t* out_count, void*) {
    if (n < 0 || groups < 0) return LZ_ERR_ARG;
    if (groups == 0) return LZ_OK;
    if (!group_begin || !out_planes || !out_masks || !out_policy || !out_value || !out_soft || !out_count) return LZ_ERR_ARG;
    if (n > 0 && !(planes && masks && policy && value && soft && sym && order)) return LZ_ERR_ARG;
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t begin = group_begin[g], end = group_begin[g + 1];
        bool bad = begin < 0 || end <= begin || end > n;      // an empty or impossible range: a zero row
        for (int64_t i = begin; !bad && i < end; ++i)
            bad = order[i] < 0 || order[i] >= n || sym[order[i]] < 0 || sym[order[i]] >= kSyms;
        if (bad) {
            std::memset(out_planes + g * kPlaneFloats, 0, kPlaneFloats * sizeof(float));
            std::memset(out_masks + g * kActions, 0, kActions);
            std::memset(out_policy + g * kActions, 0, kActions * sizeof(float));
            out_value[g] = 0.f; out_soft[g] = 0.f; out_count[g] = 0;
            continue;
        }
        const int64_t f = order[begin], c = end - begin;
        std::memcpy(out_planes + g * kPlaneFloats, planes + f * kPlaneFloats, kPlaneFloats * sizeof(float));
        std::memcpy(out_masks + g * kActions, masks + f * kActions, kActions);
        merge_group(policy, value, soft, sym, order + begin, c, out_policy + g * kActions, out_value + g, out_soft + g);
        out_count[g] = (int32_t)(c > 0x7FFFFFFF ? 0x7FFFFFFF : c);
    }
    return LZ_OK;
}

int lz_replay_position_keys(const void* records, int64_t capacity, const int64_t* slot, int64_t m, int32_t symmetric,
                            int64_t* keys, int8_t* sym, int32_t* not_representable, void*) {
    if (m < 0 || capacity < 0 || (symmetric != 0 && symmetric != 1)) return LZ_ERR_ARG;
    if (m == 0) return LZ_OK;
    if (!slot || !keys || !sym || !not_representable || (capacity > 0 && !records)) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(keys)) % 8 ||
        reinterpret_cast<uintptr_t>(not_representable) % 4) return LZ_ERR_ALIGN;
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(records);
    for (int64_t j = 0; j < m; ++j) {
        const int64_t s = slot[j];
        if (s < 0 || s >= capacity) {                         // outside the ring: a key of its own
            key_not_representable(j, keys + j * kKeyWords);
            sym[j] = 0;
            *not_representable += 1;
            continue;
        }
        lzrmerge::record_key(rec + s * lzrmerge::kRecBytes, symmetric != 0, keys + j * kKeyWords, sym + j);
    }
    return LZ_OK;
}

int lz_replay_merge_records(const void* records, int64_t capacity, const int64_t* slot, int64_t m, const int8_t* sym,
                            const int64_t* order, const int64_t* group_begin, int64_t groups, void* out_records,
                            int32_t* out_count, int32_t* not_representable, void*) {
    if (m < 0 || groups < 0 || capacity < 0) return LZ_ERR_ARG;
    if (m == 0 || groups == 0) return LZ_OK;
    if (!slot || !sym || !order || !group_begin || !out_records || !out_count || !not_representable ||
        (capacity > 0 && !records)) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(order) |
         reinterpret_cast<uintptr_t>(group_begin) | reinterpret_cast<uintptr_t>(out_records)) % 8 ||
        (reinterpret_cast<uintptr_t>(out_count) | reinterpret_cast<uintptr_t>(not_representable)) % 4) return LZ_ERR_ALIGN;
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(records);
    uint8_t* out = reinterpret_cast<uint8_t*>(out_records);
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t begin = group_begin[g], end = group_begin[g + 1];
        bool bad = begin < 0 || end <= begin || end > m;      // an empty or impossible range: a zero record
        for (int64_t i = begin; !bad && i < end; ++i) {
            const int64_t p = order[i];
            bad = p < 0 || p >= m || slot[p] < 0 || slot[p] >= capacity || sym[p] < 0 || sym[p] >= kSyms;
        }
        if (bad) {
            std::memset(out + g * lzrmerge::kRecBytes, 0, lzrmerge::kRecBytes);
            out_count[g] = 0;
            continue;
        }
        const int64_t c = end - begin;
        if (lzrmerge::merge_record_group(rec, slot, sym, order + begin, c, out + g * lzrmerge::kRecBytes))
            *not_representable += 1;
        out_count[g] = (int32_t)(c > 0x7FFFFFFF ? 0x7FFFFFFF : c);
    }
    return LZ_OK;
}

}  // extern "C"
