// lz_value_dist_host.cpp -- host (CPU-tensor) build of lz_merge_value_distributions (include/liuzhou_hip.h), part of
// libliuzhou_host.so: the arithmetic of csrc/lz_value_dist.h as a plain loop over the groups, with the semantics of
// lz_value_dist.hip.  `stream` is ignored.
#include <cstdint>
#include <cstring>

#include "../../include/liuzhou_hip.h"
#include "lz_value_dist.h"

using namespace lzvdist;

extern "C" int lz_merge_value_distributions(const void* value_base, const void* soft_base, int64_t stride_bytes, int64_t n,
                                            const int64_t* index, int64_t m, const int64_t* order,
                                            const int64_t* group_begin, int64_t groups, const int32_t* dist_row,
                                            float alpha, float* dist, int64_t D, void*) {
    if (n < 0 || m < 0 || groups < 0 || D < 0 || stride_bytes < 4) return LZ_ERR_ARG;
    if (groups == 0 || D == 0) return LZ_OK;
    if (!group_begin || !dist_row || !dist || (m > 0 && !order) || (n > 0 && (!value_base || !soft_base)))
        return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(order) | reinterpret_cast<uintptr_t>(group_begin)) % 8 ||
        (reinterpret_cast<uintptr_t>(value_base) | reinterpret_cast<uintptr_t>(soft_base) | (uintptr_t)stride_bytes |
         reinterpret_cast<uintptr_t>(dist_row) | reinterpret_cast<uintptr_t>(dist)) % 4)
        return LZ_ERR_ALIGN;
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t d = dist_row[g];
        if (d < 0 || d >= D) continue;                        // this group has no row of the table
        const int64_t begin = group_begin[g], end = group_begin[g + 1];
        bool bad = begin < 0 || end <= begin || end > m;      // an empty or impossible range: a zero row
        for (int64_t i = begin; !bad && i < end; ++i) {
            const int64_t p = order[i];
            bad = p < 0 || p >= m;
            if (!bad) {
                const int64_t e = index ? index[p] : p;
                bad = e < 0 || e >= n;
            }
        }
        float* row = dist + d * kBins;
        if (bad) {
            std::memset(row, 0, kBins * sizeof(float));
            continue;
        }
        group_distribution(value_base, soft_base, stride_bytes, index, order + begin, end - begin, alpha, row);
    }
    return LZ_OK;
}
