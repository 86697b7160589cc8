// lz_value_dist.hip -- gfx950 kernel of lz_merge_value_distributions (include/liuzhou_hip.h, csrc/lz_value_dist.h;
// DESIGN.md section 31).
//
// One wave per group, four waves per block, as lz_dedup.hip and lz_replay_merge.hip.  The members are taken 64 at a
// time: lane t loads member t's position, element, value and soft, so that 64 members cost one chain of memory
// latencies, and computes that member's lo / hi / frac (once per member, 64 members side by side); then member after
// member lo and frac are broadcast from the lanes and lane l adds the member's mass on bins l and l + 64 to its two
// double accumulators -- the sequential sum of lz_value_dist.h.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/liuzhou_hip.h"
#include "lz_value_dist.h"

using namespace lzvdist;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kBlock) void merge_value_distributions_kernel(
        const uint8_t* __restrict__ value_base, const uint8_t* __restrict__ soft_base, int64_t stride_bytes, int64_t n,
        const int64_t* __restrict__ index, int64_t m, const int64_t* __restrict__ order,
        const int64_t* __restrict__ group_begin, int64_t groups, const int32_t* __restrict__ dist_row, float alpha,
        float* __restrict__ dist, int64_t D) {
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t g = (int64_t)blockIdx.x * kWavesPerBlock + wv;
    if (g >= groups) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int d = __builtin_amdgcn_readfirstlane(dist_row[g]);
    if (d < 0 || (int64_t)d >= D) return;                      // this group has no row of the table
    const int64_t begin = uniform64(group_begin[g]), end = uniform64(group_begin[g + 1]);
    bool bad = begin < 0 || end <= begin || end > m;           // an empty or impossible range: a zero row
    double s0 = 0.0, s1 = 0.0;
    if (!bad) {
#pragma unroll 1
        for (int64_t c0 = begin; c0 < end; c0 += kWave) {
            const int lim = (int)(end - c0 < kWave ? end - c0 : kWave);
            const bool have = lane < lim;
            const int64_t p = have ? order[c0 + lane] : 0;
            const bool in_p = p >= 0 && p < m;
            const int64_t e = !(have && in_p) ? 0 : (index != nullptr ? index[p] : p);
            const bool valid = in_p && e >= 0 && e < n;
            if (__any(have && !valid)) { bad = true; break; }
            float v = 0.f, s = 0.f;
            if (have) {
                v = *reinterpret_cast<const float*>(value_base + e * stride_bytes);
                s = *reinterpret_cast<const float*>(soft_base + e * stride_bytes);
            }
            const TwoHot mine = two_hot(v, s, alpha);          // lane t: member t's bins, once per member
            for (int t = 0; t < lim; ++t) {
                TwoHot th;                                     // member t's, broadcast: wave-uniform
                th.lo = __builtin_amdgcn_readlane(mine.lo, t);
                th.hi = th.lo + 1 > kBins - 1 ? kBins - 1 : th.lo + 1;
                th.frac = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.frac), t));
                s0 += (double)bin_mass(th, lane);
                s1 += (double)bin_mass(th, lane + kWave);
            }
        }
    }
    float* row = dist + (int64_t)d * kBins;
    const double c = (double)(end - begin);
    row[lane] = bad ? 0.f : (float)(s0 / c);
    if (lane + kWave < kBins) row[lane + kWave] = bad ? 0.f : (float)(s1 / c);
}

}  // namespace

extern "C" int lz_merge_value_distributions(const void* value_base, const void* soft_base, int64_t stride_bytes, int64_t n,
                                            const int64_t* index, int64_t m, const int64_t* order,
                                            const int64_t* group_begin, int64_t groups, const int32_t* dist_row,
                                            float alpha, float* dist, int64_t D, void* stream) {
    if (n < 0 || m < 0 || groups < 0 || D < 0 || stride_bytes < 4) return LZ_ERR_ARG;
    if (groups == 0 || D == 0) return LZ_OK;
    if (!group_begin || !dist_row || !dist || (m > 0 && !order) || (n > 0 && (!value_base || !soft_base)))
        return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(order) | reinterpret_cast<uintptr_t>(group_begin)) % 8 ||
        (reinterpret_cast<uintptr_t>(value_base) | reinterpret_cast<uintptr_t>(soft_base) | (uintptr_t)stride_bytes |
         reinterpret_cast<uintptr_t>(dist_row) | reinterpret_cast<uintptr_t>(dist)) % 4)
        return LZ_ERR_ALIGN;
    const unsigned grid = (unsigned)((groups + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(merge_value_distributions_kernel, dim3(grid), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint8_t*>(value_base), reinterpret_cast<const uint8_t*>(soft_base),
                       stride_bytes, n, index, m, order, group_begin, groups, dist_row, alpha, dist, D);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}
