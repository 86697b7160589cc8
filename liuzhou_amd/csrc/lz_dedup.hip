// lz_dedup.hip -- gfx950 kernels of the position-dedup entry points (include/liuzhou_hip.h, csrc/lz_dedup.h).
//
// position_keys: one wave per row.  Lanes 0..35 load the four board planes, one ballot per board gives the bit words;
// the seven phase planes are 252 consecutive floats, read with four lane-strided loads and cut out of the ballots; the
// eight images come from ballots of the inverse cell (lz_symmetry.h: sym_packed_wave); the mask is permuted with
// lane-strided loads, one ballot per 64 actions.  Lane 0 stores 64 + 1 bytes.
//
// merge_groups: one wave per group.  Lane l owns the output actions l, l+64, l+128, l+192 and GATHERS each member's
// policy at the action that the member's frame map sends there; the sums follow the association of lz_dedup.h (chunks of
// 256 members).  Planes and mask are copied from the first member.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz_dedup.h"
#include "lz_soa.h"

using namespace lz;
using namespace lzdedup;

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int launch_status() { return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH; }
inline unsigned grid_waves(int64_t items) { return (unsigned)((items + kWavesPerBlock - 1) / kWavesPerBlock); }

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ int64_t wave_item() {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    return (int64_t)blockIdx.x * kWavesPerBlock + w;
}
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// 36 bits at bit offset `off` (a constant after unrolling) of the 256-bit string b0 | b1<<64 | b2<<128 | b3<<192
__device__ __forceinline__ uint64_t field36(uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3, int off) {
    const int w = off >> 6, sh = off & 63;
    const uint64_t lo = w == 0 ? b0 : w == 1 ? b1 : w == 2 ? b2 : b3;
    const uint64_t hi = w == 0 ? b1 : w == 1 ? b2 : w == 2 ? b3 : 0ull;
    return ((lo >> sh) | (sh ? hi << (64 - sh) : 0ull)) & kFull;
}

__global__ __launch_bounds__(kBlock) void position_keys_kernel(const float* __restrict__ planes, const uint8_t* __restrict__ masks,
                                                               int64_t n, int symmetric, int64_t* __restrict__ keys,
                                                               int8_t* __restrict__ sym, int32_t* __restrict__ not_representable) {
    const int64_t i = wave_item();
    if (i >= n) return;
    const int lane = lane_id();
    const bool in = lane < 36;
    const float* pl = planes + i * kPlaneFloats;
    uint64_t w[4];
    bool ok = true;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float x = in ? pl[p * 36 + lane] : 0.f;
        w[p] = (uint64_t)__ballot(in && value_set(x));
        ok = board_plane_ok((uint64_t)__ballot(value_good(x))) && ok;
    }
    uint64_t ps[4], pg[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int q = it * kWave + lane;
        const float x = q < 252 ? pl[144 + q] : 0.f;
        ps[it] = (uint64_t)__ballot(value_set(x));
        pg[it] = (uint64_t)__ballot(value_good(x));
    }
    int phase = 0;
#pragma unroll
    for (int ph = 1; ph <= 7; ++ph)
        ok = phase_plane_step(field36(ps[0], ps[1], ps[2], ps[3], 36 * (ph - 1)),
                              field36(pg[0], pg[1], pg[2], pg[3], 36 * (ph - 1)), ph, phase) && ok;
    if (!ok) {                                                // wave-uniform
        if (lane == 0) {
            key_not_representable(i, keys + i * kKeyWords);
            sym[i] = 0;
            atomicAdd(not_representable, 1);
        }
        return;
    }
    uint64_t b0 = w[0], b1 = w[1], b2 = w[2], b3 = w[3];
    int best = 0;
    if (symmetric) {
#pragma unroll
        for (int k = 1; k < kSyms; ++k) {
            const int src = in ? sym_cell(sym_inverse(k), lane) : 0;
            const uint64_t c0 = (uint64_t)__ballot(in && ((w[0] >> src) & 1ull));
            const uint64_t c1 = (uint64_t)__ballot(in && ((w[1] >> src) & 1ull));
            const uint64_t c2 = (uint64_t)__ballot(in && ((w[2] >> src) & 1ull));
            const uint64_t c3 = (uint64_t)__ballot(in && ((w[3] >> src) & 1ull));
            if (tuple_less(c0, c1, c2, c3, b0, b1, b2, b3)) { b0 = c0; b1 = c1; b2 = c2; b3 = c3; best = k; }
        }
    }
    best = __builtin_amdgcn_readfirstlane(best);
    const int inv = sym_inverse(best);
    const uint8_t* mk = masks + i * kActions;
    uint64_t mw[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int b = it * kWave + lane;
        const bool have = b < kActions;
        const int a = have ? kSym.action[inv][b] : 0;          // image bit b = mask[P^-1(b)]
        mw[it] = (uint64_t)__ballot(have && mk[a] != 0);
    }
    if (lane == 0) {
        int64_t* out = keys + i * kKeyWords;
        out[0] = (int64_t)(b0 | ((uint64_t)phase << 36)); out[1] = (int64_t)b1; out[2] = (int64_t)b2; out[3] = (int64_t)b3;
        out[4] = (int64_t)mw[0]; out[5] = (int64_t)mw[1]; out[6] = (int64_t)mw[2]; out[7] = (int64_t)mw[3];
        sym[i] = (int8_t)best;
    }
}

__global__ __launch_bounds__(kBlock) void merge_groups_kernel(
        const float* __restrict__ planes, const uint8_t* __restrict__ masks, const float* __restrict__ policy,
        const float* __restrict__ value, const float* __restrict__ soft, int64_t n, const int8_t* __restrict__ sym,
        const int64_t* __restrict__ order, const int64_t* __restrict__ group_begin, int64_t groups,
        float* __restrict__ out_planes, uint8_t* __restrict__ out_masks, float* __restrict__ out_policy,
        float* __restrict__ out_value, float* __restrict__ out_soft, int32_t* __restrict__ out_count) {
    const int64_t g = wave_item();
    if (g >= groups) return;
    const int lane = lane_id();
    const int64_t begin = uniform64(group_begin[g]), end = uniform64(group_begin[g + 1]);
    bool bad = begin < 0 || end <= begin || end > n;           // an empty or impossible range: a zero row
    const int64_t c = bad ? 0 : end - begin;
    const bool own3 = lane + 192 < kActions;
    int64_t first = -1;
    int sf = 0;
    if (!bad) {
        first = uniform64(order[begin]);
        bad = first < 0 || first >= n;
        if (!bad) { sf = __builtin_amdgcn_readfirstlane((int)sym[first]); bad = sf < 0 || sf >= kSyms; }
    }
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0, ov = 0, os = 0;     // the output row's policy / value / soft bits
    if (!bad && c == 1) {                                      // a group of one: a bit copy
        const uint32_t* p = reinterpret_cast<const uint32_t*>(policy + first * kActions);
        o0 = p[lane]; o1 = p[lane + 64]; o2 = p[lane + 128]; o3 = own3 ? p[lane + 192] : 0u;
        ov = reinterpret_cast<const uint32_t*>(value)[first]; os = reinterpret_cast<const uint32_t*>(soft)[first];
    } else if (!bad) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, tv = 0.0, ts = 0.0;
        int64_t cp = 0;
        for (int64_t c0 = begin; c0 < end; c0 += kChunk) {
            const int cnt = (int)(c0 + kChunk < end ? kChunk : end - c0);
            // the chunk's members and their frame maps, 64 at a time: lane t holds member 64 j + t
            int64_t mj[4];
            int ej[4];
            bool wrong = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = j * kWave + lane;
                const bool have = idx < cnt;
                const int64_t m = have ? order[c0 + idx] : 0;
                const bool in = m >= 0 && m < n;
                const int sm = have && in ? (int)sym[m] : 0;
                wrong = wrong || !in || sm < 0 || sm >= kSyms;
                mj[j] = m;
                // out[b] takes policy[m][P_e^-1(b)], e = sym[f]^-1 o sym[m]; e^-1 = sym[m]^-1 o sym[f]
                ej[j] = kSym.comp[sym_inverse(sm & 7)][sf];
            }
            if (__any(wrong)) { bad = true; break; }
            double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0, pv = 0.0, pS = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int lim = cnt - j * kWave < kWave ? cnt - j * kWave : kWave;
                // four members' loads in flight, their terms added in member order; a slot past the end rereads
                // member t and contributes +0.0, which changes no sum (no partial sum is ever -0.0)
                for (int t = 0; t < lim; t += 4) {
                    float x0[4], x1[4], x2[4], x3[4], xv[4], xs[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool on = t + u < lim;
                        const int tt = on ? t + u : t;
                        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)(uint64_t)mj[j], tt);
                        const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)mj[j] >> 32), tt);
                        const int64_t m = (int64_t)(((uint64_t)hi << 32) | lo);
                        const int16_t* tab = kSym.action[__builtin_amdgcn_readlane(ej[j], tt)];
                        const float* p = policy + m * kActions;
                        const float a0 = p[tab[lane]], a1 = p[tab[lane + 64]], a2 = p[tab[lane + 128]];
                        const float a3 = own3 ? p[tab[lane + 192]] : 0.f;
                        x0[u] = on ? a0 : 0.f; x1[u] = on ? a1 : 0.f; x2[u] = on ? a2 : 0.f; x3[u] = on ? a3 : 0.f;
                        xv[u] = on ? value[m] : 0.f; xs[u] = on ? soft[m] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        p0 += (double)x0[u]; p1 += (double)x1[u]; p2 += (double)x2[u]; p3 += (double)x3[u];
                        cp += __any(x0[u] != 0.f || x1[u] != 0.f || x2[u] != 0.f || x3[u] != 0.f) ? 1 : 0;
                        pv += (double)xv[u]; pS += (double)xs[u];
                    }
                }
            }
            t0 += p0; t1 += p1; t2 += p2; t3 += p3; tv += pv; ts += pS;
        }
        if (!bad) {
            const double d = (double)cp;
            o0 = cp > 0 ? __float_as_uint((float)(t0 / d)) : 0u; o1 = cp > 0 ? __float_as_uint((float)(t1 / d)) : 0u;
            o2 = cp > 0 ? __float_as_uint((float)(t2 / d)) : 0u; o3 = cp > 0 ? __float_as_uint((float)(t3 / d)) : 0u;
            ov = __float_as_uint((float)(tv / (double)c)); os = __float_as_uint((float)(ts / (double)c));
        }
    }
    uint32_t* po = reinterpret_cast<uint32_t*>(out_policy + g * kActions);
    uint4* plo = reinterpret_cast<uint4*>(out_planes + g * kPlaneFloats);        // 1584 bytes = 99 pieces of 16
    uint32_t* mo = reinterpret_cast<uint32_t*>(out_masks + g * kActions);        // 220 bytes = 55 words
    if (bad) {                                                 // a zero row, count 0
        po[lane] = 0u; po[lane + 64] = 0u; po[lane + 128] = 0u;
        if (own3) po[lane + 192] = 0u;
        for (int q = lane; q < 99; q += kWave) plo[q] = make_uint4(0u, 0u, 0u, 0u);
        if (lane < 55) mo[lane] = 0u;
        if (lane == 0) { out_value[g] = 0.f; out_soft[g] = 0.f; out_count[g] = 0; }
        return;
    }
    po[lane] = o0; po[lane + 64] = o1; po[lane + 128] = o2;
    if (own3) po[lane + 192] = o3;
    const uint4* pli = reinterpret_cast<const uint4*>(planes + first * kPlaneFloats);
    for (int q = lane; q < 99; q += kWave) plo[q] = pli[q];
    if (lane < 55) mo[lane] = reinterpret_cast<const uint32_t*>(masks + first * kActions)[lane];
    if (lane == 0) {
        reinterpret_cast<uint32_t*>(out_value)[g] = ov; reinterpret_cast<uint32_t*>(out_soft)[g] = os;
        out_count[g] = (int32_t)(c > 0x7FFFFFFF ? 0x7FFFFFFF : c);
    }
}

}  // namespace

extern "C" {

int lz_dedup_position_keys(const float* planes, const uint8_t* masks, int64_t n, int32_t symmetric, int64_t* keys,
                           int8_t* sym, int32_t* not_representable, void* stream) {
    if (n < 0 || (symmetric != 0 && symmetric != 1)) return LZ_ERR_ARG;
    if (n == 0) return LZ_OK;
    if (!planes || !masks || !keys || !sym || !not_representable) return LZ_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(planes) % 4 || reinterpret_cast<uintptr_t>(keys) % 8 ||
        reinterpret_cast<uintptr_t>(not_representable) % 4) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(position_keys_kernel, dim3(grid_waves(n)), dim3(kBlock), 0, as_stream(stream), planes, masks, n,
                       (int)symmetric, keys, sym, not_representable);
    return launch_status();
}

int lz_dedup_merge_groups(const float* planes, const uint8_t* masks, const float* policy, const float* value,
                          const float* soft, int64_t n, const int8_t* sym, const int64_t* order,
                          const int64_t* group_begin, int64_t groups, float* out_planes, uint8_t* out_masks,
                          float* out_policy, float* out_value, float* out_soft, int32_t* out_count, void* stream) {
    if (n < 0 || groups < 0) return LZ_ERR_ARG;
    if (groups == 0) return LZ_OK;
    if (!group_begin || !out_planes || !out_masks || !out_policy || !out_value || !out_soft || !out_count) return LZ_ERR_ARG;
    if (n > 0 && !(planes && masks && policy && value && soft && sym && order)) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(out_planes)) % 16 ||
        (reinterpret_cast<uintptr_t>(masks) | reinterpret_cast<uintptr_t>(out_masks) | reinterpret_cast<uintptr_t>(policy) |
         reinterpret_cast<uintptr_t>(out_policy) | reinterpret_cast<uintptr_t>(value) | reinterpret_cast<uintptr_t>(soft) |
         reinterpret_cast<uintptr_t>(out_value) | reinterpret_cast<uintptr_t>(out_soft) |
         reinterpret_cast<uintptr_t>(out_count)) % 4 ||
        (reinterpret_cast<uintptr_t>(order) | reinterpret_cast<uintptr_t>(group_begin)) % 8) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(merge_groups_kernel, dim3(grid_waves(groups)), dim3(kBlock), 0, as_stream(stream), planes, masks,
                       policy, value, soft, n, sym, order, group_begin, groups, out_planes, out_masks, out_policy,
                       out_value, out_soft, out_count);
    return launch_status();
}

}  // extern "C"
