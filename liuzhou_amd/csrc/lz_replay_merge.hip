// lz_replay_merge.hip -- gfx950 kernels of the record-to-record dedup entry points over the replay window
// (include/liuzhou_hip.h, csrc/lz_replay_merge.h).
//
// replay_position_keys: one wave per selected record.  The 11 header words (4 boards, 7 mask words) have a wave-uniform
// address and are loaded once; the eight board images come from ballots of the inverse cell, as position_keys_kernel
// takes them from its planes; image bit b of the legal words is the record's bit kSym.action[k*^-1][b], one ballot per 64
// actions.  88 bytes are read per row, lane 0 stores 64 + 1.
//
// replay_merge_records: one wave per group.  Lane l owns the output policy slots l and l + 64 (72 slots), that is the
// first member's l-th and (l + 64)-th legal actions, found once per group by a select on the mask words.  The members
// are taken 64 at a time: lane t loads member t's slot, frame, mask words, value and soft and scans its policy slots for
// c_p, so that 64 headers cost one memory latency; then member after member the words are broadcast from the lanes and
// the lane's value is fetched from the member's record at the rank of the action that the member's frame map sends to
// the lane's action: prefix popcounts of the mask words, one popcount per lane, as in replay_gather_rows_kernel.  The sums follow the association of lz_dedup.h (chunks of 256 members).  No LDS, no
// atomics but the counter, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz_replay_merge.h"
#include "lz_soa.h"

using namespace lz;
using namespace lzdedup;
using namespace lzrmerge;

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
__device__ __forceinline__ uint32_t readlane32(uint32_t v, int t) {     // the builtin returns int: no sign extension
    return (uint32_t)__builtin_amdgcn_readlane((int)v, t);
}
__device__ __forceinline__ int64_t readlane64(int64_t v, int t) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)(uint64_t)v, t);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), t);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kBlock) void replay_position_keys_kernel(
        const uint8_t* __restrict__ in, int64_t capacity, const int64_t* __restrict__ slot, int64_t m, int symmetric,
        int64_t* __restrict__ keys, int8_t* __restrict__ sym, int32_t* __restrict__ not_representable) {
    const int64_t j = wave_item();
    if (j >= m) return;
    const int lane = lane_id();
    const int64_t s = uniform64(slot[j]);
    if (s < 0 || s >= capacity) {                              // wave-uniform: outside the ring
        if (lane == 0) {
            key_not_representable(j, keys + j * kKeyWords);
            sym[j] = 0;
            atomicAdd(not_representable, 1);
        }
        return;
    }
    const Header h = read_header(in + s * kRecBytes);          // uniform address: once per row
    const bool inb = lane < 36;
    const uint64_t w0 = h.w[0] & kFull, w1 = h.w[1] & kFull, w2 = h.w[2] & kFull, w3 = h.w[3] & kFull;
    uint64_t b0 = w0, b1 = w1, b2 = w2, b3 = w3;
    int best = 0;
    if (symmetric) {
#pragma unroll
        for (int k = 1; k < kSyms; ++k) {
            const int src = inb ? sym_cell(sym_inverse(k), lane) : 0;
            const uint64_t c0 = (uint64_t)__ballot(inb && ((w0 >> src) & 1ull));
            const uint64_t c1 = (uint64_t)__ballot(inb && ((w1 >> src) & 1ull));
            const uint64_t c2 = (uint64_t)__ballot(inb && ((w2 >> src) & 1ull));
            const uint64_t c3 = (uint64_t)__ballot(inb && ((w3 >> src) & 1ull));
            if (tuple_less(c0, c1, c2, c3, b0, b1, b2, b3)) { b0 = c0; b1 = c1; b2 = c2; b3 = c3; best = k; }
        }
    }
    best = __builtin_amdgcn_readfirstlane(best);
    const int inv = sym_inverse(best);
    uint64_t mw[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int b = it * kWave + lane;
        const bool have = b < kActions;
        const int a = have ? kSym.action[inv][b] : 0;          // image bit b = legal bit P^-1(b)
        mw[it] = (uint64_t)__ballot(have && legal_bit(h, a));
    }
    if (lane == 0) {
        int64_t* out = keys + j * kKeyWords;
        out[0] = (int64_t)(b0 | ((uint64_t)header_phase(h) << 36)); out[1] = (int64_t)b1; out[2] = (int64_t)b2;
        out[3] = (int64_t)b3;
        out[4] = (int64_t)mw[0]; out[5] = (int64_t)mw[1]; out[6] = (int64_t)mw[2]; out[7] = (int64_t)mw[3];
        sym[j] = (int8_t)best;
    }
}

__global__ __launch_bounds__(kBlock) void replay_merge_records_kernel(
        const uint8_t* __restrict__ in, int64_t capacity, const int64_t* __restrict__ slot, int64_t m,
        const int8_t* __restrict__ sym, const int64_t* __restrict__ order, const int64_t* __restrict__ group_begin,
        int64_t groups, uint8_t* __restrict__ out, int32_t* __restrict__ out_count,
        int32_t* __restrict__ not_representable) {
    const int64_t g = wave_item();
    if (g >= groups) return;
    const int lane = lane_id();
    const int64_t begin = uniform64(group_begin[g]), end = uniform64(group_begin[g + 1]);
    bool bad = begin < 0 || end <= begin || end > m;           // an empty or impossible range: a zero record
    const int64_t c = bad ? 0 : end - begin;
    int64_t sfirst = -1;
    int sf = 0;
    if (!bad) {
        const int64_t first = uniform64(order[begin]);
        bad = first < 0 || first >= m;
        if (!bad) {
            sfirst = uniform64(slot[first]);
            sf = __builtin_amdgcn_readfirstlane((int)sym[first]);
            bad = sfirst < 0 || sfirst >= capacity || sf < 0 || sf >= kSyms;
        }
    }
    Header hf = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    int legal = 0;
    bool own0 = false, own1 = false;                           // whether the lane's slots l, l + 64 are legal slots
    int a0 = 0, a1 = 0;                                        // the first member's actions of those slots
    if (!bad) {
        hf = read_header(in + sfirst * kRecBytes);
        legal = legal_count(hf);
        const int used = legal < kPolicySlots ? legal : kPolicySlots;
        own0 = lane < used; own1 = lane + kWave < used;
        a0 = own0 ? legal_action(hf, lane) : 0; a1 = own1 ? legal_action(hf, lane + kWave) : 0;
    }
    uint32_t o0 = 0, o1 = 0, ov = 0, os = 0;                    // the output record's policy / value / soft bits
    if (!bad && c == 1) {                                      // a group of one: a bit copy
        const uint32_t* pf = reinterpret_cast<const uint32_t*>(in + sfirst * kRecBytes + kPolicyOff);
        const uint32_t* vf = reinterpret_cast<const uint32_t*>(in + sfirst * kRecBytes + kValueOff);
        o0 = own0 ? pf[lane] : 0u; o1 = own1 ? pf[lane + kWave] : 0u;
        ov = vf[0]; os = vf[1];
    } else if (!bad) {
        double t0 = 0.0, t1 = 0.0, tv = 0.0, ts = 0.0;
        int64_t cp = 0;
        for (int64_t c0 = begin; c0 < end; c0 += kChunk) {
            const int cnt = (int)(c0 + kChunk < end ? kChunk : end - c0);
            double p0 = 0.0, p1 = 0.0, pv = 0.0, pS = 0.0;
#pragma unroll 1
            for (int j = 0; j < kChunk / kWave && !bad; ++j) {
                const int lim = cnt - j * kWave < kWave ? cnt - j * kWave : kWave;
                if (lim <= 0) break;
                // 64 members at a time, one per lane: the lane loads ITS member's slot, frame, mask words, value and
                // soft and scans its policy slots, so that 64 headers cost one memory latency; below, the members are
                // taken in order and their words broadcast from the lanes
                const bool have = lane < lim;
                const int64_t p = have ? order[c0 + j * kWave + lane] : 0;
                const bool in_p = p >= 0 && p < m;
                const int64_t s = have && in_p ? slot[p] : 0;
                const int sm = have && in_p ? (int)sym[p] : 0;
                const bool valid = in_p && s >= 0 && s < capacity && sm >= 0 && sm < kSyms;
                if (__any(have && !valid)) { bad = true; break; }
                const uint8_t* rl = in + (have ? s : sfirst) * kRecBytes;       // an idle lane rereads the first member
                const uint32_t* ml = reinterpret_cast<const uint32_t*>(rl + kMaskOff);
                const uint32_t m0 = ml[0], m1 = ml[1], m2 = ml[2], m3 = ml[3], m4 = ml[4], m5 = ml[5],
                               m6 = ml[6] & kLastMaskWord;
                const uint32_t vb = reinterpret_cast<const uint32_t*>(rl + kValueOff)[0],
                               sb = reinterpret_cast<const uint32_t*>(rl + kValueOff)[1];
                const int lc = __builtin_popcount(m0) + __builtin_popcount(m1) + __builtin_popcount(m2) + __builtin_popcount(m3) +
                               __builtin_popcount(m4) + __builtin_popcount(m5) + __builtin_popcount(m6);
                const int lm = lc < kPolicySlots ? lc : kPolicySlots;
                const float* pl = reinterpret_cast<const float*>(rl + kPolicyOff);
                bool mine = false;                             // c_p: a non-zero entry among the first min(count, 72) slots
#pragma unroll 8
                for (int r = 0; r < kPolicySlots; ++r) mine = mine || (r < lm && pl[r] != 0.f);
                cp += __popcll(__ballot(have && mine));
                // slot of action b takes the member's policy at P_e^-1(b), e = sym[f]^-1 o sym[m]; e^-1 = sym[m]^-1 o sym[f]
                const int ei = kSym.comp[sym_inverse(sm & 7)][sf];
                // four members' loads in flight, their terms added in member order; a place past the end rereads
                // member t and contributes +0.0, which changes no sum (no partial sum is ever -0.0)
                for (int t = 0; t < lim; t += 4) {
                    float x0[4], x1[4], xv[4], xs[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool on = t + u < lim;
                        const int tt = on ? t + u : t;
                        const uint8_t* rm = in + readlane64(s, tt) * kRecBytes;
                        const int16_t* tab = kSym.action[__builtin_amdgcn_readlane(ei, tt)];
                        Header hm = {{0, 0, 0, 0}, {0, 0, 0, 0}};
                        hm.b[0] = (uint64_t)readlane32(m0, tt) | ((uint64_t)readlane32(m1, tt) << 32);
                        hm.b[1] = (uint64_t)readlane32(m2, tt) | ((uint64_t)readlane32(m3, tt) << 32);
                        hm.b[2] = (uint64_t)readlane32(m4, tt) | ((uint64_t)readlane32(m5, tt) << 32);
                        hm.b[3] = (uint64_t)readlane32(m6, tt);
                        const uint32_t q0 = policy_bits(rm, hm, tab[a0]), q1 = policy_bits(rm, hm, tab[a1]);
                        x0[u] = on && own0 ? __uint_as_float(q0) : 0.f; x1[u] = on && own1 ? __uint_as_float(q1) : 0.f;
                        xv[u] = on ? __uint_as_float(readlane32(vb, tt)) : 0.f;
                        xs[u] = on ? __uint_as_float(readlane32(sb, tt)) : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        p0 += (double)x0[u]; p1 += (double)x1[u];
                        pv += (double)xv[u]; pS += (double)xs[u];
                    }
                }
            }
            if (bad) break;
            t0 += p0; t1 += p1; tv += pv; ts += pS;
        }
        if (!bad) {
            const double d = (double)cp;
            o0 = cp > 0 && own0 ? __float_as_uint((float)(t0 / d)) : 0u;
            o1 = cp > 0 && own1 ? __float_as_uint((float)(t1 / d)) : 0u;
            ov = __float_as_uint((float)(tv / (double)c)); os = __float_as_uint((float)(ts / (double)c));
        }
    }
    if (bad) {                                                 // a zero record, count 0
        hf = Header{{0, 0, 0, 0}, {0, 0, 0, 0}};
        o0 = 0u; o1 = 0u; ov = 0u; os = 0u; legal = 0;
    }
    uint8_t* rec = out + g * kRecBytes;
    uint32_t* po = reinterpret_cast<uint32_t*>(rec + kPolicyOff);
    po[lane] = o0;
    if (lane < kPolicySlots - kWave) po[lane + kWave] = o1;
    if (lane == 0) {
        write_header(hf, rec);
        uint32_t* vo = reinterpret_cast<uint32_t*>(rec + kValueOff);
        vo[0] = ov; vo[1] = os; vo[2] = 0u;
        out_count[g] = bad ? 0 : (int32_t)(c > 0x7FFFFFFF ? 0x7FFFFFFF : c);
        if (legal > kPolicySlots) atomicAdd(not_representable, 1);
    }
}

}  // namespace

extern "C" {

int lz_replay_position_keys(const void* records, int64_t capacity, const int64_t* slot, int64_t m, int32_t symmetric,
                            int64_t* keys, int8_t* sym, int32_t* not_representable, void* stream) {
    if (m < 0 || capacity < 0 || (symmetric != 0 && symmetric != 1)) return LZ_ERR_ARG;
    if (m == 0) return LZ_OK;
    if (!slot || !keys || !sym || !not_representable || (capacity > 0 && !records)) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(keys)) % 8 ||
        reinterpret_cast<uintptr_t>(not_representable) % 4) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(replay_position_keys_kernel, dim3(grid_waves(m)), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<const uint8_t*>(records), capacity, slot, m, (int)symmetric, keys, sym,
                       not_representable);
    return launch_status();
}

int lz_replay_merge_records(const void* records, int64_t capacity, const int64_t* slot, int64_t m, const int8_t* sym,
                            const int64_t* order, const int64_t* group_begin, int64_t groups, void* out_records,
                            int32_t* out_count, int32_t* not_representable, void* stream) {
    if (m < 0 || groups < 0 || capacity < 0) return LZ_ERR_ARG;
    if (m == 0 || groups == 0) return LZ_OK;
    if (!slot || !sym || !order || !group_begin || !out_records || !out_count || !not_representable ||
        (capacity > 0 && !records)) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(order) |
         reinterpret_cast<uintptr_t>(group_begin) | reinterpret_cast<uintptr_t>(out_records)) % 8 ||
        (reinterpret_cast<uintptr_t>(out_count) | reinterpret_cast<uintptr_t>(not_representable)) % 4) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(replay_merge_records_kernel, dim3(grid_waves(groups)), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<const uint8_t*>(records), capacity, slot, m, sym, order, group_begin, groups,
                       reinterpret_cast<uint8_t*>(out_records), out_count, not_representable);
    return launch_status();
}

}  // extern "C"
