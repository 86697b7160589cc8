// lz_net.hip -- fused policy + bucketed-value ResNet forward for 6x6 Liuzhou boards on gfx950.
//
// One persistent workgroup (8 waves, two per SIMD) owns S samples (S*36 board cells) and runs the WHOLE
// network on them without touching HBM in between:
//   * the fp32 residual stream lives in MFMA accumulator registers for the whole trunk
//     (each wave owns 9 tiles of 16 cells x 2 tiles of 16 channels = 72 registers, plus 72 for the
//     conv1 output: 144 accumulators fit the AGPR half of the 256-register budget of 2 waves/SIMD);
//   * conv inputs are staged as fp16 [cell][channel] rows in LDS (one buffer, rewritten per layer);
//   * every 3x3 conv is 9 shifted GEMMs on v_mfma_f32_16x16x32_f16 with the WEIGHTS as the A operand
//     (pre-packed in fragment order, streamed from L2 with one 16-byte load per lane) and the
//     activations as the B operand (one ds_read_b128 per lane; out-of-board taps read a zero row),
//     so the D tile has the cell on the lane and 4 consecutive channels in registers -> 8-byte LDS
//     writes for the next layer;
//   * BatchNorm is folded at pack time (liuzhou_amd/net_pack.py); heads (global pooling, small FCs,
//     log-softmax, bucket expectation) run on the same workgroup from LDS.
// Reference architecture: src/neural_network.py:67-259 (ChessNet.forward).  fp16 operands, fp32
// accumulate -- the counterpart of the reference's autocast-fp16 inference (v1/python/mcts_gpu.py:640-646).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <utility>
#include <vector>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/liuzhou_hip.h"
#include "lz_net_dev.h"
#include "lz_live_index.h"

namespace {

template <int C, int S, int W>
__global__ __launch_bounds__(W * 64, (C == 128 && W == 4) ? 1 : 2) void net_forward_kernel(NetParams P, const float* __restrict__ planes,
                                                            const uint64_t* __restrict__ packed,
                                                            int64_t N, float* __restrict__ lp1,
                                                            float* __restrict__ lp2, float* __restrict__ lpm,
                                                            float* __restrict__ vlogits, float* __restrict__ value) {
    if (P.n_dev != nullptr) { const long long nd = *P.n_dev; N = nd < N ? nd : N; }   // count produced on the device
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    NetCtx<C, S, W> ctx;
#ifdef LZ_EXP_HEAD_STAMPS
    ctx.t_entry = __builtin_readcyclecounter();
#endif
    net_setup<C, S, W>(P, lds, ctx);
#ifdef LZ_EXP_HEAD_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    ctx.t_setup = __builtin_readcyclecounter();
#endif
    // diagnostic (LZ_NET_DEBUG_STOP=99): shader clock held by this kernel = s_memtime ticks per 100 MHz wall tick
    const uint64_t dbg_t0 = P.debug_stop == 99 ? __builtin_readcyclecounter() : 0;
    const uint64_t dbg_w0 = P.debug_stop == 99 ? wall_clock64() : 0;
    const int64_t n_pass = (N + S - 1) / S;
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int64_t n0 = pass * S;
        const int nvalid = (int)((N - n0) < S ? (N - n0) : S);
        net_pass<C, S, W>(P, lds, ctx, planes, packed, n0, nvalid, lp1, lp2, lpm, vlogits, value);
    }
    if (P.debug_stop == 99 && blockIdx.x == 7 && threadIdx.x == 0) {
        const uint64_t dt = __builtin_readcyclecounter() - dbg_t0, dw = wall_clock64() - dbg_w0;
        value[0] = (float)dt; value[1] = (float)dw;
    }
}

template <int C, int S, int W>
int launch_net(const NetParams& P, const float* planes, const uint64_t* packed, int64_t N, float* lp1, float* lp2,
               float* lpm, float* vlogits, float* value, int max_blocks, hipStream_t st) {
    using K = Cfg<C, S, W>;
    auto kern = net_forward_kernel<C, S, W>;
    const int64_t n_pass = (N + S - 1) / S;
    int grid = (int)(n_pass < max_blocks ? n_pass : max_blocks);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(K::THREADS), K::LDS_BYTES, st, P, planes, packed, N, lp1, lp2, lpm, vlogits, value);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}

// ---- several networks of one architecture in one launch (lz_net_forward_packed_multi_f16) --------------------------------
// Network k owns the rows [align16(seg_off[k]), seg_off[k + 1]): every segment starts on a 16-row boundary (16 = the
// largest S), so no pass of S samples mixes two networks; rows between a segment's end and the next boundary are padding
// and no pass covers them.  The networks differ only in their two buffers: a pass looks up its segment (wave-uniform,
// from the pass index) and, when that differs from the workgroup's previous pass, points the buffer descriptors at that
// network's weights.  That is the whole per-network set-up: net_setup loads nothing network-specific (the head
// parameters are fetched by the pass that uses them) and every pass starts with a workgroup barrier.
constexpr int kMaxNets = 8;
struct MultiNets {
    const _Float16* wfrag[kMaxNets];
    const float* fp[kMaxNets];
};

template <int C, int S, int W>
__global__ __launch_bounds__(W * 64, (C == 128 && W == 4) ? 1 : 2) void net_forward_multi_kernel(
        NetParams P, MultiNets M, int num_nets, const uint64_t* __restrict__ packed, int64_t capacity,
        const long long* __restrict__ seg_off, float* __restrict__ lp1, float* __restrict__ lp2, float* __restrict__ lpm,
        float* __restrict__ vlogits, float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    NetCtx<C, S, W> ctx;
    net_setup<C, S, W>(P, lds, ctx);
    const long long total = seg_off[num_nets];
    const int last = (int)(total < capacity ? total : capacity);
    const int n_pass = (last + S - 1) / S;
    int cur = -1;
    const float* fp = nullptr;
    for (int pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int n0 = pass * S;
        // the pass's segment: the last one that starts at or before it (an empty segment starts where the next one does).
        // Re-read per pass (scalar loads, a few per pass of a whole network): nothing network-specific held in SGPRs
        int k = 0;
        for (int j = 1; j < num_nets; ++j)
            if (((seg_off[j] + 15) & ~15LL) <= n0) k = j;
        k = __builtin_amdgcn_readfirstlane(k);
        const long long b = (seg_off[k] + 15) & ~15LL, e = seg_off[k + 1] < last ? seg_off[k + 1] : last;
        const int nvalid = (int)((e - n0) < S ? (e - n0) : S);
        if (n0 < b || nvalid <= 0) continue;                       // padding behind a segment's live rows
        if (k != cur) {
            fp = M.fp[k];
            net_use_weights<C, S, W>(P, ctx, M.wfrag[k], fp);
            cur = k;
        }
        net_pass<C, S, W>(P, lds, ctx, nullptr, packed, (int64_t)n0, nvalid, lp1, lp2, lpm, vlogits, value, fp);
    }
}

template <int C, int S, int W>
int launch_net_multi(const NetParams& P, const MultiNets& M, int num_nets, const uint64_t* packed, int64_t capacity,
                     const int64_t* seg_off, float* lp1, float* lp2, float* lpm, float* vlogits, float* value,
                     int max_blocks, hipStream_t st) {
    using K = Cfg<C, S, W>;
    // the rows are known on the device only (seg_off[num_nets] <= capacity): size the grid for a full list
    const int64_t n_pass = (capacity + S - 1) / S;
    int grid = (int)(n_pass < max_blocks ? n_pass : max_blocks);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((net_forward_multi_kernel<C, S, W>), dim3(grid), dim3(K::THREADS), K::LDS_BYTES, st, P, M, num_nets,
                       packed, capacity, reinterpret_cast<const long long*>(seg_off), lp1, lp2, lpm, vlogits, value);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}

// ---- the gathering launch (lz_net_forward_packed_gather_f16) ---------------------------------------------------------------
// The batch is not a list but the slots g of `packed` whose leaf_kind[g] == kLiveKind, evaluated in place: slot g's
// outputs go to row g.  Every workgroup finds the live slots for itself (no communication between workgroups): it reads
// all B flags (coalesced rounds of THREADS games, the loads of a group of rounds in flight together), each wave ballots
// its 64 games into one mask word in LDS, and one wave turns the popcounts of the words into an exclusive prefix.  Row r
// of the launch is then the r-th live slot in ascending order (lz_live_index.h); the pass loop is the plain kernel's
// over those rows: before each pass S lanes look its S slots up and write them to a table of S ints (one workgroup
// barrier; a look-up is ~10 dependent LDS reads, 0.7 us against the ~220 us of a pass).  Extra LDS behind
// Cfg::LDS_BYTES: two slot tables (alternating, so that the stores at the end of a pass may still read theirs while the
// next pass's is written), the live count, the masks, the prefix.
constexpr int kLiveKind = 1;                        // lz_tree_dev.h: kLeafExpand
constexpr int kGatherUnroll = 8;                    // rounds of flag loads in flight together, as in tree_live_scan_kernel
template <int S> constexpr int gather_head_bytes() { return ((2 * S + 1) * 4 + 15) & ~15; }
template <int C, int S, int W> constexpr int gather_lds_limit() { return (C == 64 && W == 4) ? 80 * 1024 : 160 * 1024; }
template <int C, int S, int W>
int64_t gather_lds_bytes(int64_t B) {                // whole dynamic LDS of a launch over B slots
    const int64_t words = (B + 63) >> 6;
    return Cfg<C, S, W>::LDS_BYTES + gather_head_bytes<S>() + words * 12;
}

template <int C, int S, int W>
__global__ __launch_bounds__(W * 64, (C == 128 && W == 4) ? 1 : 2) void net_forward_gather_kernel(
        NetParams P, const uint64_t* __restrict__ packed, const int* __restrict__ leaf_kind, int B,
        unsigned long long* __restrict__ count_out, int even_rounds, float* __restrict__ lp1, float* __restrict__ lp2,
        float* __restrict__ lpm, float* __restrict__ vlogits, float* __restrict__ value) {
    using K = Cfg<C, S, W>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    NetCtx<C, S, W> ctx;
    net_setup<C, S, W>(P, lds, ctx);
    const int words = (B + 63) >> 6;
    int* tab = reinterpret_cast<int*>(lds + K::LDS_BYTES);                 // [2][S] slots, then the live count
    uint64_t* masks = reinterpret_cast<uint64_t*>(lds + K::LDS_BYTES + gather_head_bytes<S>());
    int* prefix = reinterpret_cast<int*>(masks + words);
    const int tid = ctx.tid, lane = ctx.lane, wave = ctx.wave;
    const int rounds = (B + K::THREADS - 1) / K::THREADS;
    for (int r0 = 0; r0 < rounds; r0 += kGatherUnroll) {
        int kind[kGatherUnroll];
#pragma unroll
        for (int u = 0; u < kGatherUnroll; ++u) {
            const int g = (r0 + u) * K::THREADS + tid;
            kind[u] = g < B ? leaf_kind[g] : kLiveKind - 1;
        }
#pragma unroll
        for (int u = 0; u < kGatherUnroll; ++u) {
            const unsigned long long m = __ballot(kind[u] == kLiveKind);
            const int w = (r0 + u) * W + wave;                             // games w * 64 .. w * 64 + 63
            if (lane == 0 && w < words) masks[w] = m;
        }
    }
    __syncthreads();
    if (wave == 0) {                                                       // exclusive prefix of the popcounts, 64 words a step
        int run = 0;
        for (int w0 = 0; w0 < words; w0 += 64) {
            const int w = w0 + lane;
            const int c = w < words ? lzlive::popc64(masks[w]) : 0;
            int incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(incl, d, 64);
                if (lane >= d) incl += v;
            }
            if (w < words) prefix[w] = run + incl - c;
            run += __shfl(incl, 63, 64);
        }
        if (lane == 0) tab[2 * S] = run;
    }
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane(tab[2 * S]);
    if (blockIdx.x == 0 && tid == 0) *count_out = (unsigned long long)n;
    const int n_pass = (n + S - 1) / S;
    // even rounds: the same number of rounds on the fewest workgroups that need no round more -- the CUs of a partial
    // last round would idle anyway, and the chip at its power limit runs the others faster without them (n = 12 337:
    // 1 543 passes are seven rounds of 221 workgroups instead of six of 256 and one of 7)
    int stride = gridDim.x;
    if (even_rounds && n_pass > 0) {
        const int r = (n_pass + stride - 1) / stride;
        stride = (n_pass + r - 1) / r;
    }
    if ((int)blockIdx.x >= stride) return;
    int par = 0;
    for (int pass = blockIdx.x; pass < n_pass; pass += stride, par ^= 1) {
        const int n0 = pass * S;
        const int nvalid = (n - n0) < S ? (n - n0) : S;
        int* slot_tab = tab + par * S;
        if (tid < S) slot_tab[tid] = tid < nvalid ? lzlive::row_to_game(masks, prefix, words, n0 + tid) : 0;
        __syncthreads();
        net_pass<C, S, W, true>(P, lds, ctx, nullptr, packed, 0, nvalid, lp1, lp2, lpm, vlogits, value, nullptr, slot_tab);
    }
}

template <int C, int S, int W>
int launch_net_gather(const NetParams& P, const uint64_t* packed, const int* leaf_kind, int64_t B,
                      unsigned long long* count_out, int even_rounds, float* lp1, float* lp2, float* lpm, float* vlogits,
                      float* value, int max_blocks, hipStream_t st) {
    using K = Cfg<C, S, W>;
    const int64_t lds = gather_lds_bytes<C, S, W>(B);
    if (lds > gather_lds_limit<C, S, W>()) return LZ_ERR_UNSUPPORTED;
    const int64_t n_pass = (B + S - 1) / S;
    int grid = (int)(n_pass < max_blocks ? n_pass : max_blocks);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((net_forward_gather_kernel<C, S, W>), dim3(grid), dim3(K::THREADS), (size_t)lds, st, P, packed,
                       leaf_kind, (int)B, count_out, even_rounds, lp1, lp2, lpm, vlogits, value);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}

template <int C, int S, int W>
int configure_net_gather() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(net_forward_gather_kernel<C, S, W>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, gather_lds_limit<C, S, W>()) == hipSuccess
               ? LZ_OK : LZ_ERR_LAUNCH;
}

template <int C, int S, int W>
int configure_net_multi() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(net_forward_multi_kernel<C, S, W>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<C, S, W>::LDS_BYTES) == hipSuccess
               ? LZ_OK : LZ_ERR_LAUNCH;
}

template <int C, int S, int W>
int configure_net() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(net_forward_kernel<C, S, W>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, Cfg<C, S, W>::LDS_BYTES) == hipSuccess
               ? LZ_OK : LZ_ERR_LAUNCH;
}

}  // namespace

// ---- optional live timing of the network kernel (bench.py roofline): HIP events on the launch stream ----
namespace {
struct NetProf {
    bool on = false;
    int used = 0;
    static constexpr int kMax = 8192;
    hipEvent_t ev[2 * kMax];
    bool created = false;
    double flops = 0.0;
    int64_t evals = 0;
} g_prof;
}  // namespace

extern "C" void lz_prof_aux_reset(void);

extern "C" {

int lz_prof_enable(int on) {
    if (on && !g_prof.created) {
        for (int i = 0; i < 2 * NetProf::kMax; ++i)
            if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) return LZ_ERR_LAUNCH;
        g_prof.created = true;
    }
    g_prof.on = on != 0;
    g_prof.used = 0;
    g_prof.evals = 0;
    lz_prof_aux_reset();
    return LZ_OK;
}

/* call after the stream has been synchronised: total / count of the timed network launches */
int lz_prof_net_summary(double* total_ms, int64_t* launches, int64_t* evals) {
    double t = 0.0;
    for (int i = 0; i < g_prof.used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) return LZ_ERR_LAUNCH;
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = g_prof.used;
    if (evals) *evals = g_prof.evals;
    return LZ_OK;
}

/* Launches bracketed on several streams may overlap: `busy_ms` is the length of the union of their [start, end]
 * intervals (event times relative to the first recorded event), i.e. the time during which at least one network
 * kernel was running; equal to total_ms when everything ran on one stream. */
int lz_prof_net_busy(double* busy_ms) {
    if (!busy_ms) return LZ_ERR_ARG;
    *busy_ms = 0.0;
    const int n = g_prof.used;
    if (n == 0) return LZ_OK;
    std::vector<std::pair<float, float>> iv((size_t)n);
    for (int i = 0; i < n; ++i) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, g_prof.ev[0], g_prof.ev[2 * i]) != hipSuccess ||
            hipEventElapsedTime(&b, g_prof.ev[0], g_prof.ev[2 * i + 1]) != hipSuccess)
            return LZ_ERR_LAUNCH;
        iv[(size_t)i] = {a, b};
    }
    std::sort(iv.begin(), iv.end());
    double busy = 0.0;
    float lo = iv[0].first, hi = iv[0].second;
    for (int i = 1; i < n; ++i) {
        if (iv[(size_t)i].first > hi) { busy += (double)(hi - lo); lo = iv[(size_t)i].first; hi = iv[(size_t)i].second; }
        else if (iv[(size_t)i].second > hi) hi = iv[(size_t)i].second;
    }
    *busy_ms = busy + (double)(hi - lo);
    return LZ_OK;
}

/* internal (not exported): bracket any other kernel of the path like a network launch -- the persistent search kernel
 * of lz_search.hip, whose `evals` network evaluations happen inside one launch */
int lz_prof_mark_begin(void* stream) {
    if (!(g_prof.on && g_prof.used < NetProf::kMax)) return LZ_OK;
    return hipEventRecord(g_prof.ev[2 * g_prof.used], reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}
int lz_prof_mark_end(void* stream, int64_t evals) {
    if (!(g_prof.on && g_prof.used < NetProf::kMax)) return LZ_OK;
    (void)hipEventRecord(g_prof.ev[2 * g_prof.used + 1], reinterpret_cast<hipStream_t>(stream));
    g_prof.used += 1; g_prof.evals += evals;
    return LZ_OK;
}

/* Secondary brackets for the HBM-bound kernels of the search (bench.py `roofline.secondary`): kind 0 = the fused
 * expand + backup + select kernel of a simulation, kind 1 = the subtree compaction of a move.  Same mechanism as the
 * network brackets (events on the launch stream, only while lz_prof_enable(1)); begin / end are internal. */
namespace {
struct AuxProf {
    static constexpr int kKinds = 2, kMax = 4096;
    hipEvent_t ev[kKinds][2 * kMax];
    int used[kKinds] = {0, 0};
    int64_t units[kKinds] = {0, 0};
    bool created = false;
} g_aux;
}  // namespace

void lz_prof_aux_reset(void) {
    for (int k = 0; k < AuxProf::kKinds; ++k) { g_aux.used[k] = 0; g_aux.units[k] = 0; }
}
int lz_prof_aux_begin(int kind, void* stream) {
    if (!g_prof.on || kind < 0 || kind >= AuxProf::kKinds) return LZ_OK;
    if (!g_aux.created) {
        for (int k = 0; k < AuxProf::kKinds; ++k)
            for (int i = 0; i < 2 * AuxProf::kMax; ++i)
                if (hipEventCreate(&g_aux.ev[k][i]) != hipSuccess) return LZ_ERR_LAUNCH;
        g_aux.created = true;
    }
    if (g_aux.used[kind] >= AuxProf::kMax) return LZ_OK;
    return hipEventRecord(g_aux.ev[kind][2 * g_aux.used[kind]], reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}
int lz_prof_aux_end(int kind, void* stream, int64_t units) {
    if (!g_prof.on || !g_aux.created || kind < 0 || kind >= AuxProf::kKinds || g_aux.used[kind] >= AuxProf::kMax) return LZ_OK;
    (void)hipEventRecord(g_aux.ev[kind][2 * g_aux.used[kind] + 1], reinterpret_cast<hipStream_t>(stream));
    g_aux.used[kind] += 1; g_aux.units[kind] += units;
    return LZ_OK;
}
/* exported: call after synchronising; lz_prof_enable() resets the counts */
int lz_prof_aux_summary(int kind, double* total_ms, int64_t* launches, int64_t* units) {
    if (kind < 0 || kind >= AuxProf::kKinds) return LZ_ERR_ARG;
    double t = 0.0;
    for (int i = 0; i < g_aux.used[kind]; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_aux.ev[kind][2 * i], g_aux.ev[kind][2 * i + 1]) != hipSuccess) return LZ_ERR_LAUNCH;
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = g_aux.used[kind];
    if (units) *units = g_aux.units[kind];
    return LZ_OK;
}

int64_t lz_net_desc_bytes(void) { return (int64_t)sizeof(LzNetDesc); }

int lz_net_configure(void) {
    const int a = configure_net<64, 16, 8>(), b = configure_net<128, 8, 8>(), c = configure_net<64, 8, 4>(),
              e = configure_net<128, 8, 4>();
    const int ma = configure_net_multi<64, 16, 8>(), mb = configure_net_multi<128, 8, 8>(),
              mc = configure_net_multi<64, 8, 4>(), me = configure_net_multi<128, 8, 4>();
    const int ga = configure_net_gather<64, 16, 8>(), gb = configure_net_gather<128, 8, 8>(),
              gc = configure_net_gather<64, 8, 4>(), ge = configure_net_gather<128, 8, 4>();
    for (int rc : {a, b, c, e, ma, mb, mc, me, ga, gb, gc, ge})
        if (rc != LZ_OK) return rc;
    return LZ_OK;
}

// fp32-operand parity mode (lz_net_f32.hip)
int lz_net_forward_f32_dispatch(const LzNetDesc* d, const float* planes, const uint64_t* packed, int64_t N, float* lp1,
                                float* lp2, float* lpmc, float* value_logits, float* value, const int64_t* n_dev,
                                void* stream);

static int net_forward_impl(const LzNetDesc* d, const float* planes, const uint64_t* packed, int64_t N, float* lp1,
                            float* lp2, float* lpmc, float* value_logits, float* value, void* stream,
                            const int64_t* n_dev = nullptr) {
    if (!d || N < 0) return LZ_ERR_ARG;
    if (N == 0) return LZ_OK;
    if (!d->wfrag || !d->fparams || (!planes && !packed)) return LZ_ERR_ARG;
    const bool heads = lp1 && lp2 && lpmc;
    if (!heads && (lp1 || lp2 || lpmc || !value)) return LZ_ERR_ARG;     // all three policy outputs, or values only
    if (d->blocks < 0 || d->blocks > (LZ_NET_MAX_LAYERS - 2) / 2 || d->num_layers != 2 + 2 * d->blocks) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d->wfrag) & 15) || (reinterpret_cast<uintptr_t>(d->fparams) & 15)) return LZ_ERR_ALIGN;
    if (d->flags & (4 | 8))
        return lz_net_forward_f32_dispatch(d, planes, packed, N, lp1, lp2, lpmc, value_logits, value, n_dev, stream);
    NetParams P = make_net_params(d);
#ifdef LZ_EXP_SAME_LAYER    /* compile-time only, like the other LZ_EXP_* experiments: never in the shipped library.  Timing
                             * experiment (results are wrong): every trunk conv reads the first block's weights, so the weight
                             * set fits the 4 MB XCD L2 -- bounds what L2 misses on the 5.9 MB set of 10x128 cost */
    for (int i = 3; i < 1 + 2 * d->blocks; ++i) P.layer_off[i] = d->layer_offsets[1 + ((i - 1) & 1)];
#endif
    P.n_dev = reinterpret_cast<const long long*>(n_dev);
    P.debug_stop = getenv("LZ_NET_DEBUG_STOP") ? atoi(getenv("LZ_NET_DEBUG_STOP")) : 0;
    // flags bit 0 (64 channels): 4-wave workgroups of 8 samples, two per CU -- twice as many workgroups per batch, so
    // that a half-size batch still covers every CU when two of them are evaluated concurrently on two streams
    const bool half_wg = d->channels == 64 && (d->flags & 1);
    const int max_blocks = d->max_blocks > 0 ? d->max_blocks : (half_wg ? 512 : 256);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d->channels != 64 && d->channels != 128) return LZ_ERR_UNSUPPORTED;
    const bool prof = g_prof.on && g_prof.used < NetProf::kMax;
    if (prof) (void)hipEventRecord(g_prof.ev[2 * g_prof.used], st);
    // Two 4-wave workgroups of 8 samples per CU (<64,8,4>) were measured, also staggered by half a layer: 9 % fewer
    // shader cycles per pass, but the chip then holds 1.87 GHz instead of 2.05 GHz -- the same wall time.
    // flags bit 1 (128 channels): 4-wave workgroups, one wave per SIMD with 512 registers and 4 channel tiles per wave
    // (half the LDS operand reads of the 8-wave shape)
    const bool wide = d->channels == 128 && (d->flags & 2);
    const int rc = d->channels == 64
                       ? (half_wg
                              ? launch_net<64, 8, 4>(P, planes, packed, N, lp1, lp2, lpmc, value_logits, value, max_blocks, st)
                              : launch_net<64, 16, 8>(P, planes, packed, N, lp1, lp2, lpmc, value_logits, value, max_blocks, st))
                       : (wide ? launch_net<128, 8, 4>(P, planes, packed, N, lp1, lp2, lpmc, value_logits, value, max_blocks, st)
                               : launch_net<128, 8, 8>(P, planes, packed, N, lp1, lp2, lpmc, value_logits, value, max_blocks, st));
    if (prof) { (void)hipEventRecord(g_prof.ev[2 * g_prof.used + 1], st); g_prof.used += 1; g_prof.evals += N; }
    return rc;
}

int lz_net_forward_f16(const LzNetDesc* d, const float* planes, int64_t N, float* lp1, float* lp2, float* lpmc,
                       float* value_logits, float* value, void* stream) {
    return net_forward_impl(d, planes, nullptr, N, lp1, lp2, lpmc, value_logits, value, stream);
}

int lz_net_forward_packed_f16(const LzNetDesc* d, const void* packed_states, int64_t N, float* lp1, float* lp2,
                              float* lpmc, float* value_logits, float* value, void* stream) {
    return net_forward_impl(d, nullptr, reinterpret_cast<const uint64_t*>(packed_states), N, lp1, lp2, lpmc,
                            value_logits, value, stream);
}

int lz_net_forward_packed_counted_f16(const LzNetDesc* d, const void* packed_states, int64_t capacity,
                                      const int64_t* count, float* lp1, float* lp2, float* lpmc, float* value_logits,
                                      float* value, void* stream) {
    if (!count) return LZ_ERR_ARG;
    return net_forward_impl(d, nullptr, reinterpret_cast<const uint64_t*>(packed_states), capacity, lp1, lp2, lpmc,
                            value_logits, value, stream, count);
}

// Does a launch of num_slots slots of this network fit the gathering kernel?  (internal: lz_tree_search asks before it
// chooses its path)
static int net_gather_shape(const LzNetDesc* d, int64_t num_slots) {
    if (d->flags & (4 | 8)) return LZ_ERR_UNSUPPORTED;
    if (d->channels != 64 && d->channels != 128) return LZ_ERR_UNSUPPORTED;
    if (num_slots > (int64_t)INT32_MAX - 1024) return LZ_ERR_UNSUPPORTED;
    const bool half_wg = d->channels == 64 && (d->flags & 1), wide = d->channels == 128 && (d->flags & 2);
    const int64_t need = d->channels == 64 ? (half_wg ? gather_lds_bytes<64, 8, 4>(num_slots) : gather_lds_bytes<64, 16, 8>(num_slots))
                                           : (wide ? gather_lds_bytes<128, 8, 4>(num_slots) : gather_lds_bytes<128, 8, 8>(num_slots));
    const int64_t limit = half_wg ? gather_lds_limit<64, 8, 4>() : gather_lds_limit<128, 8, 8>();
    return need <= limit ? LZ_OK : LZ_ERR_UNSUPPORTED;
}
int lz_net_gather_supported(const LzNetDesc* d, int64_t num_slots) {
    return d && num_slots > 0 && net_gather_shape(d, num_slots) == LZ_OK;
}
/* internal: workgroups and samples per pass of a launch of this network (the gate of lz_tree_search) */
void lz_net_launch_shape(const LzNetDesc* d, int* max_blocks, int* samples) {
    const bool half_wg = d->channels == 64 && (d->flags & 1);
    *max_blocks = d->max_blocks > 0 ? d->max_blocks : (half_wg ? 512 : 256);
    *samples = d->channels == 64 && !half_wg ? 16 : 8;
}

int lz_net_forward_packed_gather_f16(const LzNetDesc* d, const void* packed_states, const int32_t* leaf_kind,
                                     int64_t num_slots, int64_t* count_out, float* lp1, float* lp2, float* lpmc,
                                     float* value_logits, float* value, void* stream) {
    if (!d || num_slots < 0) return LZ_ERR_ARG;
    if (num_slots == 0) return LZ_OK;
    if (!d->wfrag || !d->fparams || !packed_states || !leaf_kind || !count_out) return LZ_ERR_ARG;
    const bool heads = lp1 && lp2 && lpmc;
    if (!heads && (lp1 || lp2 || lpmc || !value)) return LZ_ERR_ARG;     // all three policy outputs, or values only
    if (d->blocks < 0 || d->blocks > (LZ_NET_MAX_LAYERS - 2) / 2 || d->num_layers != 2 + 2 * d->blocks) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d->wfrag) & 15) || (reinterpret_cast<uintptr_t>(d->fparams) & 15)) return LZ_ERR_ALIGN;
    const int src = net_gather_shape(d, num_slots);
    if (src) return src;
    NetParams P = make_net_params(d);
    P.debug_stop = getenv("LZ_NET_DEBUG_STOP") ? atoi(getenv("LZ_NET_DEBUG_STOP")) : 0;
    const char* ev = getenv("LZ_NET_EVEN_ROUNDS");                       // on unless 0 (A/B runs)
    const int even_rounds = ev && ev[0] == '0' ? 0 : 1;
    const bool half_wg = d->channels == 64 && (d->flags & 1);
    const bool wide = d->channels == 128 && (d->flags & 2);
    const int max_blocks = d->max_blocks > 0 ? d->max_blocks : (half_wg ? 512 : 256);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint64_t* packed = reinterpret_cast<const uint64_t*>(packed_states);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count_out);
    const bool prof = g_prof.on && g_prof.used < NetProf::kMax;
    if (prof) (void)hipEventRecord(g_prof.ev[2 * g_prof.used], st);
    const int rc = d->channels == 64
                       ? (half_wg ? launch_net_gather<64, 8, 4>(P, packed, leaf_kind, num_slots, cnt, even_rounds, lp1, lp2, lpmc,
                                                                value_logits, value, max_blocks, st)
                                  : launch_net_gather<64, 16, 8>(P, packed, leaf_kind, num_slots, cnt, even_rounds, lp1, lp2, lpmc,
                                                                 value_logits, value, max_blocks, st))
                       : (wide ? launch_net_gather<128, 8, 4>(P, packed, leaf_kind, num_slots, cnt, even_rounds, lp1, lp2, lpmc,
                                                              value_logits, value, max_blocks, st)
                               : launch_net_gather<128, 8, 8>(P, packed, leaf_kind, num_slots, cnt, even_rounds, lp1, lp2, lpmc,
                                                              value_logits, value, max_blocks, st));
    if (prof) { (void)hipEventRecord(g_prof.ev[2 * g_prof.used + 1], st); g_prof.used += 1; g_prof.evals += num_slots; }
    return rc;
}

// Networks that may share one launch: the same kernel shape and the same layout of both buffers -- everything but the
// two buffer pointers.  fp32-operand / split-fp16 networks (flags bits 2-3) are not supported here.
static int multi_net_check(const LzNetDesc* a, const LzNetDesc* b) {
    if (a->channels != b->channels || a->blocks != b->blocks || a->num_layers != b->num_layers ||
        a->max_blocks != b->max_blocks || a->wfrag_bytes != b->wfrag_bytes || a->fparams_bytes != b->fparams_bytes ||
        (a->flags & 3) != (b->flags & 3))
        return LZ_ERR_ARG;
    for (int i = 0; i < LZ_NET_MAX_LAYERS; ++i)
        if (i < a->num_layers && a->layer_offsets[i] != b->layer_offsets[i]) return LZ_ERR_ARG;
    for (int i = 0; i < 4; ++i)
        if (a->head_frag_offsets[i] != b->head_frag_offsets[i]) return LZ_ERR_ARG;
    const int32_t oa[13] = {a->off_stem_bias, a->off_block0, a->off_trunk_a, a->off_trunk_b, a->off_head_bias, a->off_p_gwT,
                            a->off_p_a2, a->off_p_b2, a->off_p_out, a->off_v_w1T, a->off_v_b1, a->off_v_w2T, a->off_v_b2};
    const int32_t ob[13] = {b->off_stem_bias, b->off_block0, b->off_trunk_a, b->off_trunk_b, b->off_head_bias, b->off_p_gwT,
                            b->off_p_a2, b->off_p_b2, b->off_p_out, b->off_v_w1T, b->off_v_b1, b->off_v_w2T, b->off_v_b2};
    for (int i = 0; i < 13; ++i)
        if (oa[i] != ob[i]) return LZ_ERR_ARG;
    return LZ_OK;
}

/* internal (not exported; lz_tree_search_multi checks its networks before it launches anything) */
int lz_net_multi_validate(const LzNetDesc* const* nets, int num_nets) {
    if (!nets || num_nets < 1 || num_nets > kMaxNets) return LZ_ERR_ARG;
    for (int k = 0; k < num_nets; ++k) {
        const LzNetDesc* n = nets[k];
        if (!n || !n->wfrag || !n->fparams) return LZ_ERR_ARG;
        if (n->flags & (4 | 8)) return LZ_ERR_UNSUPPORTED;
        if ((reinterpret_cast<uintptr_t>(n->wfrag) & 15) || (reinterpret_cast<uintptr_t>(n->fparams) & 15)) return LZ_ERR_ALIGN;
    }
    const LzNetDesc* d = nets[0];
    if (d->blocks < 0 || d->blocks > (LZ_NET_MAX_LAYERS - 2) / 2 || d->num_layers != 2 + 2 * d->blocks) return LZ_ERR_ARG;
    for (int k = 1; k < num_nets; ++k) {
        const int rc = multi_net_check(d, nets[k]);
        if (rc) return rc;
    }
    return d->channels == 64 || d->channels == 128 ? LZ_OK : LZ_ERR_UNSUPPORTED;
}

int lz_net_forward_packed_multi_f16(const LzNetDesc* const* nets, int32_t num_nets, const void* packed_states,
                                    int64_t capacity, const int64_t* seg_off, float* lp1, float* lp2, float* lpmc,
                                    float* value_logits, float* value, void* stream) {
    if (!nets || num_nets < 1 || num_nets > kMaxNets || capacity < 0 || capacity > (int64_t)INT32_MAX - 64) return LZ_ERR_ARG;
    if (capacity == 0) return LZ_OK;
    if (!packed_states || !seg_off) return LZ_ERR_ARG;
    const bool heads = lp1 && lp2 && lpmc;
    if (!heads && (lp1 || lp2 || lpmc || !value)) return LZ_ERR_ARG;
    const int vrc = lz_net_multi_validate(nets, num_nets);
    if (vrc) return vrc;
    const LzNetDesc* d = nets[0];
    MultiNets M{};
    for (int k = 0; k < kMaxNets; ++k) {                        // unused entries repeat network 0 (never selected)
        const LzNetDesc* n = nets[k < num_nets ? k : 0];
        M.wfrag[k] = reinterpret_cast<const _Float16*>(n->wfrag);
        M.fp[k] = n->fparams;
    }
    const NetParams P = make_net_params(d);
    const bool half_wg = d->channels == 64 && (d->flags & 1);
    const bool wide = d->channels == 128 && (d->flags & 2);
    const int max_blocks = d->max_blocks > 0 ? d->max_blocks : (half_wg ? 512 : 256);
    const uint64_t* packed = reinterpret_cast<const uint64_t*>(packed_states);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return d->channels == 64
               ? (half_wg ? launch_net_multi<64, 8, 4>(P, M, num_nets, packed, capacity, seg_off, lp1, lp2, lpmc, value_logits,
                                                       value, max_blocks, st)
                          : launch_net_multi<64, 16, 8>(P, M, num_nets, packed, capacity, seg_off, lp1, lp2, lpmc, value_logits,
                                                        value, max_blocks, st))
               : (wide ? launch_net_multi<128, 8, 4>(P, M, num_nets, packed, capacity, seg_off, lp1, lp2, lpmc, value_logits,
                                                     value, max_blocks, st)
                       : launch_net_multi<128, 8, 8>(P, M, num_nets, packed, capacity, seg_off, lp1, lp2, lpmc, value_logits,
                                                     value, max_blocks, st));
}

}  // extern "C"
