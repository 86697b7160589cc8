// lz_symmetry.hip -- gfx950 kernels of the board-symmetry entry points (include/liuzhou_hip.h, csrc/lz_symmetry.h).
//
// gather_samples is the trainer's augmentation: ONE pass that gathers a batch of training rows and applies a per-row
// element of D4, replacing three index_selects.  One wave per output row: every store is a contiguous run of the
// output row (coalesced), every load a permuted read inside one 1.6 KB source row (the same cache lines).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz_soa.h"
#include "lz_symmetry.h"

using namespace lz;

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
// the element id of row j, wave-uniform; -1 for an id outside 0..7
__device__ __forceinline__ int load_sym(const void* sym, int width, int64_t j) {
    const int k = width == 1 ? (int)reinterpret_cast<const int8_t*>(sym)[j] : (int)reinterpret_cast<const int32_t*>(sym)[j];
    return __builtin_amdgcn_readfirstlane(k >= 0 && k < kSyms ? k : -1);
}

__global__ __launch_bounds__(kBlock) void gather_samples_kernel(
        const float* __restrict__ planes, const uint8_t* __restrict__ masks, const float* __restrict__ policy,
        int64_t n_src, const int64_t* __restrict__ idx, const void* __restrict__ sym, int width,
        float* __restrict__ out_planes, uint8_t* __restrict__ out_masks, float* __restrict__ out_policy, int64_t m) {
    const int64_t j = wave_item();
    if (j >= m) return;
    const int k = load_sym(sym, width, j);
    const int64_t src = idx ? idx[j] : j;
    if (k < 0 || src < 0 || src >= n_src) {                   // invalid id or index: the output row is zeroed
        for (int q = lane_id(); q < 396; q += kWave) out_planes[j * 396 + q] = 0.f;
        if (masks != nullptr)
            for (int b = lane_id(); b < kActions; b += kWave) { out_masks[j * kActions + b] = 0; out_policy[j * kActions + b] = 0.f; }
        return;
    }
    const int inv = sym_inverse(k);
    const float* pin = planes + src * 396;
    float* pout = out_planes + j * 396;
    for (int q = lane_id(); q < 396; q += kWave) {
        const int plane = q / 36, cell = q - plane * 36;
        pout[q] = pin[plane * 36 + sym_cell(inv, cell)];
    }
    if (masks != nullptr) {
        const uint8_t* min_ = masks + src * kActions;
        const uint32_t* qin = reinterpret_cast<const uint32_t*>(policy + src * kActions);
        uint32_t* qout = reinterpret_cast<uint32_t*>(out_policy + j * kActions);
        uint8_t* mout = out_masks + j * kActions;
        for (int b = lane_id(); b < kActions; b += kWave) {
            const int a = kSym.action[inv][b];                  // out[P(a)] = in[a]
            mout[b] = min_[a];
            qout[b] = qin[a];                                   // bit copy
        }
    }
}

// the nine int64 fields of a state batch by number (a switch: no private array indexed by lane)
__device__ __forceinline__ int64_t* soa_field(const LzStateSoA& s, int f) {
    switch (f) {
        case 0: return s.phase;
        case 1: return s.current_player;
        case 2: return s.pending_marks_required;
        case 3: return s.pending_marks_remaining;
        case 4: return s.pending_captures_required;
        case 5: return s.pending_captures_remaining;
        case 6: return s.forced_removals_done;
        case 7: return s.move_count;
        default: return s.moves_since_capture;
    }
}

__global__ __launch_bounds__(kBlock) void transform_states_kernel(LzStateSoA in, const void* __restrict__ sym, int width,
                                                                  LzStateSoA out, int64_t B) {
    const int64_t i = wave_item();
    if (i >= B) return;
    const int k = load_sym(sym, width, i);
    if (k < 0) return;
    const int lane = lane_id();
    if (lane < 36) {
        const int s = sym_cell(sym_inverse(k), lane);
        out.board[i * 36 + lane] = in.board[i * 36 + s];
        out.marks_black[i * 36 + lane] = in.marks_black[i * 36 + s];
        out.marks_white[i * 36 + lane] = in.marks_white[i * 36 + s];
    } else if (lane < 45) {
        const int f = lane - 36;
        soa_field(out, f)[i] = soa_field(in, f)[i];
    }
}

__global__ __launch_bounds__(kBlock) void transform_packed_kernel(const Packed* __restrict__ in, const void* __restrict__ sym,
                                                                  int width, Packed* __restrict__ out, int64_t B) {
    const int64_t i = wave_item();
    if (i >= B) return;
    const int k = load_sym(sym, width, i);
    if (k < 0) return;
    const Packed p = in[i];
    const Packed o = sym_packed_wave(k, p, lane_id());
    if (lane_id() == 0) out[i] = o;
}

bool soa_ok(const LzStateSoA* s) {
    return s && s->board && s->marks_black && s->marks_white && s->phase && s->current_player &&
           s->pending_marks_required && s->pending_marks_remaining && s->pending_captures_required &&
           s->pending_captures_remaining && s->forced_removals_done && s->move_count && s->moves_since_capture;
}

}  // namespace

extern "C" {

int lz_symmetry_tables(int32_t* cells, int32_t* actions, int32_t* inverse, int32_t* compose, int32_t* directions) {
    for (int k = 0; k < kSyms; ++k) {
        if (cells) for (int x = 0; x < 36; ++x) cells[k * 36 + x] = kSym.cell[k][x];
        if (actions) for (int a = 0; a < kActions; ++a) actions[k * kActions + a] = kSym.action[k][a];
        if (inverse) inverse[k] = kSym.inv[k];
        if (compose) for (int b = 0; b < kSyms; ++b) compose[k * kSyms + b] = kSym.comp[k][b];
        if (directions) for (int d = 0; d < 4; ++d) directions[k * 4 + d] = kSym.dir[k][d];
    }
    return LZ_OK;
}

int lz_symmetry_gather_samples(const float* planes, const uint8_t* masks, const float* policy, int64_t n_src,
                               const int64_t* idx, const void* sym, int32_t sym_width, float* out_planes,
                               uint8_t* out_masks, float* out_policy, int64_t m, void* stream) {
    if (m < 0 || n_src < 0 || (sym_width != 1 && sym_width != 4)) return LZ_ERR_ARG;
    if (m == 0) return LZ_OK;
    if (!planes || !sym || !out_planes) return LZ_ERR_ARG;
    const bool rows = masks || policy || out_masks || out_policy;
    if (rows && !(masks && policy && out_masks && out_policy)) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(policy) | reinterpret_cast<uintptr_t>(out_policy)) % 4) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(gather_samples_kernel, dim3(grid_waves(m)), dim3(kBlock), 0, as_stream(stream), planes,
                       rows ? masks : nullptr, policy, n_src, idx, sym, (int)sym_width, out_planes, out_masks,
                       out_policy, m);
    return launch_status();
}

int lz_symmetry_transform_states(const LzStateSoA* in, const void* sym, int32_t sym_width, const LzStateSoA* out,
                                 int64_t B, void* stream) {
    if (B < 0 || (sym_width != 1 && sym_width != 4)) return LZ_ERR_ARG;
    if (B == 0) return LZ_OK;
    if (!soa_ok(in) || !soa_ok(out) || !sym) return LZ_ERR_ARG;
    hipLaunchKernelGGL(transform_states_kernel, dim3(grid_waves(B)), dim3(kBlock), 0, as_stream(stream), *in, sym,
                       (int)sym_width, *out, B);
    return launch_status();
}

int lz_symmetry_transform_packed(const int64_t* in, const void* sym, int32_t sym_width, int64_t* out, int64_t B,
                                 void* stream) {
    if (B < 0 || (sym_width != 1 && sym_width != 4)) return LZ_ERR_ARG;
    if (B == 0) return LZ_OK;
    if (!in || !out || !sym) return LZ_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16) return LZ_ERR_ALIGN;
    hipLaunchKernelGGL(transform_packed_kernel, dim3(grid_waves(B)), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<const Packed*>(in), sym, (int)sym_width, reinterpret_cast<Packed*>(out), B);
    return launch_status();
}

}  // extern "C"
