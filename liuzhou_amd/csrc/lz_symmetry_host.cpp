// lz_symmetry_host.cpp -- host (CPU-tensor) build of the board-symmetry entry points of include/liuzhou_hip.h, part of
// libliuzhou_host.so: the same tables (csrc/lz_symmetry.h) and the same semantics as lz_symmetry.hip, as plain loops
// over rows.  `stream` is ignored.
#include <cstdint>
#include <cstring>

#include "lz_soa.h"
#include "lz_symmetry.h"

using namespace lz;

namespace {

int load_sym(const void* sym, int width, int64_t j) {
    const int k = width == 1 ? (int)static_cast<const int8_t*>(sym)[j] : (int)static_cast<const int32_t*>(sym)[j];
    return k >= 0 && k < kSyms ? k : -1;
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
                               uint8_t* out_masks, float* out_policy, int64_t m, void*) {
    if (m < 0 || n_src < 0 || (sym_width != 1 && sym_width != 4)) return LZ_ERR_ARG;
    if (m == 0) return LZ_OK;
    if (!planes || !sym || !out_planes) return LZ_ERR_ARG;
    const bool rows = masks || policy || out_masks || out_policy;
    if (rows && !(masks && policy && out_masks && out_policy)) return LZ_ERR_ARG;
    for (int64_t j = 0; j < m; ++j) {
        const int k = load_sym(sym, sym_width, j);
        const int64_t src = idx ? idx[j] : j;
        if (k < 0 || src < 0 || src >= n_src) {               // invalid id or index: the output row is zeroed
            std::memset(out_planes + j * 396, 0, 396 * sizeof(float));
            if (rows) { std::memset(out_masks + j * kActions, 0, kActions); std::memset(out_policy + j * kActions, 0, kActions * sizeof(float)); }
            continue;
        }
        for (int plane = 0; plane < 11; ++plane)
            for (int x = 0; x < 36; ++x)
                out_planes[j * 396 + plane * 36 + kSym.cell[k][x]] = planes[src * 396 + plane * 36 + x];
        if (!rows) continue;
        for (int a = 0; a < kActions; ++a) {
            const int b = kSym.action[k][a];
            out_masks[j * kActions + b] = masks[src * kActions + a];
            std::memcpy(out_policy + j * kActions + b, policy + src * kActions + a, sizeof(float));   // bit copy
        }
    }
    return LZ_OK;
}

int lz_symmetry_transform_states(const LzStateSoA* in, const void* sym, int32_t sym_width, const LzStateSoA* out,
                                 int64_t B, void*) {
    if (B < 0 || (sym_width != 1 && sym_width != 4)) return LZ_ERR_ARG;
    if (B == 0) return LZ_OK;
    if (!soa_ok(in) || !soa_ok(out) || !sym) return LZ_ERR_ARG;
    for (int64_t i = 0; i < B; ++i) {
        const int k = load_sym(sym, sym_width, i);
        if (k < 0) continue;
        for (int x = 0; x < 36; ++x) {
            const int y = kSym.cell[k][x];
            out->board[i * 36 + y] = in->board[i * 36 + x];
            out->marks_black[i * 36 + y] = in->marks_black[i * 36 + x];
            out->marks_white[i * 36 + y] = in->marks_white[i * 36 + x];
        }
        out->phase[i] = in->phase[i]; out->current_player[i] = in->current_player[i];
        out->pending_marks_required[i] = in->pending_marks_required[i];
        out->pending_marks_remaining[i] = in->pending_marks_remaining[i];
        out->pending_captures_required[i] = in->pending_captures_required[i];
        out->pending_captures_remaining[i] = in->pending_captures_remaining[i];
        out->forced_removals_done[i] = in->forced_removals_done[i];
        out->move_count[i] = in->move_count[i]; out->moves_since_capture[i] = in->moves_since_capture[i];
    }
    return LZ_OK;
}

int lz_symmetry_transform_packed(const int64_t* in, const void* sym, int32_t sym_width, int64_t* out, int64_t B, void*) {
    if (B < 0 || (sym_width != 1 && sym_width != 4)) return LZ_ERR_ARG;
    if (B == 0) return LZ_OK;
    if (!in || !out || !sym) return LZ_ERR_ARG;
    for (int64_t i = 0; i < B; ++i) {
        const int k = load_sym(sym, sym_width, i);
        if (k < 0) continue;
        Packed p;
        std::memcpy(&p, in + i * 4, sizeof(Packed));
        const Packed o = sym_packed(k, p);
        std::memcpy(out + i * 4, &o, sizeof(Packed));
    }
    return LZ_OK;
}

}  // extern "C"
