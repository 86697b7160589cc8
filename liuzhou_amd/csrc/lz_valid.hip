// lz_valid.hip -- validation metrics of the policy + bucketed-value network on rows it was not trained on
// (liuzhou_amd/validation.py; the scalar rules and the output layout: csrc/lz_valid.h).
//
// valid_row_metrics_kernel: one wavefront per row, lanes over the 220 actions / 101 value bins, like the loss kernel of
// lz_train.hip, whose conventions are restated here (lz_train.hip itself is untouched):
//   combined logits     placement = lp1[cell], movement = lp2[from] + lp1[to] (-inf off the board), selections =
//                       lpmc[cell], auxiliary = 0
//   masked log-softmax  legal entries only; no legal entry or a non-finite log-sum-exp => lse 0; non-finite
//                       log-probabilities => -50
//   two-hot target      on clamp((1 - alpha) z + alpha soft, -1, 1), 101 bins; no anti-draw substitution
// A row reads ~2 KB and writes 64 B; there are no gradients, so nothing has to be scattered between lanes: no LDS, no
// atomics.  Every index is a function of the row number and the lane only, so every bit pattern of every input ends in
// defined outputs (possibly NaN) and no access outside the row.
//
// valid_reduce_kernel: one wavefront per group of csrc/lz_valid.h, the association written there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/liuzhou_hip.h"
#include "lz_valid.h"
#include "lz_wave.h"

namespace {

using namespace lzvalid;

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBins = 101;
constexpr int kTotal = 220;

__device__ __forceinline__ int move_dest_cell(int from, int dir) {      // DIRECTIONS: up, down, left, right
    const int r = from / 6, c = from - 6 * r;
    const int nr = r + (dir == 0 ? -1 : dir == 1 ? 1 : 0), nc = c + (dir == 2 ? -1 : dir == 3 ? 1 : 0);
    return (nr < 0 || nr > 5 || nc < 0 || nc > 5) ? -1 : nr * 6 + nc;
}

// the lowest action whose lane holds `hit`, given the four ballots of the four 64-action slots; -1 if none
__device__ __forceinline__ int lowest_action(uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3) {
    if (b0) return __builtin_ctzll(b0);
    if (b1) return 64 + __builtin_ctzll(b1);
    if (b2) return 128 + __builtin_ctzll(b2);
    if (b3) return 192 + __builtin_ctzll(b3);
    return -1;
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void valid_row_metrics_kernel(
    const float* __restrict__ lp1, const float* __restrict__ lp2, const float* __restrict__ lpm,
    const float* __restrict__ vlogits, const uint8_t* __restrict__ legal, const float* __restrict__ target,
    const float* __restrict__ value, const float* __restrict__ soft, const float* __restrict__ planes, int64_t B,
    float alpha, float* __restrict__ rows, int32_t* __restrict__ cls) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wv;
    if (s >= B) return;
    const float raw_v = value[s];
    const bool hard_draw = fabsf(raw_v) < 1e-8f;

    // ---- phase: cell 0 of planes 4..10 ----
    const float ph_cell = lane < kPhases ? planes[s * kPlaneFloats + (kPhasePlane0 + lane) * 36] : 0.f;
    const int phase = phase_of_bits((uint32_t)__ballot(lane < kPhases && ph_cell != 0.f));

    // ---- policy ----
    float h1 = 0.f, h2 = 0.f, hm = 0.f;
    if (lane < 36) { h1 = lp1[s * 36 + lane]; h2 = lp2[s * 36 + lane]; hm = lpm[s * 36 + lane]; }
    float c[4], t[4]; bool lg[4];
    float mx = -INFINITY, tmx = -INFINITY, tsum = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int a = it * kWave + lane;
        const bool in = a < kTotal;
        int from = 0, dest = 0, cell = 0;
        bool dest_ok = true;
        if (a >= 36 && a < 180) {
            from = (a - 36) >> 2;
            const int d = move_dest_cell(from, (a - 36) & 3);
            dest_ok = d >= 0;
            dest = d < 0 ? 0 : d;
        } else if (a >= 180 && a < 216) cell = a - 180;
        else if (a < 36) cell = a;
        const float p1d = __shfl(h1, dest), p2f = __shfl(h2, from), p1c = __shfl(h1, cell), pmc = __shfl(hm, cell);
        float x = a < 36 ? p1c : a < 180 ? (dest_ok ? p2f + p1d : -INFINITY) : a < 216 ? pmc : 0.f;
        lg[it] = in && legal[s * kTotal + (in ? a : 0)] != 0;
        t[it] = in ? target[s * kTotal + a] : 0.f;
        c[it] = lg[it] ? x : -INFINITY;
        mx = fmaxf(mx, c[it]);
        tmx = fmaxf(tmx, lg[it] ? t[it] : -INFINITY);
        tsum += t[it];
    }
    mx = lzw::wave_max(mx);
    tmx = lzw::wave_max(tmx);
    tsum = lzw::wave_sum(tsum);
    float se = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) se += (lg[it] && c[it] > -INFINITY) ? expf(c[it] - mx) : 0.f;
    se = lzw::wave_sum(se);
    const uint64_t l0 = __ballot(lg[0]), l1 = __ballot(lg[1]), l2 = __ballot(lg[2]), l3 = __ballot(lg[3]);
    const bool any_legal = (l0 | l1 | l2 | l3) != 0;
    float lse = mx + logf(se);
    const bool lse_ok = any_legal && isfinite(lse);
    if (!lse_ok) lse = 0.f;
    float ce = 0.f, ent = 0.f, hnet = 0.f;
    float p[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        float lp = lg[it] ? c[it] - lse : 0.f;
        if (!isfinite(lp)) lp = -50.f;
        const float lps = fmaxf(lp, -50.f);
        ce -= t[it] * lps;
        ent -= t[it] * logf(fmaxf(t[it], 1e-8f));
        p[it] = (lse_ok && lg[it] && c[it] > -INFINITY) ? expf(c[it] - lse) : 0.f;
        hnet -= p[it] > 0.f ? p[it] * (c[it] - lse) : 0.f;
    }
    ce = lzw::wave_sum(ce);
    ent = lzw::wave_sum(ent);
    hnet = lzw::wave_sum(hnet);
    // arg-maxima over the legal actions: the wave maximum of the keys (NaN as -inf), then the lowest action that holds it
    const int net_top = lowest_action(__ballot(lg[0] && argmax_key(c[0]) == mx), __ballot(lg[1] && argmax_key(c[1]) == mx),
                                      __ballot(lg[2] && argmax_key(c[2]) == mx), __ballot(lg[3] && argmax_key(c[3]) == mx));
    const int tgt_arg = lowest_action(__ballot(lg[0] && argmax_key(t[0]) == tmx), __ballot(lg[1] && argmax_key(t[1]) == tmx),
                                      __ballot(lg[2] && argmax_key(t[2]) == tmx), __ballot(lg[3] && argmax_key(t[3]) == tmx));
    const bool policy_valid = tsum > 1e-8f && any_legal;
    const int tgt_top = policy_valid ? tgt_arg : -1;
    float p_top = 0.f;
    if (tgt_arg >= 0) {                                                  // wave-uniform: p of the lane that owns the action
        const int slot = tgt_arg >> 6;
        const float ps = slot == 0 ? p[0] : slot == 1 ? p[1] : slot == 2 ? p[2] : p[3];
        p_top = lzw::lane_bcast(ps, __builtin_amdgcn_readfirstlane(tgt_arg & 63));
    }

    // ---- value: two-hot bucket cross entropy on clamp((1-alpha)*v + alpha*soft, -1, 1), expectation over the centres ----
    float mixed = (1.0f - alpha) * raw_v + alpha * soft[s];
    mixed = fminf(fmaxf(mixed, -1.0f), 1.0f);
    const float step = 2.0f / (float)(kBins - 1);
    const float u = (mixed + 1.0f) / step;
    int lo = (int)floorf(u);
    lo = lo < 0 ? 0 : (lo > kBins - 1 ? kBins - 1 : lo);
    const int hi = lo + 1 > kBins - 1 ? kBins - 1 : lo + 1;
    float frac = fminf(fmaxf(u - (float)lo, 0.f), 1.f);
    if (hi == lo) frac = 0.f;
    const float v0 = vlogits[s * kBins + lane];
    const bool has1 = lane + 64 < kBins;
    const float v1 = has1 ? vlogits[s * kBins + lane + 64] : -INFINITY;
    const float vm = lzw::wave_max(fmaxf(v0, v1));
    const float e0 = expf(v0 - vm), e1 = has1 ? expf(v1 - vm) : 0.f;
    const float vs = lzw::wave_sum(e0 + e1);
    const float vlse = vm + logf(vs);
    const float tg0 = (lane == lo ? 1.0f - frac : 0.f) + (lane == hi ? frac : 0.f);
    const float tg1 = (lane + 64 == lo ? 1.0f - frac : 0.f) + (lane + 64 == hi ? frac : 0.f);
    float cev = -(tg0 * (v0 - vlse)) - (has1 ? tg1 * (v1 - vlse) : 0.f);
    cev = lzw::wave_sum(cev);
    const float sm0 = e0 / vs, sm1 = e1 / vs;
    const float ctr0 = (float)(lane - 50) * 0.02f, ctr1 = (float)(lane + 14) * 0.02f;      // -1 + k / 50
    const float v_hat = lzw::wave_sum(sm0 * ctr0 + (has1 ? sm1 * ctr1 : 0.f));
    const float dv = v_hat - raw_v;

    if (lane == 0) {
        float* r = rows + s * kRowCols;
        r[kKl] = policy_valid ? ce - ent : 0.f;
        r[kCe] = policy_valid ? ce : 0.f;
        r[kHTarget] = policy_valid ? ent : 0.f;
        r[kHNet] = policy_valid ? hnet : 0.f;
        r[kTop1] = (policy_valid && net_top == tgt_arg) ? 1.f : 0.f;
        r[kPTop] = policy_valid ? p_top : 0.f;
        r[kBucketCe] = cev;
        r[kVHat] = v_hat;
        r[kSqErr] = dv * dv;
        r[kSignOk] = (!hard_draw && v_hat * raw_v > 0.f) ? 1.f : 0.f;
        r[kDecisive] = hard_draw ? 0.f : 1.f;
        r[kPolicyValid] = policy_valid ? 1.f : 0.f;
        int32_t* k = cls + s * kClsCols;
        k[0] = phase;
        k[1] = calib_bin(v_hat);
        k[2] = net_top;
        k[3] = tgt_top;
    }
}

__device__ __forceinline__ double xor_f64(double v, int d) {
    const int lo = __shfl_xor(__double2loint(v), d), hi = __shfl_xor(__double2hiint(v), d);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kWave) void valid_reduce_kernel(const float* __restrict__ rows, const int32_t* __restrict__ cls,
                                                             const float* __restrict__ value, int64_t B,
                                                             double* __restrict__ acc, double* __restrict__ zsum) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x;
    double part[kSumCols];
#pragma unroll
    for (int c = 0; c < kSumCols; ++c) part[c] = 0.0;
    for (int64_t i = lane; i < B; i += kLanes) {
        if (!in_group(g, cls[i * kClsCols + 0], cls[i * kClsCols + 1])) continue;
        float r[kRowCols];
#pragma unroll
        for (int c = 0; c < kRowCols; ++c) r[c] = rows[i * kRowCols + c];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < kRowCols; ++c) ok = ok && is_finite_f32(r[c]);
        if (ok) {
#pragma unroll
            for (int c = 0; c < kRowCols; ++c) part[c] = part[c] + (double)r[c];
            part[kRowCols] = part[kRowCols] + 1.0;
            if (value != nullptr) part[kAccCols] = part[kAccCols] + (double)value[i];
        } else {
            part[kRowCols + 1] = part[kRowCols + 1] + 1.0;
        }
    }
#pragma unroll
    for (int d = kLanes / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < kSumCols; ++c) part[c] = part[c] + xor_f64(part[c], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kAccCols; ++c) acc[g * kAccCols + c] = acc[g * kAccCols + c] + part[c];
        if (value != nullptr) zsum[g] = zsum[g] + part[kAccCols];
    }
}

__global__ __launch_bounds__(256) void valid_classify_kernel(const float* __restrict__ planes, const float* __restrict__ v_hat,
                                                             int64_t stride, int64_t B, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    out[i * 2 + 0] = phase_of_planes(planes + i * kPlaneFloats);
    out[i * 2 + 1] = calib_bin(v_hat[i * stride]);
}

}  // namespace

extern "C" int lz_valid_row_metrics(const float* log_p1, const float* log_p2, const float* log_pmc,
                                    const float* value_logits, const uint8_t* legal_mask, const float* policy_target,
                                    const float* value_target, const float* soft_value_target, const float* planes,
                                    int64_t batch, float soft_label_alpha, float* rows, int32_t* cls, void* stream) {
    if (batch < 0) return LZ_ERR_ARG;
    if (batch == 0) return LZ_OK;
    if (!log_p1 || !log_p2 || !log_pmc || !value_logits || !legal_mask || !policy_target || !value_target ||
        !soft_value_target || !planes || !rows || !cls)
        return LZ_ERR_ARG;
    if ((batch + kWavesPerBlock - 1) / kWavesPerBlock > 0x7FFFFFFF) return LZ_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)((batch + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(valid_row_metrics_kernel, dim3(grid), dim3(kWave * kWavesPerBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), log_p1, log_p2, log_pmc, value_logits, legal_mask,
                       policy_target, value_target, soft_value_target, planes, batch, soft_label_alpha, rows, cls);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}

extern "C" int lz_valid_reduce(const float* rows, const int32_t* cls, const float* value, int64_t batch, double* acc,
                               double* zsum, void* stream) {
    if (batch < 0 || (value == nullptr) != (zsum == nullptr)) return LZ_ERR_ARG;
    if (batch == 0) return LZ_OK;
    if (!rows || !cls || !acc) return LZ_ERR_ARG;
    hipLaunchKernelGGL(valid_reduce_kernel, dim3(kGroups), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), rows, cls,
                       value, batch, acc, zsum);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}

extern "C" int lz_valid_classify(const float* planes, const float* v_hat, int64_t v_hat_stride, int64_t batch,
                                 int32_t* phase_bin, void* stream) {
    if (batch < 0 || v_hat_stride < 1) return LZ_ERR_ARG;
    if (batch == 0) return LZ_OK;
    if (!planes || !v_hat || !phase_bin) return LZ_ERR_ARG;
    if ((batch + 255) / 256 > 0x7FFFFFFF) return LZ_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(valid_classify_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), planes, v_hat, v_hat_stride, batch, phase_bin);
    return hipGetLastError() == hipSuccess ? LZ_OK : LZ_ERR_LAUNCH;
}
