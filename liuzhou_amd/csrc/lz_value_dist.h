// lz_value_dist.h -- scalar arithmetic of the distributional value target of merged positions (lz_value_dist.hip,
// lz_value_dist_host.cpp; the loss reads the table in lz_train.hip; DESIGN.md section 31 has the reasons).
//
// The value head is a distribution over 101 bins trained by cross entropy against a two-hot target.  Cross entropy is
// linear in its target, so the target of a row merged from c rows is the mean of the members' two-hot distributions,
// not the two-hot of their mean value.  `two_hot` is the bin assignment of the loss kernel (policy_value_loss_kernel,
// anti_draw == 0) in float32, `group_distribution` the mean of a group in ONE association: per bin a double, summed
// sequentially from 0.0 in member order, divided by the count, rounded once.  A group whose members share their
// (value, soft) bits therefore gets that member's two-hot exactly: c * x / c is exact in double for a float x and
// c < 2^29.
//
// Compiles for device and host; the mix is never contracted into an FMA (both builds pass -ffp-contract=off, and the
// function says so itself), so the device, the host build and numpy give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lz_rules.h"

#if defined(__clang__)
#define LZ_VD_NO_CONTRACT _Pragma("clang fp contract(off)")
#define LZ_VD_NO_CONTRACT_ATTR
#elif defined(__GNUC__)
#define LZ_VD_NO_CONTRACT
#define LZ_VD_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#else
#define LZ_VD_NO_CONTRACT
#define LZ_VD_NO_CONTRACT_ATTR
#endif

namespace lzvdist {

constexpr int kBins = 101;

struct TwoHot {
    int lo, hi;
    float frac;                                                // the mass of bin hi; bin lo holds 1 - frac
};

// Total on any input bits: the clamp sends a NaN to -1 (fmaxf returns its other operand), so u is finite, and no
// float is converted to int outside [0, 100].
LZ_VD_NO_CONTRACT_ATTR LZ_HD TwoHot two_hot(float value, float soft, float alpha) {
    LZ_VD_NO_CONTRACT
    const float a = (1.0f - alpha) * value;
    const float b = alpha * soft;
    float mixed = a + b;
    mixed = fminf(fmaxf(mixed, -1.0f), 1.0f);
    const float step = 2.0f / (float)(kBins - 1);
    const float u = (mixed + 1.0f) / step;
    const float fl = floorf(u);
    TwoHot t;
    t.lo = fl >= 0.0f ? (fl < (float)(kBins - 1) ? (int)fl : kBins - 1) : 0;       // a NaN compares false: bin 0
    t.hi = t.lo + 1 > kBins - 1 ? kBins - 1 : t.lo + 1;
    t.frac = fminf(fmaxf(u - (float)t.lo, 0.f), 1.f);
    if (t.hi == t.lo) t.frac = 0.f;
    return t;
}

// what a member adds to bin b: formed in float32 as the loss kernel forms tg0, widened by the caller
LZ_HD float bin_mass(const TwoHot& t, int b) { return (b == t.lo ? 1.0f - t.frac : 0.f) + (b == t.hi ? t.frac : 0.f); }

// ---- one group, sequentially (the host build; the kernel keeps bins l and l + 64 of lane l in the same order) ------------
// value / soft: the element e lives at base + e * stride_bytes.  members[0..c): positions, taken through `index` when it
// is given.  The caller has checked every member.
LZ_HD float load_f32(const void* base, int64_t stride_bytes, int64_t e) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(base) + e * stride_bytes);
}
LZ_HD void group_distribution(const void* value_base, const void* soft_base, int64_t stride_bytes, const int64_t* index,
                              const int64_t* members, int64_t c, float alpha, float* dist /*[101]*/) {
    double S[kBins];
    for (int b = 0; b < kBins; ++b) S[b] = 0.0;
    for (int64_t i = 0; i < c; ++i) {
        const int64_t e = index ? index[members[i]] : members[i];
        const TwoHot t = two_hot(load_f32(value_base, stride_bytes, e), load_f32(soft_base, stride_bytes, e), alpha);
        for (int b = 0; b < kBins; ++b) S[b] += (double)bin_mass(t, b);
    }
    for (int b = 0; b < kBins; ++b) dist[b] = (float)(S[b] / (double)c);
}

}  // namespace lzvdist
