// lz_valid.h -- scalar rules of the validation metrics (lz_valid.hip, lz_valid_host.cpp; liuzhou_amd/validation.py is the
// interface, DESIGN.md section 28 the reasons).
//
// A validated row leaves the row kernel as 12 floats and 4 integers:
//   rows[12] = kl, ce, h_target, h_net, top1, p_top, bucket_ce, v_hat, sq_err, sign_ok, decisive, policy_valid
//   cls[4]   = phase (-1, 0..6), calibration bin (0..9), network top action, target top action (-1: none)
// The reduction adds a batch's rows into acc f64[18,14]: group 0 is every row, groups 1..7 the phases 0..6, groups 8..17
// the calibration bins 0..9; columns 0..11 the sums of the row columns, column 12 the rows counted, column 13 the rows
// skipped.  A row with a non-finite entry among its 12 floats is skipped in each of its groups (column 13 only).  The
// value target z is not among the 12 floats; the calibration table needs its mean, so the reduction optionally adds the z
// of every counted row into zsum f64[18], as a fifteenth column with the same membership and association.
//
// The sums have one association, so that the kernel, the host build and the numpy restatement (tests/valid_ref.py) agree
// bit for bit: lane l of 64 adds its rows l, l + 64, ... in ascending order to a partial that starts at 0.0; the 64
// partials are combined by a butterfly, v[l] = v[l] + v[l ^ d] for d = 32, 16, 8, 4, 2, 1 (after which every lane holds
// the same total); the total is added to acc.  All double.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lz_rules.h"

namespace lzvalid {

constexpr int kRowCols = 12;
constexpr int kClsCols = 4;
constexpr int kPhases = 7;                  // planes 4..10
constexpr int kCalBins = 10;
constexpr int kGroups = 1 + kPhases + kCalBins;
constexpr int kAccCols = kRowCols + 2;
constexpr int kSumCols = kAccCols + 1;      // + the optional sum of z
constexpr int kLanes = 64;
constexpr int kPlaneFloats = 396;
constexpr int kPhasePlane0 = 4;

enum RowCol { kKl = 0, kCe, kHTarget, kHNet, kTop1, kPTop, kBucketCe, kVHat, kSqErr, kSignOk, kDecisive, kPolicyValid };

// ---- classification --------------------------------------------------------------------------------------------------------
// calibration bin of v_hat: min(9, max(0, (int)floorf((v_hat + 1) * 5))), written so that no float outside the range of
// int is converted; NaN gives bin 0
LZ_HD int calib_bin(float v_hat) {
    const float u = floorf((v_hat + 1.f) * 5.f);
    return u >= 9.f ? 9 : (u >= 0.f ? (int)u : 0);
}
// phase: the lowest k whose plane 4 + k is not zero at cell 0 (NaN is not zero); -1 if none.  `planes` is one row.
LZ_HD int phase_of_planes(const float* planes) {
    for (int k = 0; k < kPhases; ++k)
        if (planes[(kPhasePlane0 + k) * 36] != 0.f) return k;
    return -1;
}
// the same from a bit word: bit k set iff plane 4 + k is not zero at cell 0
LZ_HD int phase_of_bits(uint32_t set) {
    set &= (1u << kPhases) - 1u;
    if (!set) return -1;
    int k = 0;
    while (!((set >> k) & 1u)) ++k;
    return k;
}

// ---- arg-maximum over the legal actions ------------------------------------------------------------------------------------
// NaN compares as -inf; among equal keys the lowest action index wins
LZ_HD float argmax_key(float x) { return x == x ? x : -INFINITY; }
// does candidate (x, ix) replace (best, ibest)?  ibest < 0: nothing yet
LZ_HD bool argmax_better(float x, int ix, float best, int ibest) {
    if (ibest < 0) return true;
    const float a = argmax_key(x), b = argmax_key(best);
    return a > b || (a == b && ix < ibest);
}
// the rule over a whole row (host and tests; the kernel takes the same decision with a wave maximum and a ballot)
LZ_HD int argmax_legal(const float* x, const uint8_t* legal, int n) {
    int ibest = -1;
    float best = -INFINITY;
    for (int a = 0; a < n; ++a)
        if (legal[a] != 0 && argmax_better(x[a], a, best, ibest)) { best = x[a]; ibest = a; }
    return ibest;
}

// ---- membership --------------------------------------------------------------------------------------------------------------
LZ_HD bool is_finite_f32(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN
LZ_HD bool row_is_counted(const float* r) {
    bool ok = true;
    for (int c = 0; c < kRowCols; ++c) ok = ok && is_finite_f32(r[c]);
    return ok;
}
// is a row of this phase and calibration bin a member of group g?  Values outside -1..6 / 0..9 belong to group 0 only.
LZ_HD bool in_group(int g, int phase, int bin) {
    if (g == 0) return true;
    if (g <= kPhases) return phase == g - 1;
    return g < kGroups && bin == g - 1 - kPhases;
}

// ---- the reduction ----------------------------------------------------------------------------------------------------------
// lane `lane`'s partial sums of group g over a batch: part[15] must start at 0.0; `value` may be null (part[14] stays 0)
LZ_HD void lane_partial(int g, int lane, const float* rows, const int32_t* cls, const float* value, int64_t batch,
                        double* part) {
    for (int64_t i = lane; i < batch; i += kLanes) {
        if (!in_group(g, cls[i * kClsCols + 0], cls[i * kClsCols + 1])) continue;
        const float* r = rows + i * kRowCols;
        if (row_is_counted(r)) {
            for (int c = 0; c < kRowCols; ++c) part[c] = part[c] + (double)r[c];
            part[kRowCols] = part[kRowCols] + 1.0;
            if (value) part[kAccCols] = part[kAccCols] + (double)value[i];
        } else {
            part[kRowCols + 1] = part[kRowCols + 1] + 1.0;
        }
    }
}
// the butterfly over the 64 partials of one column, in place; afterwards every entry is the total
inline void butterfly64(double* v) {
    for (int d = kLanes / 2; d >= 1; d >>= 1) {
        double t[kLanes];
        for (int l = 0; l < kLanes; ++l) t[l] = v[l] + v[l ^ d];
        for (int l = 0; l < kLanes; ++l) v[l] = t[l];
    }
}

}  // namespace lzvalid
