// lz_surprise.h -- scalar arithmetic of policy surprise weighting (lz_ops.hip: wave_note_surprise_kernel,
// wave_surprise_resample_kernel; liuzhou_amd/policy_surprise.py states the rule, DESIGN.md section 20 the reasons).
// A finished game's N recorded rows share the total weight N: w_j = (1 - alpha) + alpha N s_j / S with s_j the row's
// surprise KL(policy target || network prior) and S their sum.  The weights become integer copy counts by systematic
// resampling with one uniform u per game, so the game keeps its N row slots: with C_j the running sum of the weights,
// row j is written floor(C_j + u) - floor(C_(j-1) + u) times.  Everything is double; compiled for the device and for
// the host (tests/surprise_host_check.cpp checks it against the numpy restatement tests/policy_surprise.py).
#pragma once
#include <stdint.h>
#include <math.h>

#include "lz_rng.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZ_SURPRISE_HD __host__ __device__
#else
#define LZ_SURPRISE_HD
#endif

namespace lzsurprise {

constexpr double kPriorFloor = 1e-30;     // p is clamped here under the logarithm
constexpr double kFlatSum = 1e-12;        // S <= kFlatSum * N: no surprise to hand out, every weight is 1

// one action's term of the surprise: pi (log pi - log max(p, floor)) for a legal action with pi > 0, else 0
LZ_SURPRISE_HD inline double term(bool legal, float pi, float p) {
    if (!legal || !(pi > 0.0f)) return 0.0;
    const double q = (double)p > kPriorFloor ? (double)p : kPriorFloor;
    return (double)pi * (log((double)pi) - log(q));
}

// weight of a row with surprise s in a game of n rows whose surprises sum to S
LZ_SURPRISE_HD inline double weight(double alpha, int64_t n, double s, double S) {
    if (!(S > kFlatSum * (double)n)) return 1.0;
    return (1.0 - alpha) + alpha * (double)n * s / S;
}

// copies of a row whose weights' running sum goes from c_prev to c_cur
LZ_SURPRISE_HD inline int64_t count(double c_prev, double c_cur, double u) {
    return (int64_t)floor(c_cur + u) - (int64_t)floor(c_prev + u);
}

// the game's uniform in [0, 1): one Philox draw, a pure function of (seed, game id) -- purpose 3, ply 0, index 1022
LZ_SURPRISE_HD inline float game_u(uint64_t seed, int64_t game) {
    return lzrng::u01(lzrng::draw(seed, game, 0, lzrng::kPurposeGumbel, lzrng::kIndexPolicySurprise, 0u).x);
}

// Plain sequential plan of one game: src[k] (0 <= k < n) = the row that output slot k takes, non-decreasing.  C_n is
// set to n exactly, so the counts sum to n whatever the rounding of the running sum.  Returns the rows that got no
// slot (= the extra copies written); *sum_out (optional) = S.
LZ_SURPRISE_HD inline int64_t plan(const float* s, int64_t n, double alpha, double u, int32_t* src, double* sum_out) {
    double S = 0.0;
    for (int64_t j = 0; j < n; ++j) S += (double)s[j];
    if (sum_out) *sum_out = S;
    double c_prev = 0.0;
    int64_t k = 0, dropped = 0;
    for (int64_t j = 0; j < n; ++j) {
        const double c_cur = j == n - 1 ? (double)n : c_prev + weight(alpha, n, (double)s[j], S);
        const int64_t c = count(c_prev, c_cur, u);
        if (c == 0) ++dropped;
        for (int64_t i = 0; i < c && k < n; ++i) src[k++] = (int32_t)j;
        c_prev = c_cur;
    }
    return dropped;
}

}  // namespace lzsurprise
