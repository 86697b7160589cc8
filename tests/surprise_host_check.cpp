// Host build of csrc/lz_surprise.h (tests/test_policy_surprise_cpu.py): the game's resampling offset and the plain
// sequential plan of a whole game, as the kernels use them, against the numpy restatement tests/policy_surprise.py.
#include <stdint.h>
#include <stddef.h>

#include "../liuzhou_amd/csrc/lz_surprise.h"

extern "C" {

// the game's u in [0, 1) as float32
float lzsurprise_game_u(uint64_t seed, int64_t game) { return lzsurprise::game_u(seed, game); }

// src[0..n) of one game; returns the rows that got no slot, *sum_out = S
int64_t lzsurprise_plan(const float* s, int64_t n, double alpha, double u, int32_t* src, double* sum_out) {
    return lzsurprise::plan(s, n, alpha, u, src, sum_out);
}

// one row's surprise from its legal mask, policy target and prior (the note kernel's terms, summed in action order)
double lzsurprise_row(const uint8_t* legal, const float* pi, const float* p, int T) {
    double acc = 0.0;
    for (int a = 0; a < T; ++a) acc += lzsurprise::term(legal[a] != 0, pi[a], p[a]);
    return acc > 0.0 ? acc : 0.0;
}

double lzsurprise_weight(double alpha, int64_t n, double s, double S) { return lzsurprise::weight(alpha, n, s, S); }

int64_t lzsurprise_count(double c_prev, double c_cur, double u) { return lzsurprise::count(c_prev, c_cur, u); }

}
