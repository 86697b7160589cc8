// Host build of the Gumbel variates of liuzhou_amd/csrc/lz_rng.h for tests/test_gumbel_rng.py (compiled on demand into
// tests/_build/): the uniforms must equal the numpy restatement over oracle/rng_oracle.py bit for bit.
#include <stdint.h>

#include "../liuzhou_amd/csrc/lz_rng.h"

extern "C" {

// u[g * count + k], out[g * count + k] for child rank k < count of (game[g], ply[g])
void hc_rng_gumbel(uint64_t seed, const int64_t* game, const int64_t* ply, int64_t B, int64_t count, float* u, float* out) {
    for (int64_t g = 0; g < B; ++g)
        for (int64_t k = 0; k < count; ++k) {
            u[g * count + k] = lzrng::gumbel_u(lzrng::draw(seed, game[g], ply[g], lzrng::kPurposeGumbel, 1u + (uint32_t)k, 0u).x);
            out[g * count + k] = lzrng::gumbel_draw(seed, game[g], ply[g], (uint32_t)k);
        }
}

}  // extern "C"
