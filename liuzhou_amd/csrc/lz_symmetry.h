// lz_symmetry.h -- the 8 symmetries of the 6x6 board (the dihedral group D4) on cells, move directions, the 220-d
// action index and the packed state record (host + device).
//
// No rule of Liuzhou chess names a particular cell: a Fang is any 2x2 square, a Zhou any full row or column, a move
// one step up, down, left or right.  So every element sigma of D4 maps a game onto an equivalent game, and a network
// evaluation of sigma(s) mapped back by sigma^-1 is an evaluation of s.
//
// Numbering (cells are r*6+c):
//   0 identity (r, c)       1 rotate 90 (c, 5-r)     2 rotate 180 (5-r, 5-c)   3 rotate 270 (5-c, r)
//   4 flip left-right (r, 5-c)   5 flip up-down (5-r, c)   6 transpose (c, r)   7 anti-transpose (5-c, 5-r)
// Every table below is computed from `sym_rc` at compile time; none is typed in.
//
// A transformed state has the piece of cell x on cell sigma(x): out[p] = in[sigma^-1(p)].  Actions move the same way:
// placement a -> sigma(a), movement 36+4*from+d -> 36+4*sigma(from)+sigma_d(d), selection 180+cell -> 180+sigma(cell),
// the auxiliary indices 216..219 stay.  compose(a, b) is "b first, then a": sigma_compose(a,b)(x) = sigma_a(sigma_b(x)).
#pragma once
#include <stdint.h>

#include "lz_rules.h"

namespace lz {

constexpr int kSyms = 8;
constexpr int kActions = 220;

// (r, c) -> cell under element k (the table of the header comment)
LZ_HD constexpr int sym_rc(int k, int r, int c) {
    switch (k & 7) {
        case 0: return r * 6 + c;
        case 1: return c * 6 + (5 - r);
        case 2: return (5 - r) * 6 + (5 - c);
        case 3: return (5 - c) * 6 + r;
        case 4: return r * 6 + (5 - c);
        case 5: return (5 - r) * 6 + c;
        case 6: return c * 6 + r;
        default: return (5 - c) * 6 + (5 - r);
    }
}
LZ_HD constexpr int sym_cell(int k, int cell) { return sym_rc(k, cell / 6, cell % 6); }

struct SymTables {
    int8_t cell[kSyms][36];        // sigma_k(cell)
    int8_t inv[kSyms];             // sigma_inv[k] = sigma_k^-1
    int8_t comp[kSyms][kSyms];     // comp[a][b] = sigma_a o sigma_b
    int8_t dir[kSyms][4];          // direction d of lz_rules.h:move_dest (-6, +6, -1, +1) -> its image
    int16_t action[kSyms][kActions];
};

constexpr SymTables make_sym_tables() {
    SymTables t{};
    for (int k = 0; k < kSyms; ++k)
        for (int x = 0; x < 36; ++x) t.cell[k][x] = (int8_t)sym_cell(k, x);
    // composition and inverse: the element whose cell map equals the composed map
    for (int a = 0; a < kSyms; ++a)
        for (int b = 0; b < kSyms; ++b) {
            t.comp[a][b] = -1;
            for (int k = 0; k < kSyms; ++k) {
                bool same = true;
                for (int x = 0; x < 36; ++x) same = same && t.cell[k][x] == t.cell[a][t.cell[b][x]];
                if (same) { t.comp[a][b] = (int8_t)k; break; }
            }
            if (t.comp[a][b] == 0) t.inv[a] = (int8_t)b;
        }
    // directions: the step of d from an interior cell, mapped, is the step of dir[k][d] from the mapped cell
    constexpr int dr[4] = {-1, 1, 0, 0}, dc[4] = {0, 0, -1, 1};
    for (int k = 0; k < kSyms; ++k)
        for (int d = 0; d < 4; ++d) {
            const int from = sym_rc(k, 2, 2), dest = sym_rc(k, 2 + dr[d], 2 + dc[d]);
            t.dir[k][d] = -1;
            for (int e = 0; e < 4; ++e)
                if (from + 6 * dr[e] + dc[e] == dest) t.dir[k][d] = (int8_t)e;
        }
    for (int k = 0; k < kSyms; ++k)
        for (int a = 0; a < kActions; ++a) {
            int b = a;
            if (a < 36) b = t.cell[k][a];
            else if (a < 180) b = 36 + 4 * t.cell[k][(a - 36) >> 2] + t.dir[k][(a - 36) & 3];
            else if (a < 216) b = 180 + t.cell[k][a - 180];
            t.action[k][a] = (int16_t)b;
        }
    return t;
}
constexpr SymTables kSym = make_sym_tables();

static_assert(kSym.comp[1][kSym.inv[1]] == 0 && kSym.inv[1] == 3 && kSym.inv[6] == 6, "D4 inverses");
static_assert(kSym.comp[1][1] == 2 && kSym.comp[4][5] == 2, "D4 composition");
static_assert(kSym.dir[1][0] == 3 && kSym.dir[4][2] == 3 && kSym.dir[6][0] == 2, "direction permutation");

// inverse by formula (wave-uniform device code keeps k in a scalar register; no table load)
LZ_HD constexpr int sym_inverse(int k) { return (k & 7) == 1 ? 3 : (k & 7) == 3 ? 1 : (k & 7); }
static_assert(sym_inverse(0) == kSym.inv[0] && sym_inverse(1) == kSym.inv[1] && sym_inverse(2) == kSym.inv[2] &&
              sym_inverse(3) == kSym.inv[3] && sym_inverse(4) == kSym.inv[4] && sym_inverse(5) == kSym.inv[5] &&
              sym_inverse(6) == kSym.inv[6] && sym_inverse(7) == kSym.inv[7], "sym_inverse agrees with the table");

// 36-bit board: bit x -> bit sigma_k(x)
LZ_HD uint64_t sym_board(int k, uint64_t b) {
    uint64_t o = 0;
    for (int x = 0; x < 36; ++x) o |= ((b >> x) & 1ull) << sym_cell(k, x);
    return o;
}
// packed record (lz_rules.h:pack): the four boards permuted, the metadata of w0 above bit 35 kept
LZ_HD Packed sym_packed(int k, const Packed& p) {
    Packed o;
    o.w0 = (p.w0 & ~kFull) | sym_board(k, p.w0 & kFull);
    o.w1 = sym_board(k, p.w1 & kFull); o.w2 = sym_board(k, p.w2 & kFull); o.w3 = sym_board(k, p.w3 & kFull);
    return o;
}

#if defined(__HIPCC__)
// the same by a whole wave (k wave-uniform, p the same in every lane): lane q < 36 fetches the bit of sigma_k^-1(q),
// one ballot per word
__device__ __forceinline__ Packed sym_packed_wave(int k, const Packed& p, int lane) {
    const int src = lane < 36 ? sym_cell(sym_inverse(k), lane) : 0;
    const bool in = lane < 36;
    Packed o;
    o.w0 = (p.w0 & ~kFull) | (uint64_t)__ballot(in && ((p.w0 >> src) & 1ull));
    o.w1 = (uint64_t)__ballot(in && ((p.w1 >> src) & 1ull));
    o.w2 = (uint64_t)__ballot(in && ((p.w2 >> src) & 1ull));
    o.w3 = (uint64_t)__ballot(in && ((p.w3 >> src) & 1ull));
    return o;
}
#endif

}  // namespace lz
