// value_dist_host_check.cpp -- the host build of lz_merge_value_distributions (csrc/lz_value_dist_host.cpp,
// csrc/lz_value_dist.h) run over its edge cases as a stand-alone program, built by tests/test_value_dist_cpu.py with
// -fsanitize=address,undefined.  Every buffer is a heap block of exactly the size the ABI states, so a read outside the
// ring, the index or the order, or a write outside a table row, is an error of the address sanitizer; a float converted
// to int out of range is one of the undefined-behaviour sanitizer.  The checks below are the properties that need no
// second implementation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "liuzhou_hip.h"

namespace {

constexpr int kBins = 101, kRec = 360;
int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Heap {                                                  // an exact, 8-byte aligned heap block
    void* p;
    explicit Heap(size_t bytes) : p(std::malloc(bytes ? bytes : 1)) {}
    ~Heap() { std::free(p); }
    template <class T> T* as() { return static_cast<T*>(p); }
};

float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

const uint32_t kSentinel = 0x7FC0BEEFu;

}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const std::vector<float> specials = {
        -1.f, 1.f, 0.f, -0.f, 0.02f, -0.02f, 0.5f, std::nextafterf(0.5f, 2.f), std::nextafterf(0.5f, -2.f), 1.5f, -1.5f,
        from_bits(0x7FC00123u), from_bits(0xFFC00001u), from_bits(0x7F800001u), inf, -inf, from_bits(1u),
        from_bits(0x80000001u), from_bits(0x007FFFFFu), 3.0e38f, -3.0e38f};
    const int S = (int)specials.size();
    const float alphas[3] = {0.f, 0.25f, 1.f};

    // ---- tensor addressing: stride 4, no index.  Element e: value specials[e % S], soft specials[(e / S) % S]
    const int64_t n = (int64_t)S * S + 300;
    Heap value_h(n * 4), soft_h(n * 4);
    float* value = value_h.as<float>();
    float* soft = soft_h.as<float>();
    for (int64_t e = 0; e < n; ++e) { value[e] = specials[e % S]; soft[e] = specials[(e / S) % S]; }
    for (int64_t e = (int64_t)S * S; e < n; ++e) { value[e] = 0.3f; soft[e] = -0.7f; }      // 300 identical members
    // groups: every element alone, then pairs (e, n-1-e), then triples, then the 300 identical, then the bad ones
    std::vector<int64_t> order, begin;
    begin.push_back(0);
    for (int64_t e = 0; e < n; ++e) { order.push_back(e); begin.push_back((int64_t)order.size()); }
    const int64_t singles = n;
    for (int64_t e = 0; e + 1 < 40; e += 2) { order.push_back(e); order.push_back(n - 1 - e); begin.push_back((int64_t)order.size()); }
    for (int64_t e = 0; e + 2 < 60; e += 3) { order.push_back(e + 2); order.push_back(e); order.push_back(e + 1); begin.push_back((int64_t)order.size()); }
    const int64_t big = (int64_t)begin.size() - 1;
    for (int64_t e = (int64_t)S * S; e < n; ++e) order.push_back(e);
    begin.push_back((int64_t)order.size());
    const int64_t real = (int64_t)begin.size() - 1;
    const int64_t bad_entry = real;                            // a group with an order entry of -1
    order.push_back(3); order.push_back(-1); begin.push_back((int64_t)order.size());
    const int64_t empty = real + 1;                            // an empty range
    begin.push_back((int64_t)order.size());
    const int64_t groups = (int64_t)begin.size() - 1;
    const int64_t m = (int64_t)order.size();
    Heap order_h(m * 8), begin_h((groups + 1) * 8), row_h(groups * 4);
    std::memcpy(order_h.p, order.data(), m * 8);
    std::memcpy(begin_h.p, begin.data(), (groups + 1) * 8);
    int32_t* dist_row = row_h.as<int32_t>();
    // rows: group g -> row g, except three skipped ones; D = groups, so row `groups` is outside
    for (int64_t g = 0; g < groups; ++g) dist_row[g] = (int32_t)g;
    dist_row[5] = -1; dist_row[6] = (int32_t)groups; dist_row[7] = INT32_MIN;
    const int64_t D = groups;
    Heap dist_h(D * kBins * 4);
    float* dist = dist_h.as<float>();
    // NOTE: order entries index elements directly here, so m (the bound of an order entry) must cover n
    CHECK(m >= n);
    for (int ai = 0; ai < 3; ++ai) {
        const float alpha = alphas[ai];
        for (int64_t i = 0; i < D * kBins; ++i) dist[i] = from_bits(kSentinel);
        CHECK(lz_merge_value_distributions(value, soft, 4, n, nullptr, m, order_h.as<int64_t>(), begin_h.as<int64_t>(), groups,
                                           dist_row, alpha, dist, D, nullptr) == LZ_OK);
        for (int64_t g = 0; g < groups; ++g) {
            const float* row = dist + g * kBins;
            if (g == 5 || g == 6 || g == 7) {                  // skipped: the sentinel stays
                for (int b = 0; b < kBins; ++b) CHECK(bits_of(row[b]) == kSentinel);
                continue;
            }
            if (g == bad_entry || g == empty) {
                for (int b = 0; b < kBins; ++b) CHECK(bits_of(row[b]) == 0u);
                continue;
            }
            double sum = 0.0;
            int nonzero = 0;
            for (int b = 0; b < kBins; ++b) { CHECK(row[b] >= 0.f && row[b] <= 1.f); sum += row[b]; nonzero += row[b] != 0.f; }
            CHECK(std::fabs(sum - 1.0) <= 101 * 1.1920929e-7);
            const int64_t c = begin[g + 1] - begin[g];
            CHECK(nonzero >= 1 && nonzero <= 2 * c);
            if (g < singles) {                                 // a group of one: a two-hot, and a NaN value at alpha 0 is bin 0
                CHECK(nonzero <= 2);
                if (alpha == 0.f && std::isnan(value[g])) CHECK(row[0] == 1.f);
                const bool plain = alpha == 0.f && std::isfinite(soft[g]);      // 0 * inf is a NaN: bin 0 again
                if (plain && value[g] == 0.f) CHECK(row[50] == 1.f);
                if (plain && value[g] >= 1.f) CHECK(row[100] == 1.f);
                if (plain && value[g] <= -1.f) CHECK(row[0] == 1.f);
                if (alpha == 0.f && !std::isfinite(soft[g])) CHECK(row[0] == 1.f);
            }
        }
        // the 300 identical members give their member's two-hot exactly: the same bits as the single member's row
        CHECK(std::memcmp(dist + big * kBins, dist + ((int64_t)S * S) * kBins, kBins * 4) == 0);
    }
    // the (+1, -1) pair at alpha 0: halves on bins 0 and 100
    {
        Heap v2(8), s2(8), o2(16), b2(16), r2(4), d2(kBins * 4);
        v2.as<float>()[0] = 1.f; v2.as<float>()[1] = -1.f; s2.as<float>()[0] = 0.f; s2.as<float>()[1] = 0.f;
        o2.as<int64_t>()[0] = 0; o2.as<int64_t>()[1] = 1; b2.as<int64_t>()[0] = 0; b2.as<int64_t>()[1] = 2;
        r2.as<int32_t>()[0] = 0;
        CHECK(lz_merge_value_distributions(v2.p, s2.p, 4, 2, nullptr, 2, o2.as<int64_t>(), b2.as<int64_t>(), 1, r2.as<int32_t>(),
                                           0.f, d2.as<float>(), 1, nullptr) == LZ_OK);
        const float* row = d2.as<float>();
        for (int b = 0; b < kBins; ++b) CHECK(row[b] == ((b == 0 || b == 100) ? 0.5f : 0.f));
    }

    // ---- ring addressing: stride 360 with an index; the ring is exactly `capacity` records and the bases point at
    // bytes 348 / 352 of record 0, so the last record's floats end 4 bytes before the end of the block
    {
        const int64_t capacity = 37, sel = 50;
        Heap ring_h(capacity * kRec), slot_h(sel * 8), ord_h(sel * 8), beg_h(5 * 8), rows_h(4 * 4), out_h(3 * kBins * 4);
        uint8_t* ring = ring_h.as<uint8_t>();
        std::memset(ring, 0xA5, capacity * kRec);
        for (int64_t s = 0; s < capacity; ++s) {
            const float v = specials[s % S], sf = specials[(s * 7 + 3) % S];
            std::memcpy(ring + s * kRec + 348, &v, 4);
            std::memcpy(ring + s * kRec + 352, &sf, 4);
        }
        int64_t* slot = slot_h.as<int64_t>();
        for (int64_t j = 0; j < sel; ++j) slot[j] = (j * 11) % capacity;
        slot[0] = 0; slot[1] = capacity - 1;                   // both ends of the ring
        slot[48] = capacity; slot[49] = -1;                    // outside the ring
        int64_t* ord = ord_h.as<int64_t>();
        for (int64_t j = 0; j < sel; ++j) ord[j] = j;
        int64_t* beg = beg_h.as<int64_t>();
        beg[0] = 0; beg[1] = 2; beg[2] = 48; beg[3] = 49; beg[4] = 50;
        int32_t* rows = rows_h.as<int32_t>();
        rows[0] = 2; rows[1] = 0; rows[2] = 1; rows[3] = 1;     // groups 2 and 3 (both outside the ring) share row 1
        float* out = out_h.as<float>();
        for (int ai = 0; ai < 3; ++ai) {
            for (int i = 0; i < 3 * kBins; ++i) out[i] = from_bits(kSentinel);
            CHECK(lz_merge_value_distributions(ring + 348, ring + 352, kRec, capacity, slot, sel, ord, beg, 4, rows, alphas[ai],
                                               out, 3, nullptr) == LZ_OK);
            for (int r = 0; r < 3; ++r) {
                double sum = 0.0;
                for (int b = 0; b < kBins; ++b) sum += out[r * kBins + b];
                if (r == 1) CHECK(sum == 0.0);
                else CHECK(std::fabs(sum - 1.0) <= 101 * 1.1920929e-7);
            }
        }
        // capacity 0: every member is outside -> zero rows; NULL bases are then allowed
        for (int i = 0; i < 3 * kBins; ++i) out[i] = from_bits(kSentinel);
        CHECK(lz_merge_value_distributions(nullptr, nullptr, kRec, 0, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_OK);
        for (int i = 0; i < 3 * kBins; ++i) CHECK(bits_of(out[i]) == 0u);
        // impossible ranges
        beg[0] = -1;
        CHECK(lz_merge_value_distributions(ring + 348, ring + 352, kRec, capacity, slot, sel, ord, beg, 1, rows, 0.f, out, 3, nullptr) == LZ_OK);
        for (int b = 0; b < kBins; ++b) CHECK(out[2 * kBins + b] == 0.f);
        beg[0] = 0; beg[1] = sel + 1;
        CHECK(lz_merge_value_distributions(ring + 348, ring + 352, kRec, capacity, slot, sel, ord, beg, 1, rows, 0.f, out, 3, nullptr) == LZ_OK);
        for (int b = 0; b < kBins; ++b) CHECK(out[2 * kBins + b] == 0.f);
        beg[1] = 2;

        // ---- nothing to do, refusals
        CHECK(lz_merge_value_distributions(nullptr, nullptr, 4, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0.f, nullptr, 0, nullptr) == LZ_OK);
        CHECK(lz_merge_value_distributions(ring + 348, ring + 352, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f, nullptr, 0, nullptr) == LZ_OK);
        CHECK(lz_merge_value_distributions(ring + 348, ring + 352, kRec, capacity, slot, sel, ord, nullptr, 0, nullptr, 0.f, out, 3, nullptr) == LZ_OK);
        const void* vb = ring + 348; const void* sb = ring + 352;
        CHECK(lz_merge_value_distributions(vb, sb, kRec, -1, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, -1, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, ord, beg, -1, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, -1, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, 3, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, 0, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(nullptr, sb, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, nullptr, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, nullptr, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, ord, nullptr, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, ord, beg, 4, nullptr, 0.f, out, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f, nullptr, 3, nullptr) == LZ_ERR_ARG);
        CHECK(lz_merge_value_distributions(ring + 350, sb, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ALIGN);
        CHECK(lz_merge_value_distributions(vb, sb, 362, capacity, slot, sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ALIGN);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, reinterpret_cast<const int64_t*>(ring + 4), sel, ord, beg, 4, rows, 0.f, out, 3, nullptr) == LZ_ERR_ALIGN);
        CHECK(lz_merge_value_distributions(vb, sb, kRec, capacity, slot, sel, ord, beg, 4, rows, 0.f,
                                           reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out) + 2), 2, nullptr) == LZ_ERR_ALIGN);
    }
    if (failures) { std::printf("value_dist_host_check: %d failures\n", failures); return 1; }
    std::printf("value_dist_host_check: ok\n");
    return 0;
}
