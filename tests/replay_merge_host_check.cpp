// replay_merge_host_check.cpp -- the host build of lz_replay_position_keys / lz_replay_merge_records (csrc/lz_dedup_host.cpp,
// csrc/lz_replay_merge.h) run over the edge cases as a stand-alone program, built by tests/test_replay_merge_cpu.py with
// -fsanitize=address,undefined.  Every buffer is a heap block of exactly the size the ABI states, so a read or a write
// outside a record, a key row or an output record is an error of the address sanitizer; the checks below are the
// properties that need no second implementation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "liuzhou_hip.h"

namespace {

constexpr int kRec = 360;
int failures = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t next() {                                              // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Heap {                                                  // an exact, 8-byte aligned heap block
    void* p;
    explicit Heap(size_t bytes) : p(std::malloc(bytes ? bytes : 1)) {}
    ~Heap() { std::free(p); }
    template <class T> T* as() { return static_cast<T*>(p); }
};

// a record with `legal` legal actions (the lowest ones of a random rotation), junk in every unowned bit when asked
void make(uint8_t* rec, int legal, bool junk, bool zero_policy) {
    uint64_t w[4];
    for (int p = 0; p < 4; ++p) w[p] = next() & ((1ull << 36) - 1);
    w[0] |= (next() % 8) << 36;
    if (junk) { w[0] |= next() << 39; for (int p = 1; p < 4; ++p) w[p] |= next() << 36; }
    std::memcpy(rec, w, 32);
    uint32_t mq[7] = {0, 0, 0, 0, 0, 0, 0};
    const int start = (int)(next() % 220);
    for (int i = 0; i < legal; ++i) { const int a = (start + i * 7) % 220; mq[a >> 5] |= 1u << (a & 31); }
    if (junk) mq[6] |= 0xF0000000u;
    std::memcpy(rec + 32, mq, 28);
    for (int r = 0; r < 72; ++r) {
        float x = zero_policy ? 0.f : (float)(next() % 1000) / 1000.f;
        uint32_t bits;
        std::memcpy(&bits, &x, 4);
        if (junk && r % 9 == 0) bits = r % 2 ? 0x7FC00123u : 0x80000000u;      // NaN payloads and -0.0
        std::memcpy(rec + 60 + 4 * r, &bits, 4);
    }
    const float v[2] = {(float)((int)(next() % 3) - 1), (float)(next() % 1000) / 500.f - 1.f};
    std::memcpy(rec + 348, v, 8);
    const uint32_t pad = junk ? 0xDEADBEEFu : 0u;
    std::memcpy(rec + 356, &pad, 4);
}

int popcount_mask(const uint8_t* rec) {
    uint32_t mq[7];
    std::memcpy(mq, rec + 32, 28);
    mq[6] &= 0x0FFFFFFFu;
    int c = 0;
    for (int k = 0; k < 7; ++k) c += __builtin_popcount(mq[k]);
    return c;
}

void canonical_header(const uint8_t* rec, uint8_t* out) {
    uint64_t w[4];
    std::memcpy(w, rec, 32);
    w[0] &= (1ull << 39) - 1;
    for (int p = 1; p < 4; ++p) w[p] &= (1ull << 36) - 1;
    std::memcpy(out, w, 32);
    uint32_t mq[7];
    std::memcpy(mq, rec + 32, 28);
    mq[6] &= 0x0FFFFFFFu;
    std::memcpy(out + 32, mq, 28);
}

}  // namespace

int main() {
    const int legal_counts[6] = {0, 1, 71, 72, 73, 220};
    const int group_sizes[7] = {1, 2, 3, 255, 256, 257, 600};
    // ---- the ring: for every legal count one position held c times (c = every chunk boundary), the copies identical
    // in header so that they share a key; slot 0 and the last slot are used, so the ends of the block are touched
    std::vector<int> first_of, size_of, legal_of;
    int64_t capacity = 0;
    for (int s = 0; s < 7; ++s) capacity += group_sizes[s];
    capacity += 6;                                             // + a lone junk record per legal count
    Heap ring(capacity * kRec);
    uint8_t* rec = ring.as<uint8_t>();
    int64_t at = 0;
    for (int s = 0; s < 7; ++s) {
        const int legal = legal_counts[s % 6];
        make(rec + at * kRec, legal, true, false);
        for (int i = 1; i < group_sizes[s]; ++i) {
            uint8_t* r = rec + (at + i) * kRec;
            make(r, legal, false, i % 5 == 3);
            std::memcpy(r, rec + at * kRec, 60);               // the same position, junk and all
        }
        first_of.push_back((int)at); size_of.push_back(group_sizes[s]); legal_of.push_back(legal);
        at += group_sizes[s];
    }
    for (int s = 0; s < 6; ++s) {
        make(rec + at * kRec, legal_counts[s], true, false);
        first_of.push_back((int)at); size_of.push_back(1); legal_of.push_back(legal_counts[s]);
        ++at;
    }
    CHECK(at == capacity);

    // ---- keys: every slot once in order, plus slots outside the ring
    const int64_t m = capacity + 4;
    Heap slot_h(m * 8), keys_h(m * 64), sym_h(m), bad_h(4);
    int64_t* slot = slot_h.as<int64_t>();
    for (int64_t j = 0; j < capacity; ++j) slot[j] = j;
    slot[capacity] = -1; slot[capacity + 1] = capacity; slot[capacity + 2] = INT64_MAX; slot[capacity + 3] = INT64_MIN;
    int64_t* keys = keys_h.as<int64_t>();
    int8_t* sym = sym_h.as<int8_t>();
    int32_t* bad = bad_h.as<int32_t>();
    for (int symmetric = 0; symmetric < 2; ++symmetric) {
        *bad = 0;
        CHECK(lz_replay_position_keys(rec, capacity, slot, m, symmetric, keys, sym, bad, nullptr) == LZ_OK);
        CHECK(*bad == 4);
        for (int64_t j = capacity; j < m; ++j) {
            CHECK(keys[j * 8] == (INT64_MIN | j) && sym[j] == 0);
            for (int w = 1; w < 8; ++w) CHECK(keys[j * 8 + w] == 0);
        }
        for (size_t g = 0; g < first_of.size(); ++g)             // the copies of a position share their key and frame
            for (int i = 1; i < size_of[g]; ++i) {
                CHECK(std::memcmp(keys + (first_of[g] + i) * 8, keys + first_of[g] * 8, 64) == 0);
                CHECK(sym[first_of[g] + i] == sym[first_of[g]]);
            }
        for (int64_t j = 0; j < capacity; ++j) CHECK(sym[j] >= 0 && sym[j] < 8 && (symmetric || sym[j] == 0));

        // ---- merge: the groups as laid out, then a singleton per record, then the bad groups
        const int64_t groups = (int64_t)first_of.size() + 5;
        Heap order_h(m * 8), begin_h((groups + 1) * 8), out_h(groups * kRec), count_h(groups * 4), over_h(4);
        int64_t* order = order_h.as<int64_t>();
        int64_t* begin = begin_h.as<int64_t>();
        uint8_t* out = out_h.as<uint8_t>();
        int32_t* count = count_h.as<int32_t>();
        int32_t* over = over_h.as<int32_t>();
        for (int64_t j = 0; j < m; ++j) order[j] = j;
        for (size_t g = 0; g < first_of.size(); ++g) begin[g] = first_of[g];
        const int64_t real = (int64_t)first_of.size();
        begin[real] = capacity;                                // group `real`: the slot -1 alone
        begin[real + 1] = capacity + 1;                        // the slot == capacity alone
        begin[real + 2] = capacity + 2;                        // both far slots
        begin[real + 3] = m;                                   // an empty range
        begin[real + 4] = m;                                   // a range past the end
        begin[real + 5] = m + 3;
        *over = 0;
        std::memset(out, 0xA5, groups * kRec);
        CHECK(lz_replay_merge_records(rec, capacity, slot, m, sym, order, begin, groups, out, count, over, nullptr) == LZ_OK);
        int expect_over = 0;
        for (int64_t g = 0; g < real; ++g) {
            const uint8_t* f = rec + (int64_t)first_of[g] * kRec;
            uint8_t head[60];
            canonical_header(f, head);
            CHECK(count[g] == size_of[g]);
            CHECK(std::memcmp(out + g * kRec, head, 60) == 0);
            const int legal = popcount_mask(f), used = legal < 72 ? legal : 72;
            CHECK(legal == legal_of[g]);
            expect_over += legal > 72;
            for (int r = used; r < 72; ++r) { uint32_t b; std::memcpy(&b, out + g * kRec + 60 + 4 * r, 4); CHECK(b == 0); }
            uint32_t pad;
            std::memcpy(&pad, out + g * kRec + 356, 4);
            CHECK(pad == 0);
            if (size_of[g] == 1) {                             // a bit copy of the legal slots, value and soft
                CHECK(std::memcmp(out + g * kRec + 60, f + 60, 4 * used) == 0);
                CHECK(std::memcmp(out + g * kRec + 348, f + 348, 8) == 0);
            }
        }
        CHECK(*over == expect_over);
        for (int64_t g = real; g < groups; ++g) {
            CHECK(count[g] == 0);
            for (int i = 0; i < kRec; ++i) CHECK(out[g * kRec + i] == 0);
        }
        // a bad sym and a bad order entry inside the last chunk of the 600-member group
        const int64_t big = 6, where = first_of[6] + 555;
        const int8_t keep = sym[where];
        sym[where] = 8;
        CHECK(lz_replay_merge_records(rec, capacity, slot, m, sym, order, begin, groups, out, count, over, nullptr) == LZ_OK);
        CHECK(count[big] == 0 && count[big - 1] == 257);
        sym[where] = keep;
        order[where] = m;
        CHECK(lz_replay_merge_records(rec, capacity, slot, m, sym, order, begin, groups, out, count, over, nullptr) == LZ_OK);
        CHECK(count[big] == 0);
        order[where] = where;
        // members under every frame: whatever sym says, nothing outside the records is read
        for (int64_t j = 0; j < capacity; ++j) sym[j] = (int8_t)(next() % 8);
        CHECK(lz_replay_merge_records(rec, capacity, slot, m, sym, order, begin, groups, out, count, over, nullptr) == LZ_OK);
        CHECK(count[big] == 600);
    }
    // ---- nothing to do, refusals
    CHECK(lz_replay_position_keys(nullptr, 0, nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr) == LZ_OK);
    CHECK(lz_replay_position_keys(rec, capacity, slot, -1, 1, keys, sym, bad, nullptr) == LZ_ERR_ARG);
    CHECK(lz_replay_position_keys(rec, capacity, slot, m, 2, keys, sym, bad, nullptr) == LZ_ERR_ARG);
    CHECK(lz_replay_position_keys(rec, capacity, nullptr, m, 1, keys, sym, bad, nullptr) == LZ_ERR_ARG);
    CHECK(lz_replay_position_keys(rec + 4, capacity - 1, slot, m, 1, keys, sym, bad, nullptr) == LZ_ERR_ALIGN);
    CHECK(lz_replay_merge_records(nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == LZ_OK);
    CHECK(lz_replay_merge_records(rec, capacity, slot, m, sym, nullptr, nullptr, -1, nullptr, nullptr, nullptr, nullptr) == LZ_ERR_ARG);
    CHECK(lz_replay_merge_records(rec, capacity, slot, m, sym, nullptr, nullptr, 2, nullptr, nullptr, nullptr, nullptr) == LZ_ERR_ARG);
    if (failures) { std::printf("replay_merge_host_check: %d failures\n", failures); return 1; }
    std::printf("replay_merge_host_check: ok\n");
    return 0;
}
