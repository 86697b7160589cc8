// Stand-alone host program over csrc/lz_valid.h and csrc/lz_valid_host.cpp (tests/test_valid_ref_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a child process): reads a case file, calls the host reduction, the
// classification and the arg-maximum rule on it, writes the results.  Every buffer has exactly the documented size, so an
// access past a row or a batch is an error report, not a wrong number.
//
// case file:  i64 batches; per batch: i64 B, i64 has_value, f32 rows[B,12], i32 cls[B,4], f32 value[B] (if has_value),
//             f32 planes[B,396]; then i64 n_arg; per entry: f32 x[220], u8 legal[220]
// result:     f64 acc[18,14], f64 zsum[18]; per batch: i32 phase_bin[B,2]; per arg entry: i32 index
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/liuzhou_hip.h"
#include "../liuzhou_amd/csrc/lz_valid.h"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASES RESULT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    std::vector<double> acc(lzvalid::kGroups * lzvalid::kAccCols, 0.0), zsum(lzvalid::kGroups, 0.0);
    std::vector<std::vector<int32_t>> classes;
    const int64_t batches = take<int64_t>(in, 1)[0];
    for (int64_t b = 0; b < batches; ++b) {
        const std::vector<int64_t> head = take<int64_t>(in, 2);
        const size_t B = (size_t)head[0];
        const std::vector<float> rows = take<float>(in, B * lzvalid::kRowCols);
        const std::vector<int32_t> cls = take<int32_t>(in, B * lzvalid::kClsCols);
        const std::vector<float> value = take<float>(in, head[1] ? B : 0);
        const std::vector<float> planes = take<float>(in, B * lzvalid::kPlaneFloats);
        const int st = lz_valid_reduce(rows.data(), cls.data(), head[1] ? value.data() : nullptr, (int64_t)B, acc.data(),
                                       head[1] ? zsum.data() : nullptr, nullptr);
        if (st != LZ_OK) { fprintf(stderr, "lz_valid_reduce: %d\n", st); return 3; }
        std::vector<int32_t> pb(B * 2, -7);
        if (lz_valid_classify(planes.data(), rows.data() + lzvalid::kVHat, lzvalid::kRowCols, (int64_t)B, pb.data(), nullptr) != LZ_OK)
            return 3;
        classes.push_back(pb);
    }
    fwrite(acc.data(), sizeof(double), acc.size(), out);
    fwrite(zsum.data(), sizeof(double), zsum.size(), out);
    for (const auto& pb : classes) fwrite(pb.data(), sizeof(int32_t), pb.size(), out);
    const int64_t n_arg = take<int64_t>(in, 1)[0];
    for (int64_t k = 0; k < n_arg; ++k) {
        const std::vector<float> x = take<float>(in, 220);
        const std::vector<uint8_t> legal = take<uint8_t>(in, 220);
        const int32_t a = lzvalid::argmax_legal(x.data(), legal.data(), 220);
        fwrite(&a, sizeof(a), 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
