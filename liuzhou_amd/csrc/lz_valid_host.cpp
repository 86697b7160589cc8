// lz_valid_host.cpp -- host (CPU-array) build of the reduction and the classification of the validation metrics
// (include/liuzhou_hip.h), part of libliuzhou_host.so: the arithmetic of csrc/lz_valid.h as plain loops, with the
// association of lz_valid.hip.  The row metrics themselves (expf / logf on the device) have no host twin.  `stream` is
// ignored.
#include <cstdint>

#include "lz_valid.h"
#include "lz_soa.h"

using namespace lzvalid;

extern "C" {

int lz_valid_reduce(const float* rows, const int32_t* cls, const float* value, int64_t batch, double* acc, double* zsum,
                    void*) {
    if (batch < 0 || (value == nullptr) != (zsum == nullptr)) return LZ_ERR_ARG;
    if (batch == 0) return LZ_OK;
    if (!rows || !cls || !acc) return LZ_ERR_ARG;
    for (int g = 0; g < kGroups; ++g) {
        double part[kSumCols][kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            double p[kSumCols] = {0.0};
            lane_partial(g, lane, rows, cls, value, batch, p);
            for (int c = 0; c < kSumCols; ++c) part[c][lane] = p[c];
        }
        for (int c = 0; c < kSumCols; ++c) butterfly64(part[c]);
        for (int c = 0; c < kAccCols; ++c) acc[g * kAccCols + c] = acc[g * kAccCols + c] + part[c][0];
        if (value) zsum[g] = zsum[g] + part[kAccCols][0];
    }
    return LZ_OK;
}

int lz_valid_classify(const float* planes, const float* v_hat, int64_t v_hat_stride, int64_t batch, int32_t* phase_bin,
                      void*) {
    if (batch < 0 || v_hat_stride < 1) return LZ_ERR_ARG;
    if (batch == 0) return LZ_OK;
    if (!planes || !v_hat || !phase_bin) return LZ_ERR_ARG;
    for (int64_t i = 0; i < batch; ++i) {
        phase_bin[i * 2 + 0] = phase_of_planes(planes + i * kPlaneFloats);
        phase_bin[i * 2 + 1] = calib_bin(v_hat[i * v_hat_stride]);
    }
    return LZ_OK;
}

}  // extern "C"
