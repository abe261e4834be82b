// group_sums.h - group_stats.hip's accumulation for a caller inside the library (codebook.hip: the centroid update of k-means):
// per id the mass sum w, the member count and the feature sums sum w f, every sum in fp64 - the same kernels, the same runs of
// equal ids aggregated in registers and one atomic per run and channel, with the position moments switched off (no xyz: a row is a
// member iff 0 <= id < G and 0 < w < inf).  The sums stay in `scratch` (group_feature_sums_bytes(G, C) bytes, 8-byte aligned,
// cleared by a launch of the call); two launches, none of them reads back.
#pragma once

#include "common.h"

namespace f3dgs {

struct GroupSums {
    const double* mass;        // G
    const double* feat;        // G x C
    const uint32_t* count;     // G
};

size_t group_feature_sums_bytes(int G, int C);
GroupSums launch_group_feature_sums(int P, int G, int C, const int32_t* groups, const float* weight /* or nullptr */,
                                    const float* features, int64_t stride, void* scratch, hipStream_t st);

}  // namespace f3dgs
