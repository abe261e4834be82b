// leaf_walk.h - the two tests every walk over knn.hip's Morton-sorted leaves makes, shared by neighbors.hip (the K nearest
// neighbours) and outliers.hip (the fixed-radius count): which points take part at all, and how near a leaf's box comes to a query.
// Both units are built with -ffp-contract=off: the bound is MONOTONE with a candidate's distance only when it is formed from the
// same uncontracted operations - subtraction, squaring and addition are each monotone, so the bound of a box never exceeds the
// computed distance of a point inside it.
#pragma once

#include <math.h>

#include "common.h"

namespace f3dgs {

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;      // false for a NaN
}

// the squared distance from (x, y, z) to the box: the operations of a candidate's distance, on the nearest face
__device__ __forceinline__ float box_bound(const KnnBox& b, float x, float y, float z) {
    const float dx = fmaxf(fmaxf(b.lo[0] - x, x - b.hi[0]), 0.f);
    const float dy = fmaxf(fmaxf(b.lo[1] - y, y - b.hi[1]), 0.f);
    const float dz = fmaxf(fmaxf(b.lo[2] - z, z - b.hi[2]), 0.f);
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

}  // namespace f3dgs
