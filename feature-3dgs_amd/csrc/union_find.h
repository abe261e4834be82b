// union_find.h - the lock-free union-find of mask_regions.hip (runs of packed masks) and components.hip (points over their
// neighbour lists).  One array of parents, every node its own parent at the start.  A union links the LARGER root to the smaller
// by compare-and-swap: a parent is only ever lowered, a walk to the root visits strictly decreasing indices, and the root of a
// component is its smallest member.  Agent-scope atomics on both sides: other workgroups' links are seen.  Every walk carries a
// cap (the number of nodes) besides, and a walk that reaches it sets bits of the caller's error word.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace f3dgs {

__device__ __forceinline__ int32_t load_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of node i: parents only decrease, so the walk ends; `cap` (the number of nodes) bounds it besides.  Path halving by
// atomicMin keeps "a parent is only lowered".
__device__ __forceinline__ int find_root(int32_t* parent, int i, int cap, int32_t* err) {
    int p = load_agent(parent + i);
    for (int it = 0; p != i; it++) {
        if (it >= cap || p > i) {
            atomicOr(err, 1);
            return -1;
        }
        const int g = load_agent(parent + p);
        if (g != p) atomicMin(parent + i, g);
        i = p;
        p = g;
    }
    return i;
}

__device__ __forceinline__ void unite(int32_t* parent, int a, int b, int cap, int32_t* err) {
    for (int it = 0; it <= cap; it++) {
        a = find_root(parent, a, cap, err);
        b = find_root(parent, b, cap, err);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(parent + a, a, b);                       // the larger root under the smaller
        if (old == a) return;
        a = old;                                                           // another link came first: go on from where it points
    }
    atomicOr(err, 2);
}

}  // namespace f3dgs
