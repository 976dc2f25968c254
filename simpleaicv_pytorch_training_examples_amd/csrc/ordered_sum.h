// The ordered two-stage sum every pixel loss takes its totals from ("The ordered sum").  No atomics: the bits of a total
// depend on the problem's shape alone, in every mode.
//   stage 1, per workgroup: each lane adds its elements to +0 in index order (the kernel's own lane stride), wave_sum (common.h)
//            adds the 64 lanes of a wavefront, and the four wavefront sums are added as ((w0 + w1) + w2) + w3 -> one partial row;
//   stage 2, one workgroup per total: lane t adds partial rows t, t + 256, ... to +0, then the same wave_sum and four-way tree.
// What a fold does with its totals (divide by the row count, scale, store through strides) differs from loss to loss and rounds
// differently: it stays in a thin __global__ wrapper next to the kernels it serves.
//
// Preconditions: 256-thread workgroups (four wavefronts), every thread of the workgroup makes the call, and a kernel that makes two
// calls with the same NS puts a barrier between them (they share the LDS staging).
//
// Two traps:
//   - Values that are ALREADY wave-uniform (a row reduced with wave_sum inside the loop, as in pixel_ce_fwd_kernel and
//     pct_wave_fwd_kernel) go to block_fold, never to block_sums: wave_sum would add the 64 copies.
//   - The tree does not start from zero.  `v = 0; v += w[k]` gives the same bits only because no wavefront sum is ever -0 (a lane
//     sum starts at +0, and x + y is -0 only when both are): the SAM statistics kernels relied on that before they came here.
#pragma once
#include "common.h"

// w: this wavefront's NS sums (lane 0's copy counts) -> in thread j < NS the workgroup's sum of column j, 0 in the other threads
template <int NS>
DEVINL float block_tree(const float (&w)[NS]) {
    static_assert(NS >= 1 && NS <= 64, "one thread of the first wavefront per column");
    __shared__ float p[4][NS];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) p[threadIdx.x >> 6][j] = w[j];
    }
    __syncthreads();
    const int j = threadIdx.x;
    return j < NS ? ((p[0][j] + p[1][j]) + p[2][j]) + p[3][j] : 0.f;
}

// wave-uniform (or lane-0) wavefront sums -> dst[0 .. NS)
template <int NS>
DEVINL void block_fold(const float (&w)[NS], float* dst) {
    const float v = block_tree<NS>(w);
    if (threadIdx.x < NS) dst[threadIdx.x] = v;
}

// per-lane sums -> dst[0 .. NS)
template <int NS>
DEVINL void block_sums(float (&s)[NS], float* dst) {
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = wave_sum(s[j]);
    block_fold<NS>(s, dst);
}

// stage 2 over src[n][ld]: -> in thread j < NS the total of column j
template <int NS>
DEVINL float fold_rows(const float* __restrict__ src, int n, int ld) {
    float s[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] += src[(size_t)i * ld + j];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = wave_sum(s[j]);
    return block_tree<NS>(s);
}
