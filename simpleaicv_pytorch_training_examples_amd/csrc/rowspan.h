// The row span of the per-pixel class losses (semseg.hip, parsing.hip): a workgroup owns tile_rows consecutive rows of the [rows][C]
// logits = ONE contiguous span, copied into LDS (and, with the gradient, back) in 16-byte chunks.
#pragma once
#include "common.h"

// LDS bytes of a span, a whole number of 16-byte chunks
__host__ __device__ inline size_t span_bytes(int tile_rows, int C, size_t elem) {
    return ((size_t)tile_rows * C * elem + 15) & ~(size_t)15;
}

// global [e0, e0 + n) <-> LDS [0, n): 16-byte chunks, then the (last tile's) scalar tail
template <typename T>
DEVINL void stage_in(const T* __restrict__ g, T* lds, size_t e0, int n) {
    constexpr int EPC = ElemTraits<T>::EPC;
    const int chunks = n / EPC;
    for (int i = threadIdx.x; i < chunks; i += blockDim.x) st_chunk(lds + (size_t)i * EPC, ld_chunk_nt(g + e0 + (size_t)i * EPC));
    for (int i = chunks * EPC + threadIdx.x; i < n; i += blockDim.x) lds[i] = g[e0 + i];
}
template <typename T>
DEVINL void stage_out(T* __restrict__ g, const T* lds, size_t e0, int n) {
    constexpr int EPC = ElemTraits<T>::EPC;
    const int chunks = n / EPC;
    for (int i = threadIdx.x; i < chunks; i += blockDim.x) st_chunk(g + e0 + (size_t)i * EPC, ld_chunk(lds + (size_t)i * EPC));
    for (int i = chunks * EPC + threadIdx.x; i < n; i += blockDim.x) g[e0 + i] = lds[i];
}

// the class a float label names, -1 outside [0, C)
DEVINL int class_label(float lab, int C) { return (lab >= 0.f && lab < (float)C) ? (int)lab : -1; }
