// The gradient dy of the stem's convolution output behind BatchNorm + ReLU + MaxPool2d(3, 2, 1), one pixel chunk at a time: the ONE
// statement of it, shared by the kernel that stores dy (pool.hip, bn_relu_maxpool_bwd_apply_k3s2_kernel) and the one that feeds it
// straight into the weight gradient (stembwd.hip).
#pragma once
#include "common.h"

// Pixel (h, w) = (2a + r, 2b + c) lies in the windows (a + dyq, b + dxq), q = dyq * 2 + dxq: an even row (column) in window a (b) only,
// at tap 1; an odd one in a (tap 2) and a + 1 (tap 0).  -> whether window q covers the pixel, and at which window position.
DEVINL bool k3s2_window(int r, int c, int q, bool wok, int& want) {
    const int dyq = q >> 1, dxq = q & 1;
    const int kh = r == 0 ? 1 : (dyq == 0 ? 2 : 0), kw = c == 0 ? 1 : (dxq == 0 ? 2 : 0);
    want = kh * 3 + kw;
    return !((r == 0 && dyq == 1) || (c == 0 && dxq == 1)) && wok;
}

// d[q] / ib[q]: pooled gradient and recorded positions of the four windows; the covering windows are added ascending in oh, then ow,
// the ReLU gate is scale * y + shift > 0, dy = k0 * (g - mean(g) - xhat * mean(g xhat)) rounded to T by Chunk<T>::pack.
template <typename T>
DEVINL u32x4 k3s2_dy(const float (&yv)[Chunk<T>::N], const float (&d)[4][Chunk<T>::N], const uint8_t (&ib)[4][Chunk<T>::N],
                     const bool (&use)[4], const int (&want)[4], const float (&sc)[Chunk<T>::N], const float (&sh)[Chunk<T>::N],
                     const float (&k0)[Chunk<T>::N], const float (&mg)[Chunk<T>::N], const float (&mu)[Chunk<T>::N],
                     const float (&is)[Chunk<T>::N], const float (&mx)[Chunk<T>::N]) {
    constexpr int N = Chunk<T>::N;
    float g[N], o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!use[q]) continue;
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] += (ib[q][j] == want[q]) ? d[q][j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float gj = fmaf(sc[j], yv[j], sh[j]) > 0.f ? g[j] : 0.f;
        o[j] = k0[j] * (gj - mg[j] - (yv[j] - mu[j]) * is[j] * mx[j]);
    }
    return Chunk<T>::pack(o);
}
