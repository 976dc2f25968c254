"""Bit-exact checks of every implicit-GEMM launch form (csrc/igemm.hip, csrc/pwstream.hip) on integer operands.

The kernels multiply bf16 (or fp32) operands and accumulate in fp32.  With small-integer operands whose sums of absolute
products stay below 2^24, every partial sum is an exactly representable integer in any order, tile split, split-K grouping or
atomic interleaving: an fp32 result must EQUAL the float64 CPU reference bit for bit, a bf16 result its round-to-nearest-even.
Every comparison in this module is `torch.equal`; there is no tolerance.  (The premise -- v_mfma_f32_16x16x32_bf16,
v_mfma_f32_16x16x4_f32 and fp32 atomics add integers below 2^24 exactly -- holds on an MI355X: every case below is equal there.)  A dropped row, a double-counted split boundary, a wrong
border tap, a stale LDS slot, an unwritten tail element all show as an inequality.

One table of cases (CASES), one runner per entry-point family.  The table needs no GPU: tests/test_igemm_plan_host.py imports it,
asks saicv_igemm_plan which kernel form each case launches (closure over the compiled forms) and checks the operand bounds on
the CPU.  Each GPU case asserts its plan (route / tile / 128-byte K slices / splits) and its bounds BEFORE it launches.

Operand regimes:
  narrow  ternary operands, thinned so that every output stays below 256 in magnitude (exact in bf16) and every per-column sum
          of |y|, y^2, |g|, |g| (|y| + |mean|) and every sum_m |dy| |x| stays below 2^24 over the whole M: statistics and weight
          gradients are exact under any grouping.
  wide    operands in {-3..3} x {-2..2}, only where the checked result is the output tensor: outputs pass 256, so the bf16
          store (ties included) is exercised.  Bound: conv(|x|, |w|).max() < 2^24.
No 16-byte chunk of an operand is entirely zero (a dropped chunk always changes the reference); the zero-padded channels of the
stem are the one exception.

Memory discipline: outputs and non-atomic partial rows are pre-filled with NaN; `+=` targets (dw, dbias, atomic rows) with an
integer pattern (expected = pattern + result); every tensor a kernel sees lives inside a larger allocation with NaN guard bands
(0xAA for the bit masks) of at least one 256-row tile before and after it, compared afterwards."""
import ctypes
import os
import zlib
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

BF, FP = torch.bfloat16, torch.float32
LIMIT = float(1 << 24)

# op: 'conv_fwd' | 'conv_dgrad' | 'conv_wgrad' | 'lin_fwd' | 'lin_dgrad' | 'lin_wgrad'
# shape: conv (N, H, W, Cin, Cout, k, stride, pad) | linear (M, K, N)
# flags: rounding (the case is there for the bf16 store: tests/test_igemm_plan_host.py checks that its outputs pass 256 and hold ties),
#        bias, stats (0 none / -1 one row per tile row or workgroup / n > 0 atomic rows), out_f32, addend, gate, bn ('mask' | 'nomask'),
#        part_rows, row_scale (rows per scale), dbias, det (also in deterministic mode; both results must be identical), stem
# expect: fields of saicv_plan this case must get
Case = namedtuple('Case', 'id op shape dt regime density env flags expect')
CASES = []


def _add(id_, op, shape, dt, regime, expect, density=0.5, env=None, **flags):
    CASES.append(Case(f'{id_}-{"bf16" if dt == BF else "fp32"}', op, tuple(shape), dt, regime, density, dict(env or {}), flags, dict(expect)))


TILES = [(256, 256), (256, 128), (128, 128), (128, 64)]
TILED, PW, PW3, TN = 0, 1, 2, 3


def _tile_sweep():
    """Every tile geometry of igemm_nt1_kernel (forced with SAICV_NT_TILE), pointwise and gathered, forward and data gradient, both data
    types: M % bm != 0 with N % bn != 0, M < bm, exactly one full tile."""
    for t, (bm, bn) in enumerate(TILES):
        for dt in (BF, FP):
            if dt == FP and t == 0:
                continue                    # an fp32 256 x 256 output tile does not fit the epilogue LDS: never planned
            env = {'SAICV_NT_TILE': str(t)}
            for k in (1, 3):
                pad = k // 2
                ex = dict(route=TILED, tile=t, plain=int(k == 1), kc8=0)
                small = 40 if k == 1 else 8                   # the GEMM K: 40 (one 64-byte slice + a tail) / 72
                rag, one = (1, 17, 19), ((1, 16, 16) if bm == 256 else (1, 8, 16))
                for tag, (n, h, w), nn in (('ragged', rag, bn + 8), ('below', (1, 5, 7), bn + 8), ('one', one, bn)):
                    pre = f'sweep-t{t}-k{k}-{tag}'
                    # forward: rows = output pixels (stride 1: the same grid), columns = Cout
                    fs = (n, h, w, small, nn, k, 1, pad)
                    _add(pre + '-fwd', 'conv_fwd', fs, dt, 'wide', ex, env=env)
                    _add(pre + '-fwd-stats', 'conv_fwd', fs, dt, 'narrow', ex, env=env, stats=-1)
                    # data gradient: rows = input pixels, columns = Cin, K = k k Cout
                    ds = (n, h, w, nn, small, k, 1, pad)
                    _add(pre + '-dgrad', 'conv_dgrad', ds, dt, 'wide', ex, env=env)
                    if tag == 'ragged' and dt == BF:
                        # K = 2304: a good part of the outputs passes 256, where bf16 keeps even integers only -- every odd sum is a tie
                        deep = 2304 // (k * k)
                        _add(pre + '-fwd-rounding', 'conv_fwd', (n, h, w, deep, nn, k, 1, pad), dt, 'wide', ex, env=env, rounding=1)
                        _add(pre + '-dgrad-rounding', 'conv_dgrad', (n, h, w, nn, deep, k, 1, pad), dt, 'wide', ex, env=env, rounding=1)
                    if tag == 'ragged':
                        _add(pre + '-fwd-atomic64', 'conv_fwd', fs, dt, 'narrow', ex, env=env, stats=64)
                        _add(pre + '-fwd-bias', 'conv_fwd', fs, dt, 'wide', ex, env=env, bias=1)
                        if dt == BF and t > 0:
                            _add(pre + '-fwd-f32out', 'conv_fwd', fs, dt, 'wide', dict(ex, out_f32=1), env=env, out_f32=1)
                        _add(pre + '-dgrad-add', 'conv_dgrad', ds, dt, 'narrow', ex, env=env, addend=1)
                        _add(pre + '-dgrad-fused', 'conv_dgrad', ds, dt, 'narrow', ex, env=env, addend=1, gate=1, bn='mask')
                        _add(pre + '-dgrad-bn-rows3', 'conv_dgrad', ds, dt, 'narrow', ex, env=env, bn='nomask', part_rows=3)


def _special_shapes():
    """Shapes where tile kernels go wrong, on the plan's own choice of tile (pinned here)."""
    t3 = dict(route=TILED, tile=3, kc8=0)
    for dt in (BF, FP):
        # 3 x 3 stride 2 on odd H != W: four parity classes of unequal size in the data gradient
        s = (2, 15, 13, 24, 40, 3, 2, 1)
        _add('s2-odd-fwd-stats', 'conv_fwd', s, dt, 'narrow', t3, stats=-1)
        _add('s2-odd-fwd-atomic1', 'conv_fwd', s, dt, 'narrow', t3, stats=1)
        _add('s2-odd-fwd', 'conv_fwd', s, dt, 'wide', t3, bias=1)
        _add('s2-odd-dgrad', 'conv_dgrad', s, dt, 'wide', t3)
        _add('s2-odd-dgrad-bn', 'conv_dgrad', s, dt, 'narrow', dict(t3, stat_rows=4), addend=1, gate=1, bn='mask')
        _add('s2-odd-dgrad-bn-rows5', 'conv_dgrad', s, dt, 'narrow', t3, bn='nomask', part_rows=5)
        _add('s2-odd-wgrad', 'conv_wgrad', s, dt, 'narrow', dict(route=TN, bm=64, bn=128), det=1)
        # 1 x 1 stride 2, padding 0 (the downsample shortcut): gathered in the data gradient, pointwise in the forward
        s = (3, 9, 7, 40, 72, 1, 2, 0)
        _add('pw-s2-fwd', 'conv_fwd', s, dt, 'wide', dict(t3, plain=1))
        _add('pw-s2-dgrad', 'conv_dgrad', s, dt, 'wide', dict(t3, plain=0))
        _add('pw-s2-dgrad-bn', 'conv_dgrad', s, dt, 'narrow', dict(t3, plain=0), bn='mask')
        _add('pw-s2-wgrad', 'conv_wgrad', s, dt, 'narrow', dict(route=TN, bm=128, bn=64, plain=0), dbias=1, det=1)
        # the 7 x 7 stride 2 padding 3 stem (3 channels padded to 8) with H != W, and on an image smaller than its reach
        for tag, hw in (('stem', (23, 18)), ('stem-tiny', (5, 4))):
            s = (2, hw[0], hw[1], 8, 64, 7, 2, 3)
            _add(tag + '-fwd-stats', 'conv_fwd', s, dt, 'narrow', t3, stats=-1, stem=1)
            _add(tag + '-fwd', 'conv_fwd', s, dt, 'wide', t3, stem=1)
            _add(tag + '-wgrad', 'conv_wgrad', s, dt, 'narrow', dict(route=TN, bm=64, bn=128), stem=1, det=1)
        _add('stem-dgrad', 'conv_dgrad', (2, 23, 18, 8, 64, 7, 2, 3), dt, 'wide', t3)
        # 3 x 3 on a 2 x 2 image, batch 1; padding 0 (the output shrinks)
        _add('tiny-3x3-fwd', 'conv_fwd', (1, 2, 2, 8, 8, 3, 1, 1), dt, 'wide', t3)
        _add('tiny-3x3-dgrad', 'conv_dgrad', (1, 2, 2, 8, 8, 3, 1, 1), dt, 'wide', t3)
        _add('tiny-3x3-wgrad', 'conv_wgrad', (1, 2, 2, 8, 8, 3, 1, 1), dt, 'narrow', dict(route=TN, bm=64, bn=128, total_rt=1, splits=1), det=1)
        _add('pad0-3x3-fwd', 'conv_fwd', (2, 9, 11, 8, 264, 3, 1, 0), dt, 'wide', dict(route=TILED, kc8=0), bias=1)
        _add('pad0-3x3-dgrad', 'conv_dgrad', (2, 9, 11, 8, 264, 3, 1, 0), dt, 'wide', dict(route=TILED, kc8=0))
        _add('pad0-3x3-wgrad', 'conv_wgrad', (2, 9, 11, 8, 264, 3, 1, 0), dt, 'narrow', dict(route=TN, bm=128, bn=128), dbias=1, det=1)
        # K of one 16-byte chunk (8 bf16 / 4 fp32 channels) and a deep K
        one = 8 if dt == BF else 4
        _add('k-one-chunk-fwd', 'conv_fwd', (2, 6, 5, one, 40, 1, 1, 0), dt, 'wide', t3)
        _add('k-one-chunk-dgrad', 'conv_dgrad', (2, 6, 5, 40, one, 1, 1, 0), dt, 'wide', t3)
        _add('k-one-chunk-wgrad', 'conv_wgrad', (2, 6, 5, one, 40, 1, 1, 0), dt, 'narrow', dict(route=TN, bm=64, bn=64), dbias=1, det=1)
        _add('deep-k-fwd', 'conv_fwd', (2, 7, 7, 512, 512, 3, 1, 1), dt, 'wide', dict(route=TILED, kc8=0), density=0.2)
        _add('deep-k-fwd-stats', 'conv_fwd', (2, 7, 7, 512, 512, 3, 1, 1), dt, 'narrow', dict(route=TILED, kc8=0), stats=7, density=0.15)
        _add('deep-k-dgrad', 'conv_dgrad', (2, 7, 7, 512, 512, 3, 1, 1), dt, 'wide', dict(route=TILED, kc8=0))
        _add('deep-k-wgrad', 'conv_wgrad', (2, 7, 7, 512, 512, 3, 1, 1), dt, 'narrow', dict(route=TN, bm=128, bn=128), det=1)
        # linear: K = 72, N without 16-byte rows (element stores), fp32 logits, residual add, drop-path scale per 7 rows
        _add('lin-fwd', 'lin_fwd', (333, 72, 264), dt, 'wide', dict(route=TILED, plain=1), bias=1)
        _add('lin-fwd-n10', 'lin_fwd', (77, 72, 10), dt, 'wide', dict(route=TILED, plain=1), bias=1)
        _add('lin-fwd-n10-f32out', 'lin_fwd', (77, 72, 10), dt, 'wide', dict(route=TILED, plain=1, out_f32=1), bias=1, out_f32=1)
        _add('lin-fwd-add', 'lin_fwd', (333, 72, 264), dt, 'narrow', dict(route=TILED, plain=1), bias=1, addend=1)
        _add('lin-fwd-scale', 'lin_fwd', (333, 72, 264), dt, 'narrow', dict(route=TILED, plain=1), bias=1, addend=1, row_scale=7)
        if dt == BF:
            _add('lin-fwd-add-f32out', 'lin_fwd', (333, 72, 264), dt, 'narrow', dict(route=TILED, plain=1, out_f32=1), bias=1, addend=1, row_scale=7, out_f32=1)
        _add('lin-fwd-scale-only', 'lin_fwd', (333, 72, 264), dt, 'narrow', dict(route=TILED, plain=1), row_scale=1)
        _add('lin-dgrad', 'lin_dgrad', (333, 72, 264), dt, 'wide', dict(route=TILED, plain=1))
        _add('lin-dgrad-add', 'lin_dgrad', (333, 72, 264), dt, 'narrow', dict(route=TILED, plain=1), addend=1)
        _add('lin-wgrad', 'lin_wgrad', (333, 72, 264), dt, 'narrow', dict(route=TN, bm=128, bn=128, plain=1), dbias=1, det=1)
        _add('lin-wgrad-nobias', 'lin_wgrad', (333, 72, 264), dt, 'narrow', dict(route=TN, bm=128, bn=128, plain=1), det=1)


def _kc8():
    """128-byte K slices: SAICV_NT_KC8=1 on both 256-row tiles (forward and data gradient), and the default rule's own boundary
    (N >= 2048, K >= 512, at least 1024 tiles of 256 x 256) with one step below each."""
    for t in (0, 1):
        env = {'SAICV_NT_KC8': '1', 'SAICV_NT_TILE': str(t)}
        ex = dict(route=TILED, tile=t, kc8=1, plain=1)
        _add(f'kc8-t{t}-fwd', 'lin_fwd', (300, 264, 136), BF, 'wide', ex, env=env, bias=1)
        _add(f'kc8-t{t}-fwd-k256', 'lin_fwd', (256, 256, TILES[t][1]), BF, 'wide', ex, env=env)
        _add(f'kc8-t{t}-dgrad', 'lin_dgrad', (300, 136, 264), BF, 'wide', ex, env=env)
        _add(f'kc8-t{t}-conv-fwd-stats', 'conv_fwd', (2, 13, 11, 264, 136, 1, 1, 0), BF, 'narrow', ex, env=env, stats=-1)
        _add(f'kc8-t{t}-conv-dgrad-bn', 'conv_dgrad', (2, 13, 11, 136, 264, 1, 1, 0), BF, 'narrow', ex, env=env, addend=1, gate=1, bn='mask')
        _add(f'kc8-t{t}-k248', 'lin_fwd', (300, 248, 136), BF, 'wide', dict(ex, kc8=0), env=env)          # K < 256: 64-byte slices
    m = 32768                                                                     # 128 x 8 = 1024 tiles of 256 x 256 at N = 2048
    _add('kc8-rule', 'lin_fwd', (m, 512, 2048), BF, 'narrow', dict(route=TILED, tile=0, kc8=1), density=0.2)
    _add('kc8-rule-n2040', 'lin_fwd', (m, 512, 2040), BF, 'narrow', dict(route=TILED, kc8=0), density=0.2)
    _add('kc8-rule-k504', 'lin_fwd', (m, 504, 2048), BF, 'narrow', dict(route=TILED, kc8=0), density=0.2)
    _add('kc8-rule-m-1tile', 'lin_fwd', (m - 256, 512, 2048), BF, 'narrow', dict(route=TILED, kc8=0), density=0.2)
    _add('kc8-rule-dgrad', 'lin_dgrad', (m, 2048, 512), BF, 'narrow', dict(route=TILED, tile=0, kc8=1), density=0.2)


PW_SHAPES = [(64, 64), (64, 256), (256, 64), (128, 128), (128, 512), (128, 256)]         # (K, N) of pwstream.hip's kShapes
PW_CAP = {(64, 64): 512, (64, 256): 512, (256, 64): 512, (128, 128): 512, (128, 512): 256, (128, 256): 512}


def _streams():
    """pw_stream_kernel, every (K, N) form, and the nine-tap form, with SAICV_PW_MIN_ROWS lowered: a row count that is no multiple of
    16 and below one workgroup's share; M = 67 032 = 21 x 56 x 57, where a workgroup loops over several tiles (want > cap)."""
    env = {'SAICV_PW_MIN_ROWS': '1'}
    for kd, nd in PW_SHAPES:
        for tag, (n, h, w) in (('small', (1, 5, 7)), ('m67032', (21, 56, 57))):
            big = tag != 'small'
            ex = dict(route=PW, blocks=PW_CAP[(kd, nd)]) if big else dict(route=PW)
            dens = 0.3 if big else 0.5
            fs, ds = (n, h, w, kd, nd, 1, 1, 0), (n, h, w, nd, kd, 1, 1, 0)       # forward K = Cin; data gradient K = Cout, columns = Cin
            pre = f'pw-{kd}x{nd}-{tag}'
            if kd < 256:                    # K = 256: the plan streams the fused data gradient only
                _add(pre + '-fwd-stats', 'conv_fwd', fs, BF, 'narrow', ex, env=env, stats=-1, density=dens)
                _add(pre + '-fwd', 'conv_fwd', fs, BF, 'wide', ex, env=env)
                _add(pre + '-dgrad', 'conv_dgrad', ds, BF, 'wide', ex, env=env)
            else:
                _add(pre + '-fwd-stats', 'conv_fwd', fs, BF, 'narrow', dict(route=TILED), env=env, stats=-1, density=dens)
                _add(pre + '-dgrad', 'conv_dgrad', ds, BF, 'wide', dict(route=TILED), env=env)
            _add(pre + '-dgrad-gate', 'conv_dgrad', ds, BF, 'narrow', ex, env=env, addend=1, gate=1, density=dens)
            _add(pre + '-dgrad-bn', 'conv_dgrad', ds, BF, 'narrow', ex, env=env, bn='mask', density=dens)
            if big:
                _add(pre + '-dgrad-fused-rows64', 'conv_dgrad', ds, BF, 'narrow', ex, env=env, addend=1, gate=1, bn='nomask', part_rows=64, density=dens)
    _add('pw-64x256-m67032-fwd-atomic1', 'conv_fwd', (21, 56, 57, 64, 256, 1, 1, 0), BF, 'narrow', dict(route=PW), env=env, stats=1, density=0.3)
    _add('pw-64x256-m67032-fwd-atomic7', 'conv_fwd', (21, 56, 57, 64, 256, 1, 1, 0), BF, 'narrow', dict(route=PW), env=env, stats=7, density=0.3)
    _add('pw-64x256-m67032-fwd-atomic64', 'conv_fwd', (21, 56, 57, 64, 256, 1, 1, 0), BF, 'narrow', dict(route=PW), env=env, stats=64, density=0.3)
    # a product of the same shape that must NOT stream: fp32 data, and a bias
    _add('pw-64x64-fp32-stays-tiled', 'conv_fwd', (1, 5, 7, 64, 64, 1, 1, 0), FP, 'narrow', dict(route=TILED), env=env, stats=-1)
    _add('pw-64x64-bias-stays-tiled', 'conv_fwd', (1, 5, 7, 64, 64, 1, 1, 0), BF, 'wide', dict(route=TILED), env=env, bias=1)
    # nine taps: batch 1 with H != W (border taps), several small images (seams between images inside one 16-row tile), many tiles per stream
    for tag, (n, h, w) in (('b1', (1, 5, 7)), ('seams', (3, 9, 7)), ('one-pixel', (5, 1, 1)), ('m67032', (21, 56, 57))):
        big = tag == 'm67032'
        ex = dict(route=PW3, blocks=256) if big else dict(route=PW3)
        dens = 0.25 if big else 0.4
        s = (n, h, w, 64, 64, 3, 1, 1)
        pre = 'pw3-' + tag
        _add(pre + '-fwd-stats', 'conv_fwd', s, BF, 'narrow', ex, env=env, stats=-1, density=dens)
        _add(pre + '-fwd', 'conv_fwd', s, BF, 'wide', ex, env=env)
        _add(pre + '-dgrad', 'conv_dgrad', s, BF, 'wide', ex, env=env)
        _add(pre + '-dgrad-gate', 'conv_dgrad', s, BF, 'narrow', ex, env=env, addend=1, gate=1, density=dens)
        _add(pre + '-dgrad-bn', 'conv_dgrad', s, BF, 'narrow', ex, env=env, addend=1, gate=1, bn='mask', density=dens)
    _add('pw3-m67032-fwd-atomic7', 'conv_fwd', (21, 56, 57, 64, 64, 3, 1, 1), BF, 'narrow', dict(route=PW3), env=env, stats=7, density=0.25)
    _add('pw3-m67032-dgrad-bn-rows64', 'conv_dgrad', (21, 56, 57, 64, 64, 3, 1, 1), BF, 'narrow', dict(route=PW3), env=env, bn='nomask', part_rows=64, density=0.25)


def _weight_gradients():
    """igemm_tn: the five tiles in the LDS-DMA kernel (bf16), the register-staged kernel (bf16 with SAICV_TN_DMA=0, fp32), plain and
    gathered; reduction lengths below one step, one row into a new step with the last split owning one step, SAICV_TN_SLOTS_PCT=85."""
    for dt in (BF, FP):
        step = 64 if dt == BF else 32
        for dma in ((1, 0) if dt == BF else (0,)):
            env = {} if dma else {'SAICV_TN_DMA': '0'}
            tag = 'dma' if dma else 'reg'
            for ba, bb, co, ci in ((64, 64, 40, 64), (64, 128, 64, 72), (128, 64, 72, 40), (128, 128, 136, 264)):
                ex = dict(route=TN, bm=ba, bn=bb, dma=dma)
                pre = f'tn-{tag}-{ba}x{bb}'
                # plain (1 x 1, stride 1) and gathered (1 x 1 stride 2: K = Cin stays inside the tile)
                _add(pre + '-plain', 'conv_wgrad', (2, 9, 7, ci, co, 1, 1, 0), dt, 'narrow', dict(ex, plain=1), env=env, det=1)
                _add(pre + '-gathered', 'conv_wgrad', (2, 9, 7, ci, co, 1, 2, 0), dt, 'narrow', dict(ex, plain=0), env=env, dbias=1, det=1)
                _add(pre + '-below-one-step', 'lin_wgrad', (25, ci, co), dt, 'narrow', dict(ex, plain=1, total_rt=1, splits=1), env=env, dbias=1, det=1)
            # 512 resident slots over one 64 x 64 tile: total_rt = 513 -> 257 splits of 2 steps, the last owns one step of one row
            _add(f'tn-{tag}-last-split-one-row', 'lin_wgrad', (512 * step + 1, 64, 64), dt, 'narrow',
                 dict(route=TN, bm=64, bn=64, dma=dma, total_rt=513, rt_per=2, splits=257), env=env, dbias=1, det=1, density=0.25)
            _add(f'tn-{tag}-3x3-last-split', 'conv_wgrad', (1, 181, 181, 8, 40, 3, 1, 1), dt, 'narrow',
                 dict(route=TN, bm=64, bn=128, dma=dma, plain=0), env=env, det=1, density=0.25)
            _add(f'tn-{tag}-slots85', 'lin_wgrad', (512 * step + 1, 64, 64), dt, 'narrow',
                 dict(route=TN, bm=64, bn=64, dma=dma, splits=(513 + 1) // 2), env=dict(env, SAICV_TN_SLOTS_PCT='85'), dbias=1, det=1, density=0.25)
            # the 256 x 256 tile by its natural rule (>= 48 reduction steps per resident workgroup), plain and gathered
            _add(f'tn-{tag}-256x256-plain', 'lin_wgrad', (768 * step, 1024, 1024), dt, 'narrow',
                 dict(route=TN, bm=256, bn=256, dma=dma, plain=1), env=env, dbias=1, det=1, density=0.2)
            _add(f'tn-{tag}-256x256-gathered', 'conv_wgrad', (24 * step // 64, 64, 57, 256, 256, 3, 1, 1), dt, 'narrow',
                 dict(route=TN, bm=256, bn=256, dma=dma, plain=0), env=env, det=1, density=0.2)


def _baseline_rows():
    """BASELINE-size rows, so that the real split counts and workgroup loops run: three ResNet-50 shapes at batch 256 (one per route)
    and ViT-B fc1 at M = 50 432 tokens."""
    b = 256
    s = (b, 56, 56, 64, 256, 1, 1, 0)
    _add('r50-64to256-fwd-stats', 'conv_fwd', s, BF, 'narrow', dict(route=PW, blocks=512, stat_rows=512), stats=-1, density=0.15)
    _add('r50-64to256-dgrad-bn', 'conv_dgrad', s, BF, 'narrow', dict(route=PW, blocks=512), addend=1, gate=1, bn='mask', density=0.15)
    _add('r50-64to256-wgrad', 'conv_wgrad', s, BF, 'narrow', dict(route=TN, bm=128, bn=64, dma=1, plain=1), det=1, density=0.15)
    s = (b, 56, 56, 64, 64, 3, 1, 1)
    _add('r50-64to64-3x3-fwd-stats', 'conv_fwd', s, BF, 'narrow', dict(route=PW3, blocks=256, stat_rows=256), stats=-1, density=0.1)
    _add('r50-64to64-3x3-dgrad-bn', 'conv_dgrad', s, BF, 'narrow', dict(route=PW3, blocks=256), bn='mask', density=0.1)
    _add('r50-64to64-3x3-wgrad', 'conv_wgrad', s, BF, 'narrow', dict(route=TN, bm=64, bn=128, dma=1, plain=0), det=1, density=0.1)
    s = (b, 14, 14, 1024, 256, 1, 1, 0)
    _add('r50-1024to256-fwd-stats', 'conv_fwd', s, BF, 'narrow', dict(route=TILED, tile=1, kc8=0, stat_rows=196), stats=-1, density=0.1)
    _add('r50-1024to256-dgrad-bn', 'conv_dgrad', s, BF, 'narrow', dict(route=TILED, kc8=0), addend=1, gate=1, bn='mask', density=0.1)
    _add('r50-1024to256-wgrad', 'conv_wgrad', s, BF, 'narrow', dict(route=TN, bm=128, bn=128, dma=1, plain=1), det=1, density=0.1)
    fc1 = (197 * b, 768, 3072)
    _add('vit-fc1-fwd', 'lin_fwd', fc1, BF, 'narrow', dict(route=TILED, tile=0, kc8=1), bias=1, density=0.1)
    _add('vit-fc1-dgrad', 'lin_dgrad', fc1, BF, 'narrow', dict(route=TILED), density=0.1)
    _add('vit-fc1-wgrad', 'lin_wgrad', fc1, BF, 'narrow', dict(route=TN, bm=256, bn=256, dma=1, plain=1), dbias=1, det=1, density=0.1)


_tile_sweep()
_special_shapes()
_kc8()
_streams()
_weight_gradients()
_baseline_rows()
assert len({c.id for c in CASES}) == len(CASES)


# ----------------------------------------------------------------------------------------------------------- plan (no GPU)
def plan_of(case):
    """saicv_igemm_plan for the case, under its switches -> dict of the plan's fields.  Host only."""
    from simpleaicv_pytorch_training_examples_amd import _lib, ops
    q = _lib.PlanQuery()
    f = case.flags
    if case.op.startswith('conv'):
        n, h, w, ci, co, k, s, p = case.shape
        q.conv = ops._desc(n, h, w, ci, co, k, k, s, p, case.dt)
        q.op = {'conv_fwd': _lib.PLAN_CONV_FWD, 'conv_dgrad': _lib.PLAN_CONV_DGRAD, 'conv_wgrad': _lib.PLAN_CONV_WGRAD}[case.op]
    else:
        q.M, q.K, q.N = case.shape
        q.dtype = _lib.dtype_code(case.dt)
        q.op = {'lin_fwd': _lib.PLAN_LINEAR_FWD, 'lin_dgrad': _lib.PLAN_LINEAR_DGRAD, 'lin_wgrad': _lib.PLAN_LINEAR_WGRAD}[case.op]
    q.out_f32, q.bias, q.stats = int(bool(f.get('out_f32'))), int(bool(f.get('bias'))), int(bool(f.get('stats')))
    q.addend, q.row_scale, q.bn_sums = int(bool(f.get('addend'))), int(bool(f.get('row_scale'))), int(bool(f.get('bn')))
    pl = _lib.Plan()
    saved = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    try:
        rc = _lib.lib().saicv_igemm_plan(ctypes.byref(q), ctypes.byref(pl))
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert rc == 0, (case.id, _lib.lib().saicv_last_error_string())
    return {n: getattr(pl, n) for n, _ in pl._fields_}


def assert_plan(case):
    pl = plan_of(case)
    for k, v in case.expect.items():
        assert pl[k] == v, (case.id, k, pl[k], v, pl)
    if pl['route'] == TN:
        assert (pl['splits'] - 1) * pl['rt_per'] < pl['total_rt'], (case.id, pl)
    return pl


# ------------------------------------------------------------------------------------------------ operands and reference (CPU)
def _gen(case, salt):
    return torch.Generator().manual_seed(zlib.crc32(f'{case.id}/{salt}'.encode()))


def _ints(case, salt, shape, lo, hi, density=1.0, chunked=True, zero_from=None):
    """Integers in [lo, hi] (thinned to `density` non-zeros) as float64, innermost dimension = the 16-byte-chunk axis: no chunk is
    entirely zero.  zero_from: channels from this index on are zero (the stem's padding), which lifts that condition for them."""
    g = _gen(case, salt)
    t = torch.randint(lo, hi + 1, shape, generator=g).double()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density)
    epc = 8 if case.dt == BF else 4
    if zero_from is not None:
        t[..., zero_from:] = 0
    if chunked and shape[-1] % epc == 0:
        c = t.reshape(-1, epc)
        dead = (c == 0).all(1)
        if zero_from is not None:            # chunks that lie wholly in the padding stay zero
            dead &= (torch.arange(c.shape[0]) % (shape[-1] // epc)) * epc < zero_from
        rows = dead.nonzero().squeeze(1)
        sign = torch.randint(0, 2, (len(rows),), generator=g).double() * 2 - 1
        pos = torch.randint(0, epc if zero_from is None else min(epc, zero_from), (len(rows),), generator=g)
        c[rows, pos] = sign
        t = c.reshape(shape)
    return t


def no_zero_chunk(t, dt, zero_from=None):
    epc = 8 if dt == BF else 4
    if t.shape[-1] % epc:
        return bool((t != 0).any(-1).all())           # rows without whole chunks (N = 10): no row entirely zero
    alive = (t.reshape(-1, t.shape[-1] // epc, epc) != 0).any(-1)
    if zero_from is not None:
        alive = alive[:, :(zero_from + epc - 1) // epc]
    return bool(alive.all())


def _bits(case, salt, rows, cols):
    """Random one-bit-per-element mask [rows][cols] (bool) and its packed form: one byte per 16-byte chunk, bit e = element e."""
    epc = 8 if case.dt == BF else 4
    m = torch.rand((rows, cols), generator=_gen(case, salt)) < 0.6
    w = (1 << torch.arange(epc)).to(torch.int64)
    packed = (m.reshape(rows, cols // epc, epc).to(torch.int64) * w).sum(-1).to(torch.uint8)
    return m, packed


Problem = namedtuple('Problem', 'inputs expected bounds exact')        # exact: the output before it is stored, float64


def _dot_bound(a, rows):
    """An upper bound of every sum of absolute products between elements of `a` and one row of `rows` [n][len]:
    max |a| * max_n sum |rows[n]| >= conv(|x|, |w|).max() (and the same for the transposed products)."""
    return float(a.abs().max()) * float(rows.abs().sum(1).max())


def make_problem(case):
    """Operands (CPU float64 / uint8, in the kernels' layouts), expected results and the magnitudes the exactness argument needs.
    inputs / expected: dicts of tensors.  bounds: [(name, value, limit)], all must hold (value < limit)."""
    f, narrow = case.flags, case.regime == 'narrow'
    lo_x, lo_w = (1, 1) if narrow else (3, 2)
    dens = case.density if narrow else 1.0
    stem = 3 if f.get('stem') else None
    bounds, inp, exp = [], {}, {}
    if case.op.startswith('conv'):
        n, h, w, ci, co, k, s, p = case.shape
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        wt = _ints(case, 'w', (co, k, k, ci), -lo_w, lo_w, dens, zero_from=stem)           # [Cout][R][S][Cin]
        w_nchw = wt.permute(0, 3, 1, 2).contiguous()
        if case.op == 'conv_fwd':
            x = _ints(case, 'x', (n, h, w, ci), -lo_x, lo_x, dens, zero_from=stem)
            inp.update(x=x, wf=wt)
            y = F.conv2d(x.permute(0, 3, 1, 2), w_nchw, None, s, p).permute(0, 2, 3, 1).contiguous()
            bounds.append(('sum |x||w|', _dot_bound(x, wt.reshape(co, -1)), LIMIT))
            assert no_zero_chunk(x, case.dt, stem) and no_zero_chunk(wt, case.dt, stem), case.id
            rows, cols = n * oh * ow, co
        elif case.op == 'conv_dgrad':
            dy = _ints(case, 'dy', (n, oh, ow, co), -lo_x, lo_x, dens)
            wd = _ints(case, 'wd', (ci, k, k, co), -lo_w, lo_w, dens)                       # [Cin][R][S][Cout]: its chunks run along Cout
            w_nchw = wd.permute(3, 0, 1, 2).contiguous()
            inp.update(dy=dy, wd=wd)
            y = F.conv_transpose2d(dy.permute(0, 3, 1, 2), w_nchw, None, s, p,
                                   output_padding=(h - ((oh - 1) * s - 2 * p + k), w - ((ow - 1) * s - 2 * p + k))).permute(0, 2, 3, 1).contiguous()
            bounds.append(('sum |dy||w|', _dot_bound(dy, wd.reshape(ci, -1)), LIMIT))
            assert no_zero_chunk(dy, case.dt) and no_zero_chunk(wd, case.dt), case.id
            rows, cols = n * h * w, ci
        else:
            x = _ints(case, 'x', (n, h, w, ci), -lo_x, lo_x, dens, zero_from=stem)
            dy = _ints(case, 'dy', (n, oh, ow, co), -lo_x, lo_x, dens)
            inp.update(x=x, dy=dy)
            assert no_zero_chunk(x, case.dt, stem) and no_zero_chunk(dy, case.dt), case.id
            cols_x = F.unfold(x.permute(0, 3, 1, 2), k, 1, p, s)                            # [N][Cin k k][OH OW]
            a = cols_x.transpose(1, 2).reshape(n * oh * ow, ci, k, k).permute(0, 2, 3, 1).reshape(n * oh * ow, k * k * ci)
            d2 = dy.reshape(n * oh * ow, co)
            dw = (d2.t() @ a).reshape(co, k, k, ci)
            bounds.append(('sum |dy||x| + |pattern|', _dot_bound(x, d2.t()) + 3, LIMIT))
            _wgrad_outputs(case, inp, exp, bounds, dw, d2)
            return Problem(inp, exp, bounds, None)
    else:
        m, kk, nn = case.shape
        wt = _ints(case, 'w', (nn, kk), -lo_w, lo_w, dens)                                  # [N][K]
        if case.op == 'lin_fwd':
            x = _ints(case, 'x', (m, kk), -lo_x, lo_x, dens)
            inp.update(x=x, wf=wt)
            y = x @ wt.t()
            bounds.append(('sum |x||w|', _dot_bound(x, wt), LIMIT))
            assert no_zero_chunk(x, case.dt) and no_zero_chunk(wt, case.dt), case.id
            rows, cols = m, nn
        elif case.op == 'lin_dgrad':
            dy = _ints(case, 'dy', (m, nn), -lo_x, lo_x, dens)
            wd = _ints(case, 'wd', (kk, nn), -lo_w, lo_w, dens)                             # [K][N]: its chunks run along N
            wt = wd.t()
            inp.update(dy=dy, wd=wd)
            y = dy @ wt
            bounds.append(('sum |dy||w|', _dot_bound(dy, wd), LIMIT))
            assert no_zero_chunk(dy, case.dt) and no_zero_chunk(wd, case.dt), case.id
            rows, cols = m, kk
        else:
            x = _ints(case, 'x', (m, kk), -lo_x, lo_x, dens)
            dy = _ints(case, 'dy', (m, nn), -lo_x, lo_x, dens)
            inp.update(x=x, dy=dy)
            assert no_zero_chunk(x, case.dt) and no_zero_chunk(dy, case.dt), case.id
            bounds.append(('sum |dy||x| + |pattern|', _dot_bound(x, dy.t()) + 3, LIMIT))
            _wgrad_outputs(case, inp, exp, bounds, dy.t() @ x, dy)
            return Problem(inp, exp, bounds, None)

    # ---- epilogue of a forward / data-gradient product: y [rows][cols] in float64, exact integers
    y = y.reshape(rows, cols)
    store = (lambda t: t.float()) if (case.dt == FP or f.get('out_f32')) else (lambda t: t.to(BF))
    if narrow:
        bounds.append(('max |acc| (exact in bf16)', float(y.abs().max()), 256.0))
    if f.get('bias'):
        b = _ints(case, 'bias', (cols,), -5, 5, chunked=False)
        inp['bias'] = b
        y = y + b
        bounds.append(('max |acc + bias|', float(y.abs().max()), 256.0 if narrow else LIMIT))
    if f.get('row_scale'):
        rps = f['row_scale']
        sc = 2.0 ** torch.randint(0, 3, ((rows + rps - 1) // rps,), generator=_gen(case, 'scale')).double()      # 1, 2, 4
        inp['row_scale'] = sc
        y = y * sc.repeat_interleave(rps)[:rows, None]
    big = rows > 200000          # BASELINE-size rows: smaller side operands keep the column sums over the whole M below 2^24
    if f.get('addend'):
        a = _ints(case, 'addend', (rows, cols), *((-1, 1, 0.3) if big else (-9, 9)), chunked=False)
        inp['addend'] = a
        if f.get('gate'):
            gm, inp['gate'] = _bits(case, 'gate', rows, cols)
            a = a * gm
        y = y + a
    if narrow:
        bounds.append(('max |out| (exact in bf16)', float(y.abs().max()), 256.0))
    exp['out'] = store(y)
    if f.get('stats'):
        bounds.append(('sum |y|', float(y.abs().sum(0).max()) + 3 * 64, LIMIT))
        bounds.append(('sum y^2', float((y * y).sum(0).max()) + 3 * 64, LIMIT))
        exp['stat_sum'], exp['stat_sq'] = y.sum(0), (y * y).sum(0)
    if f.get('bn'):
        by = _ints(case, 'bn_y', (rows, cols), *((-1, 1, 0.5) if big else (-4, 4)), chunked=False)
        mean = _ints(case, 'bn_mean', (cols,), *((-1, 1) if big else (-3, 3)), chunked=False)
        invstd = 2.0 ** torch.randint(-2, 1 if big else 3, (cols,), generator=_gen(case, 'invstd')).double()
        inp.update(bn_y=by, bn_mean=mean, bn_invstd=invstd)
        g = y
        if f['bn'] == 'mask':
            mm, inp['bn_mask'] = _bits(case, 'bn_mask', rows, cols)
            g = y * mm
        bounds.append(('sum |g|', float(g.abs().sum(0).max()) + 3 * 64, LIMIT))
        bounds.append(('sum |g| (|y| + |mean|) invstd', float(((g.abs() * (by.abs() + mean.abs())).sum(0) * invstd.clamp_min(1.0)).max()) + 3 * 64, LIMIT))
        exp['part_g'], exp['part_gx'] = g.sum(0), (g * (by - mean) * invstd).sum(0)
    return Problem(inp, exp, bounds, y)


def _wgrad_outputs(case, inp, exp, bounds, dw, dy2):
    """`+=` contract: dw / dbias start from an integer pattern."""
    pat = ((torch.arange(dw.numel()) % 7) - 3).double().reshape(dw.shape)
    inp['dw0'] = pat
    exp['dw'] = (pat + dw).float()
    if case.flags.get('dbias'):
        pb = ((torch.arange(dy2.shape[1]) % 5) - 2).double()
        inp['db0'] = pb
        exp['dbias'] = (pb + dy2.sum(0)).float()
        bounds.append(('sum |dy| + |pattern|', float(dy2.abs().sum(0).max()) + 2, LIMIT))


# ------------------------------------------------------------------------------------------------------------- device side
class Guarded:
    """A tensor inside a larger device allocation with guard bands on both sides (NaN; 0xAA for uint8)."""

    def __init__(self, shape, dtype, row_len, fill=None, src=None):
        n = 1
        for s in shape:
            n *= s
        self.guard = max(4096, 256 * row_len)
        self.guard = (self.guard + 63) // 64 * 64
        self.fillv = 0xAA if dtype == torch.uint8 else float('nan')
        self.buf = torch.full((self.guard + n + self.guard + 64,), self.fillv, dtype=dtype, device='cuda')
        self.t = self.buf[self.guard:self.guard + n].view(shape)
        if src is not None:
            self.t.copy_(src.to(dtype))
        elif fill is not None:
            self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        lo, hi = self.buf[:self.guard], self.buf[self.guard + self.t.numel():]
        if self.buf.dtype == torch.uint8:
            return bool((lo == 0xAA).all()) and bool((hi == 0xAA).all())
        return bool(lo.isnan().all()) and bool(hi.isnan().all())


def _run(case, monkeypatch):
    from simpleaicv_pytorch_training_examples_amd import _lib, ops
    from simpleaicv_pytorch_training_examples_amd._lib import check, lib
    L, st = lib(), _lib.stream()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    pl = assert_plan(case)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    try:
        prob = make_problem(case)
    finally:
        torch.set_num_threads(threads)
    for name, value, limit in prob.bounds:                    # the exactness argument, asserted before anything is launched
        assert value < limit, (case.id, name, value, limit)
    f, dt, inp, exp = case.flags, case.dt, prob.inputs, prob.expected
    code = _lib.dtype_code(dt)
    conv = case.op.startswith('conv')
    if conv:
        n, h, w, ci, co, k, s, p = case.shape
        d = ops._desc(n, h, w, ci, co, k, k, s, p, dt)
        dref = ctypes.byref(d)
    dev, outs = {}, {}

    def up(name, dtype=None, row_len=None):
        t = inp[name]
        dev[name] = Guarded(tuple(t.shape), dtype or dt, row_len or t.shape[-1], src=t)
        return dev[name].ptr()

    def out(name, shape, dtype, fill=float('nan'), src=None):
        outs[name] = Guarded(tuple(shape), dtype, shape[-1], fill=fill, src=src)
        return outs[name].ptr()

    results = []
    modes = (0, 1) if f.get('det') else (0,)
    prev = L.saicv_get_deterministic()
    try:
        for det in modes:
            L.saicv_set_deterministic(det)
            dev.clear()
            outs.clear()
            got = {}
            if case.op in ('conv_fwd', 'lin_fwd'):
                rows, cols = tuple(exp['out'].shape)
                odt = FP if (dt == FP or f.get('out_f32')) else BF
                px, pw_ = up('x'), up('wf')
                pb = up('bias', FP) if f.get('bias') else 0
                py = out('out', (rows, cols), odt)
                if conv:
                    nst = f.get('stats', 0)
                    if nst:
                        srows = L.saicv_conv2d_stat_rows(dref) if nst < 0 else nst
                        assert nst > 0 or srows == pl['stat_rows'], (case.id, srows, pl)
                        pat = ((torch.arange(srows * cols) % 5) - 2).double().reshape(srows, cols) if nst > 0 else None
                        ps1 = out('stat_sum', (srows, cols), FP, src=pat)
                        ps2 = out('stat_sq', (srows, cols), FP, src=pat)
                        if nst > 0:
                            check(L.saicv_conv2d_fwd_stats(dref, px, pw_, py, ps1, ps2, srows, st), case.id)
                        else:
                            check(L.saicv_conv2d_fwd(dref, px, pw_, 0, py, 0, ps1, ps2, st), case.id)
                    else:
                        check(L.saicv_conv2d_fwd(dref, px, pw_, pb, py, int(bool(f.get('out_f32'))), 0, 0, st), case.id)
                else:
                    m, kk, nn = case.shape
                    pa = up('addend', odt) if f.get('addend') else 0
                    psc = up('row_scale', FP) if f.get('row_scale') else 0
                    check(L.saicv_linear_fwd(code, px, pw_, pb, py, m, kk, nn, int(bool(f.get('out_f32'))), pa, psc, f.get('row_scale') or 1, st), case.id)
                torch.cuda.synchronize()
                got['out'] = outs['out'].t.cpu()
                if conv and f.get('stats'):
                    base = pat.sum(0) if pat is not None else 0
                    got['stat_sum'] = outs['stat_sum'].t.double().cpu().sum(0) - base
                    got['stat_sq'] = outs['stat_sq'].t.double().cpu().sum(0) - base
            elif case.op in ('conv_dgrad', 'lin_dgrad'):
                rows, cols = tuple(exp['out'].shape)
                pdy, pwd = up('dy'), up('wd')
                pdx = out('out', (rows, cols), dt)
                pa = up('addend') if f.get('addend') else 0
                if not conv:
                    m, kk, nn = case.shape
                    check(L.saicv_linear_dgrad(code, pdy, pwd, pdx, m, kk, nn, pa, st), case.id)
                elif f.get('gate') or f.get('bn'):
                    fu = _lib.DgradFuse()
                    fu.addend = pa
                    fu.addend_gate = up('gate', torch.uint8) if f.get('gate') else 0
                    if f.get('bn'):
                        prow = f.get('part_rows', 0)
                        srows = prow or L.saicv_conv2d_dgrad_stat_rows(dref)
                        assert prow or srows == pl['stat_rows'], (case.id, srows, pl)
                        pat = ((torch.arange(srows * cols) % 5) - 2).double().reshape(srows, cols) if prow else None
                        fu.bn_y = up('bn_y')
                        fu.bn_mask = up('bn_mask', torch.uint8) if f['bn'] == 'mask' else 0
                        fu.bn_mean, fu.bn_invstd = up('bn_mean', FP), up('bn_invstd', FP)
                        fu.part_g = out('part_g', (srows, cols), FP, src=pat)
                        fu.part_gx = out('part_gx', (srows, cols), FP, src=pat)
                        fu.part_rows = prow
                    check(L.saicv_conv2d_dgrad_fused(dref, pdy, pwd, ctypes.byref(fu), pdx, st), case.id)
                elif f.get('addend'):
                    check(L.saicv_conv2d_dgrad_add(dref, pdy, pwd, pa, pdx, st), case.id)
                else:
                    check(L.saicv_conv2d_dgrad(dref, pdy, pwd, pdx, st), case.id)
                torch.cuda.synchronize()
                got['out'] = outs['out'].t.cpu()
                if f.get('bn'):
                    base = pat.sum(0) if pat is not None else 0
                    got['part_g'] = outs['part_g'].t.double().cpu().sum(0) - base
                    got['part_gx'] = outs['part_gx'].t.double().cpu().sum(0) - base
            else:
                pdy, px = up('dy'), up('x')
                pdw = out('dw', tuple(exp['dw'].shape), FP, src=inp['dw0'])
                pdb = out('dbias', tuple(exp['dbias'].shape), FP, src=inp['db0']) if f.get('dbias') else 0
                if conv and f.get('dbias'):
                    check(L.saicv_conv2d_wgrad_bias(dref, pdy, px, pdw, pdb, st), case.id)
                elif conv:
                    check(L.saicv_conv2d_wgrad(dref, pdy, px, pdw, st), case.id)
                else:
                    m, kk, nn = case.shape
                    check(L.saicv_linear_wgrad(code, pdy, px, pdw, pdb, m, kk, nn, st), case.id)
                torch.cuda.synchronize()
                got['dw'] = outs['dw'].t.cpu()
                if f.get('dbias'):
                    got['dbias'] = outs['dbias'].t.cpu()
            for name, g in {**dev, **outs}.items():
                assert g.guards_intact(), (case.id, 'guard band of ' + name, 'deterministic' if det else 'atomic')
            results.append(got)
    finally:
        L.saicv_set_deterministic(prev)
    for det, got in zip(modes, results):
        assert set(got) == set(exp), (case.id, sorted(got), sorted(exp))
        for name, e in exp.items():
            g = got[name]
            e = e.reshape(g.shape)
            if g.dtype == torch.float64:
                e = e.double()
            assert g.dtype == e.dtype, (case.id, name, g.dtype, e.dtype)
            if not torch.equal(g, e):
                bad = (g != e) | g.isnan()
                idx = bad.nonzero()[0].tolist()
                raise AssertionError(f'{case.id} [{"deterministic" if det else "atomic"}] {name}: {int(bad.sum())} of {bad.numel()} differ, first at '
                                     f'{idx}: got {g[tuple(idx)].item()} expected {e[tuple(idx)].item()}; plan {pl}')
    if len(results) == 2:                    # both reduction modes are exact, so they must agree bit for bit
        for name in results[0]:
            assert torch.equal(results[0][name], results[1][name]), (case.id, name)


def _cases(*ops_):
    return [pytest.param(c, id=c.id) for c in CASES if c.op in ops_]


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', _cases('conv_fwd'))
def test_conv_forward_equals_the_integer_reference(case, monkeypatch):
    """saicv_conv2d_fwd (plain, + bias, + partial statistics, fp32 output) and saicv_conv2d_fwd_stats (atomic rows)."""
    _run(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', _cases('conv_dgrad'))
def test_conv_data_gradient_equals_the_integer_reference(case, monkeypatch):
    """saicv_conv2d_dgrad, _dgrad_add and _dgrad_fused (gated addend; BatchNorm-backward sums with and without mask, in partial rows and in atomic rows)."""
    _run(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', _cases('conv_wgrad'))
def test_conv_weight_gradient_equals_the_integer_reference(case, monkeypatch):
    """saicv_conv2d_wgrad and _wgrad_bias on top of a non-zero dw / dbias, with fp32 atomics and in deterministic mode."""
    _run(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', _cases('lin_fwd', 'lin_dgrad'))
def test_linear_forward_and_data_gradient_equal_the_integer_reference(case, monkeypatch):
    """saicv_linear_fwd (bias, addend, power-of-two row scales over groups of rows, fp32 output) and saicv_linear_dgrad (+ addend)."""
    _run(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', _cases('lin_wgrad'))
def test_linear_weight_gradient_equals_the_integer_reference(case, monkeypatch):
    """saicv_linear_wgrad (+ dbias) on top of a non-zero dw / dbias, with fp32 atomics and in deterministic mode."""
    _run(case, monkeypatch)
