"""Host-side contract of the BN partial-statistics buffers (no GPU): `saicv_conv2d_stat_rows` and `saicv_conv2d_dgrad_stat_rows`
are what the Python wrapper sizes the [2, rows, C] buffers with BEFORE the convolution launch, so they must be pure functions of
the descriptor and agree with the launch: one row per tile row of a 256- or 128-row tile (per parity class of a strided data
gradient), or one row per workgroup of the streaming kernels (csrc/pwstream.hip)."""
import ctypes

import pytest
import torch

from simpleaicv_pytorch_training_examples_amd import ops
from simpleaicv_pytorch_training_examples_amd._lib import lib

# (Cin, Cout, k, stride, H) of ResNet-50 at 224 x 224
SHAPES = [(8, 64, 7, 2, 224), (64, 64, 1, 1, 56), (64, 256, 1, 1, 56), (256, 128, 1, 1, 56), (128, 128, 3, 2, 56),
          (512, 1024, 1, 2, 28), (256, 256, 3, 1, 14), (512, 2048, 1, 1, 7), (512, 512, 3, 1, 7)]


@pytest.mark.parametrize('batch', [2, 256])
@pytest.mark.parametrize('ci,co,k,s,h', SHAPES)
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32])
def test_stat_rows_is_one_row_per_wavefront_row(ci, co, k, s, h, batch, dt):
    d = ops._desc(batch, h, h, ci, co, k, k, s, k // 2, dt)
    L = lib()
    rows = L.saicv_conv2d_stat_rows(ctypes.byref(d))
    m = batch * d.OH * d.OW
    # r06: pointwise stride-1 products of the shapes of csrc/pwstream.hip over >= 65 536 rows run as ONE resident round of the streaming kernel
    # (csrc/pwstream.hip): one row per workgroup, 2 workgroups per CU
    streamed = dt == torch.bfloat16 and k == 1 and s == 1 and m >= 65536 and (ci, co) in {(64, 64), (64, 256)}
    streamed3 = dt == torch.bfloat16 and k == 3 and s == 1 and m >= 65536 and (ci, co) == (64, 64)      # the same stream over nine taps: one workgroup per CU
    if streamed or streamed3:
        assert rows == (512 if streamed else 256), (rows, m)
    else:
        assert rows in {-(-m // 256), -(-m // 128)}, (rows, m)
    assert rows == L.saicv_conv2d_stat_rows(ctypes.byref(d))          # pure function of the descriptor


@pytest.mark.parametrize('batch', [2, 256])
@pytest.mark.parametrize('ci,co,k,s,h', SHAPES)
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32])
def test_dgrad_stat_rows_is_one_row_per_tile_row_and_parity_class(ci, co, k, s, h, batch, dt):
    d = ops._desc(batch, h, h, ci, co, k, k, s, k // 2, dt)
    L = lib()
    rows = L.saicv_conv2d_dgrad_stat_rows(ctypes.byref(d))
    m = batch * h * h                                                  # rows = input pixels
    # the data gradient with BatchNorm-backward sums streams the pointwise products (K = R S Cout, N = Cin) of csrc/pwstream.hip, the
    # K = 256 one included: one row per workgroup, 2 workgroups per CU
    streamed = dt == torch.bfloat16 and k == 1 and s == 1 and m >= 65536 and (ci, co) in {(64, 64), (256, 64), (64, 256), (128, 128), (256, 128)}
    streamed3 = dt == torch.bfloat16 and k == 3 and s == 1 and m >= 65536 and (ci, co) == (64, 64)
    if streamed or streamed3:
        assert rows == (512 if streamed else 256), (rows, m)
    else:
        mt = batch * (-(-h // s)) ** 2                                 # rows of the largest parity class
        assert rows in {-(-mt // 256) * s * s, -(-mt // 128) * s * s}, (rows, mt, s)
    assert rows == L.saicv_conv2d_dgrad_stat_rows(ctypes.byref(d))


def test_conv_fwd_refuses_statistics_with_an_fp32_output():
    """saicv_conv2d_stat_rows sizes the statistics buffer for an output in the data type; the fp32-output launch would pick another
    plan, so it is refused before anything reaches the GPU."""
    d = ops._desc(2, 56, 56, 64, 64, 1, 1, 1, 0, torch.bfloat16)
    L = lib()
    buf = (ctypes.c_float * 4)()
    rc = L.saicv_conv2d_fwd(ctypes.byref(d), None, None, None, None, 1, ctypes.addressof(buf), ctypes.addressof(buf), None)
    assert rc == -1
    assert b'out_f32' in L.saicv_last_error_string()
