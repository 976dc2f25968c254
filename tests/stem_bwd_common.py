"""Inputs and launches shared by test_gpu_stem_pool_keep.py and test_gpu_stem_bwd_stream.py: a pooled stem block (64 channels, pool
(3, 2, 1)) over a convolution output of (n, h, w) pixels, built once per shape and left unchanged.

y is off-centre (per-channel means up to +-6 against a spread of ~1), the statistics are y's own, channel NEG is negative everywhere
behind the BatchNorm (beta = -50: the ReLU gate is closed at every recorded maximum), channel TIE is constant (every window ties:
position of the first tap inside the image)."""
import ctypes
import functools

import torch

C, CQ, TAPS, POOL = 64, 16, 4, (3, 2, 1)
NEG, TIE = 5, 9
EPS = 1e-5


def L():
    from simpleaicv_pytorch_training_examples_amd import _lib
    return _lib, _lib.lib(), _lib.stream()


@functools.lru_cache(maxsize=None)
def case(n, h, w):
    """-> dict of CUDA tensors: y, x (space-to-depth image), dout, gamma, mean, invstd, scale, shift; sizes ph, pw"""
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w)
    off = torch.linspace(-6, 6, C)[torch.randperm(C, generator=g)]
    y = (torch.randn(n, h, w, C, generator=g) * torch.empty(C).uniform_(0.5, 2.0, generator=g) + off).bfloat16()
    y[..., TIE] = 1.25
    yf = y.double().view(-1, C)
    mean = yf.mean(0)
    invstd = 1.0 / torch.sqrt(yf.var(0, unbiased=False) + EPS)
    gamma = torch.empty(C).uniform_(0.5, 1.5, generator=g)
    beta = torch.randn(C, generator=g) * 0.3
    beta[NEG] = -50.0
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * gamma.double() * invstd).float()
    ph, pw = (h + 1) // 2, (w + 1) // 2
    dout = torch.randn(n, ph, pw, C, generator=g).bfloat16()
    x = torch.randn(n, h + TAPS - 1, w + TAPS - 1, CQ, generator=g).bfloat16()
    t = dict(y=y, x=x, dout=dout, gamma=gamma, mean=mean.float(), invstd=invstd.float(), scale=scale, shift=shift)
    t = {k: v.cuda().contiguous() for k, v in t.items()}
    t.update(n=n, h=h, w=w, ph=ph, pw=pw)
    return t


def forward(t, keep):
    """saicv_bn_relu_maxpool_fwd (keep = False) or _fwd_keep -> (out, idx, ya or None)"""
    _lib, lib, st = L()
    ptr = _lib.ptr
    n, h, w, ph, pw = t['n'], t['h'], t['w'], t['ph'], t['pw']
    out = torch.full((n, ph, pw, C), float('nan'), dtype=torch.bfloat16, device='cuda')
    idx = torch.full((n, ph, pw, C), 255, dtype=torch.uint8, device='cuda')
    if keep:
        ya = torch.full((n, ph, pw, C), float('nan'), dtype=torch.bfloat16, device='cuda')
        _lib.check(lib.saicv_bn_relu_maxpool_fwd_keep(0, ptr(t['y']), ptr(t['scale']), ptr(t['shift']), ptr(out), ptr(idx), ptr(ya), n, h, w, C,
                                                      ph, pw, *POOL, st), 'fwd_keep')
    else:
        ya = None
        _lib.check(lib.saicv_bn_relu_maxpool_fwd(0, ptr(t['y']), ptr(t['scale']), ptr(t['shift']), ptr(out), ptr(idx), n, h, w, C, ph, pw,
                                                 *POOL, st), 'fwd')
    torch.cuda.synchronize()
    return out, idx, ya


def backward_two_kernels(t, idx, dgamma, dbeta, accumulate):
    """saicv_bn_relu_maxpool_bwd -> (dy, sums): the sums are what its first pass left in the workspace"""
    _lib, lib, st = L()
    ptr = _lib.ptr
    n, h, w, ph, pw = t['n'], t['h'], t['w'], t['ph'], t['pw']
    dy = torch.full((n, h, w, C), float('nan'), dtype=torch.bfloat16, device='cuda')
    ws = torch.full((lib.saicv_bn_relu_maxpool_bwd_ws_floats(C),), float('nan'), device='cuda')
    _lib.check(lib.saicv_bn_relu_maxpool_bwd(0, ptr(t['dout']), ptr(idx), ptr(t['y']), ptr(t['gamma']), ptr(t['mean']), ptr(t['invstd']),
                                             ptr(t['scale']), ptr(t['shift']), ptr(dy), ptr(dgamma), ptr(dbeta), accumulate, ptr(ws), n, h, w,
                                             C, ph, pw, *POOL, st), 'bwd')
    torch.cuda.synchronize()
    return dy, ws[:2 * C].clone()


def wgrad_two_kernels(t, dy, dw):
    """saicv_conv2d_wgrad of the space-to-depth stem: dw += dy^T x"""
    from simpleaicv_pytorch_training_examples_amd import ops
    _lib, lib, st = L()
    d = ops._desc(t['n'], t['h'] + TAPS - 1, t['w'] + TAPS - 1, CQ, C, TAPS, TAPS, 1, 0, torch.bfloat16)
    _lib.check(lib.saicv_conv2d_wgrad(ctypes.byref(d), _lib.ptr(dy), _lib.ptr(t['x']), _lib.ptr(dw), st), 'wgrad')
    torch.cuda.synchronize()


def stream(t, idx, sums, dw, dgamma, dbeta, accumulate, co=C):
    """saicv_stem_bwd_stream -> its return code"""
    _lib, lib, st = L()
    ptr = _lib.ptr
    n, h, w = t['n'], t['h'], t['w']
    ws = torch.full((lib.saicv_stem_bwd_stream_ws_floats(n, h, w),), float('nan'), device='cuda')
    rc = lib.saicv_stem_bwd_stream(0, ptr(t['dout']), ptr(idx), ptr(t['y']), ptr(t['gamma']), ptr(t['mean']), ptr(t['invstd']), ptr(t['scale']),
                                   ptr(t['shift']), ptr(sums), ptr(t['x']), ptr(dw), ptr(dgamma), ptr(dbeta), accumulate, ptr(ws), n, h, w, co,
                                   CQ, TAPS, TAPS, *POOL, st)
    torch.cuda.synchronize()
    return rc


def ulp32(v):
    """one fp32 unit in the last place of |v|"""
    import math
    return 2.0 ** (math.floor(math.log2(max(abs(float(v)), 1e-37))) - 23)
