"""Judge and yardsticks of the LSTM tests (tests/test_lstm_host.py on the CPU, tests/test_gpu_lstm_kernels.py on the GPU).

Judge: a hand-written float64 recursion of one bidirectional LSTM layer (zero initial state, gate order i, f, g, o, both biases)
with analytic backward; it never calls nn.LSTM.  For an upstream gradient dy it returns y, dx and the eight parameter gradients.

fp32 yardstick: the reference's own module, torch.nn.LSTM in fp32 on the CPU, on the same inputs; its error against the judge, per
tensor.  bf16 yardstick: the same recursion in fp32 on bf16-rounded inputs and weights with the operands of every matrix product
(x, W, h_{t-1}, dgates_t) rounded to bf16 and y and dx rounded to bf16 on output; its error against the judge on the same rounded
inputs.

Bound for every kernel output:  |kernel - judge|_max <= 4 x yardstick error + floor, the floor being one fp32 ulp of the judge
tensor's largest magnitude, plus half a bf16 ulp of it in bf16.  4 x is the project's standing margin (CTC and pixel-loss tests):
room for another summation order and the device's exp."""
import math

import numpy as np
import torch

NAMES = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0',
         'weight_ih_l0_reverse', 'weight_hh_l0_reverse', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse')
MARGIN = 4.0


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def make_case(b, t, i, h, seed=0, scale=1.0, bf16=False, dy_kind='dense'):
    """x [B, T, I], the eight weights with nn.LSTM's own initialisation range (uniform +- 1 / sqrt(H)) times `scale`, dy [B, T, 2H];
    float32 tensors on the CPU, bf16-representable when bf16."""
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / math.sqrt(h)
    x = torch.randn(b, t, i, generator=g)
    w = {}
    for n in NAMES:
        shape = (4 * h, i) if 'weight_ih' in n else (4 * h, h) if 'weight_hh' in n else (4 * h,)
        w[n] = (torch.rand(shape, generator=g) * 2 - 1) * k * scale
    dy = torch.randn(b, t, 2 * h, generator=g)
    if dy_kind == 'first_frame':
        dy[:, 1:] = 0
    elif dy_kind == 'last_frame':
        dy[:, :-1] = 0
    elif dy_kind == 'forward_half':
        dy[:, :, h:] = 0
    elif dy_kind == 'reverse_half':
        dy[:, :, :h] = 0
    else:
        assert dy_kind == 'dense', dy_kind
    if bf16:
        x, dy = bf16_round(x), bf16_round(dy)
        w = {n: bf16_round(v) for n, v in w.items()}
    return x, w, dy


def recursion(x, w, dy, dtype=torch.float64, rnd=None):
    """The layer by hand in `dtype`; rnd (None = identity) is applied to the operands of every matrix product and to y and dx on
    output.  -> dict(y, dx, <the eight names>)."""
    rnd = rnd or (lambda v: v)
    x, dy = x.to(dtype), dy.to(dtype)
    w = {n: v.to(dtype) for n, v in w.items()}
    b, t, _ = x.shape
    h = w['weight_hh_l0'].shape[1]
    xr = rnd(x)
    y = torch.zeros(b, t, 2 * h, dtype=dtype)
    dx = torch.zeros_like(x)
    out = {}
    for d, sfx in enumerate(('', '_reverse')):
        wih, whh = rnd(w['weight_ih_l0' + sfx]), rnd(w['weight_hh_l0' + sfx])
        bias = w['bias_ih_l0' + sfx] + w['bias_hh_l0' + sfx]
        order = list(range(t)) if d == 0 else list(range(t - 1, -1, -1))
        hs = torch.zeros(b, h, dtype=dtype)
        cs = torch.zeros(b, h, dtype=dtype)
        saved = {}
        for s in order:
            a = xr[:, s] @ wih.T + bias + hs @ whh.T
            gi, gf, gg, go = torch.sigmoid(a[:, :h]), torch.sigmoid(a[:, h:2 * h]), torch.tanh(a[:, 2 * h:3 * h]), torch.sigmoid(a[:, 3 * h:])
            cn = gf * cs + gi * gg
            hn = rnd(go * torch.tanh(cn))                    # what is stored is what is fed back
            saved[s] = (gi, gf, gg, go, cs, cn, hs)
            y[:, s, d * h:(d + 1) * h] = hn
            hs, cs = hn, cn
        dh = torch.zeros(b, h, dtype=dtype)
        dc = torch.zeros(b, h, dtype=dtype)
        dwih, dwhh, db = torch.zeros_like(wih), torch.zeros_like(whh), torch.zeros_like(bias)
        for s in reversed(order):
            gi, gf, gg, go, cp, cn, hp = saved[s]
            dht = dy[:, s, d * h:(d + 1) * h] + dh
            tc = torch.tanh(cn)
            dct = dc + dht * go * (1 - tc * tc)
            da = rnd(torch.cat([dct * gg * gi * (1 - gi), dct * cp * gf * (1 - gf), dct * gi * (1 - gg * gg), dht * tc * go * (1 - go)], 1))
            dwih += da.T @ xr[:, s]
            dwhh += da.T @ hp
            db += da.sum(0)
            dx[:, s] += da @ wih
            dh = da @ whh
            dc = dct * gf
        out['weight_ih_l0' + sfx], out['weight_hh_l0' + sfx] = dwih, dwhh
        out['bias_ih_l0' + sfx], out['bias_hh_l0' + sfx] = db, db.clone()
    out['y'], out['dx'] = y, rnd(dx)
    return out


def judge(x, w, dy):
    return recursion(x, w, dy, torch.float64)


def module_run(x, w, dy, dtype=torch.float32):
    """torch.nn.LSTM on the CPU in `dtype` with the weights loaded, forward and autograd backward -> the same dict"""
    h = w['weight_hh_l0'].shape[1]
    rnn = torch.nn.LSTM(x.shape[2], h, bidirectional=True, batch_first=True).to(dtype)
    with torch.no_grad():
        for n, p in rnn.named_parameters():
            p.copy_(w[n].to(dtype))
    xin = x.to(dtype).clone().requires_grad_(True)
    y = rnn(xin)[0]
    y.backward(dy.to(dtype))
    out = {n: p.grad.detach() for n, p in rnn.named_parameters()}
    out['y'], out['dx'] = y.detach(), xin.grad.detach()
    return out


def errors(got, ref):
    return {k: float((got[k].double() - ref[k].double()).abs().max()) for k in ref}


def yardstick(x, w, dy, bf16):
    """(judge outputs, yardstick error per tensor) for the case"""
    ref = judge(x, w, dy)
    run = recursion(x, w, dy, torch.float32, bf16_round) if bf16 else module_run(x, w, dy, torch.float32)
    return ref, errors(run, ref)


def floor_of(ref_tensor, bf16):
    m = float(ref_tensor.abs().max())
    if m == 0.0:
        return 0.0
    e = math.floor(math.log2(m))
    return 2.0 ** (e - 23) + (2.0 ** (e - 8) if bf16 else 0.0)


def bounds(ref, yard, bf16):
    return {k: MARGIN * yard[k] + floor_of(ref[k], bf16) for k in ref}


def as_numpy(d):
    return {k: np.asarray(v.detach().double().cpu()) for k, v in d.items()}
