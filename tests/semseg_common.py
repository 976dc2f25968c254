"""Float64 judges of the two semantic-segmentation kernels (csrc/semseg.hip), in plain torch on the CPU, and the input recipes of
their tests.  tests/test_semseg_host.py checks the judges themselves against torch autograd / F.conv2d."""
import math

import torch

LO = 1e-4
HI = 1. - 1e-4
NEAR = 1e-3              # a row is "near a bound" when p_t or 1 - p_t lies within this RELATIVE distance of 1e-4


def pixel_ce_judge(x, label, upstream=1.0):
    """The analytic clamped softmax cross-entropy and its gradient in float64.
    x [rows, C] (any float dtype: taken as it is, upcast), label [rows] float class ids.
    -> dict: loss, grad [rows, C], grad_open (the unclamped gradient (p - onehot) * upstream / rows of every valid row),
       p_t, q = 1 - p_t (summed over the other classes: relative accuracy near 1), valid, lower / inside / upper / near [rows] bool."""
    x = x.detach().double().cpu()
    label = label.detach().double().cpu().reshape(-1)
    rows, C = x.shape
    valid = (label >= 0) & (label < C)
    t = torch.where(valid, label, torch.zeros_like(label)).long()
    lse = torch.logsumexp(x, dim=1)
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p)
    onehot[torch.arange(rows), t] = 1.
    onehot = onehot * valid[:, None]
    p_t = p[torch.arange(rows), t]
    q = (p * (1. - onehot)).sum(dim=1) if C > 1 else torch.zeros(rows, dtype=torch.float64)
    lower = valid & (p_t < LO)
    upper = valid & (q < LO)
    inside = valid & ~lower & ~upper
    row_loss = torch.where(lower, torch.full_like(p_t, -math.log(LO)),
                           torch.where(upper, torch.full_like(p_t, -math.log(HI)), lse - x[torch.arange(rows), t]))
    row_loss = row_loss * valid
    grad_open = (p - onehot) * valid[:, None] * (upstream / rows)
    near = valid & (((p_t - LO).abs() <= NEAR * LO) | ((q - LO).abs() <= NEAR * LO))
    return {'loss': row_loss.sum() / rows, 'grad': grad_open * inside[:, None], 'grad_open': grad_open, 'p_t': p_t, 'q': q,
            'valid': valid, 'lower': lower, 'inside': inside, 'upper': upper, 'near': near}


def pixel_ce_restated(x, label):
    """The reference formula (softmax, clamp, log, one-hot, sum, mean) restated in float64 torch ops under autograd."""
    C = x.shape[1]
    pr = torch.clamp(torch.softmax(x.double(), dim=-1), min=LO, max=HI)
    onehot = torch.nn.functional.one_hot(label.reshape(-1).long(), num_classes=C).double()
    return ((-torch.log(pr)) * onehot).sum(dim=-1).mean()


def pixel_ce_inputs(rows, C, seed, dtype=torch.float32):
    """x = randn * s with s drawn per pixel from {1, 6, 14}; the true class gets a per-pixel boost sized from the row itself so that
    the row lands in the regime r % 3 (0: p_t < 1e-4, 1: inside the clamp, 2: p_t > 1 - 1e-4) with a margin of at least 2 in the
    logit -- far more than a bf16 rounding of these values moves it.  Returned in `dtype` (what the kernel and the judge both read)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.tensor([1., 6., 14.])[torch.randint(0, 3, (rows,), generator=g)]
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * s[:, None].double()
    label = torch.randint(0, C, (rows,), generator=g)
    regime = torch.arange(rows) % 3
    u = torch.rand(rows, generator=g, dtype=torch.float64)
    edge = math.log(1. / LO - 1.)                                    # logit(p_t) at the bounds is -edge / +edge
    delta = torch.where(regime == 0, -edge - 2. - 8. * u, torch.where(regime == 1, -(edge - 2.) + 2. * (edge - 2.) * u, edge + 2. + 8. * u))
    others = x.clone()
    others[torch.arange(rows), label] = -float('inf')
    if C > 1:
        x[torch.arange(rows), label] = torch.logsumexp(others, dim=1) + delta             # logit(p_t) = x_t - lse(others) = delta
    return x.to(dtype), label.float()


def cpfe_restated(x, w_1x1, w_dilated, dilations):
    """The one-GEMM-plus-gather form of the CPFE convolutions in torch ops (any dtype, autograd flows):
    Z = x . W_all^T with W_all = (1x1 weight | per branch its nine taps, tap-major), then every dilated branch sums its nine shifted
    taps; taps outside the image count as zero.  x [N, Cin, H, W] -> [N, (1 + branches) * P, H, W]."""
    N, Cin, H, W = x.shape
    P = w_1x1.shape[0]
    w_all = torch.cat([w_1x1.reshape(P, Cin)] + [w.permute(2, 3, 0, 1).reshape(9 * P, Cin) for w in w_dilated], dim=0)
    z = torch.einsum('nchw,oc->nhwo', x, w_all)
    parts = [z[..., :P]]
    for j, d in enumerate(dilations):
        acc = torch.zeros(N, H, W, P, dtype=x.dtype)
        for t in range(9):
            dy, dx = (t // 3 - 1) * d, (t % 3 - 1) * d
            h0, h1, w0, w1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if h0 >= h1 or w0 >= w1:
                continue
            src = z[..., P + 9 * P * j + P * t:P + 9 * P * j + P * (t + 1)]
            pad = torch.zeros(N, H, W, P, dtype=x.dtype)
            pad[:, h0:h1, w0:w1] = src[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx]
            acc = acc + pad
        parts.append(acc)
    return torch.cat(parts, dim=-1).permute(0, 3, 1, 2)


def cpfe_operands(shape, seed, integer):
    """(N, Cin, H, W, P) -> x, w_1x1, [w_d3, w_d5, w_d7] (fp32 leaves) and an upstream gradient; `integer`: everything from {-1, 0, 1}"""
    N, Cin, H, W, P = shape
    g = torch.Generator().manual_seed(seed)

    def draw(*s):
        return torch.randint(-1, 2, s, generator=g).float() if integer else torch.randn(*s, generator=g)

    x = draw(N, H, W, Cin).permute(0, 3, 1, 2)                        # NHWC memory
    w1 = draw(P, Cin, 1, 1) if integer else draw(P, Cin, 1, 1) / Cin ** 0.5
    wd = [draw(P, Cin, 3, 3) if integer else draw(P, Cin, 3, 3) / (9 * Cin) ** 0.5 for _ in range(3)]
    dout = draw(N, H, W, 4 * P).permute(0, 3, 1, 2)
    return x, w1, wd, dout
