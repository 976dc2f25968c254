"""Float64 judges of the two salient-object-detection kernels (csrc/salient.hip), in plain torch on the CPU, and the input recipes of
their tests.  tests/test_salient_host.py checks the judges themselves: the loss judge against the values the REFERENCE losses
produced (tests/golden/pfan_sal_r18_tiny.pt), the head judge against F.conv2d + sigmoid under autograd."""
import numpy as np
import torch

LO = float(np.float32(1e-4))                 # torch.clamp(pred_fp32, min=1e-4, max=1. - 1e-4) compares in fp32
HI = float(np.float32(1. - 1e-4))
SMOOTH = 1e-4

LOSS_CASES = [(1, 1), (3, 7), (2, 4099), (2, 9100)]          # (B, P): the cases the fixture holds reference loss values for
LOSS_NAMES = ('BCELoss', 'BCEIouloss', 'BCEDiceLoss')


def loss_inputs(B, P):
    """p = sigmoid(6 * randn), label = rand, fp32 [B, P]; the seed is the case itself"""
    g = torch.Generator().manual_seed(1000 * B + P)
    p = torch.sigmoid(6. * torch.randn(B, P, generator=g))
    label = torch.rand(B, P, generator=g)
    return p, label


def stats_judge(p, label, g=None):
    """The four sums per sample in float64 from the fp32 inputs as they are: p-hat = clamp(p, LO, HI) with the fp32 bounds.
    -> dict: stats [B, 4] = (sum bce, sum ph, sum l, sum ph * l); mag [B, 4] = the sums of the terms' magnitudes (every term of
    every sum is non-negative, the two logarithm terms of bce included, so mag == stats); below / inside / above [B, P] bool,
    decided exactly on the fp32 input.  With g [B, 4] = dL/dstats also dp [B, P] and dp_mag, the sum of the magnitudes of dp's
    terms: |g0| (l / ph + (1 - l) / (1 - ph)) + |g1| + |g3| l."""
    assert p.dtype == torch.float32 and label.dtype == torch.float32
    lo32, hi32 = torch.tensor(LO, dtype=torch.float32), torch.tensor(HI, dtype=torch.float32)
    below, above = p < lo32, p > hi32
    inside = (p >= lo32) & (p <= hi32)
    ph = torch.clamp(p.double(), min=LO, max=HI)
    l = label.double()
    bce = -(l * torch.log(ph) + (1. - l) * torch.log(1. - ph))
    stats = torch.stack([bce.sum(1), ph.sum(1), l.sum(1), (ph * l).sum(1)], dim=1)
    out = {'stats': stats, 'mag': stats.clone(), 'below': below, 'inside': inside, 'above': above, 'ph': ph}
    if g is not None:
        g = g.double()
        g0, g1, g3 = g[:, 0:1], g[:, 1:2], g[:, 3:4]
        out['dp'] = inside * (g0 * (-l / ph + (1. - l) / (1. - ph)) + g1 + g3 * l)
        out['dp_mag'] = g0.abs() * (l / ph + (1. - l) / (1. - ph)) + g1.abs() + g3.abs() * l
    return out


# (B, P) of the summation-order test: both lane forms (P % 4 == 0 or not), one and two workgroups per sample, and 257 and 258 workgroup
# partials per sample -- the smallest counts at which the fold's second stride trip has one lane and two lanes at work
ORDER_CASES = [(2, 1), (2, 4099), (2, 4100), (2, 1048583), (1, 1052680)]
ORDER_SPAN = 4096                            # elements of one sample per workgroup (BSS_SPAN of csrc/salient.hip)


def order_inputs(B, P):
    """p, label = torch.rand [B, P] fp32, drawn one after the other from one generator seeded with P"""
    g = torch.Generator().manual_seed(P)
    return torch.rand(B, P, generator=g), torch.rand(B, P, generator=g)


def _lanes_then_tree(rounds):
    """rounds float32 [n, R, 256]: lane t of workgroup n adds rounds[n, 0, t], rounds[n, 1, t], ... to +0 in that order; then the
    wave_sum butterfly of csrc/common.h inside each 64-lane wavefront (partners lane ^ 1, ^ 2, the mirror within 8 lanes = ^ 7, the
    mirror within 16 = ^ 15, ^ 16, ^ 32: fp32 addition commutes, so every lane ends with the same bits), then ((w0 + w1) + w2) + w3.
    -> float32 [n]"""
    assert rounds.dtype == np.float32
    v = np.zeros((rounds.shape[0], 256), dtype=np.float32)
    for r in range(rounds.shape[1]):
        v = v + rounds[:, r]
    lane = np.arange(256)
    for mask in (1, 2, 7, 15, 16, 32):
        v = v + v[:, lane ^ mask]
    w = v[:, ::64]
    out = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    assert out.dtype == np.float32
    return out


def ordered_sum(x, vec):
    """The fp32 sum of x (float32 [P], no element -0) in the order of csrc/ordered_sum.h as binary_seg_stats runs it: a workgroup per
    ORDER_SPAN elements -- vec: lane t takes elements 4 t .. 4 t + 3 of each round of 1024, in order; scalar: lane t takes element
    t of each round of 256 -- then the fold of the workgroup partials with lane stride 256.  An element past the end is +0 here and
    skipped on the GPU: s + 0 == s in bits for every s but -0, and a sum that starts at +0 never becomes -0."""
    x = np.asarray(x, dtype=np.float32)
    nblk = -(-x.size // ORDER_SPAN)
    xp = np.zeros(nblk * ORDER_SPAN, dtype=np.float32)
    xp[:x.size] = x
    if vec:
        rounds = xp.reshape(nblk, 4, 256, 4).transpose(0, 1, 3, 2).reshape(nblk, 16, 256)      # [n, round * 4 + j, lane]
    else:
        rounds = xp.reshape(nblk, 16, 256)
    part = _lanes_then_tree(rounds)
    trips = -(-nblk // 256)
    pp = np.zeros(trips * 256, dtype=np.float32)
    pp[:nblk] = part
    return _lanes_then_tree(pp.reshape(1, trips, 256))[0]


def ordered_stats_emulation(p, label):
    """columns 1 (sum clamp(p)) and 2 (sum label) of binary_seg_stats in its own summation order -> float32 [B, 2].  Both are pure fp32
    additions (the clamp selects, it does not round): the GPU's bits can be predicted exactly."""
    B, P = p.shape
    ph = torch.clamp(p, min=LO, max=HI).numpy()
    assert ph.dtype == np.float32
    vec = P % 4 == 0                         # (the tests' operands are fresh allocations: 16-byte aligned)
    return np.array([[ordered_sum(ph[b], vec), ordered_sum(label[b].numpy(), vec)] for b in range(B)], dtype=np.float32)


def loss_from_stats(stats, P, name, smooth=SMOOTH):
    """the reference formulas of BCELoss / BCEIouloss / BCEDiceLoss on the four sums (any float dtype)"""
    bce, sp, sl, inter = stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3]
    if name == 'BCELoss':
        return bce.sum() / (stats.shape[0] * P)
    if name == 'BCEIouloss':
        return (1. - (inter + smooth) / (sp + sl - inter + smooth)).mean()
    if name == 'BCEDiceLoss':
        return (1. - (2 * inter + smooth) / (sp + sl + smooth)).mean()
    raise KeyError(name)


def head_operands(N, C, H, W, seed, integer, dtype=torch.float32):
    """x [N, C, H, W] over NHWC memory in `dtype`, weight fp32 [1, C, 3, 3], bias fp32 [1], dout fp32 [N, 1, H, W].
    integer: x, w, dout from {-1, 0, 1} and an integer bias -- every sum of the convolution and of its gradients is an integer
    (|z| <= 9 C + 1 = 577, |dw| <= N H W = 12 288 at the largest case), exact in fp32 in any order, and exact in bf16 storage."""
    g = torch.Generator().manual_seed(seed)

    def draw(*s):
        return torch.randint(-1, 2, s, generator=g).float() if integer else torch.randn(*s, generator=g)

    x = draw(N, H, W, C).to(dtype).permute(0, 3, 1, 2)
    w = draw(1, C, 3, 3) if integer else draw(1, C, 3, 3) / (9 * C) ** 0.5
    b = torch.tensor([float(seed % 3 - 1)]) if integer else draw(1)
    dout = draw(N, 1, H, W)
    return x, w, b, dout


def head_judge(x, w, b, dout, sigmoid):
    """The head and its gradients in float64 from the operands as they are, written as nine shifted products (no convolution call):
    z = sum_{r, s, c} x[., c, h + r - 1, w + s - 1] w[c, r, s] + b, out = sigmoid(z) or z; dz = dout * out * (1 - out) or dout;
    dx[., c, h, w] = sum_{r, s} dz[h + 1 - r, w + 1 - s] w[c, r, s]; dw[c, r, s] = sum dz[h, w] x[., c, h + r - 1, w + s - 1]; db = sum dz."""
    x, w, b, dout = x.double(), w.double(), b.double(), dout.double()
    N, C, H, W = x.shape
    xp = torch.zeros(N, C, H + 2, W + 2, dtype=torch.float64)
    xp[:, :, 1:-1, 1:-1] = x
    z = torch.zeros(N, H, W, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            z += torch.einsum('nchw,c->nhw', xp[:, :, r:r + H, s:s + W], w[0, :, r, s])
    z = z + b[0]
    out = torch.sigmoid(z) if sigmoid else z
    dz = dout[:, 0] * (out * (1. - out) if sigmoid else 1.)
    dzp = torch.zeros(N, H + 2, W + 2, dtype=torch.float64)
    dzp[:, 1:-1, 1:-1] = dz
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for r in range(3):
        for s in range(3):
            dx += dzp[:, None, 2 - r:2 - r + H, 2 - s:2 - s + W] * w[0, :, r, s].view(1, C, 1, 1)
            dw[0, :, r, s] = torch.einsum('nhw,nchw->c', dz, xp[:, :, r:r + H, s:s + W])
    return {'out': out[:, None], 'dx': dx, 'dw': dw, 'db': dz.sum().view(1)}


def eval_inputs():
    """two seeded batches of predictions [b, 1, 20, 24] and soft masks [b, 20, 24] for the EvalMeter check"""
    g = torch.Generator().manual_seed(7)
    return [(torch.rand(b, 1, 20, 24, generator=g), torch.rand(b, 20, 24, generator=g) ** 2) for b in (3, 2)]


EVAL_THRESH = [0.2, 0.5]
EVAL_SQUARED_BETA = 0.3
EVAL_KEYS = ('precision_list', 'recall_list', 'miou_list', 'f_squared_beta_list', 'f_squared_beta_average', 'f_squared_beta_max',
             'miou_average', 'miou_max', 'precision_average', 'precision_max', 'recall_average', 'recall_max', 'sample_num')


def model_inputs(shape):
    """the seeded image batch (NHWC memory) and soft mask the fixture's model step ran on"""
    b, c, h, w = shape
    x = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2)
    mask = torch.rand(b, h, w, generator=torch.Generator().manual_seed(2)) ** 2
    return x, mask
