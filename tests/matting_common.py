"""Float64 judges of the human-matting kernels (csrc/matting.hip), in plain torch on the CPU, and the input recipes of their tests.
tests/test_matting_host.py checks the judges themselves: against the values the REFERENCE losses produced
(tests/golden/pfan_mat_r18_tiny.pt), against autograd of the reference formulas, and the pyramid adjoint by a dot-product test."""
import numpy as np
import torch
import torch.nn.functional as F

LO = float(np.float32(1e-4))                 # torch.clamp(pred_fp32, min=1e-4, max=1. - 1e-4) compares in fp32
HI = float(np.float32(1. - 1e-4))
EPS = float(np.float32(1e-12))               # sqrt(diff ** 2 + 1e-12) on fp32 tensors adds the fp32 constant
SMOOTH = 1e-4
LEVELS = 5

PIXEL_CASES = [(1, 1, 1), (2, 7, 9), (3, 33, 70), (1, 128, 160)]
LAP_CASES = [(2, 32, 32), (1, 37, 45), (1, 33, 70), (2, 64, 96), (1, 160, 288)]
LOSS_NAMES = ('GlobalTrimapCELoss', 'GloabelTrimapIouLoss', 'LocalAlphaLoss', 'LocalLaplacianLoss', 'FusionAlphaLoss',
              'FusionLaplacianLoss', 'CompositionLoss')
ARGMAX_FREE = ('GlobalTrimapCELoss', 'GloabelTrimapIouLoss', 'LocalAlphaLoss', 'LocalLaplacianLoss')
TRIMAP_PLANTED = [0., 0.5, 1., 2., 3., 128., 254., 255.]
TRIMAP_PLANTED_CLASS = [0, 0, 1, 2, 1, 1, 1, 2]


def gauss_table():
    """the reference's build_gauss_kernel(size=5, sigma=1.0) in its own numpy calls: the SUM of the two axis Gaussians over the
    grid (not their product), normalised; float32 [5, 5]"""
    size, sigma = 5, 1.0
    grid = np.float32(np.mgrid[0:size, 0:size].T)
    kernel = np.sum(np.exp(-((grid - size // 2) ** 2) / (2 * sigma ** 2)), axis=2)
    kernel /= np.sum(kernel)
    return torch.from_numpy(np.float32(kernel))


def product_gauss_corner():
    g = np.exp(-((np.arange(5) - 2.) ** 2) / 2.)
    return float(g[0] * g[0] / (g.sum() ** 2))


def dyadic_table(seed):
    """four taps of 1/4 (= 16/64) at seeded places of the 5x5 window, no symmetry: with integer d0 every pyramid entry down to the
    sixth is a multiple of 2^-20 below 2 in magnitude, exact in fp32 (a tap costs 2 bits per level, a pooling 2 more)"""
    idx = torch.randperm(25, generator=torch.Generator().manual_seed(seed))[:4]
    k = torch.zeros(25)
    k[idx] = 0.25
    return k.view(5, 5)


# ------------------------------------------------------------------------------------------------ inputs
def trimap_blocks(B, H, W, block, gen):
    """blocks of `block` pixels: 128 on the even diagonals, 0 or 255 elsewhere (no two neighbouring blocks are both outside)"""
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    other = torch.tensor([0., 255.])[torch.randint(0, 2, (B, by, bx), generator=gen)]
    iy, ix = torch.meshgrid(torch.arange(by), torch.arange(bx), indexing='ij')
    t = torch.where(((iy + ix) % 2 == 0)[None], torch.tensor(128.), other)
    return t.repeat_interleave(block, 1).repeat_interleave(block, 2)[:, :H, :W].contiguous()


def pixel_inputs(B, H, W):
    """fp32: global_pred [B, 3, H, W], local_pred [B, 1, H, W], alpha [B, H, W], trimap [B, H, W] (per-pixel 0 / 128 / 255),
    fg, bg, image [B, 3, H, W].  image lies 0.01 to 0.5 away from the composition of local_pred: the composition loss is then
    well conditioned (d sqrt(e^2 + 1e-12) / de is flat away from 0) and the float64 judge arbitrates it."""
    g = torch.Generator().manual_seed(10000 * B + 100 * H + W)
    gp = torch.sigmoid(4. * torch.randn(B, 3, H, W, generator=g))
    local = torch.sigmoid(4. * torch.randn(B, 1, H, W, generator=g))
    alpha = torch.rand(B, H, W, generator=g)
    trimap = torch.tensor([0., 128., 255.])[torch.randint(0, 3, (B, H, W), generator=g)]
    fg, bg = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    ph = torch.clamp(local, min=LO, max=HI)
    delta = (0.01 + 0.49 * torch.rand(B, 3, H, W, generator=g)) * (torch.randint(0, 2, (B, 3, H, W), generator=g) * 2. - 1.)
    image = ph * fg + (1. - ph) * bg + delta
    return dict(global_pred=gp, local_pred=local, alpha=alpha, trimap=trimap, fg=fg, bg=bg, image=image)


def lap_float_inputs(B, H, W, masked):
    """pred [B, 1, H, W] in (0, 1), alpha [B, H, W], trimap (8-pixel blocks) or None"""
    g = torch.Generator().manual_seed(11 + 10000 * B + 100 * H + W + (50000 if masked else 0))
    pred = torch.sigmoid(2. * torch.randn(B, 1, H, W, generator=g))
    alpha = torch.rand(B, H, W, generator=g)
    return pred, alpha, (trimap_blocks(B, H, W, 8, g) if masked else None)


def lap_integer_inputs(B, H, W, masked):
    """pred = 1/2 everywhere, alpha in {-1/2, 1/2, 3/2}: d0 in {1, 0, -1}; trimap per pixel"""
    g = torch.Generator().manual_seed(3 + 10000 * B + 100 * H + W)
    pred = torch.full((B, 1, H, W), 0.5)
    alpha = torch.randint(-1, 2, (B, H, W), generator=g).float() + 0.5
    trimap = torch.tensor([0., 128., 255.])[torch.randint(0, 3, (B, H, W), generator=g)] if masked else None
    return pred, alpha, trimap


def model_inputs(shape):
    """the seeded batch the fixture's model step ran on: image (NHWC memory), alpha, trimap (16-pixel blocks), fg, bg"""
    b, c, h, w = shape
    x = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2)
    g = torch.Generator().manual_seed(2)
    alpha = torch.rand(b, h, w, generator=g) ** 2
    trimap = trimap_blocks(b, h, w, 16, g)
    fg, bg = torch.rand(b, 3, h, w, generator=g), torch.rand(b, 3, h, w, generator=g)
    return x, alpha, trimap, fg, bg


def eval_inputs():
    """two seeded batches of fused predictions [b, 1, 20, 24] and soft masks [b, 20, 24] for the EvalMeter check"""
    g = torch.Generator().manual_seed(7)
    return [(torch.rand(b, 1, 20, 24, generator=g), torch.rand(b, 20, 24, generator=g) ** 2) for b in (3, 2)]


EVAL_THRESH = [0.2, 0.5]
EVAL_SQUARED_BETA = 0.3
EVAL_KEYS = ('precision_list', 'recall_list', 'miou_list', 'f_squared_beta_list', 'f_squared_beta_average', 'f_squared_beta_max',
             'miou_average', 'miou_max', 'precision_average', 'precision_max', 'recall_average', 'recall_max', 'sad', 'mae', 'mse',
             'grad', 'conn', 'sample_num')


# ------------------------------------------------------------------------------------------------ judges
def _inside(p):
    return (p >= torch.tensor(LO)) & (p <= torch.tensor(HI))


def trimap_class(trimap):
    """losses.py:36-40 in the order it rewrites: 0 -> 0, 255 -> 2, then anything > 2 -> 1, then .long()"""
    t = trimap.clone()
    t[t == 0] = 0
    t[t == 255] = 2
    t[t > 2] = 1
    return t.long()


def trimap_stats_judge(gp, trimap, smooth=SMOOTH, g=None):
    """gp fp32 [B, 3, H, W] (any memory format), trimap fp32 [B, H, W] -> stats [B, 2] = (sum bce, sum iou term) in float64 from the
    fp32 inputs as they are, mag [B, 2] the sums of the terms' magnitudes; with g [B, 2] = dL/dstats also dgp and dgp_mag."""
    assert gp.dtype == torch.float32 and trimap.dtype == torch.float32
    B = gp.shape[0]
    inside = _inside(gp)
    ph = torch.clamp(gp.double(), min=LO, max=HI)
    oh = F.one_hot(trimap_class(trimap), 3).permute(0, 3, 1, 2).double()
    bce = -(oh * torch.log(ph) + (1. - oh) * torch.log(1. - ph))
    num = (ph * oh).sum(1) + smooth
    den = ph.sum(1) + oh.sum(1) - (ph * oh).sum(1) + smooth
    iou = 1. - num / den
    out = {'stats': torch.stack([bce.reshape(B, -1).sum(1), iou.reshape(B, -1).sum(1)], dim=1),
           'mag': torch.stack([bce.reshape(B, -1).sum(1), (1. + num / den).reshape(B, -1).sum(1)], dim=1), 'inside': inside}
    if g is not None:
        g = g.double()
        g0, g1 = g[:, 0].view(B, 1, 1, 1), g[:, 1].view(B, 1, 1, 1)
        dbce = torch.where(oh > 0, -1. / ph, 1. / (1. - ph))
        diou = torch.where(oh > 0, (-1. / den)[:, None].expand_as(ph), (num / den ** 2)[:, None].expand_as(ph))
        out['dgp'] = inside * (g0 * dbce + g1 * diou)
        out['dgp_mag'] = g0.abs() * dbce.abs() + g1.abs() * diou.abs()
    return out


def alpha_judge(pred, alpha, trimap=None, g=None):
    """pred fp32 [B, 1, H, W], alpha [B, H, W], trimap [B, H, W] or None -> sums [B, 2] = (sum sqrt(((ph - a) w)^2 + 1e-12), sum w)"""
    B = pred.shape[0]
    p = pred.reshape(B, -1)
    ph = torch.clamp(p.double(), min=LO, max=HI)
    w = torch.ones_like(ph) if trimap is None else (trimap.reshape(B, -1) == 128).double()
    d = (ph - alpha.reshape(B, -1).double()) * w
    q = torch.sqrt(d ** 2 + EPS)
    out = {'sums': torch.stack([q.sum(1), w.sum(1)], dim=1), 'inside': _inside(p)}
    out['mag'] = out['sums'].clone()
    if g is not None:
        g0 = g.double()[:, 0:1]
        out['dp'] = out['inside'] * (g0 * d * w / q)
        out['dp_mag'] = g0.abs() * (d * w / q).abs()
    return out


def composition_judge(pred, fg, bg, image, g=None):
    """pred [B, 1, H, W]; fg, bg, image [B, 3, H, W] -> sums [B] and e (the three residuals); with g [B] also dp and dp_mag"""
    B = pred.shape[0]
    ph = torch.clamp(pred.double(), min=LO, max=HI)
    e = ph * fg.double() + (1. - ph) * bg.double() - image.double()
    q = torch.sqrt(e ** 2 + EPS)
    out = {'sums': q.reshape(B, -1).sum(1), 'e': e, 'inside': _inside(pred)}
    out['mag'] = out['sums'].clone()
    if g is not None:
        g0 = g.double().view(B, 1, 1, 1)
        terms = (e / q) * (fg.double() - bg.double())
        out['dp'] = out['inside'] * (g0 * terms.sum(1, keepdim=True))
        out['dp_mag'] = g0.abs() * terms.abs().sum(1, keepdim=True)
    return out


def fuse_judge(gp, local):
    """-> fused [B, 1, H, W] (the dtype of local), argmax [B, 1, H, W] by torch.max: the first maximum"""
    idx = torch.max(gp, dim=1)[1].unsqueeze(1)
    return local * (idx == 1).to(local.dtype) + (idx == 2).to(local.dtype), idx


def conv_gauss(x, K):
    """x [B, 1, h, w], K [5, 5]: replicate pad 2 and a one-channel F.conv2d, as the reference's conv_gauss"""
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode='replicate'), K.to(x.dtype).view(1, 1, 5, 5))


def conv_gauss_T(g, K):
    """the adjoint of conv_gauss: the transposed convolution onto the padded grid, then the two padding rows / columns of every side
    folded onto the border pixel they replicated"""
    gp = F.conv_transpose2d(g, K.to(g.dtype).view(1, 1, 5, 5))
    gy = gp[:, :, 2:-2].clone()
    gy[:, :, 0] += gp[:, :, 0] + gp[:, :, 1]
    gy[:, :, -1] += gp[:, :, -2] + gp[:, :, -1]
    gx = gy[:, :, :, 2:-2].clone()
    gx[:, :, :, 0] += gy[:, :, :, 0] + gy[:, :, :, 1]
    gx[:, :, :, -1] += gy[:, :, :, -2] + gy[:, :, :, -1]
    return gx


def pool_T(g, h, w):
    """the adjoint of F.avg_pool2d(., 2) on an [h, w] map: a quarter to each source pixel, nothing to a dropped odd row / column"""
    out = torch.zeros(g.shape[0], 1, h, w, dtype=g.dtype)
    up = g.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
    out[:, :, :up.shape[2], :up.shape[3]] = up
    return out


def level_shapes(h, w):
    return [(h >> l, w >> l) for l in range(LEVELS + 1)]


def lap_d0(pred, alpha, trimap):
    ph = torch.clamp(pred.double(), min=LO, max=HI)
    w = torch.ones_like(ph) if trimap is None else (trimap.unsqueeze(1) == 128).double()
    return (ph - alpha.unsqueeze(1).double()) * w, w


def lap_judge(d0, K, gs=None):
    """ONE pyramid of d0 float64 [B, 1, h, w] with the table K: curs (the six maps), es (the five residuals), sums [6, B] =
    sum |e_l| and sum |cur_5|; with gs [6, B] = dL/dsums also g0 = dL/dd0 by the explicit adjoint (sign(0) = 0)."""
    K = K.double()
    cur, curs, es, sums = d0, [d0], [], []
    for _ in range(LEVELS):
        f = conv_gauss(cur, K)
        es.append(cur - f)
        sums.append(es[-1].abs().sum((1, 2, 3)))
        cur = F.avg_pool2d(f, 2)
        curs.append(cur)
    sums.append(cur.abs().sum((1, 2, 3)))
    out = {'curs': curs, 'es': es, 'sums': torch.stack(sums)}
    if gs is not None:
        gs = gs.double()
        g = gs[LEVELS].view(-1, 1, 1, 1) * torch.sign(curs[LEVELS])
        gcurs, gfs = [g], []
        for l in range(LEVELS - 1, -1, -1):
            s = gs[l].view(-1, 1, 1, 1) * torch.sign(es[l])
            gfs.append(pool_T(g, *curs[l].shape[2:]) - s)
            g = s + conv_gauss_T(gfs[-1], K)
            gcurs.append(g)
        out['g0'], out['gcurs'], out['gfs'] = g, gcurs[::-1], gfs[::-1]
    return out


def lap_loss_weights(B, h, w):
    """dL/dsums [6, B] of the loss sum_l mean |pyramid entry l| (F.l1_loss per level, then their sum)"""
    return torch.tensor([[1. / (B * max(hl * wl, 1))] * B for hl, wl in level_shapes(h, w)], dtype=torch.float64)


def lap_loss_judge(pred, alpha, trimap=None, K=None):
    """the Laplacian loss and its gradient towards pred in float64 by the one-pyramid form -> loss, dpred [B, 1, h, w], judge dict"""
    K = gauss_table() if K is None else K
    B, _, h, w = pred.shape
    d0, wgt = lap_d0(pred, alpha, trimap)
    gs = lap_loss_weights(B, h, w)
    j = lap_judge(d0, K, gs)
    return (j['sums'] * gs).sum(), j['g0'] * wgt * _inside(pred), j


def lap_loss_reference_form(pred, alpha, trimap=None, K=None):
    """the reference formula as it is written (two pyramids, then l1_loss of their entries), in the dtype of pred, differentiable"""
    K = (gauss_table() if K is None else K).to(pred.dtype)
    p = torch.clamp(pred, min=1e-4, max=1. - 1e-4) if pred.dtype == torch.float32 else torch.clamp(pred, min=LO, max=HI)
    a = alpha.unsqueeze(1).to(pred.dtype)
    if trimap is not None:
        wgt = (trimap.unsqueeze(1) == 128).to(pred.dtype)
        p, a = p * wgt, a * wgt

    def pyramid(x):
        pyr = []
        for _ in range(LEVELS):
            f = conv_gauss(x, K)
            pyr.append(x - f)
            x = F.avg_pool2d(f, 2)
        return pyr + [x]
    return sum(F.l1_loss(u, v) for u, v in zip(pyramid(a), pyramid(p)))


def seven_losses(global_pred, local_pred, fused_pred, image, alpha, trimap, fg, bg, smooth=SMOOTH):
    """the seven reference losses from the judges, float64 -> {name: value}"""
    B, _, H, W = global_pred.shape
    n = B * H * W
    ts = trimap_stats_judge(global_pred, trimap, smooth)['stats']
    la = alpha_judge(local_pred, alpha, trimap)['sums']
    fa = alpha_judge(fused_pred, alpha)['sums']
    return {
        'GlobalTrimapCELoss': ts[:, 0].sum() / (3 * n), 'GloabelTrimapIouLoss': ts[:, 1].sum() / n,
        'LocalAlphaLoss': la[:, 0].sum() / (la[:, 1].sum() + 1.), 'LocalLaplacianLoss': lap_loss_judge(local_pred, alpha, trimap)[0],
        'FusionAlphaLoss': fa[:, 0].sum() / n, 'FusionLaplacianLoss': lap_loss_judge(fused_pred, alpha)[0],
        'CompositionLoss': composition_judge(fused_pred, fg, bg, image)['sums'].sum() / n,
    }
