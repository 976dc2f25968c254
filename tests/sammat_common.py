"""Float64 judges of the grouped matting kernels and of the SAM matting losses (csrc/matting.hip, interactive_segmentation/
losses_matting.py), built from the judges of tests/matting_common.py: each is applied per (b, m) with the targets of sample b.
tests/test_sammat_host.py pins the composed judges to values recorded from the reference's own classes
(tests/golden/sam_matting_tiny.pt) and asserts that the arg-min of every case used on the GPU is decided.

Inputs are seeded recipes.  Predictions are built FROM the targets: local and fused lie 0.018 .. 0.4 away from alpha (0.06 .. 0.4
times a per-(b, m) scale of 0.3 .. 1), fg and bg differ by at least 0.35 in every channel and the image is the exact composition of
alpha, so every residual under a sqrt(e^2 + 1e-12) stays at least 5e-3 away from its kink, after a rounding of the predictions to
bf16 too (kink_distance measures it; the host test asserts it); the clamp bounds, one ulp inside and one ulp outside them are
planted in every prediction map."""
import numpy as np
import torch

import matting_common as M

K = 8
STATS_CASES = [(1, 1, 1, 1), (2, 3, 7, 9), (3, 4, 33, 70), (1, 4, 128, 160)]
LAP_CASES = [(2, 4, 32, 32), (1, 3, 37, 45), (2, 2, 64, 96)]
LOSS_CASES = [(2, 4, 64, 96), (3, 1, 32, 32)]
MODEL_CASES = {'all': [0, 1, 2, 3], 'subset': [1, 3]}
LOSS_KEYS = ('global_pred_trimap_ce_loss', 'global_pred_trimap_iou_loss', 'local_pred_alpha_loss', 'local_pred_laplacian_loss',
             'fusion_pred_alpha_loss', 'fusion_pred_laplacian_loss', 'composition_loss', 'iou_predict_loss')
THR = 0.5
KINK = 5e-3


def planted_values():
    lo, hi = np.float32(M.LO), np.float32(M.HI)
    return torch.tensor([lo, hi, np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)), np.nextafter(lo, np.float32(0)),
                         np.nextafter(hi, np.float32(1))], dtype=torch.float32)


def group_inputs(B, Mk, H, W, seed=0):
    """fp32: global_preds [B, M, 3, H, W], local_preds, fused_preds [B, M, 1, H, W], iou_preds [B, M], alpha [B, 1, H, W],
    trimap [B, H, W], image, fg, bg [B, 3, H, W].  scale[b, m] in 0.3 .. 1 separates the masks' losses."""
    g = torch.Generator().manual_seed(977 * seed + 100000 * B + 10000 * Mk + 100 * H + W)
    alpha = 0.1 + 0.8 * torch.rand(B, 1, H, W, generator=g)
    trimap = torch.tensor([0., 128., 255.])[torch.randint(0, 3, (B, H, W), generator=g)]
    fg = torch.rand(B, 3, H, W, generator=g)
    bg = fg + (0.35 + 0.4 * torch.rand(B, 3, H, W, generator=g)) * (torch.randint(0, 2, (B, 3, H, W), generator=g) * 2. - 1.)
    image = alpha * fg + (1. - alpha) * bg
    scale = (0.3 + 0.7 * torch.rand(B, Mk, generator=g)).view(B, Mk, 1, 1, 1)

    def near_alpha():
        mag = (0.06 + 0.34 * torch.rand(B, Mk, 1, H, W, generator=g)) * scale           # 0.018 .. 0.4
        sign = torch.randint(0, 2, (B, Mk, 1, H, W), generator=g) * 2. - 1.
        a = alpha.unsqueeze(1)
        sign = torch.where(a + mag > 0.99, torch.tensor(-1.), sign)
        sign = torch.where(a - mag < 0.01, torch.tensor(1.), sign)
        return a + sign * mag

    local, fused = near_alpha(), near_alpha()
    cls = M.trimap_class(trimap)
    onehot = torch.nn.functional.one_hot(cls, 3).permute(0, 3, 1, 2).float().unsqueeze(1)           # [B, 1, 3, H, W]
    gp = torch.sigmoid(4. * torch.randn(B, Mk, 3, H, W, generator=g) + (2. * onehot - 1.) * 3. * (1. - scale))
    if H * W >= 16:
        pv = planted_values()
        gflat, lflat, fflat = gp.view(B, Mk, 3, -1), local.view(B, Mk, -1), fused.view(B, Mk, -1)
        for i in range(6):
            gflat[:, :, i % 3, i] = pv[i]
            lflat[:, :, i] = pv[i]
            fflat[:, :, 6 + i] = pv[i]
        trimap.view(B, -1)[:, 0:6] = 128.                    # the planted local values carry weight
        gflat[:, :, :, 12] = 0.5
    if B >= 2:
        trimap[0][trimap[0] == 128] = 255.                   # a sample with no 128 pixel: sum w = 0
    iou = torch.rand(B, Mk, generator=g)
    return dict(global_preds=gp, local_preds=local, fused_preds=fused, iou_preds=iou, alpha=alpha, trimap=trimap, image=image,
                fg=fg, bg=bg)


def as_dtype(d, dtype):
    """the predictions rounded to dtype and back: what a bf16 test hands to the kernel, as fp32 for the judge"""
    out = dict(d)
    for k in ('global_preds', 'local_preds', 'fused_preds'):
        out[k] = d[k].to(dtype).float()
    return out


def kink_distance(d):
    """the smallest |residual| under a sqrt(e^2 + 1e-12) whose weight is not zero, over every mask"""
    a = d['alpha'].unsqueeze(1).double()
    lp = torch.clamp(d['local_preds'].double(), min=M.LO, max=M.HI)
    fp = torch.clamp(d['fused_preds'].double(), min=M.LO, max=M.HI)
    w = (d['trimap'] == 128).view(a.shape[0], 1, 1, *d['trimap'].shape[1:])
    e_local = (lp - a).abs()[w.expand_as(lp)]
    comp = fp * d['fg'].unsqueeze(1).double() + (1. - fp) * d['bg'].unsqueeze(1).double() - d['image'].unsqueeze(1).double()
    parts = [(fp - a).abs().min(), comp.abs().min()]
    if e_local.numel():
        parts.append(e_local.min())
    return float(torch.stack(parts).min())


def group_judge(d, thr=THR, g=None):
    """-> stats, mag [B, M, 8] float64; with g [B, M, 8] = dL/dstats also dgp / dlp / dfp, their magnitudes and inside masks"""
    gp, lp, fp = d['global_preds'], d['local_preds'], d['fused_preds']
    B, Mk = gp.shape[:2]
    alpha = d['alpha'][:, 0]
    stats, mag = torch.zeros(B, Mk, K, dtype=torch.float64), torch.zeros(B, Mk, K, dtype=torch.float64)
    out = {k: [] for k in ('dgp', 'dgp_mag', 'dlp', 'dlp_mag', 'dfp', 'dfp_mag', 'gp_inside', 'lp_inside', 'fp_inside')}
    for m in range(Mk):
        gm = None if g is None else g[:, m].double()
        ts = M.trimap_stats_judge(gp[:, m].contiguous(), d['trimap'], M.SMOOTH, None if gm is None else gm[:, 0:2])
        la = M.alpha_judge(lp[:, m], alpha, d['trimap'], None if gm is None else gm[:, 2:4])
        fa = M.alpha_judge(fp[:, m], alpha, None, None if gm is None else gm[:, 4:5])
        co = M.composition_judge(fp[:, m], d['fg'], d['bg'], d['image'], None if gm is None else gm[:, 5])
        pb = torch.clamp(fp[:, m], min=M.LO, max=M.HI).reshape(B, -1) > thr
        ab = alpha.reshape(B, -1) > thr
        counts = torch.stack([(pb & ab).sum(1), (pb | ab).sum(1)], dim=1).double()
        stats[:, m] = torch.cat([ts['stats'], la['sums'], fa['sums'][:, 0:1], co['sums'][:, None], counts], dim=1)
        mag[:, m] = torch.cat([ts['mag'], la['mag'], fa['mag'][:, 0:1], co['mag'][:, None], counts], dim=1)
        if g is not None:
            out['dgp'].append(ts['dgp'])
            out['dgp_mag'].append(ts['dgp_mag'])
            out['dlp'].append(la['dp'].view_as(lp[:, m]))
            out['dlp_mag'].append(la['dp_mag'].view_as(lp[:, m]))
            out['dfp'].append(fa['dp'].view_as(fp[:, m]) + co['dp'])
            out['dfp_mag'].append(fa['dp_mag'].view_as(fp[:, m]) + co['dp_mag'])
            out['gp_inside'].append(ts['inside'])
            out['lp_inside'].append(la['inside'].view_as(lp[:, m]))
            out['fp_inside'].append(co['inside'])
    res = {'stats': stats, 'mag': mag}
    if g is not None:
        res.update({k: torch.stack(v, dim=1) for k, v in out.items()})
    return res


def lap_group_judge(pred, alpha, trimap, table=None, gs=None):
    """pred fp32 [B, M, 1, h, w], alpha [B, 1, h, w], trimap [B, h, w] or None -> sums [6, B * M] (row b * M + m) float64; with
    gs [6, B * M] also dpred [B, M, 1, h, w]"""
    B, Mk = pred.shape[:2]
    table = M.gauss_table() if table is None else table
    d0s, ws = [], []
    for m in range(Mk):
        d0, w = M.lap_d0(pred[:, m], alpha[:, 0], trimap)
        d0s.append(d0)
        ws.append(w)
    d0 = torch.stack(d0s, dim=1).view(B * Mk, 1, *pred.shape[-2:])
    j = M.lap_judge(d0, table, gs)
    out = {'sums': j['sums'], 'd0': d0}
    if gs is not None:
        w = torch.stack(ws, dim=1).view_as(d0)
        inside = M._inside(pred).view_as(d0)
        out['dpred'] = (j['g0'] * w * inside).view(B, Mk, 1, *pred.shape[-2:])
    return out


def lap_inverse_counts(h, w):
    return torch.tensor([1. / max((h >> l) * (w >> l), 1) for l in range(M.LEVELS + 1)], dtype=torch.float64).view(-1, 1)


def loss_judge(d, multilevel=False, weights=(1.,) * 8, supervise_all_iou=True, thr=THR, with_grad=False):
    """SAMMattingLoss / SAMMattingMultiLevelLoss of ONE decoder pass in float64 from the judges -> dict: losses (the eight weighted
    values by LOSS_KEYS), tables [8, B, M] (divided by B, unweighted), combine [B, M], best [B] (or None); with_grad: d global /
    local / fused preds and d iou_preds of the sum of the eight losses; d_*_mag the magnitudes of the pixel-sum terms and d_*_lap
    the Laplacian part of the gradient"""
    gp = d['global_preds']
    B, Mk, _, H, W = gp.shape
    P = float(H * W)
    gj = group_judge(d, thr)
    st = gj['stats']
    inv = lap_inverse_counts(H, W)
    lap_l = lap_group_judge(d['local_preds'], d['alpha'], d['trimap'])['sums'] if min(H, W) >= 32 else torch.zeros(6, B * Mk).double()
    lap_f = lap_group_judge(d['fused_preds'], d['alpha'], None)['sums'] if min(H, W) >= 32 else torch.zeros(6, B * Mk).double()
    gt = torch.clamp(st[..., 6] / torch.clamp(st[..., 7], min=1e-6), min=0., max=1.)
    ip = (d['iou_preds'].double() - gt) ** 2
    tables = torch.stack([st[..., 0] / (3. * P), st[..., 1] / P, st[..., 2] / (st[..., 3] + 1.), (lap_l * inv).sum(0).view(B, Mk),
                          st[..., 4] / P, (lap_f * inv).sum(0).view(B, Mk), st[..., 5] / (3. * P), ip]) / B
    wv = torch.tensor(weights, dtype=torch.float64)
    combine = (tables[:7] * wv[:7].view(7, 1, 1)).sum(0)
    best = None
    if multilevel:
        sel = torch.full((8, B, Mk), 1. / Mk, dtype=torch.float64)
    elif Mk > 1:
        best = torch.argmin(combine, dim=-1)
        onehot = torch.nn.functional.one_hot(best, Mk).double()
        sel = onehot.unsqueeze(0).repeat(8, 1, 1)
        sel[7] = torch.full((B, Mk), 1. / Mk, dtype=torch.float64) if supervise_all_iou else onehot
    else:
        sel = torch.ones(8, B, Mk, dtype=torch.float64)
    losses = {k: float((tables[i] * sel[i]).sum() * wv[i]) for i, k in enumerate(LOSS_KEYS)}
    out = {'losses': losses, 'tables': tables, 'combine': combine, 'best': best, 'stats': st}
    if with_grad:
        c = sel * wv.view(8, 1, 1) / B                                         # dL/d(table entry * B)
        gstats = torch.zeros(B, Mk, K, dtype=torch.float64)
        gstats[..., 0] = c[0] / (3. * P)
        gstats[..., 1] = c[1] / P
        gstats[..., 2] = c[2] / (st[..., 3] + 1.)
        gstats[..., 4] = c[4] / P
        gstats[..., 5] = c[6] / (3. * P)
        gj = group_judge(d, thr, gstats)
        gl = c[3].reshape(1, B * Mk) * inv
        gf = c[5].reshape(1, B * Mk) * inv
        dl = lap_group_judge(d['local_preds'], d['alpha'], d['trimap'], None, gl)['dpred']
        df = lap_group_judge(d['fused_preds'], d['alpha'], None, None, gf)['dpred']
        out.update(gstats=gstats, glap_local=gl, glap_fused=gf, d_global=gj['dgp'], d_local=gj['dlp'] + dl, d_fused=gj['dfp'] + df,
                   d_iou=c[7] * 2. * (d['iou_preds'].double() - gt),
                   d_global_mag=gj['dgp_mag'], d_local_mag=gj['dlp_mag'], d_fused_mag=gj['dfp_mag'], d_local_lap=dl, d_fused_lap=df)
    return out


def decided_margin(d, multilevel=False, **kw):
    """(second-best - best) / best of the combined loss, the smallest over the samples; inf when nothing is selected"""
    j = loss_judge(d, multilevel, **kw)
    if j['best'] is None:
        return float('inf')
    two = torch.sort(j['combine'], dim=-1)[0][:, :2]
    return float(((two[:, 1] - two[:, 0]) / two[:, 0]).min())


def model_batch(image_size, batch=2, seed=5):
    """the seeded batch of the model fixture in the SAMMattingBatchCollater contract: image, soft alpha mask [B, 1, S, S] (a blurred
    box), trimap (0 / 128 / 255 by the alpha), fg_map, bg_map, one positive point inside the box, the box, and a prompt mask"""
    g = torch.Generator().manual_seed(seed)
    s = image_size
    images = torch.randn(batch, 3, s, s, generator=g)
    masks = torch.zeros(batch, 1, s, s)
    points, boxes = [], []
    ramp = torch.linspace(0., 1., s // 8)
    for b in range(batch):
        x0, y0 = int(torch.randint(s // 8, s // 3, (1,), generator=g)), int(torch.randint(s // 8, s // 3, (1,), generator=g))
        x1, y1 = x0 + int(torch.randint(s // 3, s // 2, (1,), generator=g)), y0 + int(torch.randint(s // 3, s // 2, (1,), generator=g))
        masks[b, 0, y0:y1, x0:x1] = 1.
        masks[b, 0, y0:y1, x0:x0 + ramp.numel()] = ramp                      # a soft left edge
        points.append([[(x0 + x1) / 2., (y0 + y1) / 2., 1.]])
        boxes.append([float(x0), float(y0), float(x1), float(y1)])
    trimap = torch.full((batch, s, s), 128.)
    trimap[masks[:, 0] <= 0.] = 0.
    trimap[masks[:, 0] >= 1.] = 255.
    fg, bg = torch.rand(batch, 3, s, s, generator=g), torch.rand(batch, 3, s, s, generator=g)
    prompt_mask = torch.nn.functional.interpolate(masks, size=(s // 4, s // 4), mode='nearest')
    return dict(image=images, mask=masks, trimap=trimap, fg_map=fg, bg_map=bg, prompt_point=torch.tensor(points),
                prompt_box=torch.tensor(boxes), prompt_mask=prompt_mask)
