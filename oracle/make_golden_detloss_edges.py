"""Generates tests/golden/detloss_edges.pt by RUNNING THE REFERENCE (SimpleAICV/detection/losses.py RetinaLoss :324-411 and FCOSLoss
:619-840, imported from /root/reference; the arg-max of decode.py:229, which is numpy's) on the CPU in fp32 on the exact-regime edge
inputs tests/detloss_common.py builds: the planted IoU 1/2, 2/5 and 1, tied boxes, padding rows first / in the middle / last, an image
of only padding rows, points on a box edge, at the sampling radius and at either end of the regression range, nested and equal-area
boxes, equal maxima.  Holds int8 class targets, (l, t, r, b) (float16: half-integers below 2048 are exact), the positive counts and the
loss scalars only.  tests/test_detloss_judge_host.py holds the float64 references of detloss_common to it: the tie rules (first maximum,
first minimum) are pinned to the reference's behaviour, not to a document.

Build container only:   python oracle/make_golden_detloss_edges.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = '/root/reference'
OUT = os.path.join(ROOT, 'tests', 'golden', 'detloss_edges.pt')


def main():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, REF)
    for name in ['cv2', 'torchvision', 'torchvision.ops', 'torchvision.transforms', 'pycocotools', 'pycocotools.mask', 'pycocotools.cocoeval',
                 'pycocotools.coco', 'calflops']:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    import detloss_common as D
    from SimpleAICV.detection.losses import FCOSLoss, RetinaLoss
    out = {'retina': {}, 'fcos': {}, 'best': {}}
    cases = D.edge_cases()
    for case in cases['retina']:
        inp = D.retina_inputs(case)
        crit = RetinaLoss(box_loss_type='SmoothL1' if case.smoothl1 else 'GIoU', beta=D.EDGE_BETA)
        anchors = inp['anchors'].float().unsqueeze(0).repeat(case.B, 1, 1)
        tg = crit.get_batch_anchors_annotations(anchors, inp['annots'].float())
        rec = {'cls': tg[:, :, 4].to(torch.int8).clone(), 'pos': int((tg[:, :, 4] > 0).sum())}
        if not case.smoothl1:
            assert torch.equal(tg[:, :, :4], tg[:, :, :4].half().float())
            rec['box'] = tg[:, :, :4].half().clone()
        probs, reg = D.edge_heads(case.id, case.B, case.A)
        flat = tg.view(-1, 5)
        rec['cls_loss'] = float(crit.compute_batch_focal_loss(torch.clamp(probs.float().view(-1, D.EDGE_CLASSES), min=1e-4, max=1. - 1e-4), flat))
        if case.smoothl1:
            rec['reg_loss'] = float(crit.compute_batch_box_loss(reg.float().view(-1, 4), flat, anchors.view(-1, 4)))
        out['retina'][case.id] = rec
        print(case.id, rec['pos'], rec['cls_loss'], rec.get('reg_loss'))
    for case in cases['fcos']:
        inp = D.fcos_inputs(case)
        pts = inp['points'].float()
        strides = [s for s in D.FCOS_STRIDES if bool((pts[:, 2] == s).any())]
        assert strides == list(D.FCOS_STRIDES[:len(strides)])
        mi = [list(r) for r in D.FCOS_RANGES[case.ranges][:len(strides)]]
        crit = FCOSLoss(strides=strides, mi=mi, center_sample_radius=D.FCOS_RADIUS, use_center_sample=bool(case.center_sample))
        order = torch.cat([(pts[:, 2] == s).nonzero()[:, 0] for s in strides])            # the reference wants the points level by level
        heads_c, heads_r, heads_k, positions = [], [], [], []
        for s in strides:
            n = int((pts[:, 2] == s).sum())
            heads_c.append(torch.zeros(case.B, n, 1, D.EDGE_CLASSES))
            heads_r.append(torch.zeros(case.B, n, 1, 4))
            heads_k.append(torch.zeros(case.B, n, 1, 1))
            positions.append(pts[pts[:, 2] == s][:, :2].view(1, n, 1, 2).repeat(case.B, 1, 1, 1))
        _, _, _, tg = crit.get_batch_position_annotations(heads_c, heads_r, heads_k, positions, inp['annots'].float(),
                                                          use_center_sample=bool(case.center_sample))
        back = torch.empty_like(order)
        back[order] = torch.arange(order.numel())
        tg = tg[:, back]
        assert torch.equal(tg[0, :, 6:8], pts[:, :2])
        assert torch.equal(tg[:, :, :4], tg[:, :, :4].half().float())
        rec = {'cls': tg[:, :, 4].to(torch.int8).clone(), 'ltrb': tg[:, :, :4].half().clone(), 'pos': int((tg[:, :, 4] > 0).sum())}
        probs, _ = D.edge_heads(case.id, case.B, case.P)
        rec['cls_loss'] = float(crit.compute_batch_focal_loss(torch.clamp(probs.float().view(-1, D.EDGE_CLASSES), min=1e-4, max=1. - 1e-4),
                                                              tg.reshape(-1, 8)))
        out['fcos'][case.id] = rec
        print(case.id, rec['pos'], rec['cls_loss'])
    for case in cases['best']:
        inp = D.best_inputs(case)
        out['best'][case.id] = {'classes': torch.from_numpy(np.argmax(inp['probs'].float().numpy(), axis=2)).to(torch.int8)}
    torch.save(out, OUT)
    print('bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
