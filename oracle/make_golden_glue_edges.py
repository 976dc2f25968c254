"""Generates tests/golden/glue_edges.pt by RUNNING THE REFERENCE (rope_apply and SelfAttention.apply_rope of
SimpleAICV/detection/models/backbones/dinov3vit.py :271-282, :347-368, imported from the reference tree) on the CPU in fp32 on the
exact-regime RoPE inputs tests/glue_common.py builds: integer q / k / v, dyadic sin / cos tables whose lower and upper halves are
INDEPENDENT (the model's own tables tile one half, which hides a kernel that reads the wrong half), prefix 0, 1, 5 and N.  fp32 is exact
on these inputs, so the file holds the rotated q and k as float16 (eighths below 32 are exact) and nothing else: results only, no
program text.  tests/test_glue_judge_host.py holds the float64 reference of glue_common to it.

Build container only:   python oracle/make_golden_glue_edges.py [reference root]"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SAICV_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'glue_edges.pt')


def main():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, REF)
    for name in ['cv2', 'torchvision', 'torchvision.ops', 'torchvision.transforms', 'pycocotools', 'pycocotools.mask', 'pycocotools.cocoeval',
                 'pycocotools.coco', 'calflops']:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    import glue_common as G
    from SimpleAICV.detection.models.backbones.dinov3vit import SelfAttention, rope_apply
    out = {'rope': {}}
    for case in G.rope_edge_cases():
        inp = G.rope_inputs(case)
        qkv, sin, cos = inp['qkv'].float(), inp['sin'].float(), inp['cos'].float()
        q, k, _ = (t.transpose(1, 2) for t in torch.unbind(qkv, 2))              # [B, heads, N, D], as compute_attention hands them over
        attn = SelfAttention(case.heads * case.D, head_nums=case.heads)
        if case.prefix < case.N:
            rq, rk = attn.apply_rope(q, k, (sin, cos))
            assert torch.equal(rq[:, :, case.prefix:], rope_apply(q[:, :, case.prefix:], sin, cos))
        else:
            rq, rk = q, k                                                         # no token left to rotate: apply_rope's prefix is all of them
        rq, rk = rq.transpose(1, 2).contiguous(), rk.transpose(1, 2).contiguous()
        assert torch.equal(rq.half().float(), rq) and torch.equal(rk.half().float(), rk)
        out['rope'][case.id] = {'q': rq.half().clone(), 'k': rk.half().clone()}
        print(case.id, tuple(rq.shape))
    torch.save(out, OUT)
    print('bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
