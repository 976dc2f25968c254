"""Records tests/golden/ctc_tiny.pt by RUNNING THE REFERENCE's CTCLoss class (SimpleAICV/text_recognition/losses.py:21-46) on the
CPU in fp32: seeded logits of [T, B, C] = [10, 3, 9] (one alignment per sample raised by 6), the blank at C - 2 (the converter's
'[CTCblank]') and the garbage label C - 1 in one target (an unknown character), targets padded with the blank as
CTCTextLabelConverter.encode pads them, one sample with input_length < T and one with a repeated character.  Recorded: the inputs, and loss + gradient with respect to the logits
without focal weighting and with it (gamma 2.0).  The fixture holds tensors and settings only.

    python scripts/record_ctc_golden.py --reference /path/to/reference/checkout

No test imports this script; tests/test_ctc_host.py pins the float64 judge and the CPU CTCLoss to these values."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'ctc_tiny.pt')
T, B, C, S = 10, 3, 9, 6


def inputs():
    g = torch.Generator().manual_seed(9)
    preds = torch.randn(T, B, C, generator=g) * 1.5
    blank = C - 2
    targets = torch.full((B, S), blank, dtype=torch.long)
    labs = [[2, 2, C - 1, 0], [5], [1, 3, 1, 6, 6]]
    for b, lab in enumerate(labs):
        targets[b, :len(lab)] = torch.tensor(lab)
        path = [k for c in lab for k in (c, blank)]               # one alignment gets + 6: nll of order 1, so the focal weight matters
        for t in range(T):
            preds[t, b, path[t] if t < len(path) else blank] += 6.0
    return preds, targets, torch.IntTensor([T, T - 3, T]), torch.IntTensor([len(x) for x in labs]), blank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of a checkout of the reference implementation')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from SimpleAICV.text_recognition.losses import CTCLoss

    preds, targets, in_len, tg_len, blank = inputs()
    rec = {'preds': preds, 'targets': targets, 'input_lengths': in_len, 'target_lengths': tg_len, 'blank': blank, 'gamma': 2.0}
    for name, kw in (('plain', {}), ('focal', {'use_focal_weight': True, 'gamma': 2.0})):
        x = preds.clone().requires_grad_(True)
        loss = CTCLoss(blank_index=blank, **kw)(x, targets, in_len, tg_len)
        loss.backward()
        rec[name] = {'loss': loss.detach().clone(), 'grad': x.grad.clone()}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(rec, OUT)
    print(OUT, {k: float(rec[k]['loss']) for k in ('plain', 'focal')})


if __name__ == '__main__':
    main()
