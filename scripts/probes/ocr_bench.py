"""Text-recognition probe: the CTC loss of the reference's resnet50_ctc_model config at its per-GPU shapes -- logits [T, B, C] =
[64, 256, 12113] as the permuted view of the model's [B, T, C] output, 1 to 24 labels per sample in targets of 80 columns -- forward
plus backward, fused (ops.ctc_loss, csrc/ctc.hip) against composed (preds.float(), F.log_softmax, F.ctc_loss, the reference
formula as torch ops on the device), in bf16 and fp32.  Per route: median time of forward + backward (HIP events, 7 windows of 10
calls after 3 warm-up calls; the times include the autograd and Python work around the launches), peak memory above the inputs; for the fused route the forward and the backward alone, each as a share of
8 TB/s against its minimum traffic (forward: the logits once; backward: the logits once and the gradient once).

    SAICV_CTC_RATIOS_OUT=ratios.json python -m pytest tests/test_gpu_ctc_kernels.py -q -m gpu
    python scripts/probes/ocr_bench.py [--out profiles/ocr_step.json] [--ratios ratios.json]

--ratios takes the file tests/test_gpu_ctc_kernels.py writes (worst error ratios against the float64 judge per route and dtype,
and every case above 4 x at the plain 2^-23 floor) and stores it under `accuracy_ratios`.

`resnet50_ctc_step`: CTCModel(resnet50backbone, planes 512, 12 113 outputs) at batch 256, 32 x 512, bf16 autocast, forward +
backward of model and CTCLoss (no optimizer), and the same time split by running each part's forward + backward alone on
detached inputs of the right shape: backbone, the two bidirectional nn.LSTM (MIOpen), the five linear layers of encoder and
predictor, the loss.  Last, the probe tries to capture that forward + backward into a torch.cuda.graph and reports whether
nn.LSTM captured and what a replay costs; the file is written before the attempt and again after it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, C, S = 64, 256, 12113, 80
HBM_PEAK = 8e12


def inputs(dtype):
    g = torch.Generator().manual_seed(0)
    base = torch.randn(B, T, C, generator=g).to(dtype).cuda()
    lens = torch.randint(1, 25, (B,), generator=g, dtype=torch.int32)
    targets = torch.full((B, S), C - 2, dtype=torch.int64)
    for b in range(B):
        targets[b, :lens[b]] = torch.randint(0, C - 2, (int(lens[b]),), generator=g)
    return base, targets.cuda(), torch.full((B,), T, dtype=torch.int32).cuda(), lens.cuda()


def timed(fn, windows=7, per=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / per)
    return statistics.median(out)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ocr_step.json'))
    ap.add_argument('--ratios', default=None, help='the file tests/test_gpu_ctc_kernels.py wrote (SAICV_CTC_RATIOS_OUT)')
    args = ap.parse_args()
    from simpleaicv_pytorch_training_examples_amd import ops
    from SimpleAICV.text_recognition.losses import CTCLoss

    result = {'shape': {'T': T, 'B': B, 'C': C, 'S': S, 'labels_per_sample': '1..24', 'layout': 'permuted view of [B, T, C]'},
              'device': torch.cuda.get_device_name(0), 'hbm_peak_bytes_per_s': HBM_PEAK, 'timing': 'HIP events, median of 7 windows of 10 calls after 3 warm-up calls, autograd and Python overhead included'}
    for name, dtype in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        base, targets, il, tl = inputs(dtype)
        base.requires_grad_(True)
        nbytes = base.numel() * base.element_size()
        entry = {}
        for route in ('fused', 'composed'):
            crit = CTCLoss(blank_index=C - 2)
            crit.route = route

            def step():
                base.grad = None
                crit(base.permute(1, 0, 2), targets, il, tl).backward()

            entry[route] = {'fwd_bwd_ms': timed(step), 'peak_mib_above_inputs': peak_above_inputs(step)}
        base.grad = None
        view = base.detach().permute(1, 0, 2)
        tg32, il32, tl32 = targets.int(), il.int(), tl.int()
        fwd_ms = timed(lambda: ops.ctc_loss(view, tg32, il32, tl32, C - 2))
        grad_view = base.permute(1, 0, 2)
        loss, _ = ops.ctc_loss(grad_view, tg32, il32, tl32, C - 2)
        bwd_ms = timed(lambda: torch.autograd.grad(loss, base, retain_graph=True))
        greedy_ms = timed(lambda: ops.ctc_greedy(view, il32))
        entry['fused_kernels'] = {
            'forward_ms': fwd_ms, 'forward_share_of_hbm_peak': nbytes / (fwd_ms * 1e-3) / HBM_PEAK,
            'backward_ms': bwd_ms, 'backward_share_of_hbm_peak': 2 * nbytes / (bwd_ms * 1e-3) / HBM_PEAK,
            'greedy_ms': greedy_ms, 'greedy_share_of_hbm_peak': nbytes / (greedy_ms * 1e-3) / HBM_PEAK}
        entry['fused_faster'] = entry['fused']['fwd_bwd_ms'] < entry['composed']['fwd_bwd_ms']
        result[name] = entry
        del base, loss
    if args.ratios:
        with open(args.ratios) as f:
            result['accuracy_ratios'] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)

    write()
    model_step(result, write)
    write()
    print(json.dumps(result, indent=1))


def model_step(result, write):
    from SimpleAICV.text_recognition.losses import CTCLoss
    from SimpleAICV.text_recognition.models import CTCModel
    from SimpleAICV.text_recognition.models.encoder import linear_frames
    torch.manual_seed(0)
    model = CTCModel('resnet50backbone', planes=512, num_classes=C).cuda().train()
    crit = CTCLoss(blank_index=C - 2)
    _, targets, il, tl = inputs(torch.bfloat16)
    images = torch.rand(B, 32, 512, 3, device='cuda').permute(0, 3, 1, 2)
    amp = lambda: torch.autocast('cuda', dtype=torch.bfloat16)              # noqa: E731

    def zero():
        for p in model.parameters():
            p.grad = None

    def full():
        zero()
        with amp():
            out = model(images)
            loss = crit(out.permute(1, 0, 2), targets, il, tl)
        loss.backward()

    out = {'batch': B, 'image': '32 x 512', 'dtype': 'bf16 autocast', 'what': 'forward + backward, no optimizer',
           'step_ms': timed(full, windows=5, per=3, warm=2)}
    result['resnet50_ctc_step'] = out
    with amp(), torch.no_grad():
        feat = model.backbone(images)[-1]
        seq = torch.mean(feat, dim=2).permute(0, 2, 1).contiguous()
    frames = seq.shape[1]

    def backbone():
        zero()
        with amp():
            y = model.backbone(images)[-1]
        y.float().mean().backward()

    def lstm():
        zero()
        with amp():
            x = torch.randn(B, frames, 512, device='cuda', requires_grad=True)
            y, _ = model.encoder.rnn1(x)
            z, _ = model.encoder.rnn2(y[..., :512])
        (y.float().mean() + z.float().mean()).backward()

    def linears():
        zero()
        enc, pred = model.encoder, model.predictor
        with amp():
            a = linear_frames(seq.detach().requires_grad_(True), enc.linear0)
            b1 = linear_frames(torch.randn(B, frames, 1024, device='cuda', requires_grad=True), enc.linear1)
            b2 = linear_frames(torch.randn(B, frames, 1024, device='cuda', requires_grad=True), enc.linear2)
            c = pred(b2)
        (a.float().mean() + b1.float().mean() + c.float().mean()).backward()

    logits = torch.randn(B, frames, C, device='cuda').bfloat16().requires_grad_(True)

    def loss_only():
        logits.grad = None
        crit(logits.permute(1, 0, 2), targets, il, tl).backward()

    out['frames'] = frames
    for name, fn in (('backbone_ms', backbone), ('lstm_ms', lstm), ('linears_ms', linears), ('loss_ms', loss_only)):
        out[name] = timed(fn, windows=5, per=3, warm=2)
    out['note'] = ('the parts run alone on detached inputs and end in a mean() backward, so they do not add up to step_ms exactly; '
                   'linears_ms includes the 12 113-wide predictor')
    write()
    # does the forward + backward capture with nn.LSTM in it?
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            full()
        torch.cuda.current_stream().wait_stream(side)
        zero()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            with amp():
                o = model(images)
                loss = crit(o.permute(1, 0, 2), targets, il, tl)
            loss.backward()
        out['captured_ms'] = timed(graph.replay, windows=5, per=3, warm=2)
        out['lstm_captures'] = True
    except Exception as e:                                                   # noqa: BLE001
        out['lstm_captures'] = False
        out['capture_error'] = str(e)[:300]


if __name__ == '__main__':
    main()
