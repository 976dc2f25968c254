"""Timing of the bidirectional LSTM of the text-recognition encoder on its two routes, `library` (nn.LSTM, MIOpen) and `fused`
(ops.lstm, csrc/lstm.hip) -> profiles/ocr_lstm.json.  Both routes are measured in this one process and run; the library route of
this run is the baseline, not a number on file.

1. [B 256, T 64, I 512, H 512], bf16 and fp32: forward + backward of the two stacked bidirectional layers (rnn1, then rnn2 on the
   first 512 features of its output, ending in a mean() backward, as scripts/probes/ocr_bench.py prices the library route), peak
   memory above the inputs, and the fused route split into the recurrent forward, the recurrent backward (HIP events around the two
   launches, ops.KernelTimer) and the rest (the GEMMs, the weight packing and the glue).  For the recurrent kernels the achieved
   W_hh stream: steps x workgroups x weight bytes of one direction / time.
2. The resnet50 CTC step at batch 256, 32 x 512, bf16 autocast, forward + backward without optimizer, eager and captured.
Only the 16-row batch tile is built, so there is no tile comparison.
HIP events, median of windows after warm-up; autograd and Python overhead included.  --accuracy FILE copies the error / bound
ratios tests/test_gpu_lstm_kernels.py wrote (SAICV_LSTM_RATIOS_OUT) under the key `accuracy`; an `accuracy` entry already in the
output file is kept otherwise."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, T, I, H, C = 256, 64, 512, 512, 12113
TILE = 16


def timed(fn, windows=7, per=5, warm=3):
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


def layers(result):
    from simpleaicv_pytorch_training_examples_amd import ops
    from SimpleAICV.text_recognition.models.encoder import BiLSTMEncoder
    torch.manual_seed(0)
    for name, dtype in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        enc = {r: BiLSTMEncoder(2048, H, rnn_route=r).cuda().train() for r in ('library', 'fused')}
        enc['fused'].load_state_dict(enc['library'].state_dict())
        x = torch.randn(B, T, I, device='cuda').to(dtype).requires_grad_(True)
        entry = {}

        def step(route):
            e = enc[route]
            for p in e.parameters():
                p.grad = None
            x.grad = None
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                y = e._rnn(e.rnn1, x)
                z = e._rnn(e.rnn2, y[..., :H])
            (y.float().mean() + z.float().mean()).backward()

        rounds = {'library': [], 'fused': []}
        for _ in range(2):                                       # the two routes alternate: clock drift touches both alike
            for route in ('library', 'fused'):
                rounds[route].append(timed(lambda: step(route)))
        for route in ('library', 'fused'):
            entry[route] = {'fwd_bwd_ms': min(rounds[route]), 'fwd_bwd_ms_rounds': rounds[route],
                            'peak_mib_above_inputs': peak_above_inputs(lambda: step(route))}
        # the recurrent launches alone, by events around them
        ops.KernelTimer.enabled, ops.KernelTimer.only, ops.KernelTimer.records = True, {'lstm_fwd', 'lstm_bwd'}, []
        n = 10
        for _ in range(n):
            step('fused')
        torch.cuda.synchronize()
        summ = ops.KernelTimer.summary()
        ops.KernelTimer.enabled, ops.KernelTimer.only, ops.KernelTimer.records = False, None, []
        esz = 2 if dtype == torch.bfloat16 else 4
        stream_bytes = T * 2 * ((B + TILE - 1) // TILE) * 4 * H * H * esz          # per launch: steps x workgroups x one direction's W_hh
        fwd_ms, bwd_ms = summ['lstm_fwd']['ms'] / summ['lstm_fwd']['calls'], summ['lstm_bwd']['ms'] / summ['lstm_bwd']['calls']
        entry['fused_split'] = {
            'recurrent_forward_ms_per_layer': fwd_ms, 'recurrent_backward_ms_per_layer': bwd_ms,
            'recurrent_ms_two_layers': 2 * (fwd_ms + bwd_ms),
            'gemms_packing_and_glue_ms_two_layers': entry['fused']['fwd_bwd_ms'] - 2 * (fwd_ms + bwd_ms),
            'whh_stream_bytes_per_launch': stream_bytes,
            'forward_whh_bytes_per_s': stream_bytes / (fwd_ms * 1e-3), 'backward_whh_bytes_per_s': stream_bytes / (bwd_ms * 1e-3),
            'workgroups': 2 * ((B + TILE - 1) // TILE)}
        entry['fused_faster'] = entry['fused']['fwd_bwd_ms'] < entry['library']['fwd_bwd_ms']
        result[name] = entry
        del enc, x


def model_step(result):
    from SimpleAICV.text_recognition.losses import CTCLoss
    from SimpleAICV.text_recognition.models import CTCModel
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(1, 25, (B,), generator=g, dtype=torch.int32)
    targets = torch.full((B, 80), C - 2, dtype=torch.int64)
    for b in range(B):
        targets[b, :lens[b]] = torch.randint(0, C - 2, (int(lens[b]),), generator=g)
    targets, tl, il = targets.cuda(), lens.cuda(), torch.full((B,), T, dtype=torch.int32).cuda()
    images = torch.rand(B, 32, 512, 3, device='cuda').permute(0, 3, 1, 2)
    crit = CTCLoss(blank_index=C - 2)
    out = {'batch': B, 'image': '32 x 512', 'dtype': 'bf16 autocast', 'what': 'forward + backward, no optimizer'}
    result['resnet50_ctc_step'] = out
    for route in ('library', 'fused'):
        torch.manual_seed(0)
        model = CTCModel('resnet50backbone', planes=512, num_classes=C, rnn_route=route).cuda().train()

        def zero():
            for p in model.parameters():
                p.grad = None

        def full():
            zero()
            with torch.autocast('cuda', dtype=torch.bfloat16):
                o = model(images)
                loss = crit(o.permute(1, 0, 2), targets, il, tl)
            loss.backward()

        r = {'eager_ms': timed(full, windows=5, per=3, warm=2)}
        out[route] = r
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                full()
            torch.cuda.current_stream().wait_stream(side)
            zero()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    o = model(images)
                    loss = crit(o.permute(1, 0, 2), targets, il, tl)
                loss.backward()
            r['captured_ms'] = timed(graph.replay, windows=5, per=3, warm=2)
            del graph
        except Exception as e:                                                   # noqa: BLE001
            r['capture_error'] = str(e)[:300]
        del model
        torch.cuda.empty_cache()
    lib, fus = out['library'], out['fused']
    out['fused_faster_eager'] = fus['eager_ms'] < lib['eager_ms']
    out['fused_faster_captured'] = ('captured_ms' in fus and 'captured_ms' in lib and fus['captured_ms'] < lib['captured_ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ocr_lstm.json'))
    ap.add_argument('--accuracy', default=None, help='the file tests/test_gpu_lstm_kernels.py wrote (SAICV_LSTM_RATIOS_OUT)')
    ap.add_argument('--skip-model', action='store_true')
    args = ap.parse_args()
    result = {'shape': {'B': B, 'T': T, 'I': I, 'H': H, 'layers': 'rnn1, then rnn2 on the first 512 features of its output'},
              'device': torch.cuda.get_device_name(0), 'batch_tile': TILE,
              'timing': 'HIP events, median of 7 windows of 5 calls after 3 warm-up calls, the smaller of two alternating rounds per route; '
                        'autograd and Python overhead included'}
    keep = None
    for path in (args.accuracy, args.out):
        if keep is None and path and os.path.exists(path):
            with open(path) as f:
                keep = json.load(f).get('accuracy')
    if keep is not None:
        result['accuracy'] = keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)

    layers(result)
    write()
    if not args.skip_model:
        model_step(result)
        write()
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
