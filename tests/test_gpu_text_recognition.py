"""CTCModel (SimpleAICV/text_recognition/models) against a step RECORDED from the reference implementation
(tests/golden/ctc_model_r18_tiny.pt, scripts/record_ctc_model_golden.py): resnet18backbone, planes 32, 40 classes, 2 x 3 x 32 x 64,
fp32 -- `state_dict` keys, equal initial weights under the same seed, outputs, loss and whole-model gradients within the project's
1e-3 relative; then the model through tools/text_scripts.py: training with accumulation 1 and 2, validation, a batch of images of
different widths (the helpers are those of tests/test_gpu_text_loops.py)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
import test_gpu_text_loops as loops


def _build(fx):
    from SimpleAICV.text_recognition.models import CTCModel
    torch.manual_seed(0)
    return CTCModel(**fx['config'])


def test_state_dict_keys_and_initial_weights_are_the_reference_s():
    fx = load_golden('ctc_model_r18_tiny')
    model = _build(fx)
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sorted(sd.items())] == fx['keys']
    assert {k.split('.')[0] for k in sd} == {'backbone', 'encoder', 'predictor'}
    assert {k.split('.')[1] for k in sd if k.startswith('encoder.')} == {'linear0', 'rnn1', 'linear1', 'rnn2', 'linear2'}
    for k, ref in fx['init_sample'].items():
        v = sd[k].flatten()
        idx = torch.linspace(0, v.numel() - 1, min(16, v.numel())).long()
        assert torch.equal(v[idx].float(), ref.float()), k                     # the same draws in the same order


@pytest.mark.gpu
def test_recorded_reference_step():
    from SimpleAICV.text_recognition.losses import CTCLoss
    fx = load_golden('ctc_model_r18_tiny')
    model = _build(fx).cuda().train()
    b, c, h, w = fx['input_shape']
    x = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2).cuda()
    out = model(x)
    assert out.shape == fx['out'].shape
    e_out = rel_err(out, fx['out'])
    input_lengths = torch.full((b,), out.shape[1], dtype=torch.int32, device='cuda')
    loss = CTCLoss(blank_index=fx['blank'])(out.permute(1, 0, 2), fx['targets'].cuda(), input_lengths, fx['target_lengths'].cuda())
    loss.backward()
    e_loss = abs(float(loss) - fx['loss']) / abs(fx['loss'])
    print(f'output {e_out:.2e} loss {e_loss:.2e}')
    assert e_out < 1e-3 and e_loss < 1e-3
    worst = (0.0, '')
    params = dict(model.named_parameters())
    assert set(params) == set(fx['grad_norm'])
    for k, ref_norm in fx['grad_norm'].items():
        g = params[k].grad.detach().float().cpu().flatten()
        idx = torch.linspace(0, g.numel() - 1, min(16, g.numel())).long()
        ref = fx['grad_sample'][k].float()
        # relative to the parameter's own gradient: its norm, and for the sampled entries the larger of the largest sampled entry
        # and the gradient's rms (a handful of samples of a large tensor may all be small)
        e_norm = abs(float(g.norm()) - ref_norm) / ref_norm
        e_smp = float((g[idx] - ref).abs().max()) / max(float(ref.abs().max()), ref_norm / math.sqrt(g.numel()))
        worst = max(worst, (max(e_norm, e_smp), k))
        assert e_norm < 1e-3 and e_smp < 1e-3, (k, e_norm, e_smp)
    print(f'worst gradient deviation {worst[0]:.2e} ({worst[1]})')
    for k, ref in fx['bn_buffers'].items():
        assert rel_err(model.state_dict()[k], ref) < 1e-3, k


def _ctc_model(num_classes):
    from SimpleAICV.text_recognition.models import CTCModel
    return CTCModel('resnet18backbone', planes=32, num_classes=num_classes)


@pytest.mark.gpu
@pytest.mark.parametrize('accumulation_steps', [1, 2])
def test_three_optimizer_steps_of_the_model_lower_the_loss(accumulation_steps):
    got = loops._train(*loops._setup(4 * accumulation_steps, accumulation_steps, model_fn=_ctc_model))
    print('losses', got)
    assert len(got) == 4 and got[-1] < got[0], got


@pytest.mark.gpu
def test_validation_and_a_variable_width_batch_with_the_model():
    from simpleaicv_pytorch_training_examples_amd.tools import text_scripts
    config, model, optimizer, scheduler, loader = loops._setup(2, variable_width=True, model_fn=_ctc_model)
    assert len(loops._train(config, model, optimizer, scheduler, loader)) == 2
    result = text_scripts.test_text_recognition_for_all_dataset(config.val_loader_list, model, config.test_criterion, config)
    assert len(result) == 2
    for r in result.values():
        assert {'test_loss', 'str_acc', 'not_included_str_percent', 'final_edit_distance', 'lcs_precision', 'lcs_recall'} <= set(r)
        assert all(isinstance(r[k], (int, float)) and np.isfinite(r[k]) for k in r)


@pytest.mark.gpu
def test_entry_scripts_train_validate_and_checkpoint(tmp_path):
    """tools/train_text_recognition_model.py and tools/test_text_recognition_model.py on the benchmark configs of
    09.ocr_text_recognition_training/resnet50_ctc_model, shortened by their SAICV_OCR_* switches (resnet18backbone, 32 images of
    32 x 128, batch 8 with the config's accumulation_steps 2, two epochs: CosineLR has one warm-up epoch)"""
    import os
    import shutil
    import subprocess
    import sys
    from conftest import ROOT
    work = tmp_path / 'work'
    shutil.copytree(os.path.join(ROOT, '09.ocr_text_recognition_training', 'resnet50_ctc_model'), work)
    env = dict(os.environ, PYTHONPATH=str(ROOT), MASTER_ADDR='127.0.0.1', SAICV_OCR_BACKBONE='resnet18backbone', SAICV_OCR_TRAIN='32',
               SAICV_OCR_TEST='16', SAICV_OCR_BATCH='8', SAICV_OCR_WORKERS='0', SAICV_OCR_EPOCHS='2', SAICV_OCR_WIDTH='128',
               SAICV_OCR_PRINT='1')

    def run(module):
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr', '127.0.0.1',
               '--master-port', '29541', '-m', f'simpleaicv_pytorch_training_examples_amd.tools.{module}', '--work-dir', str(work)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout + r.stderr

    out = run('train_text_recognition_model')
    assert 'CTCLoss: ' in out and 'train: epoch 002' in out and 'train done. model: CTCModel' in out
    assert 'lcs_precision: ' in out and 'final_edit_distance: ' in out
    ck = torch.load(work / 'checkpoints' / 'latest.pth', map_location='cpu', weights_only=True)
    assert ck['epoch'] == 2 and 'module.encoder.rnn1.weight_ih_l0' in ck['model_state_dict']
    assert 'module.predictor.linear2.weight' in ck['model_state_dict']
    assert tuple(ck['model_state_dict']['module.predictor.linear2.weight'].shape) == (12113, 512)
    out = run('test_text_recognition_model')
    assert 'eval dataset:synthetic_text' in out
    for key in ('test_loss', 'str_acc', 'not_included_str_percent', 'final_edit_distance', 'lcs_precision', 'lcs_recall'):
        assert f'{key}: ' in out


@pytest.mark.gpu
def test_step_graph_replays_the_training_of_the_model(deterministic):
    """nn.LSTM captures unchanged: config.use_step_graph captures the whole iteration of CTCModel (fixed width, accumulation 1).
    One eager warm-up iteration, the capture, two replays; the losses follow the eager loop's within the project's 1e-3 (the MIOpen
    LSTM backward is not promised to be bit-repeatable, so no exact comparison)."""
    steps = 3

    def run(use_graph):
        config, model, optimizer, scheduler, loader = loops._setup(steps, model_fn=_ctc_model, use_step_graph=use_graph,
                                                                   step_graph_warmup=1)
        got = loops._train(config, model, optimizer, scheduler, loader)
        torch.cuda.synchronize()
        return got, getattr(config, '_saicv_step_graphs', {})

    eager, _ = run(False)
    graph, graphs = run(True)
    print('losses eager', eager, 'graph', graph)
    assert len(graphs) == 1 and next(iter(graphs.values())).graph is not None and next(iter(graphs.values())).replays == steps - 1
    assert len(eager) == len(graph) == steps
    assert max(abs(a - b) / abs(a) for a, b in zip(eager, graph)) < 1e-3
