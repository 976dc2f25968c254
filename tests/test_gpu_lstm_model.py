"""CTCModel with rnn_route='fused' (ops.lstm instead of nn.LSTM): the step recorded from the reference implementation
(tests/golden/ctc_model_r18_tiny.pt) at the thresholds of tests/test_gpu_text_recognition.py::test_recorded_reference_step, gradient
checkpointing, the training loop with accumulation 1 and 2, and -- the promise the library route cannot make -- a captured step
that replays bit-equal to the eager one in deterministic mode.  The loop helpers are those of tests/test_gpu_text_loops.py."""
import math

import pytest
import torch

from conftest import load_golden, rel_err
import test_gpu_text_loops as loops

pytestmark = pytest.mark.gpu


@pytest.fixture
def reproducible(deterministic):
    """Deterministic mode as tools.utils.set_seed() sets it up: the engine's ordered reductions (the `deterministic` fixture) and
    torch's deterministic convolution kernels, which the backbone's two (3, 1) stride-(2, 1) convolutions go through (their
    weight gradient is not repeatable run to run otherwise, on either rnn_route)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _build(fx, **kw):
    from SimpleAICV.text_recognition.models import CTCModel
    torch.manual_seed(0)
    return CTCModel(**dict(fx['config'], rnn_route='fused', **kw))


def _step(fx, model):
    from SimpleAICV.text_recognition.losses import CTCLoss
    b, c, h, w = fx['input_shape']
    x = torch.randn(b, h, w, c, generator=torch.Generator().manual_seed(1)).permute(0, 3, 1, 2).cuda()
    out = model(x)
    input_lengths = torch.full((b,), out.shape[1], dtype=torch.int32, device='cuda')
    loss = CTCLoss(blank_index=fx['blank'])(out.permute(1, 0, 2), fx['targets'].cuda(), input_lengths, fx['target_lengths'].cuda())
    loss.backward()
    return out, loss


def test_recorded_reference_step_on_the_fused_route():
    fx = load_golden('ctc_model_r18_tiny')
    model = _build(fx).cuda().train()
    assert model.encoder.rnn_route == 'fused'
    out, loss = _step(fx, model)
    assert out.shape == fx['out'].shape
    e_out = rel_err(out, fx['out'])
    e_loss = abs(float(loss.detach()) - fx['loss']) / abs(fx['loss'])
    print(f'output {e_out:.2e} loss {e_loss:.2e}')
    assert e_out < 1e-3 and e_loss < 1e-3
    worst = (0.0, '')
    params = dict(model.named_parameters())
    assert set(params) == set(fx['grad_norm'])
    for k, ref_norm in fx['grad_norm'].items():
        g = params[k].grad.detach().float().cpu().flatten()
        idx = torch.linspace(0, g.numel() - 1, min(16, g.numel())).long()
        ref = fx['grad_sample'][k].float()
        e_norm = abs(float(g.norm()) - ref_norm) / ref_norm
        e_smp = float((g[idx] - ref).abs().max()) / max(float(ref.abs().max()), ref_norm / math.sqrt(g.numel()))
        worst = max(worst, (max(e_norm, e_smp), k))
        assert e_norm < 1e-3 and e_smp < 1e-3, (k, e_norm, e_smp)
    print(f'worst gradient deviation {worst[0]:.2e} ({worst[1]})')
    for k, ref in fx['bn_buffers'].items():
        assert rel_err(model.state_dict()[k], ref) < 1e-3, k


def test_gradient_checkpointing_gives_the_same_step(reproducible):
    fx = load_golden('ctc_model_r18_tiny')
    plain = _build(fx).cuda().train()
    ckpt = _build(fx, use_gradient_checkpoint=True).cuda().train()
    assert ckpt.use_gradient_checkpoint and not plain.use_gradient_checkpoint
    _, la = _step(fx, plain)
    _, lb = _step(fx, ckpt)
    assert torch.equal(la, lb)
    ga, gb = dict(plain.named_parameters()), dict(ckpt.named_parameters())
    for k in ga:
        assert torch.equal(ga[k].grad, gb[k].grad), k                      # deterministic mode: bit-equal


def _fused_model(num_classes):
    from SimpleAICV.text_recognition.models import CTCModel
    return CTCModel('resnet18backbone', planes=32, num_classes=num_classes, rnn_route='fused')


@pytest.mark.parametrize('accumulation_steps', [1, 2])
def test_three_optimizer_steps_lower_the_loss(accumulation_steps):
    got = loops._train(*loops._setup(4 * accumulation_steps, accumulation_steps, model_fn=_fused_model))
    print('losses', got)
    assert len(got) == 4 and got[-1] < got[0], got


def test_captured_step_replays_bit_equal_to_the_eager_step(reproducible):
    """one eager warm-up iteration, the capture, two replays against three eager iterations: the same losses and the same
    parameters, bit for bit"""
    steps = 3

    def run(use_graph):
        config, model, optimizer, scheduler, loader = loops._setup(steps, model_fn=_fused_model, use_step_graph=use_graph,
                                                                   step_graph_warmup=1)
        got = loops._train(config, model, optimizer, scheduler, loader)
        torch.cuda.synchronize()
        return got, {k: v.detach().clone() for k, v in model.state_dict().items()}, getattr(config, '_saicv_step_graphs', {})

    eager, p_eager, _ = run(False)
    graph, p_graph, graphs = run(True)
    print('losses eager', eager, 'graph', graph)
    assert len(graphs) == 1 and next(iter(graphs.values())).graph is not None and next(iter(graphs.values())).replays == steps - 1
    assert len(eager) == len(graph) == steps
    assert eager == graph
    assert set(p_eager) == set(p_graph)
    for k in p_eager:
        assert torch.equal(p_eager[k], p_graph[k]), k
