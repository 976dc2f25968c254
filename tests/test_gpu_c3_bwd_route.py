"""The fused c3 backward route of ops.ConvBnActFn.backward (saicv_c3_bwd_stream, csrc/c3bwd.hip): a stack of two identity
bottleneck blocks (256 -> 64 -> 64 -> 256) at batch 2, 24 x 24 under bf16 autocast, SAICV_C3_BWD_MIN_ROWS=0.

The third convolution of the FIRST block qualifies: its dz is the tensor the second block's first data gradient wrote (with the
backward sums of the join in its epilogue), its shortcut gradient leaves gated.  The second block's does not (its dz comes from the
loss: no sums).  Checked: the fused entry runs exactly for that node and no dy is allocated for it; it does not run when z has a
second consumer, in fp32, for a 3 x 3 join, or with BN_FUSE off; the gate ledger ends at zero; every gradient agrees with the
three-kernel route.

Tolerance between the routes: at this size (1152 pixels, below the streaming kernels' threshold) the three-kernel route's data
gradient is the tiled kernel, whose association of the K sum is not the fused launch's, so dx of the fused node may differ by bf16
rounding flips -- one ulp, 2^-8 relative, on a fraction of its elements (test_gpu_c3_bwd_stream.py holds each route against
float64, and asserts bit-equality at the streaming size) -- and the layers below see a perturbation of that size.  A gradient tensor
therefore agrees within one bf16 ulp of relative L2 distance (2^-8) and within 4 ulp of its largest magnitude element for element
(2^-6 max|.|); tensors computed before the fused node (the second block's, and the fused node's own dgamma / dbeta: the same finalize
launch over the same sums) are bit-equal in deterministic mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Recorder:
    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)


@pytest.fixture
def env(monkeypatch):
    from simpleaicv_pytorch_training_examples_amd import ops
    rec = _Recorder(ops.lib())
    monkeypatch.setattr(ops, 'lib', lambda: rec)
    monkeypatch.setattr(ops, 'BN_FUSE', True)
    monkeypatch.setattr(ops, 'BN_INLINE', False)
    monkeypatch.setenv('SAICV_C3_BWD_MIN_ROWS', '0')
    monkeypatch.setenv('SAICV_C3_BWD_STREAM', '1')
    prev = rec._real.saicv_set_deterministic(1)
    assert rec._real.saicv_deterministic_prepare(torch.cuda.current_stream().cuda_stream) == 0
    allocs = []
    real_empty = ops._empty_nhwc

    def empty(n, c, h, w, dtype, device):
        allocs.append(c)
        return real_empty(n, c, h, w, dtype, device)

    monkeypatch.setattr(ops, '_empty_nhwc', empty)
    yield ops, rec, monkeypatch, allocs
    rec._real.saicv_set_deterministic(prev)


def _stack(block, *args):
    torch.manual_seed(3)
    blocks = torch.nn.Sequential(block(*args), block(*args)).cuda()
    for m in blocks.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    return blocks


def _grads(rec, allocs, blocks, c, autocast=True, second_consumer=False):
    """-> (fused calls in backward, 256-channel allocations in backward, {name: gradient})"""
    g = torch.Generator(device='cuda').manual_seed(11)
    x = torch.randn(2, c, 24, 24, device='cuda', generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    blocks.zero_grad(set_to_none=True)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        z1 = blocks[0](x.bfloat16() if autocast else x)
        z = blocks[1](z1)
        loss_extra = z1.float().square().mean() if second_consumer else 0.0
    dz = torch.randn(z.shape, device='cuda', generator=g).to(z.dtype).contiguous(memory_format=torch.channels_last)
    rec.names.clear()
    del allocs[:]
    if second_consumer:
        torch.autograd.backward([z, loss_extra], [dz, torch.ones((), device='cuda')])
    else:
        z.backward(dz)
    torch.cuda.synchronize()
    out = {'input': x.grad.float()}
    out.update({n: p.grad.float().clone() for n, p in blocks.named_parameters()})
    return rec.names.count('saicv_c3_bwd_stream'), sum(1 for a in allocs if a == 256), out


def test_fused_route_matches_three_kernels(env):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import Bottleneck
    ops, rec, mp, allocs = env
    blocks = _stack(Bottleneck, 256, 64)
    calls1, wide1, new = _grads(rec, allocs, blocks, 256)
    assert ops._GateLedger.pending == 0
    mp.setenv('SAICV_C3_BWD_STREAM', '0')
    calls0, wide0, old = _grads(rec, allocs, blocks, 256)
    assert ops._GateLedger.pending == 0
    assert (calls1, calls0) == (1, 0)
    assert wide1 == wide0 - 1, (wide1, wide0)          # the eligible node's dy is never allocated
    assert set(new) == set(old)
    for name in sorted(old):
        a, b = new[name], old[name]
        assert bool(torch.isfinite(a).all()), name
        rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
        worst = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        print(f'{name}: relative L2 {rel:.3e}  worst element / max {worst:.3e}')
        if name.startswith('1.') or name in ('0.conv3.layer.1.weight', '0.conv3.layer.1.bias'):
            assert torch.equal(a, b), name
        else:
            assert rel <= 2.0 ** -8 and worst <= 2.0 ** -6, (name, rel, worst)


def test_atomic_statistics_mode_takes_the_route_too(env):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import Bottleneck
    ops, rec, mp, allocs = env
    mp.setattr(ops, 'BN_INLINE', True)
    rec._real.saicv_set_deterministic(0)
    blocks = _stack(Bottleneck, 256, 64)
    calls1, _, new = _grads(rec, allocs, blocks, 256)
    mp.setenv('SAICV_C3_BWD_STREAM', '0')
    calls0, _, old = _grads(rec, allocs, blocks, 256)
    assert (calls1, calls0) == (1, 0) and ops._GateLedger.pending == 0
    for name in sorted(old):
        rel = float((new[name] - old[name]).norm() / old[name].norm().clamp_min(1e-30))
        assert rel <= 2.0 ** -8, (name, rel)


def test_second_consumer_of_z_keeps_the_old_route(env):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import Bottleneck
    ops, rec, mp, allocs = env
    calls, _, _ = _grads(rec, allocs, _stack(Bottleneck, 256, 64), 256, second_consumer=True)
    assert calls == 0 and ops._GateLedger.pending == 0


def test_fp32_keeps_the_old_route(env):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import Bottleneck
    ops, rec, mp, allocs = env
    calls, _, _ = _grads(rec, allocs, _stack(Bottleneck, 256, 64), 256, autocast=False)
    assert calls == 0 and ops._GateLedger.pending == 0


def test_3x3_join_keeps_the_old_route(env):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import BasicBlock
    ops, rec, mp, allocs = env
    calls, _, _ = _grads(rec, allocs, _stack(BasicBlock, 64, 64), 64)
    assert calls == 0 and 'saicv_c3_bwd_stream_ok' not in rec.names and ops._GateLedger.pending == 0


def test_bn_fuse_off_keeps_the_old_route(env):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import Bottleneck
    ops, rec, mp, allocs = env
    mp.setattr(ops, 'BN_FUSE', False)
    calls, _, _ = _grads(rec, allocs, _stack(Bottleneck, 256, 64), 256)
    assert calls == 0 and ops._GateLedger.pending == 0
