"""The stem backward routes of ops.ConvBnActFn (saicv_bn_relu_maxpool_fwd_keep, saicv_bn_relu_maxpool_bwd_sums, then
saicv_bn_relu_maxpool_bwd_apply + the weight gradient, or saicv_stem_bwd_stream; csrc/pool.hip, csrc/stembwd.hip): a 7 x 7 stride-2
stem block 3 -> 64 with MaxPool2d(3, 2, 1) on the space-to-depth image of a (2, 3, 66, 94) input -- 2 x 33 x 47 = 3 102 output
pixels, odd extents -- under bf16 autocast.

With SAICV_STEM_BWD_MIN_ROWS=1000 the block is above the minimum.  SAICV_STEM_BWD_STREAM=2 (both parts): forward and backward take
the new entries and no gradient tensor of the convolution output's shape is allocated.  The default (1: the stream kernel is left
unrouted, profiles/stem_bwd_stream.md): the sums come from the kept maxima, the second pass and the weight gradient are today's.
In deterministic mode the pooled output and every parameter gradient of either are bit-equal to the same block with
SAICV_STEM_BWD_STREAM=0.  At the default minimum (65 536 rows), in fp32 and with the switch off none of the new launches is fetched
(in fp32 not even the predicate)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NEW = ('saicv_bn_relu_maxpool_fwd_keep', 'saicv_bn_relu_maxpool_bwd_sums', 'saicv_bn_relu_maxpool_bwd_apply',
       'saicv_stem_bwd_stream_ws_floats', 'saicv_stem_bwd_stream')
GATE = 'saicv_stem_bwd_stream_ok'
OLD_BWD = ['saicv_bn_relu_maxpool_bwd_ws_floats', 'saicv_bn_relu_maxpool_bwd', 'saicv_conv2d_wgrad', 'saicv_unpack_wgrad_s2d']
SHAPE = (2, 3, 66, 94)
OUT = (2, 64, 33, 47)


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
    monkeypatch.setenv('SAICV_STEM_BWD_STREAM', '2')
    monkeypatch.setenv('SAICV_STEM_BWD_MIN_ROWS', '1000')
    prev = ops.set_deterministic(True)
    allocs = []
    real_empty = ops._empty_nhwc

    def empty(n, c, h, w, dtype, device):
        allocs.append((n, c, h, w))
        return real_empty(n, c, h, w, dtype, device)

    monkeypatch.setattr(ops, '_empty_nhwc', empty)
    yield ops, rec, monkeypatch, allocs
    ops.set_deterministic(prev)


def _block():
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import ConvBnActBlock
    torch.manual_seed(5)
    blk = ConvBnActBlock(3, 64, 7, 2, 3, has_act=True).cuda()
    blk.layer[0].weight.data = blk.layer[0].weight.data.contiguous(memory_format=torch.channels_last)
    blk.layer[1].weight.data.uniform_(0.5, 1.5)
    blk.layer[1].bias.data.normal_(0, 0.2)
    return blk


def _run(ops, rec, allocs, blk, bf16=True):
    """-> (names fetched in forward, in backward, full-resolution allocations in backward, pooled output, {name: gradient})"""
    g = torch.Generator(device='cuda').manual_seed(17)
    x = torch.randn(*SHAPE, device='cuda', generator=g) + 0.5
    blk.zero_grad(set_to_none=True)
    rec.names.clear()
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
        xp = ops.pack_stem_input(x, blk.layer[0], torch.bfloat16 if bf16 else torch.float32)
        assert getattr(xp, '_saicv_s2d', None) is not None
        z = blk(xp, pool=(3, 2, 1))
    fwd = list(rec.names)
    dz = torch.randn(z.shape, device='cuda', generator=g).to(z.dtype).contiguous(memory_format=torch.channels_last)
    rec.names.clear()
    del allocs[:]
    z.backward(dz)
    torch.cuda.synchronize()
    grads = {n: p.grad.float().clone() for n, p in blk.named_parameters()}
    return fwd, list(rec.names), sum(1 for a in allocs if a == OUT), z.detach().clone(), grads


def test_streamed_route_matches_two_kernels(env):
    ops, rec, mp, allocs = env
    blk = _block()
    fwd1, bwd1, full1, z1, new = _run(ops, rec, allocs, blk)
    mp.setenv('SAICV_STEM_BWD_STREAM', '0')
    fwd0, bwd0, full0, z0, old = _run(ops, rec, allocs, blk)
    print(fwd1, bwd1, fwd0, bwd0)
    assert 'saicv_bn_relu_maxpool_fwd_keep' in fwd1 and 'saicv_bn_relu_maxpool_fwd' not in fwd1
    assert bwd1 == ['saicv_bn_relu_maxpool_bwd_sums', 'saicv_stem_bwd_stream_ws_floats', 'saicv_stem_bwd_stream', 'saicv_unpack_wgrad_s2d']
    assert not any(n in fwd0 + bwd0 for n in NEW) and bwd0 == OLD_BWD
    assert (full1, full0) == (0, 1)                     # dy is never allocated
    assert torch.equal(z1.view(torch.int16), z0.view(torch.int16))
    assert set(new) == set(old) and len(new) >= 3
    for name in sorted(old):
        assert bool(torch.isfinite(new[name]).all()) and float(new[name].abs().sum()) > 0, name
        assert torch.equal(new[name], old[name]), (name, float((new[name] - old[name]).abs().max()))


def test_default_route_keeps_the_maxima_and_todays_second_pass(env):
    ops, rec, mp, allocs = env
    mp.delenv('SAICV_STEM_BWD_STREAM')
    blk = _block()
    fwd1, bwd1, full1, z1, new = _run(ops, rec, allocs, blk)
    mp.setenv('SAICV_STEM_BWD_STREAM', '0')
    _, bwd0, full0, z0, old = _run(ops, rec, allocs, blk)
    assert 'saicv_bn_relu_maxpool_fwd_keep' in fwd1 and 'saicv_bn_relu_maxpool_fwd' not in fwd1
    assert bwd1 == ['saicv_bn_relu_maxpool_bwd_sums', 'saicv_bn_relu_maxpool_bwd_apply', 'saicv_conv2d_wgrad', 'saicv_unpack_wgrad_s2d']
    assert bwd0 == OLD_BWD and (full1, full0) == (1, 1)
    assert torch.equal(z1.view(torch.int16), z0.view(torch.int16))
    for name in sorted(old):
        assert torch.equal(new[name], old[name]), (name, float((new[name] - old[name]).abs().max()))


def test_atomics_mode_takes_the_route_too(env):
    ops, rec, mp, allocs = env
    ops.set_deterministic(False)
    blk = _block()
    _, bwd1, full1, _, new = _run(ops, rec, allocs, blk)
    mp.setenv('SAICV_STEM_BWD_STREAM', '0')
    _, bwd0, _, _, old = _run(ops, rec, allocs, blk)
    assert 'saicv_stem_bwd_stream' in bwd1 and full1 == 0 and bwd0 == OLD_BWD
    for name in sorted(old):
        # the same products in another order of fp32 additions: 3 102 rows, far inside 2^-10 of the tensor's norm
        rel = float((new[name] - old[name]).norm() / old[name].norm().clamp_min(1e-30))
        assert rel <= 2.0 ** -10, (name, rel)


def test_below_the_minimum_keeps_todays_launches(env):
    ops, rec, mp, allocs = env
    mp.delenv('SAICV_STEM_BWD_MIN_ROWS')
    fwd, bwd, full, _, _ = _run(ops, rec, allocs, _block())
    assert not any(n in fwd + bwd for n in NEW) and bwd == OLD_BWD and full == 1


def test_switch_off_keeps_todays_launches(env):
    ops, rec, mp, allocs = env
    mp.setenv('SAICV_STEM_BWD_STREAM', '0')
    fwd, bwd, full, _, _ = _run(ops, rec, allocs, _block())
    assert not any(n in fwd + bwd for n in NEW) and bwd == OLD_BWD and full == 1


def test_fp32_keeps_todays_launches(env):
    ops, rec, mp, allocs = env
    fwd, bwd, full, _, _ = _run(ops, rec, allocs, _block(), bf16=False)
    assert not any(n in fwd + bwd for n in NEW + (GATE,)) and bwd == OLD_BWD and full == 1
